"""The block shell on the CPU: what stands around a core's run() for one block -- liblz4's up-front returns, the byU16 / byU32 switch
at 65547 bytes, the results.  For the fast compressor that is lz4_fast_core.h's fast_block_run, which the kernels of compress_fast.hip
and the simulator entries sim_compress_fast / _ms / _accel / _dest_size / _fast_dict all go through (tests/hostsim/block_host.h is the
simulator's side of it); the HC entries keep a shell of their own and are held to the same rules here."""
import ctypes as C

import pytest

import test_accel_hostsim as TA
import test_destsize_hostsim as TD
import test_dictc_hostsim as TDC
import test_hc_destsize_hostsim as THD
import test_hcdict_hostsim as THC
import test_hostsim as TH

_u8p = C.POINTER(C.c_uint8)
TOO_LONG = 0x7E000001   # liblz4's LZ4_MAX_INPUT_SIZE + 1


@pytest.fixture(scope="module")
def entries():
    """name -> (run(n, cap) -> (return value, consumed or None, the one-byte output buffer afterwards), is a destSize form);
    the source and every other pointer is a one-byte buffer or null: an entry that touches any of them has not returned up front"""
    h, a, d, dc, hd, hc = TH.load_sim(), TA.load_sim(), TD.load_sim(), TDC.load_sim(), THD.load_sim(), THC.load_sim()
    h.sim_compress_hc.restype = C.c_int
    h.sim_compress_hc.argtypes = [C.c_char_p, C.c_int, _u8p, C.c_int, C.c_int, C.c_uint64]

    def plain(f):
        def run(n, cap):
            out = (C.c_uint8 * 1)(0xA5)
            return f(out, n, cap), None, out[0]
        return run

    def dest(f):
        def run(n, cap):
            out = (C.c_uint8 * 1)(0xA5)
            cons = C.c_int(-7)
            return f(out, n, cap, C.byref(cons)), cons.value, out[0]
        return run

    return {
        "plain": (plain(lambda o, n, cap: h.sim_compress_fast(b"x", n, o, cap, None, 0)), False),
        "ms": (plain(lambda o, n, cap: h.sim_compress_fast_ms(b"x", n, o, cap, None, 0)), False),
        "accel": (plain(lambda o, n, cap: a.sim_compress_fast_accel(b"x", n, o, cap, 2, None, 0)), False),
        "dict": (plain(lambda o, n, cap: dc.sim_compress_fast_dict(None, 0, None, b"x", n, o, cap, None, 0)), False),
        "hc": (plain(lambda o, n, cap: h.sim_compress_hc(b"x", n, o, cap, 9, 0)), False),
        "hc dict": (plain(lambda o, n, cap: hc.sim_compress_hc_dict(None, 0, None, None, b"x", n, o, cap, 9, 0)), False),
        "dest": (dest(lambda o, n, t, c: d.sim_compress_dest_size(b"x", n, o, t, c, None, 0)), True),
        "hc dest": (dest(lambda o, n, t, c: hd.sim_compress_hc_dest_size(b"x", n, o, t, 9, c, 0)), True),
    }


@pytest.mark.parametrize("name", ["plain", "ms", "accel", "dest", "dict", "hc", "hc dest", "hc dict"])
def test_early_returns(entries, name):
    """A negative length, a negative capacity and a length above 0x7E000000 return 0 before anything is read or written (never the
    simulator's out-of-bounds code); the destSize forms also return 0 for a target of 0, and every up-front 0 of theirs leaves the
    consumed size at the length given, as liblz4 leaves *srcSizePtr."""
    run, is_dest = entries[name]
    cases = [(-1, 16), (5, -1), (TOO_LONG, 16)] + ([(5, 0)] if is_dest else [])
    for n, cap in cases:
        r, cons, byte = run(n, cap)
        assert (r, byte) == (0, 0xA5), (name, n, cap, r)
        if is_dest:
            assert cons == n, (name, n, cap, cons)


@pytest.fixture(scope="module")
def book1_edge(corpus):
    book1 = corpus["book1[:200000]"]
    return {n: book1[:n] for n in (65546, 65547)}


@pytest.mark.parametrize("n", [65546, 65547])
def test_table_boundary(n, book1_edge, ref):
    """book1[:65546] is the last byU16 block, book1[:65547] the first byU32 one: plain, window-parallel, acceleration 2 and
    destSize with target = compressBound all switch tables in the shared shell, and each gives the reference library's bytes.
    (tests/test_accel_hostsim.py's corpus holds both sizes as well; the other entries met 65547 alone before.)"""
    v = book1_edge[n]
    cap = TD.bound(n)
    lib = C.CDLL(ref.path)
    lib.LZ4_compress_fast.restype = C.c_int
    lib.LZ4_compress_fast.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_int]

    def want(accel):
        out = (C.c_uint8 * cap)()
        r = lib.LZ4_compress_fast(v, out, n, cap, accel)
        return r, bytes(out[:r])

    h = TH.load_sim()
    assert TH.sim_compress(h, v, cap)[:2] == want(1)
    assert TH.sim_compress(h, v, cap, ms=True)[:2] == want(1)
    assert TA.sim_compress(TA.load_sim(), v, cap, 2)[:2] == want(2)
    assert TD.sim_dest(TD.load_sim(), v, cap) == TD.ref_dest_size(ref)(v, cap) == (want(1)[0], n, want(1)[1])
