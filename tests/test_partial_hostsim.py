"""The partial decoder (LZ4_decompress_safe_partial) on the CPU: tests/hostsim/hostsim_partial.cpp compiles decode_block's PARTIAL switch
(lz4-java_amd/csrc/lz4_decode_core.h) against the lock-step lane simulator in the forms the partial kernels run -- the staged loop with 4
lanes, the deep loop with 8, and the plain loop with both -- with the simulator's destination bound set to min(target, cap), and this
file checks return value and bytes against the reference library's own LZ4_decompress_safe_partial."""
import ctypes as C

import pytest

from conftest import calgary
from partial_common import (caps_for, damaged, long_literal_stream, overlap_stream, ref_partial, rng_for, same_bytes,
                            targets_for)
from support import build_sim

FORMS = ((0, 4), (0, 8), (1, 4), (2, 8))   # (form, lanes): plain, plain, staged (decode_partial_kernel<4, 0, true>), deep (<8>)


def load_sim():
    l = build_sim("hostsim_partial")
    l.sim_decompress_partial.restype = C.c_int
    l.sim_decompress_partial.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def lz4p(ref):
    return ref_partial(ref)


def sim_partial(sim, s, t, c, form, gl):
    room = -1 if (t < 0 or c < 0) else min(t, c)
    out = C.create_string_buffer(max(room, 0) + 1)
    r = sim.sim_decompress_partial(bytes(s), len(s), out, t, c, form, gl)
    return r, out.raw[:max(r, 0)]


class Checker:
    def __init__(self, sim, lz4p):
        self.sim, self.lz4p, self.n = sim, lz4p, 0

    def check(self, s, t, c, what="", forms=FORMS):
        want = self.lz4p(s, t, c)
        for form, gl in forms:
            got = sim_partial(self.sim, s, t, c, form, gl)
            assert got[0] != -1000000, ("out of bounds", what, form, gl, len(s), t, c)
            assert got[0] == want[0], (what, form, gl, len(s), t, c, got[0], want[0])
            assert same_bytes(got[1], want[1], s, want[0], min(t, c)), (what, form, gl, len(s), t, c)
            self.n += 1
        return want[0]


@pytest.fixture(scope="module")
def chk(sim, lz4p):
    return Checker(sim, lz4p)


def streams(ref, O):
    """(name, stream, decoded size): Calgary blocks, App. F blocks and book1 slices, compressed by LZ4_compress_default and by
    LZ4_compress_HC level 12 (long matches)"""
    book1, geo, pic = calgary("book1"), calgary("geo"), calgary("pic")
    raw = [("book1[0:64K]", book1[:65536]), ("book1[300000:+64K]", book1[300000:365536]), ("geo[0:64K]", geo[:65536]),
           ("pic[64K:+64K]", pic[65536:131072]), ("book1[:5000]", book1[:5000]), ("appF0", O.gen_block(65536, 0)),
           ("appF7", O.gen_block(65536, 7)), ("appF(win=8)", O.gen_block(65536, 3, win=8)), ("appF(200000)", O.gen_block(200000, 5)),
           ("zeros", bytes(70000))]
    out = []
    for name, v in raw:
        out.append((name + "/fast", ref.compress_fast(v), len(v)))
        out.append((name + "/hc12", ref.compress_hc(v, 12), len(v)))
    return out


def test_partial_valid_streams_every_target_and_capacity(chk, ref, O):
    """targets 0 .. 607 around the tiers' distances, decoded -1 / +0 / +1, twice the size and random ones; capacity below, equal to and
    above each"""
    rng = rng_for(1)
    for name, s, d in streams(ref, O):
        for t in targets_for(d, rng):
            for c in caps_for(t, rng):
                chk.check(s, t, c, name)
    assert chk.n > 2000


def test_partial_whole_block_equals_safe_decode(sim, ref, O):
    """target >= decoded size: the same bytes as LZ4_decompress_safe"""
    for v in (calgary("book1")[:65536], O.gen_block(65536, 2), b"abcd      abcdefghij"):
        s = ref.compress_fast(v)
        for form, gl in FORMS:
            assert sim_partial(sim, s, len(v) + 100, len(v) + 100, form, gl) == (len(v), v)


def test_partial_truncated_streams(chk, ref, O):
    """every cut of small streams, random cuts of large ones: the prefix decodes to what its bytes hold"""
    rng = rng_for(2)
    book1 = calgary("book1")
    small = [ref.compress_fast(book1[:300]), ref.compress_hc(book1[1000:1400], 12), ref.compress_fast(O.gen_block(500, 1)),
             ref.compress_fast(bytes(300))]
    for s in small:
        for cut in range(len(s) + 1):
            for t in (rng.randrange(0, 600), 700):
                chk.check(s[:cut], t, t + rng.randrange(0, 3), "cut %d/%d" % (cut, len(s)), forms=((0, 4), (1, 4)))
    large = [ref.compress_fast(book1[:65536]), ref.compress_hc(book1[65536:131072], 12), ref.compress_fast(O.gen_block(65536, 9)),
             ref.compress_fast(O.gen_block(1 << 20, 4, win=4096))]
    for s in large:
        for _ in range(40):
            cut = rng.randrange(len(s) + 1)
            t = rng.choice([rng.randrange(1 << 21), 1 << 21, rng.randrange(2048)])
            chk.check(s[:cut], t, t, "cut %d/%d" % (cut, len(s)))


def test_partial_cut_inside_self_overlapping_match(chk):
    """matches at distance 1 .. 15 that overlap their own output, cut at every byte of the match and around it"""
    rng = rng_for(3)
    for off in range(1, 16):
        for _ in range(3):
            s, d = overlap_stream(rng, off)
            for t in range(0, d + 2):
                chk.check(s, t, t + (t & 1), "overlap off=%d" % off, forms=((0, 4), (0, 8)))
            chk.check(s, d, d, "overlap off=%d" % off)


def test_partial_damaged_and_random_streams(chk, ref, O):
    """random byte flips of valid streams and random bytes: liblz4's return value (error position included) and bytes"""
    rng = rng_for(4)
    book1 = calgary("book1")
    bases = [ref.compress_fast(book1[:4000]), ref.compress_hc(book1[9000:13000], 12), ref.compress_fast(O.gen_block(4000, 2)),
             ref.compress_fast(book1[:65536])]
    for s in bases:
        for _ in range(150):
            bad = damaged(s, rng, flips=rng.randrange(1, 4))
            t = rng.choice([rng.randrange(64), rng.randrange(5000), 70000])
            chk.check(bad, t, t + rng.randrange(0, 30), "damaged", forms=((0, 4), (2, 8)) if len(s) > 4000 else ((0, 8), (1, 4)))
    for _ in range(600):
        s = rng.randbytes(rng.randrange(0, 300))
        t = rng.randrange(0, 400)
        chk.check(s, t, t + rng.randrange(0, 5), "random", forms=((0, 4), (1, 4)))


def test_partial_edge_values(chk, sim):
    """target 0 -> 0 whatever the source; empty source, target > 0 -> -1; the single token 0x00 -> 0; negative sizes -> -1 (the
    engine's rule; the reference is not called with them)"""
    for s in (b"", b"\x00", b"\x10a", b"\xff" * 20):
        assert chk.check(s, 0, 0) == 0
        assert chk.check(s, 0, 50) == 0
    assert chk.check(b"", 5, 5) == -1
    assert chk.check(b"\x00", 5, 5) == 0
    for form, gl in FORMS:
        assert sim_partial(sim, b"\x10a", -1, 10, form, gl)[0] == -1
        assert sim_partial(sim, b"\x10a", 10, -1, form, gl)[0] == -1
        assert sim.sim_decompress_partial(b"\x10a", -1, C.create_string_buffer(16), 10, 10, form, gl) == -1


def test_partial_long_literal_run_is_cut_not_an_error(chk, ref):
    """a literal length whose extension bytes sum past 2^31 (liblz4 adds them as 32-bit unsigned): the partial decoder cuts the run
    to the input, LZ4_decompress_safe rejects the stream"""
    s, letters = long_literal_stream()
    assert ref.decompress_safe_raw(s, 1000)[0] < 0
    assert chk.check(s, 1000, 1000, "long literals") == 104
    assert chk.check(s, 50, 1000, "long literals") == 50
