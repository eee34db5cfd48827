"""The linked-block compressor (LZ4_compress_fast_continue over chains) on the CPU: tests/hostsim/hostsim_cchain.cpp compiles the chain
walk of lz4-java_amd/csrc/lz4_fast_chain.h and FastCore<..., LINK = true> of lz4_fast_core.h -- what compress_fast_chain_cu_kernel runs
-- against the lock-step lane simulator, and this file checks values and bytes against the reference library on the shared set
(tests/cchain_common.py).  Every case runs in two arena layouts.  The simulator flags a read outside the chain's kept history and its
source, a read at or past the end of the block that is running (so nothing past the chain's last byte), and a write outside the
block's slot; the bytes around every chain are guards."""
import ctypes as C
import random

import numpy as np
import pytest

from cchain_common import (CHAIN_STOPPED, CChain, CPacked, PREFIXES, RefCChain, book1, bound, case_set, chain_of, expected, hand_chains,
                           prefix_chains, stops_early)
from support import build_sim


def load_sim():
    l = build_sim("hostsim_cchain")
    l.sim_cchain_batch.restype = C.c_int
    l.sim_cchain_batch.argtypes = [C.c_void_p] * 10 + [C.c_uint32, C.c_uint32, C.c_uint64]
    l.sim_cchain_table.restype = C.c_int
    l.sim_cchain_table.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    l.sim_cchain_dict_image.restype = C.c_int
    l.sim_cchain_dict_image.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


@pytest.fixture(scope="module")
def cases(rc):
    chains = case_set(rc, random.Random(41))
    return chains, expected(rc, chains)


def run(sim, pk, layout, seed, prefix=True):
    """one call of the simulator on the packed chains; layout 0: [src | dst] in one buffer, 1: [dst | src] -> (status, dst, out, consumed)"""
    ns, nd = len(pk.src), len(pk.dst)
    arena = C.create_string_buffer(ns + nd + 1)
    base = C.addressof(arena)
    s0, d0 = (0, ns) if layout == 0 else (nd, 0)
    C.memmove(base + s0, pk.src, ns)
    C.memmove(base + d0, bytes(pk.dst), nd)
    a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
    cso, pre, sl, cf = a64(pk.chain_src_off), a32(pk.prefix), a32(pk.src_len), a32(pk.chain_first, np.uint32)
    do, dc = a64(pk.dst_off), a32(pk.dst_cap)
    out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
    r = sim.sim_cchain_batch(base + s0, cso.ctypes.data, pre.ctypes.data if prefix else None, sl.ctypes.data, cf.ctypes.data, base + d0,
                             do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains, seed)
    assert C.string_at(base + s0, ns) == pk.src
    return r, C.string_at(base + d0, nd), out, cons


def test_the_set_is_what_the_issue_asks_for(cases):
    chains, want = cases
    assert len(chains) >= 300, len(chains)
    assert stops_early(want) >= 40, stops_early(want)
    names = " | ".join(c.name for c in chains)
    for must in ("book1 70 x 1000", "book1 17 x 4096", "book1 3 x 65536", "book1 mixed"):
        assert must in names
    for c, (outs, done, by) in zip(chains, want):   # the stop rule
        if 0 in outs:
            k = outs.index(0)
            assert all(r > 0 for r in outs[:k]) and all(r == CHAIN_STOPPED for r in outs[k + 1:]) and done == sum(c.lens[:k]), c.name
        else:
            assert done == len(c.data), c.name


def test_reference_conditions(rc):
    """what the rules rely on, by the reference itself: prefixes of 0, 1 and 7 bytes give the same bytes and 8 is the first that differs;
    linking shrinks small blocks; an incompressible 4096-byte block takes 4114; a reloaded stream is not a running one; every chain of
    the set decodes (LZ4_decompress_safe_continue) to its source"""
    pre = prefix_chains()
    res = {P: [rc.compress(c)[2] for c in pre[P]] for P in PREFIXES}
    assert res[0] == res[1] == res[7]
    assert sum(a != b for a, b in zip(res[7], res[8])) >= 1
    assert all(len(set(bytes(b"".join(x)) for x in (res[P][i] for P in (8, 9, 100, 65535, 65536)))) > 1 for i in range(3))
    b = book1()
    data = b[:65536]
    linked = sum(rc.compress(chain_of("l", data, [256] * 256))[0])
    alone = sum(sum(rc.compress(chain_of("a", data[o:o + 256], [256]))[0]) for o in range(0, 65536, 256))
    assert linked < 0.8 * alone, (linked, alone)
    r = rc.compress(chain_of("rnd", random.Random(1).randbytes(8192), [4096] * 2))[0]
    assert r == [4114, 4114]
    ch = chain_of("reload", b[:64 * 1000], [1000] * 64)
    assert sum(x != y for x, y in zip(rc.compress(ch)[2], rc.compress(ch, reload_every=16)[2])) >= 32
    ch = chain_of("dec", b[3000:3000 + 20 * 700], [700] * 20, history=b[:3000])
    outs, done, by = rc.compress(ch)
    assert rc.decode(ch.history, by, ch.lens) == ch.data


def test_hand_built_cases_are_what_they_say(rc):
    """the reference's own output shows what each hand-built case is about (a mis-built case fails here)"""
    rng = random.Random(41)
    hand = {c.name: c for c in hand_chains(rng)}

    def first_seq(s):
        lit = s[0] >> 4
        p = 1
        if lit == 15:
            while True:
                lit += s[p]; p += 1
                if s[p - 1] != 255:
                    break
        p += lit
        return lit, s[p] | (s[p + 1] << 8)

    for rep in (1, 2, 3, 5, 20):   # no literals: the match was found behind the block's start and its catch-up stopped at the block's anchor
        for kind in ("prefix", "block"):
            outs, _, by = rc.compress(hand["repeat of the last %d history bytes (history = %s)" % (rep, kind)])
            assert first_seq(by[-1]) == (0, 1 if rep < 20 else 20), (rep, kind, first_seq(by[-1]))
    for shift in (1, 2):           # 20 literals, then the copy from its first byte: the catch-up went back off the grid
        outs, _, by = rc.compress(hand["copy off the grid by %d (history = prefix)" % shift])
        assert first_seq(by[-1]) == (20, 20 + 300 - (99 + shift)), (shift, first_seq(by[-1]))
    for D in (65535, 65536, 65537):   # the copy in the last block is found at 65535 and at no greater distance
        for cut in (0, 10):
            ch = hand["distance %d, boundary %d into the copy" % (D, cut)]
            outs, _, by = rc.compress(ch)
            assert (len(by[-1]) < ch.lens[-1] - 10) == (D == 65535), (D, cut, len(by[-1]), ch.lens[-1])


def test_prefix_table_is_dict_image_builds(sim):
    """the table a chain with a prefix starts with, entry by entry, against the image dict_image_build writes for the same bytes; the
    tables without a loaded prefix"""
    b = book1()
    rng = random.Random(42)
    for keep in (8, 9, 10, 11, 100, 191, 192, 193, 4096, 65535, 65536):
        tail = C.create_string_buffer(b[1000:1000 + keep], keep)
        img = C.create_string_buffer(32768)
        tab = (C.c_uint64 * 4096)()
        assert sim.sim_cchain_dict_image(tail, keep, img, rng.getrandbits(63) | 1) == 0
        assert sim.sim_cchain_table(tail, keep, 1, tab, rng.getrandbits(63) | 1) == 0
        assert list(tab) == list((C.c_uint64 * 4096).from_buffer_copy(img.raw)), keep
        assert sum(1 for e in tab if e) > 0
    four = C.create_string_buffer(b"abcd", 4)
    tab = (C.c_uint64 * 4096)()
    assert sim.sim_cchain_table(four, 0, 1, tab, 1) == 0 and set(tab) == {0}
    assert sim.sim_cchain_table(four, 0, 0, tab, 1) == 0
    fp = ((int.from_bytes(b"abcd", "little") * 2654435761) & 0xFFFFFFFF) >> 16
    assert set(tab) == {fp}


def check_all(sim, chains, want, per_call, rng, layouts=(0, 1)):
    bad = []
    for layout in layouts:
        for i in range(0, len(chains), per_call):
            pk = CPacked(chains[i:i + per_call])
            r, dst, out, cons = run(sim, pk, layout, rng.getrandbits(63) | 1)
            assert r != -1000, ("out-of-bounds access", layout, [c.name for c in pk.chains][:4])
            bad += [(layout,) + b for b in pk.check(dst, out, cons, want[i:i + per_call])]
    return bad


def test_whole_set(sim, cases):
    """every chain, both layouts, several chains per simulated wavefront (the table is left as it is between two chains): zero mismatches"""
    chains, want = cases
    bad = check_all(sim, chains, want, 7, random.Random(43))
    assert not bad, (len(bad), bad[:5])


def test_chain_order_does_not_matter(sim, cases):
    """a table carried from one chain into the next changes bytes: the small chains again in another order, all on one wavefront"""
    chains, want = cases
    idx = [i for i, c in enumerate(chains) if len(c.data) <= 3000]
    random.Random(44).shuffle(idx)
    idx = idx[:120]
    bad = check_all(sim, [chains[i] for i in idx], [want[i] for i in idx], len(idx), random.Random(45), layouts=(0,))
    assert not bad, (len(bad), bad[:5])


def test_prefix_array_null_is_zeros(sim, cases):
    chains, want = cases
    sel = [(c, w) for c, w in zip(chains, want) if not c.history][:40]
    pk = CPacked([c for c, _ in sel])
    r, dst, out, cons = run(sim, pk, 0, 7, prefix=False)
    assert r == 0 and not pk.check(dst, out, cons, [w for _, w in sel])


def test_untrusted_arrays(sim, rc):
    """the walk's handling of bad arrays: a range past n_blocks is cut, a negative prefix counts as 0, a prefix longer than the chain's
    offset is cut to it"""
    b = book1()
    ch = chain_of("bad", b[1000:1000 + 5 * 300], [300] * 5, history=b[900:1000])
    plain = CChain("plain", ch.blocks)
    pk = CPacked([ch])
    pk.prefix = [-5]
    r, dst, out, cons = run(sim, pk, 0, 3)
    assert r == 0 and not pk.check(dst, out, cons, [rc.compress(plain)])
    pk = CPacked([ch])
    off = pk.chain_src_off[0]
    pk.prefix = [off + 1000]          # cut to the offset: the guard and the history in front of the chain are its prefix
    r, dst, out, cons = run(sim, pk, 0, 3)
    assert r == 0 and not pk.check(dst, out, cons, [rc.compress(CChain("cut", ch.blocks, history=pk.src[:off]))])
    pk = CPacked([ch])
    pk.chain_first = [0, 9]           # five blocks exist
    r, dst, out, cons = run(sim, pk, 0, 3)
    pk.chain_first = [0, 5]
    assert r == 0 and not pk.check(dst, out, cons, [rc.compress(ch)])
    pk = CPacked([ch, plain])
    pk.chain_first = [0, 7, 3]        # the first chain takes seven blocks, the second range is empty once cut
    r, dst, out, cons = run(sim, pk, 0, 3)
    assert r == 0 and int(cons[1]) == 0 and list(out[7:]) == [12345] * 3


def test_span_limit(sim):
    """a block with which history, consumed bytes and src_len would exceed 0x7E000000 gives 0 without being looked at"""
    pk = CPacked([chain_of("x", book1()[:200], [100, 100])])
    pk.src_len = [100, 0x7E000000 - 99]
    r, dst, out, cons = run(sim, pk, 0, 3)
    assert r == 0 and out[0] > 0 and out[1] == 0 and int(cons[0]) == 100
