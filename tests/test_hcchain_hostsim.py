"""The HC linked-block compressor (LZ4_compress_HC_continue over chains, prefix mode) on the CPU: tests/hostsim/hostsim_hcchain.cpp
compiles hc_chain_build_segment (HcBuild<..., false, SEG = true>) and hc_chain_parse_block (HcParse<..., false, false, PREFIX = true>)
of lz4-java_amd/csrc/lz4_hc_core.h -- what hc_build_chain_kernel and hc_parse_chain_kernel run -- against the lock-step lane simulator.
The segment build is checked entry by entry against a replay of liblz4's inserts over the whole buffer; the parse is checked, value
and bytes, against the reference library on the shared set (tests/hcchain_common.py).  The simulator flags a wave access outside the
block's buffer (its kept history and itself) and outside its slot.  One test states, against the reference alone, the two facts the
design stands on."""
import ctypes as C
import random

import numpy as np
import pytest

from cchain_common import GUARD, book1, bound, chain_of
from hcchain_common import RefHCChain, case_set, clamp, hc_hand_chains, levels_of, parse, pattern_chains, source_of
from support import build_sim


def load_sim():
    l = build_sim("hostsim_hcchain")
    l.sim_hc_chain_build.restype = C.c_int
    l.sim_hc_chain_build.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_uint64]
    l.sim_hc_chain_block.restype = C.c_int
    l.sim_hc_chain_block.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rc(ref):
    return RefHCChain(ref)


def replay(buf):
    """liblz4's inserts over the whole buffer as ONE run of positions 0 .. len - 4 (LZ4HC_Insert: index 65536 + q, hash of the 4 bytes
    at q): delta[q] = distance to the previous position of the same hash, 0 where there is none within 65535"""
    n = len(buf) - 3
    if n <= 0:
        return np.zeros(0, np.uint16)
    a = np.frombuffer(buf, np.uint8).astype(np.uint32)
    h = ((a[:n] | (a[1:n + 1] << 8) | (a[2:n + 2] << 16) | (a[3:n + 3] << 24)) * np.uint32(2654435761)) >> np.uint32(17)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    prev = np.full(n, -(1 << 40), np.int64)
    same = np.nonzero(hs[1:] == hs[:-1])[0] + 1
    prev[order[same]] = order[same - 1]
    d = np.arange(n, dtype=np.int64) - prev
    return np.where(d <= 65535, d, 0).astype(np.uint16)


def kept(ch):
    """the chain's buffer: the history LZ4_loadDictHC keeps, then the source"""
    return ch.history[-65536:] + source_of(ch) if ch.history else source_of(ch)


class Built:
    """a chain's buffer in guarded memory and its delta[] from the simulator's segment build"""

    def __init__(self, sim, ch, seg, seed, order=0):
        self.data = kept(ch)
        n = len(self.data)
        self.mem = C.create_string_buffer(b"\xA5" * GUARD + self.data + b"\xA5" * GUARD, n + 2 * GUARD)
        self.base = C.addressof(self.mem) + GUARD
        self.delta = np.full(n + 8, 0xFFFF, np.uint16)
        assert sim.sim_hc_chain_build(self.base, n, seg, self.delta.ctypes.data, order, seed) == 0, ("out-of-bounds read in the build", ch.name)


def test_segment_build_is_liblz4s_inserts(sim):
    """delta[], entry by entry, for S = 4096, 65536 and one segment, the segments in either order, several lane orders of the LDS atomic:
    cuts inside blocks, on block boundaries and less than 64 KB from the buffer's start; the last three positions have no entry"""
    b = book1()
    rng = random.Random(61)
    bufs = [b[:300000], (b"ab" * 700 + rng.randbytes(5) + bytes(9000) + b[1000:3000]) * 12, bytes(150000), b[5000:5000 + 4096 * 3], b[:4099], b[:4100],
            b[:65536 + 4], rng.randbytes(70001), b[:3], b[:4], b[:5], b""]
    for buf in bufs:
        want = replay(buf)
        for seg in (4096, 65536, 1 << 30):
            if len(buf) > 100000 and seg == 4096 and buf is not bufs[0]:
                continue
            for order in (0, 1):
                ch = chain_of("b", buf, [len(buf)])
                bt = Built(sim, ch, seg, rng.getrandbits(63) | 1, order)
                got = bt.delta[:len(want)]
                assert np.array_equal(got, want), (len(buf), seg, order, np.nonzero(got != want)[0][:5])
                assert (bt.delta[len(want):] == 0xFFFF).all(), (len(buf), seg)
    assert np.count_nonzero(replay(b[:300000])) > 200000


def test_facts_1_and_2(rc):
    """The design's foundation, against the reference alone.  Fact 1: block k of a running stream is, byte for byte, what a fresh stream
    gives that has loaded (LZ4_loadDictHC) what lies in front of the block -- of which it keeps the last 64 KB.  Fact 2: a block that
    fails (capacity too small: 0) changes nothing for the blocks behind it."""
    b = book1()
    rng = random.Random(62)
    runs = (b"abc" * 50 + b"\0" * 300 + b"xyxy" * 90 + rng.randbytes(40)) * 700
    datas = (b[:300000], runs[:300000], bytes(300000))
    n = 0
    for data in datas:
        for bs, count in ((1000, 300), (4096, 60), (65536, 4), (70001, 4)):
            for P in (0, 3, 5000, 70000):
                for level in ((1, 9, 10) if bs != 1000 else (3, 4, 12)):
                    size = min(bs * count, len(data) - P) // bs * bs
                    ch = chain_of("f", data[P:P + size], [bs] * (size // bs), history=data[:P])
                    run, by = rc.compress(ch, level)
                    assert all(r > 0 for r in run)
                    assert (run, by) == rc.compress(ch, level, fresh=True), ("fact 1", len(data), bs, P, level)
                    m = len(ch.blocks) // 2
                    fail = ch.with_caps(lambda i, c: run[i] - 1 if i in (0, m) else c, "fail")
                    r2, by2 = rc.compress(fail, level)
                    assert r2[0] == 0 and r2[m] == 0, ("fact 2", bs, P, level)
                    assert [x for i, x in enumerate(zip(r2, by2)) if i not in (0, m)] == [x for i, x in enumerate(zip(run, by)) if i not in (0, m)], \
                        ("fact 2", len(data), bs, P, level)
                    n += 1
    assert n >= 100


def test_hand_built_cases_are_what_they_say(rc):
    """the reference's own level 9 output of the last block holds the sequence each hand-built case is about"""
    for ch, chk in hc_hand_chains(random.Random(51)):
        outs, by = rc.compress(ch, 9)
        assert all(r > 0 for r in outs), ch.name
        if chk:
            try:
                chk(parse(by[-1]))
            except AssertionError as e:
                raise AssertionError("hand-built case %r: %s" % (ch.name, e))


def test_the_set_is_what_the_issue_asks_for(rc):
    chains = case_set(rc)
    names = " | ".join(c.name for c in chains)
    for must in ("book1 70 x 1000", "book1 17 x 4096", "book1 3 x 65536", "book1 mixed", "distance 65535", "distance 65537", "the last 3 bytes",
                 "the last 5 bytes", "widened backwards", "pattern 199", "zeros 300000", "exact caps", "cap - 1 at", "cap 0 at", "cap -1 at", "src_len -1 at"):
        assert must in names, must
    assert len(chains) >= 400
    assert sum(1 for c in pattern_chains() if len(c.history) > 65536) == 40
    fails = goes_on = 0
    for c in chains:
        outs = rc.compress(c, 9)[0]
        if 0 in outs:
            fails += 1
            goes_on += any(r > 0 for r in outs[outs.index(0) + 1:])
    assert fails >= 40 and goes_on >= 30, (fails, goes_on)


def check_chain(sim, rc, ch, levels, rng, seg, bad):
    bt = Built(sim, ch, seg, rng.getrandbits(63) | 1)
    keep = min(len(ch.history), 65536)
    for level in levels:
        outs, by = rc.compress(ch, clamp(level))
        pos = keep
        for k, ((s, cap), sl) in enumerate(zip(ch.blocks, ch.lens)):
            out = C.create_string_buffer(b"\x5A" * (max(cap, 0) + 16), max(cap, 0) + 16)
            r = sim.sim_hc_chain_block(bt.base, pos, sl, bt.delta.ctypes.data, out, cap, level, rng.getrandbits(63) | 1)
            assert r != -1000, ("out-of-bounds access", ch.name, level, k)
            if r != outs[k] or out.raw[:max(r, 0)] != by[k]:
                bad.append((ch.name, level, k, r, outs[k]))
                break
            if out.raw[max(cap, 0):] != b"\x5A" * 16 or (r > 0 and out.raw[r:cap] != b"\x5A" * (cap - r)):
                bad.append((ch.name, level, k, "written past the result"))
                break
            pos += max(sl, 0)


def test_whole_set(sim, rc):
    """every chain of the set, every block, at the chain's levels (all seven and the two clamps up to 20 000 bytes, 9 and 10 above):
    value and bytes are the reference's, zero mismatches, no access outside the block's buffer and slot.  delta[] comes from the
    segment build, S by turns 4096, 65536 and 1 MiB"""
    rng = random.Random(63)
    bad = []
    for i, ch in enumerate(case_set(rc)):
        check_chain(sim, rc, ch, levels_of(ch), rng, (4096, 65536, 1 << 20)[i % 3], bad)
    assert not bad, (len(bad), bad[:5])


def test_untouched_delta_is_never_read_past_the_block(sim, rc):
    """a block's parse reads no entry of a later block's positions: the same results with every entry at and behind the block's end
    overwritten"""
    b = book1()
    ch = chain_of("t", b[7000:7000 + 6 * 1500], [1500] * 6, history=b[6000:7000])
    bt = Built(sim, ch, 4096, 5)
    for level in (9, 10):
        outs, by = rc.compress(ch, level)
        pos = 1000
        for k in range(6):
            d = bt.delta.copy()
            d[pos + 1500:] = 1
            out = C.create_string_buffer(bound(1500))
            r = sim.sim_hc_chain_block(bt.base, pos, 1500, d.ctypes.data, out, bound(1500), level, 9)
            assert (r, out.raw[:r]) == (outs[k], by[k]), (level, k)
            pos += 1500
