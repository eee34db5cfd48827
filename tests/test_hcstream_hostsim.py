"""The HC stream compressor for sources that land anywhere (LZ4_compress_HC_continue in both of its modes, LZ4_loadDictHC and
LZ4_saveDictHC) on the CPU: tests/hostsim/hostsim_hcstream.cpp compiles the state machine and the linear image of
lz4-java_amd/csrc/host_staging.h and the two cores of lz4_hc_core.h -- what hcstream_host_shard stages and what hc_build_stream_kernel and
hc_parse_stream_kernel run -- against the lock-step lane simulator.  Bytes, return values and the written-back state are the reference
library's own stream's on real arenas (tests/hcstream_common.py), every layout cut into calls at every block boundary, at random
boundaries and as few calls as the snapshot rule allows.  The simulator flags a wave access outside a block's view and slot."""
import ctypes as C
import random

import pytest

from cchain_common import book1, chain_of
from hcchain_common import RefHCChain
from hcstream_common import (MAXB, RefHCStream, case_set, clamp, compare, cut_into_calls, hand_scripts, is_jump_layout, layouts, levels_of, model_block,
                             model_load, model_save, run_cut, same_state, walk_offsets)
from support import build_sim


def load_sim():
    l = build_sim("hostsim_hcstream")
    l.sim_hcstream_call.restype = C.c_int
    l.sim_hcstream_call.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_uint32, C.c_uint64, C.c_void_p]
    l.sim_hcs_load_dict.restype = None
    l.sim_hcs_load_dict.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    l.sim_hcs_save_dict.restype = C.c_int
    l.sim_hcs_save_dict.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rr(ref):
    return RefHCStream(ref)


class SimEngine:
    """run_cut's three functions over the simulator"""

    def __init__(self, sim, level, rng, seg=4096):
        self.sim, self.level, self.rng, self.seg, self.oob, self.info = sim, level, rng, seg, 0, []

    def call(self, st, arena, blocks):
        nb = len(blocks)
        state = (C.c_uint64 * 5)(*st)
        offs = (C.c_uint64 * nb)(*[b[0] for b in blocks])
        lens = (C.c_int32 * nb)(*[b[1] for b in blocks])
        caps = (C.c_int32 * nb)(*[b[2] for b in blocks])
        doff, total = [], 0
        for b in blocks:
            doff.append(total + 16); total += max(b[2], 0) + 32
        dst = C.create_string_buffer(b"\x5A" * (total + 16), total + 16)
        out = (C.c_int32 * nb)()
        info = (C.c_uint64 * 3)()
        src = C.create_string_buffer(arena, len(arena))   # (exactly the arena: no byte behind it)
        rc = self.sim.sim_hcstream_call(state, src, offs, lens, nb, dst, (C.c_uint64 * nb)(*doff), caps, out, self.level, self.seg,
                                        self.rng.getrandbits(62) | 1, info)
        assert rc in (0, -1000), rc
        self.oob += rc == -1000
        self.info.append(tuple(info))
        raw = dst.raw
        bys = []
        for k, b in enumerate(blocks):
            r, cap = max(out[k], 0), max(b[2], 0)
            bys.append(raw[doff[k]:doff[k] + r])
            assert raw[doff[k] - 16:doff[k]] == b"\x5A" * 16 and raw[doff[k] + cap:doff[k] + cap + 16] == b"\x5A" * 16, "written outside the slot"
            assert r == 0 or raw[doff[k] + r:doff[k] + cap] == b"\x5A" * (cap - r), "written past the result"
        return list(out), bys, tuple(state)

    def load(self, end, n):
        st = (C.c_uint64 * 5)()
        self.sim.sim_hcs_load_dict(st, end, n)
        return tuple(st)

    def save(self, st, buf, k):
        s = (C.c_uint64 * 5)(*st)
        kept = self.sim.sim_hcs_save_dict(s, buf, k)
        return tuple(s), kept


def test_the_offsets_model_is_the_references_bookkeeping(rr):
    """fact 1 and fact 3 of the design against the reference alone: end, dictLimit, lowLimit and dictBase + dictLimit after EVERY step of
    every script are what the five-line model says -- rings that wrap with the overlap rule trimming the dictionary, double buffers,
    0-byte blocks, LZ4_loadDictHC, LZ4_saveDictHC with every k"""
    n = 0
    for sc in case_set(rr):
        for level in (1, 9):
            st = (0, 0, 0, 0, 0)
            for o, r in zip(sc.ops, rr.run(sc, level)):
                if o.kind == "L":
                    st = model_load(o.off, o.n)
                elif o.kind == "S":
                    st, kept = model_save(st, o.off, o.k)
                    assert kept == r[1], (sc.name, kept, r[1])
                else:
                    st = model_block(st, o.off, o.n)
                assert same_state(st, r[-1]), (sc.name, level, st, r[-1])
                n += 1
    assert n > 2000


def test_the_jump_layouts_jump(rr, ref):
    """conditions, not measurements: in every jump layout at least one block's reference bytes differ from the prefix-mode chain's over
    the same blocks, and at least one block carries a match whose offset exceeds its position in its run"""
    rc = RefHCChain(ref)   # the prefix-mode chain over the same blocks laid back to back
    n = 0
    for data_name, data, maxb in (("book1 4K", book1()[10000:], MAXB), ("book1 1K", book1()[300000:], 1024)):
        for sc in layouts(data_name, data, random.Random(5), tiny=False, maxb=maxb):
            if not is_jump_layout(sc):
                continue
            n += 1
            res = rr.run(sc, 9)
            blocks = sc.blocks()
            outs, by = rc.compress(chain_of("c", b"".join(o.data for o in blocks), [o.n for o in blocks]), 9)
            assert any(r[2] != x for r, x in zip(res, by)), sc.name
            assert walk_offsets(sc, res), sc.name
    assert n == 8


def check(sim, rr, sc, levels, rng, bad, left_out, hows=("each", "random", "one")):
    for level in levels:
        want = rr.run(sc, clamp(level))
        for how in hows:
            eng = SimEngine(sim, level, rng, seg=(4096, 65536, 1 << 20)[rng.randrange(3)])
            got = run_cut(sc, cut_into_calls(sc, how, rng), eng.call, eng.load, eng.save)
            assert eng.oob == 0, ("access outside the staged pieces or the slot", sc.name, level, how)
            compare(sc, want, got, level, bad, (how,), left_out)


def test_whole_set(sim, rr):
    """every script, every block, at the script's levels (all seven and the two clamps on the small ones, 9 and 10 on the large), cut three
    ways: value, bytes and the written-back state are the reference's, no access outside the staged pieces and the slots.  Levels 1..9
    leave nothing out.  Levels 10..12 leave out only blocks behind a jump on a stream older than 64 KB that differ (the header's stated
    exception: liblz4 reads stale chain entries of never-inserted positions there); they are named and counted"""
    rng = random.Random(78)
    bad, left_out = [], []
    scripts = case_set(rr)
    for sc in scripts:
        check(sim, rr, sc, levels_of(sc), rng, bad, left_out)
    assert not bad, (len(bad), bad[:6])
    assert all(clamp(x[1]) >= 10 for x in left_out)
    print("levels 10..12, left out: %d blocks" % len(left_out), sorted({x[0] for x in left_out}))
    assert len(left_out) == 0, (len(left_out), left_out[:6])   # (if one ever appears: pin the exact named set here)
    assert len(scripts) >= 150


def test_the_set_is_what_the_issue_asks_for(rr):
    names = " | ".join(s.name for s in case_set(rr))
    for must in ("contiguous", "two buffers, gap 100", "two buffers, gap 0", "ring %d" % (5 * MAXB + 100), "ring %d" % (65535 + 2 * MAXB),
                 "save area k=0", "save area k=3", "save area k=4", "save area k=100", "save area k=%d" % MAXB, "save area k=65536", "save area k=70000",
                 "elsewhere", "in front", "a 0-byte block at a jump", "a 13-byte block at a jump", "a run of 1 bytes", "a run of 7 bytes", "ext_len trimmed to 3",
                 "ext_len trimmed to 4", "ext_len trimmed to 5", "prefix 65534", "prefix 65535", "prefix 65536", "ends exactly at the external end",
                 "crosses the external end", "period 1 across", "period 2 across", "period 4 across", "exact caps", "result - 1", "bound - 1", "cap 0 at",
                 "cap -1 at", "src_len -1 at"):
        assert must in names, must
    # a block that returns 0 in mid-stream, and the stream goes on
    fails = goes_on = 0
    for sc in case_set(rr):
        outs = [r[1] for r in rr.run(sc, 9) if r[0] == "B"]
        if any(r == 0 for r in outs):
            fails += 1
            k = outs.index(0)
            goes_on += any(r > 0 for r in outs[k + 1:])
    assert fails >= 20 and goes_on >= 15, (fails, goes_on)
    # the overlap rule trims the dictionary to 3 (dropped), 4 and 5 bytes: the reference's own lowLimit says so
    for left, want in ((3, 0), (4, 4), (5, 5)):
        sc = next(s for s in case_set(rr) if s.name == "ext_len trimmed to %d" % left)
        assert rr.run(sc, 9)[1][3][3] == want, (left, rr.run(sc, 9)[1][3])


def test_hand_built_cases_reach_across_the_jump(rr):
    """the reference's own level 9 output holds what the hand-built cases are about: a match into the external piece"""
    n = 0
    for sc in hand_scripts(random.Random(77)):
        if any(k in sc.name for k in ("external end", "ext_len trimmed to 4", "ext_len trimmed to 5", "ext_len trimmed to 9", "across a jump", "with an external piece")):
            assert walk_offsets(sc, rr.run(sc, 9)), sc.name
            n += 1
    assert n >= 18


def test_shape_errors(sim):
    """the argument errors the staging arithmetic states: a history longer than its end offset, the life limit"""
    def call(st, lens):
        nb = len(lens)
        state = (C.c_uint64 * 5)(*st)
        src = C.create_string_buffer(64)
        z = (C.c_uint64 * nb)()
        out = (C.c_int32 * nb)()
        return sim.sim_hcstream_call(state, src, z, (C.c_int32 * nb)(*lens), nb, src, z, (C.c_int32 * nb)(), out, 9, 4096, 1, None)
    assert call((10, 11, 0, 0, 11), [0]) == -1
    assert call((10, 4, 5, 6, 4), [0]) == -1
    assert call((0, 0, 0, 0, (1 << 31) - 65536 - 5), [0, 6]) == -1
    assert call((0, 0, 0, 0, (1 << 31) - 65536 - 5), [0, -1, 0x7E000001]) == 0   # (blocks that cannot run consume nothing)
    assert call((0, 0, 0, 0, 0), [0]) == 0
