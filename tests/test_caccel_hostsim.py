"""The accelerated linked-block compressors on the CPU: tests/hostsim/hostsim_caccel.cpp compiles the three walks of
lz4-java_amd/csrc/lz4_fast_chain.h with their ACC switch on -- what compress_fast_chain_accel_cu_kernel, compress_fast_stream_accel_cu_kernel
and compress_fast_xstream_accel_cu_kernel run -- against the lock-step lane simulator, with the simulator's bounds checks on: nothing
read at or past a block's end, nothing read outside history and window, nothing written outside a slot.  Bytes, return values, consumed
sizes and, for streams, the record behind every call are the reference library's LZ4_compress_fast_continue on ONE LZ4_stream_t per
chain or stream at the same accelerations (tests/caccel_common.py).  A call at acceleration 1 runs the EXISTING walk on the same record
and image, as the C ABI does."""
import ctypes as C
import random

import numpy as np
import pytest

import cstream_common as S
import cxstream_common as X
from caccel_common import (ACCELS, CLAMPED, AccelPlan, RefAccelChain, RefAccelX, chain_cases, datasets, differing_share, drive_lives, overlapping_streams, tight_cases)
from cchain_common import CHAIN_STOPPED, CPacked, book1, bound, chain_of
from dstream_common import cut_pieces
from support import build_sim

PATTERNS = ((1, 8), (64, 2, 1))


def load_sim():
    l = build_sim("hostsim_caccel")
    l.sim_caccel_chain_batch.restype = C.c_int
    l.sim_caccel_chain_batch.argtypes = [C.c_void_p] * 10 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int]
    l.sim_caccel_stream_batch.restype = C.c_int
    l.sim_caccel_stream_batch.argtypes = [C.c_void_p] * 13 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int]
    l.sim_caccel_xstream_batch.restype = C.c_int
    l.sim_caccel_xstream_batch.argtypes = [C.c_void_p] * 14 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int]
    l.sim_caccel_rec_words.restype = C.c_uint32
    l.sim_caccel_clamp.restype = C.c_uint32
    l.sim_caccel_clamp.argtypes = [C.c_int]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rc(ref):
    return RefAccelChain(ref)


@pytest.fixture(scope="module")
def chains():
    return chain_cases()


@pytest.fixture(scope="module")
def want_at(rc, chains):
    """{acceleration: [(out_len, consumed, bytes)] per chain} from the reference, 1 included"""
    return {a: [rc.at(a).compress(c) for c in chains] for a in (1,) + ACCELS}


def run_chains(sim, pk, accel, seed=9):
    ns, nd = len(pk.src), len(pk.dst)
    arena = C.create_string_buffer(ns + nd + 1)
    base = C.addressof(arena)
    C.memmove(base, pk.src, ns)
    C.memmove(base + ns, bytes(pk.dst), nd)
    a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
    cso, pre, sl, cf = a64(pk.chain_src_off), a32(pk.prefix), a32(pk.src_len), a32(pk.chain_first, np.uint32)
    do, dc = a64(pk.dst_off), a32(pk.dst_cap)
    out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
    r = sim.sim_caccel_chain_batch(base, cso.ctypes.data, pre.ctypes.data, sl.ctypes.data, cf.ctypes.data, base + ns, do.ctypes.data, dc.ctypes.data,
                                   out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains, seed, accel)
    assert C.string_at(base, ns) == pk.src
    return r, C.string_at(base + ns, nd), out, cons


class SimStreams(S.Engine):
    """n streams whose state is host memory; a call runs at plan.now -- acceleration 1 through the existing walks"""

    def __init__(self, sim, n, plan, seed=5):
        self.sim, self.n, self.rw, self.plan = sim, n, sim.sim_caccel_rec_words(), plan
        self.rec = np.zeros(n * self.rw, np.uint32)
        self.tables = np.full(n * 4096, 0x1111111111111111, np.uint64)   # (a fresh stream must not read its image)
        self.rng = random.Random(seed)
        self.oob = 0

    def _arena(self, pk):
        ns, nd = len(pk.src), len(pk.dst)
        arena = C.create_string_buffer(ns + nd + 1)
        base = C.addressof(arena)
        C.memmove(base, pk.src, ns)
        C.memmove(base + ns, bytes(pk.dst), nd)
        return arena, base, ns, nd

    def call(self, ids, pk):
        assert ids == sorted(set(ids)) and all(0 <= i < self.n for i in ids)
        slot = np.ascontiguousarray(ids, dtype=np.uint32)
        arena, base, ns, nd = self._arena(pk)
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        if isinstance(pk, X.PackedX):
            so, sl, cf, he, hl, wo, wl, do, dc = pk.arrays()
            r = self.sim.sim_caccel_xstream_batch(slot.ctypes.data, self.rec.ctypes.data, self.tables.ctypes.data, base, so.ctypes.data, sl.ctypes.data,
                                                  cf.ctypes.data, he.ctypes.data, hl.ctypes.data, base + ns, do.ctypes.data, dc.ctypes.data, out.ctypes.data,
                                                  cons.ctypes.data, pk.n_blocks, pk.n_chains, self.rng.getrandbits(63) | 1, self.plan.now)
        else:
            cso, pre, sl, cf, do, dc = pk.arrays()
            r = self.sim.sim_caccel_stream_batch(slot.ctypes.data, self.rec.ctypes.data, self.tables.ctypes.data, base, cso.ctypes.data, pre.ctypes.data,
                                                 sl.ctypes.data, cf.ctypes.data, base + ns, do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data,
                                                 pk.n_blocks, pk.n_chains, self.rng.getrandbits(63) | 1, self.plan.now)
        assert C.string_at(base, ns) == pk.src
        self.oob += r == -1000
        self.plan.step()
        return C.string_at(base + ns, nd), out, cons

    def reset(self, ids):
        for i in ids:
            self.rec[i * self.rw:(i + 1) * self.rw] = 0

    def record(self, i):
        return [int(v) for v in self.rec[i * self.rw:(i + 1) * self.rw]]

    def state_is(self, i, state):
        r = self.record(i)
        return (r[0], r[1]) == tuple(state)


# ---- the reference's own conditions ----
def test_the_knob_changes_the_reference(chains, want_at):
    """A walk that ignores its acceleration must fail: over the book1 chains, blocks of 1000 bytes and more, at every acceleration of
    the list at least 90 % of the blocks have reference bytes that differ from the reference's acceleration-1 bytes of the same block of
    the same chain.  Both sides are the reference's; random and zero data are not counted."""
    for a in ACCELS:
        differ, total = differing_share(want_at[a], want_at[1], chains)
        print("acceleration %d: %d of %d book1 blocks of 1000 bytes and more differ from acceleration 1" % (a, differ, total))
        assert total >= 150 and 10 * differ >= 9 * total, (a, differ, total)
    sizes = [sum(r for r in outs if r > 0) for outs, _, _ in (want_at[a][[c.name for c in chains].index("book1 64 x 1000")] for a in (1,) + ACCELS)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes      # (a higher acceleration finds less)


def test_the_reference_clamps(rc, chains):
    ch = [c for c in chains if c.name == "book1 16 x 4096"][0]
    for raw, eff in CLAMPED:
        assert rc.at(raw).compress(ch) == rc.at(eff).compress(ch), (raw, eff)
    assert rc.at(1).compress(ch) != rc.at(65537).compress(ch)


def test_alternating_accelerations_leave_their_table(rc):
    """the table a call leaves depends on its acceleration, and a later call sees that: most blocks of a stream driven at 1, 8, 1, 8, ...
    differ from the all-1 stream's (even blocks) and the all-8 stream's (odd blocks)"""
    data = book1()[:65536]
    life = S.life_of("alternating", data, [4096] * 16, range(1, 16))

    def run(pattern):
        plan = rc.plan
        plan.pattern, plan.k = pattern, 0
        s, by = S.RefStream(rc), []
        for c in life.calls:
            by.append(s.run(c)[2][0])
            plan.k += 1
        s.close()
        return by
    mixed, ones, eights = run((1, 8)), run((1,)), run((8,))
    assert sum(mixed[k] != ones[k] for k in range(0, 16, 2)) >= 6 and sum(mixed[k] != eights[k] for k in range(1, 16, 2)) >= 6


# ---- chains ----
@pytest.mark.parametrize("accel", ACCELS)
def test_chains(sim, rc, chains, want_at, accel):
    """every chain of the set at the bound, and one byte short of the reference's result on a middle block (the chain stops): bytes,
    return values, consumed sizes, the guards; no access outside the bounds"""
    tight = tight_cases(rc, [c for c in chains if len(c.data) <= 70000 and len(c.blocks) > 1], accel)
    want_tight = [rc.at(accel).compress(c) for c in tight]
    assert sum(1 for outs, _, _ in want_tight if 0 in outs and CHAIN_STOPPED in outs) >= 20
    names = " | ".join(c.name for c in chains)
    for must in ("book1 13..20", "geo small between", "pic 16 x 4096", "zeros 1 x 65536", "random 64 x 1000", "book1 200000 in 4 KiB blocks", "book1 prefix 7,",
                 "book1 prefix 8,", "book1 prefix 4096,", "book1 prefix 65536,", "book1 prefix 70000,"):
        assert must in names, must
    for part, want in ((chains, want_at[accel]), (tight, want_tight)):
        pk = CPacked(part)
        r, dst, out, cons = run_chains(sim, pk, accel)
        assert r == 0, "out-of-bounds access"
        bad = pk.check(dst, out, cons, want)
        assert not bad, (accel, len(bad), bad[:5])


@pytest.mark.parametrize("raw,eff", CLAMPED)
def test_clamps(sim, rc, chains, want_at, raw, eff):
    """acceleration 0 and -7 are 1, 70000 and 1 << 30 are 65537: the simulator's entry clamps as the C ABI's does, and the bytes are the
    reference's for the raw value"""
    assert sim.sim_caccel_clamp(raw) == eff
    part = [c for c in chains if c.name in ("book1 16 x 4096", "geo 16 x 1000", "book1 prefix 4096, 6 x 1000")]
    want = [rc.at(raw).compress(c) for c in part]
    assert want == [want_at[eff][chains.index(c)] for c in part]
    pk = CPacked(part)
    r, dst, out, cons = run_chains(sim, pk, raw)
    assert r == 0 and not pk.check(dst, out, cons, want)


# ---- resident streams ----
def stream_lives(rc, rng, O):
    """cut at every block boundary and at random ones; kept histories cut as LZ4_saveDict does; loaded prefixes; stops"""
    b = book1()
    d = datasets()
    lives = []
    for i in range(40):
        nb = rng.choice([2, 3, 5, 8, 20])
        hist = b""
        if i % 5 == 0:
            P = rng.choice([7, 8, 500, 65536, 70000])
            o = rng.randrange(70000, 150000)
            hist = b[o - P:o]
        lives.append(S.random_life(rng, O, "random %d" % i, nb, 6000, hist, every_boundary=(i % 2 == 0)))
    lives.append(S.life_of("book1 40 x 4096", b[5000:5000 + 40 * 4096], [4096] * 40, range(3, 40, 3)))
    lives.append(S.life_of("book1 20 x 4096 every", b[:20 * 4096], [4096] * 20, range(1, 20)))
    lives.append(S.life_of("book1 64 x 1000 every", b[9000:73000], [1000] * 64, range(1, 64)))
    for name in ("geo", "pic", "zeros", "random"):
        lives.append(S.life_of(name + " 16 x 4096", d[name], [4096] * 16, range(1, 16)))
        lives.append(S.life_of(name + " 13..20 and small", d[name][:sum(range(1, 21))], list(range(1, 21)), range(2, 20, 3)))
    lives.append(S.life_of("book1 2 x 65536", b[:131072], [65536] * 2, (1,)))
    return lives + S.prefix_lives(rng, O) + S.truncation_lives(rng, O)[::2] + S.small_first_lives(rng, O)[::3]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_resident_streams(sim, rc, O, pattern):
    """every life on a stream of its own, the acceleration changing from call to call, calls at 1 through the existing walk on the same
    record and image: zero mismatches, the record behind every call is the reference stream's, no access outside the bounds"""
    rng = random.Random(81 + len(pattern))
    lives = stream_lives(rc, rng, O)
    bad = []
    for a in range(0, len(lives), 40):
        part = lives[a:a + 40]
        plan = rc.plan
        plan.pattern, plan.k, plan.used = pattern, a, []
        eng = SimStreams(sim, len(part) + 3, plan)
        ids = sorted(rng.sample(range(len(part) + 3), len(part)))
        b, results, rounds = drive_lives(eng, rc, part, rng, ids=ids, absent=0.4)
        assert eng.oob == 0, ("out-of-bounds access", a)
        assert set(plan.used) == set(pattern)
        bad += b
    assert not bad, (len(bad), bad[:5])


def test_stop_and_reset(sim, rc):
    """a capacity one byte short of the reference's result at acceleration 8 stops the stream; later calls, at any acceleration and
    through either walk, answer LZ4HIP_CHAIN_STOPPED; a reset makes it fresh"""
    b = book1()
    rng = random.Random(83)
    plan = rc.plan
    plan.pattern, plan.k = (8,), 0
    probe = S.RefStream(rc)
    exact = probe.run(S.Call([(b[:1000], bound(1000)), (b[1000:2000], bound(1000))]))[0]
    probe.close()
    life = S.Life("tight", [S.Call([(b[:1000], bound(1000)), (b[1000:2000], exact[1] - 1), (b[2000:3000], bound(1000))]),
                            S.Call([(b[3000:4000], bound(1000))]), S.Call([(b[4000:5000], bound(1000))])])
    other = S.life_of("beside it", b[7000:13000], [1000] * 6, (2, 4))
    plan.pattern, plan.k = (8, 1, 3), 0
    eng = SimStreams(sim, 2, plan)
    bad, results, _ = drive_lives(eng, rc, [life, other], rng, absent=0.0)
    assert not bad and eng.oob == 0, bad
    assert [r for c in results[0] for r in c[0]] == [exact[0], 0, CHAIN_STOPPED, CHAIN_STOPPED, CHAIN_STOPPED]
    assert eng.record(0)[2] & 4 and eng.record(0)[4] == 1000 and not eng.record(1)[2] & 4 and eng.record(1)[4] == 6000
    eng.reset([0])
    again = S.life_of("after the reset", b[:6000], [1000] * 6, (1, 3))
    plan.pattern, plan.k = (64, 2, 1), 0
    bad, results, _ = drive_lives(eng, rc, [again], rng, absent=0.0)
    assert not bad and eng.oob == 0 and all(r > 0 for c in results[0] for r in c[0])


# ---- streams whose sources land anywhere ----
EXT_LAYOUTS = ("contig", "two4096", "save", "ring73727", "dict4096", "dict70000", "overwritten")


@pytest.fixture(scope="module")
def ext_streams():
    rng = random.Random(91)
    data = book1()
    out = {lay: [X.make_xstream(lay, rng, data, "#%d" % t) for t in range(8)] for lay in EXT_LAYOUTS if lay != "overwritten"}
    out["overwritten"] = overlapping_streams(rng, 40)
    geo = datasets()["geo"]
    out["two4096"] += [X.make_xstream("two4096", rng, geo, "geo #%d" % t, n_blocks=12) for t in range(3)]
    return out


@pytest.mark.parametrize("mode", ["every", "random", "none"])
@pytest.mark.parametrize("layout", EXT_LAYOUTS)
def test_ext_streams(sim, ref, ext_streams, layout, mode):
    """back to back, two alternating buffers, the save area, the ring of 65535 + 2 x 4096 bytes that wraps, a dictionary elsewhere, a
    source written over its own history: each cut into calls three ways, the accelerations and the two walks alternating on one record.
    Bytes, values, consumed sizes and the record behind every call"""
    streams = ext_streams[layout]
    k = EXT_LAYOUTS.index(layout) * 3 + ("every", "random", "none").index(mode)
    pattern = PATTERNS[k & 1] if mode != "none" else (3, 1, 64)
    plan = AccelPlan(pattern)
    plan.k = k
    rs = RefAccelX(ref, plan)
    rng = random.Random(2000 + k)
    eng = SimStreams(sim, len(streams) + 2, plan)
    ids = sorted(rng.sample(range(len(streams) + 2), len(streams)))
    bad, made, rounds = X.drive_x(eng, rs, streams, rng, mode=mode, ids=ids, check_state=eng.state_is)
    assert eng.oob == 0, "out-of-bounds access"
    assert not bad, (len(bad), bad[:5])
    assert len(set(plan.used)) >= 2 or rounds < 2, plan.used
    if layout == "ring73727":
        assert all(any(b.off == 0 for b in xs.blocks[1:]) for xs in streams)


def test_prefix_and_ext_walks_alternate(sim, ref):
    """the resident-stream walk (the source follows its history) and the walk for sources that land anywhere alternate on one record, each
    at changing accelerations: the bytes are ONE LZ4_stream_t's"""
    data = book1()
    rng = random.Random(93)
    for trial in range(6):
        plan = AccelPlan((8, 1, 64, 2))
        rs = RefAccelX(ref, plan)
        pieces = cut_pieces(data, rng, 16, 0, 3000)
        offs, pos = [], 0
        for k, p in enumerate(pieces):     # contiguous, but every fourth block jumps to a place of its own further up
            if k and k % 4 == 0:
                pos += 5000
            offs.append(pos); pos += len(p)
        xs = X.XStream("alternating %d" % trial, "contig", pos + 16, [X.XBlock(o, p) for o, p in zip(offs, pieces)])
        r = X.RefX(rs, xs)
        eng = SimStreams(sim, 1, plan)
        for k in range(len(pieces)):
            c = r.next_call(k + 1)
            jump = k and k % 4 == 0
            if jump or (k % 2 == 0 and k % 4 != 1):
                pk = X.PackedX([c], rng)
                dst, out, cons = eng.call([0], pk)
                assert not pk.check([xs.name], dst, out, cons), (trial, k)
            else:
                s = r.win_off + offs[k]
                cap = bound(len(pieces[k]))
                call = S.Call([(pieces[k], cap)])
                pk = S.PackedCall([(c.arena[s - c.hist_len:s], c.hist_len, call)], rng)
                dst, out, cons = eng.call([0], pk)
                assert c.hist_end in (s, 0) and not pk.check([xs.name], dst, out, cons, [(c.outs, c.consumed, c.by)]), (trial, k)
            assert eng.state_is(0, c.state), (trial, k, eng.record(0), c.state)
        assert eng.oob == 0
        r.close()
