"""The resident-stream compressor (LZ4_compress_fast_continue on streams continued by any number of calls) on the CPU:
tests/hostsim/hostsim_cstream.cpp compiles cstream_walk of lz4-java_amd/csrc/lz4_fast_chain.h -- what compress_fast_stream_cu_kernel runs
-- against the lock-step lane simulator, with the streams' records and table images in host memory, and this file checks values and
bytes against ONE LZ4_stream_t of the reference library per stream (tests/cstream_common.py).  The simulator flags a read outside the
kept history and the call's source, a read at or past the end of the block that is running, a write outside the block's slot, and a
table load or store outside the stream's own image; the bytes around every chain and slot are guards."""
import ctypes as C
import random

import numpy as np
import pytest

from cstream_common import (CHAIN_STOPPED, FULL, Call, Engine, Life, PackedCall, RefCChain, RefStream, bound, case_set, chain_equals_stream, drive,
                            life_of, small_first_lives, truncation_lives)
from cchain_common import CPacked, book1
from support import build_sim
from test_cchain_hostsim import load_sim as load_chain_sim, run as run_chain


def load_sim():
    l = build_sim("hostsim_cstream")
    l.sim_cstream_batch.restype = C.c_int
    l.sim_cstream_batch.argtypes = [C.c_void_p] * 13 + [C.c_uint32, C.c_uint32, C.c_uint64]
    l.sim_cstream_rec_words.restype = C.c_uint32
    return l


class SimEngine(Engine):
    """n streams whose state is host memory; every call is one simulated wavefront that walks the call's chains in order"""

    def __init__(self, sim, n, seed=5):
        self.sim, self.n, self.rw = sim, n, sim.sim_cstream_rec_words()
        self.rec = np.zeros(n * self.rw, np.uint32)
        self.tables = np.full(n * 4096, 0x1111111111111111, np.uint64)   # (a fresh stream must not read its image)
        self.rng = random.Random(seed)
        self.oob = 0

    def call(self, ids, pk, force_stop=()):
        assert ids == sorted(set(ids)) and all(0 <= i < self.n for i in ids)
        slot = np.ascontiguousarray([i | (0x80000000 if i in force_stop else 0) for i in ids], dtype=np.uint32)
        ns, nd = len(pk.src), len(pk.dst)
        arena = C.create_string_buffer(ns + nd + 1)
        base = C.addressof(arena)
        C.memmove(base, pk.src, ns)
        C.memmove(base + ns, bytes(pk.dst), nd)
        cso, pre, sl, cf, do, dc = pk.arrays()
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        r = self.sim.sim_cstream_batch(slot.ctypes.data, self.rec.ctypes.data, self.tables.ctypes.data, base, cso.ctypes.data, pre.ctypes.data,
                                       sl.ctypes.data, cf.ctypes.data, base + ns, do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data,
                                       pk.n_blocks, pk.n_chains, self.rng.getrandbits(63) | 1)
        assert C.string_at(base, ns) == pk.src
        self.oob += r == -1000
        return C.string_at(base + ns, nd), out, cons

    def reset(self, ids):
        for i in ids:
            self.rec[i * self.rw:(i + 1) * self.rw] = 0

    def record(self, i):
        return [int(v) for v in self.rec[i * self.rw:(i + 1) * self.rw]]


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


@pytest.fixture(scope="module")
def lives(rc, O):
    return case_set(rc, random.Random(61), O)


def test_reference_conditions(rc):
    """what the rules rely on, by the reference itself: data left in place compresses as LZ4_saveDict of everything held does; a smaller
    saved size changes bytes; with nothing kept a block parses as a first block does; LZ4_saveDict keeps sizes under 8"""
    L = rc.L
    b = book1()
    sizes = [3000] * 30
    data = b[2000:2000 + sum(sizes)]
    # in place: one buffer, one stream, block after block
    buf = C.create_string_buffer(data, len(data))
    st = L.LZ4_createStream()
    inplace, o = [], 0
    for n in sizes:
        d = C.create_string_buffer(bound(n))
        r = L.LZ4_compress_fast_continue(st, C.addressof(buf) + o, d, n, bound(n), 1)
        inplace.append(d.raw[:r]); o += n
    L.LZ4_freeStream(st)
    life = life_of("saved", data, sizes, range(1, 30))
    s = RefStream(rc)
    saved = [s.run(c)[2][0] for c in life.calls]
    s.close()
    assert saved == inplace
    def second(prefix, fresh=False):
        s = RefStream(rc)
        first = Call([(data[:6000], bound(6000))])
        nxt = Call([(data[1000:5000], bound(4000))], prefix=prefix)
        if not fresh:
            s.run(first)
        r = s.run(nxt)[2][0]
        s.close()
        return r
    assert len({second(FULL), second(1000), second(0)}) == 3
    assert second(0) == second(0, fresh=True)      # (nothing kept: every stale entry is below the bound, and the block parses as a first one)
    # (sizes under 8 are kept as they are: LZ4_saveDict has no minimum, LZ4_loadDict's is its own)
    s = RefStream(rc)
    s.run(Call([(data[:100], bound(100))]))
    assert s.L.LZ4_saveDict(s.st, C.create_string_buffer(64), 3) == 3
    s.close()


def test_the_set_is_what_the_issue_asks_for(lives):
    assert len(lives) >= 350, len(lives)
    names = " | ".join(l.name for l in lives)
    for must in ("150 x up to 2000", "kept 65535 on a large stream", "kept 3 on a small stream", "kept 200000 on a dict stream", "small first [1] hist 0",
                 "fresh, 70000 loaded", "cap - 1 at block 0", "cap - 1 at block 5", "src_len -1 at block 3"):
        assert must in names, must
    assert max(len(l.calls) for l in lives) >= 100
    assert max(sum(len(c.data) for c in l.calls) for l in lives) > 140000


def test_whole_set(sim, rc, lives):
    """every life on a stream of its own, 40 streams per engine, half of the unfinished streams absent from every call, several streams
    per simulated wavefront: zero mismatches, no access outside the bounds; every stream whose history no call cuts equals the
    reference's one-call chain AND the simulator's existing chain walk on the same blocks"""
    rng = random.Random(62)
    chain_sim = load_chain_sim()
    bad, n_chain, stops = [], 0, 0
    for a in range(0, len(lives), 40):
        part = lives[a:a + 40]
        eng = SimEngine(sim, len(part) + 3)
        ids = sorted(rng.sample(range(len(part) + 3), len(part)))
        b, results, rounds = drive(eng, rc, part, rng, ids=ids)
        bad += b
        assert eng.oob == 0, ("out-of-bounds access", a)
        whole = [(lf, res) for lf, res in zip(part, results) if lf.untruncated()]
        for lf, res in whole:
            assert chain_equals_stream(rc, lf, res), lf.name
            stops += any(0 in c[0] for c in res)
        # the simulator's one-call chain on the same blocks
        want = [([r for c in res for r in c[0]], sum(c[1] for c in res), [x for c in res for x in c[2]]) for lf, res in whole]
        pk = CPacked([lf.as_chain() for lf, _ in whole])
        r, dst, out, cons = run_chain(chain_sim, pk, 0, 9)
        assert r == 0
        bad += [("one-call chain",) + x for x in pk.check(dst, out, cons, want)]
        n_chain += len(whole)
    assert not bad, (len(bad), bad[:5])
    assert n_chain >= 300 and stops >= 20, (n_chain, stops)


def test_every_stream_in_every_call(sim, rc, lives):
    """no stream ever absent, and all of a call's streams on one wavefront: a table carried from one stream into the next changes bytes"""
    sel = [l for l in lives if sum(len(c.data) for c in l.calls) <= 8000][:150]
    eng = SimEngine(sim, len(sel))
    bad, _, _ = drive(eng, rc, sel, random.Random(63), absent=0.0)
    assert eng.oob == 0 and not bad, (eng.oob, len(bad), bad[:5])


def test_truncated_histories_and_small_first_calls(sim, rc, O):
    """the two lists on their own, every stream in every call (the whole set has them too, among absent streams)"""
    rng = random.Random(64)
    sel = truncation_lives(rng, O) + small_first_lives(rng, O)
    eng = SimEngine(sim, len(sel))
    bad, results, _ = drive(eng, rc, sel, rng, absent=0.0)
    assert eng.oob == 0 and not bad, (eng.oob, len(bad), bad[:5])
    # the cut matters: the same stream with another kept size gives other bytes somewhere
    by = {lf.name: b"".join(x for c in res for x in c[2]) for lf, res in zip(sel, results)}
    assert len({by["kept %d on a small stream" % k] for k in (0, 8, 1000, 65536)}) >= 3


def test_stop_and_reset(sim, rc):
    """a stopped stream answers LZ4HIP_CHAIN_STOPPED in later calls and consumes nothing; a reset makes it fresh; the streams beside it
    are untouched; the forced stop (the host's mark of a failed call) stops a stream that has not failed"""
    b = book1()
    rng = random.Random(65)
    def blocks(o, n=4):
        return [(b[o + 1000 * i:o + 1000 * (i + 1)], bound(1000)) for i in range(n)]
    eng = SimEngine(sim, 3)
    ref = [RefStream(rc) for _ in range(3)]
    def both(ids, calls, force_stop=()):
        parts, want = [], []
        for i, c in zip(ids, calls):
            front, plen = ref[i].front(c)
            parts.append((front, plen, c)); want.append(ref[i].run(c))
        pk = PackedCall(parts, rng)
        dst, out, cons = eng.call(ids, pk, force_stop)
        return pk, dst, out, cons, want
    pk, dst, out, cons, want = both([0, 1, 2], [Call(blocks(0)), Call([(b[5000:6000], 10)] + blocks(6000, 2)), Call(blocks(9000))])
    assert not pk.check("abc", dst, out, cons, want) and list(out[4:7]) == [0, CHAIN_STOPPED, CHAIN_STOPPED]
    assert eng.record(1)[2] & 4 and not eng.record(0)[2] & 4
    pk, dst, out, cons, want = both([0, 1, 2], [Call(blocks(4000)), Call(blocks(7000)), Call(blocks(13000))])
    assert not pk.check("abc", dst, out, cons, want) and list(out[4:8]) == [CHAIN_STOPPED] * 4 and int(cons[1]) == 0
    eng.reset([1])
    ref[1].close(); ref[1] = RefStream(rc)
    pk, dst, out, cons, want = both([1, 2], [Call(blocks(7000)), Call(blocks(17000))])
    assert not pk.check("bc", dst, out, cons, want) and all(r > 0 for r in out[:8])
    assert eng.record(0)[4] == 8000 and eng.record(1)[4] == 4000 and eng.record(2)[4] == 12000
    # the forced stop
    last = Call(blocks(21000))
    front, plen = ref[2].front(last)
    pk = PackedCall([(b"", 0, Call(blocks(20000))), (front, plen, last)], rng)
    want2 = ref[2].run(last)
    dst, out, cons = eng.call([0, 2], pk, force_stop=(0,))
    assert list(out[:4]) == [CHAIN_STOPPED] * 4 and int(cons[0]) == 0 and eng.record(0)[2] & 4 and eng.record(0)[4] == 8000
    assert not pk.check("xc", dst, out, cons, [([CHAIN_STOPPED] * 4, 0, [b""] * 4), want2])
    assert eng.oob == 0
    for r in ref:
        r.close()


def test_index_limit_counts_the_streams_life(sim, rc):
    """loaded history + everything consumed + src_len above 0x7E000000 gives 0 and stops the stream, whatever the call holds"""
    b = book1()
    eng = SimEngine(sim, 1)
    rng = random.Random(66)
    c1 = Call([(b[:100], bound(100))])
    pk = PackedCall([(b[200:300], 100, c1)], rng)
    dst, out, cons = eng.call([0], pk)
    assert out[0] > 0 and eng.record(0)[3] == 200 and eng.record(0)[0] == 65536 + 100
    # (the source of the second block does not exist: it is refused before it is looked at)
    c2 = Call([(b[100:200], bound(100)), (b"", 0)], lens=[100, 0x7E000000 - 299])
    pk = PackedCall([(b[:100], 100, c2)], rng)
    dst, out, cons = eng.call([0], pk)
    assert out[0] > 0 and out[1] == 0 and int(cons[0]) == 100 and eng.record(0)[2] & 4 and eng.oob == 0
    eng.reset([0])
    c2 = Call([(b[100:200], bound(100)), (b"", 0)], lens=[100, 0x7E000000 - 100 + 1])
    pk = PackedCall([(b"", 0, c2)], rng)
    dst, out, cons = eng.call([0], pk)
    assert out[0] > 0 and out[1] == 0 and eng.oob == 0
