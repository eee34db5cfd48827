"""The resident-stream compressor for sources that land anywhere, on the CPU: tests/hostsim/hostsim_cxstream.cpp compiles cxstream_walk
of lz4-java_amd/csrc/lz4_fast_chain.h and the LINK + DICT form of FastCore -- what compress_fast_xstream_cu_kernel runs -- against the
lock-step lane simulator, with the streams' records and table images in host memory.  Values, bytes and, behind every call, the stream's
index position and held history are compared with ONE LZ4_stream_t of the reference library per stream (tests/cxstream_common.py).  The
simulator flags a read outside the block's source and the history it can reach (one span when the two lie apart: the dictionaries lie
on either side of the window), a write outside the block's slot, and a table load or store outside the stream's own image."""
import ctypes as C
import random

import numpy as np
import pytest

from cchain_common import CHAIN_STOPPED, bound
from cxstream_common import (JUMP_LAYOUTS, LAYOUTS, OFF_CUR, OFF_DSIZE, PackedX, RefX, XBlock, XStream, book1, capacity_case, drive_x, hand_built, jump_share,
                             make_xstream, placed, prefix_chain_bytes)
from dstream_common import RefStream, cut_pieces, ring_place
from support import build_sim

PER_LAYOUT = 30


def load_sim():
    l = build_sim("hostsim_cxstream")
    l.sim_cxstream_batch.restype = C.c_int
    l.sim_cxstream_batch.argtypes = [C.c_void_p] * 14 + [C.c_uint32, C.c_uint32, C.c_uint64]
    l.sim_cxstream_prefix_batch.restype = C.c_int
    l.sim_cxstream_prefix_batch.argtypes = [C.c_void_p] * 13 + [C.c_uint32, C.c_uint32, C.c_uint64]
    l.sim_cxstream_rec_words.restype = C.c_uint32
    return l


class SimX:
    """n streams whose state is host memory; every call is one simulated wavefront that walks the call's chains in order"""

    def __init__(self, sim, n, seed=5):
        self.sim, self.n, self.rw = sim, n, sim.sim_cxstream_rec_words()
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
        so, sl, cf, he, hl, wo, wl, do, dc = pk.arrays()
        # (what the C call refuses: every source inside its window)
        for t in range(pk.n_chains):
            for i in range(pk.first[t], pk.first[t + 1]):
                assert pk.win_off[t] <= pk.src_off[i] and pk.src_off[i] + max(pk.src_len[i], 0) <= pk.win_off[t] + pk.win_len[t]
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        r = self.sim.sim_cxstream_batch(slot.ctypes.data, self.rec.ctypes.data, self.tables.ctypes.data, base, so.ctypes.data, sl.ctypes.data, cf.ctypes.data,
                                        he.ctypes.data, hl.ctypes.data, base + ns, do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data,
                                        pk.n_blocks, pk.n_chains, self.rng.getrandbits(63) | 1)
        assert C.string_at(base, ns) == pk.src
        self.oob += r == -1000
        return C.string_at(base + ns, nd), out, cons

    def call_prefix(self, ids, src, chain_src_off, prefix, src_len, first, dst_len, dst_off, dst_cap):
        """the existing walk (cstream_walk) on the same records: -> (dst, out, consumed)"""
        slot = np.ascontiguousarray(ids, dtype=np.uint32)
        arena = C.create_string_buffer(len(src) + dst_len + 1)
        base = C.addressof(arena)
        C.memmove(base, src, len(src))
        a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
        cso, pre, sl, cf, do, dc = a64(chain_src_off), a32(prefix), a32(src_len), a32(first, np.uint32), a64(dst_off), a32(dst_cap)
        out, cons = np.full(max(len(src_len), 1), 12345, np.int32), np.full(max(len(ids), 1), 12345, np.uint64)
        r = self.sim.sim_cxstream_prefix_batch(slot.ctypes.data, self.rec.ctypes.data, self.tables.ctypes.data, base, cso.ctypes.data, pre.ctypes.data,
                                               sl.ctypes.data, cf.ctypes.data, base + len(src), do.ctypes.data, dc.ctypes.data, out.ctypes.data,
                                               cons.ctypes.data, len(src_len), len(ids), self.rng.getrandbits(63) | 1)
        self.oob += r == -1000
        return C.string_at(base + len(src), dst_len), out, cons

    def reset(self, ids):
        for i in ids:
            self.rec[i * self.rw:(i + 1) * self.rw] = 0

    def record(self, i):
        return [int(v) for v in self.rec[i * self.rw:(i + 1) * self.rw]]

    def state_is(self, i, state):
        r = self.record(i)
        return (r[0], r[1]) == tuple(state)


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


@pytest.fixture(scope="module")
def layout_streams():
    rng = random.Random(71)
    data = book1()
    return {lay: [make_xstream(lay, rng, data, "#%d" % t) for t in range(PER_LAYOUT)] for lay in LAYOUTS}


def test_reference_fields(rs):
    """the three fields of LZ4_stream_t_internal this file reads back are where 1.9.3 has them"""
    b = book1()
    xs = XStream("probe", "contig", 4096, [XBlock(0, b[:1000]), XBlock(2000, b[1000:1500])], dictionary=b[5000:5100])
    r = RefX(rs, xs)
    assert r.fields() == (65536, r.dict_end, 100)
    c = r.next_call(1)
    assert c.state == (65536 + 1000, 1000) and r.fields()[1] == r.win_off + 1000     # (the dictionary lay elsewhere: the block alone is held)
    c = r.next_call(2)
    assert c.state == (65536 + 1500, 500) and r.fields()[1] == r.win_off + 2500
    r.close()


def test_writer_of_the_decoder_tests_agrees(rs):
    """dstream_common.RefStream.write drives ONE LZ4_stream_t over the same layouts: where it adds no block of its own, its bytes are
    the bytes RefX records"""
    rng = random.Random(72)
    data = book1()
    for ring in (8192, 73727):
        pieces = cut_pieces(data, rng, 40, 1, 1500)
        s = rs.write("w", "g", ring, pieces, ring_place(ring), False, zero_at_jump=False)
        xs = placed("x", "ring", ring, pieces, ring_place(ring))
        assert [b.off for b in s.blocks] == [b.off for b in xs.blocks]
        r = RefX(rs, xs)
        by = []
        while r.k < len(xs.blocks):
            by += r.next_call(len(xs.blocks)).by
        r.close()
        assert by == [b.comp for b in s.blocks]


@pytest.mark.parametrize("mode", ["every", "random", "none"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(sim, rs, layout_streams, layout, mode):
    """every layout, at least 30 streams, cut into calls at every block boundary, at random ones, and only where a call must end: no
    mismatch in bytes or values, the record's index position and held history are the reference's currentOffset and min(dictSize, 64 KB)
    behind every call, no access outside the bounds"""
    streams = layout_streams[layout]
    assert len(streams) >= 30
    rng = random.Random(1000 + 3 * LAYOUTS.index(layout) + ("every", "random", "none").index(mode))
    eng = SimX(sim, len(streams) + 2)
    ids = sorted(rng.sample(range(len(streams) + 2), len(streams)))
    bad, made, rounds = drive_x(eng, rs, streams, rng, mode=mode, ids=ids, check_state=eng.state_is)
    assert eng.oob == 0, "out-of-bounds access"
    assert not bad, (len(bad), bad[:5])
    if layout == "ring200000":      # (long enough to wrap, with 64 KB of history at the jump)
        assert all(any(b.off == 0 for b in xs.blocks[1:]) for xs in streams)
    if mode == "none" and layout == "contig":
        assert all(len(m) == 1 for m in made)


def test_external_mode_is_exercised(sim, rs, layout_streams):
    """over the jump layouts at least half of all blocks differ from what the reference's prefix-mode chain gives for the same pieces
    laid back to back (the reference alone decides this: both sides of the comparison are its bytes); the share per layout is printed"""
    rng = random.Random(77)
    differ = total = 0
    for layout in JUMP_LAYOUTS:
        streams = layout_streams[layout]
        eng = SimX(sim, len(streams))
        bad, made, _ = drive_x(eng, rs, streams, rng, mode="random", absent=0.0)
        assert not bad and eng.oob == 0
        d, t = jump_share(rs, streams, made)
        print("%s: %d of %d blocks differ from the prefix-mode chain" % (layout, d, t))
        assert d > 0
        differ += d; total += t
    assert 2 * differ >= total, (differ, total)


def test_hand_built(sim, rs):
    """the joints at every distance 1 .. 20, the 0-byte block at a jump, blocks of 1 .. 12 bytes at jumps, histories of 1, 3 and 4
    bytes: call by call and in as few calls as a snapshot allows"""
    data = book1()
    rng = random.Random(73)
    streams = hand_built(rng, data)
    names = " | ".join(s.name for s in streams)
    for must in ("joint 1 ", "joint 20", "zero at a jump", "small 12 at jumps", "history 1 at a jump", "history 3 at a jump", "history 4 at a jump"):
        assert must in names + " ", must
    for mode in ("every", "none"):
        eng = SimX(sim, len(streams))
        bad, made, _ = drive_x(eng, rs, streams, rng, mode=mode, absent=0.0, check_state=eng.state_is)
        assert eng.oob == 0 and not bad, (mode, eng.oob, len(bad), bad[:5])
    by = {s.name: [x for c in m for x in c.by] for s, m in zip(streams, made)}
    # the match over the joint is there: the second block of a joint stream is shorter than the same block without its history
    flat = {s.name: prefix_chain_bytes(rs, XStream(s.name, "x", s.win_len, s.blocks[1:2])) for s in streams if s.name.startswith("joint")}
    assert all(len(by[n][1]) < len(flat[n][0]) for n in flat), [n for n in flat if len(by[n][1]) >= len(flat[n][0])]
    # the dropped history: the block behind the 0-byte block at a jump compresses as a first block does, the one in place does not
    first = prefix_chain_bytes(rs, XStream("f", "x", 8192, [XBlock(0, streams[40].blocks[2].data)]))[0]
    assert streams[40].name == "zero at a jump" and by["zero at a jump"][2] == first and by["zero in place"][2] != first


def test_capacity_one_short_at_a_jump(sim, rs):
    """the result is 0, the stream is stopped, later calls get LZ4HIP_CHAIN_STOPPED until a reset"""
    data = book1()
    rng = random.Random(74)
    xs = capacity_case(rs, data)
    eng = SimX(sim, 2)
    bad, made, _ = drive_x(eng, rs, [xs], rng, mode="every", ids=[1], absent=0.0)
    assert not bad and eng.oob == 0, bad
    outs = [r for c in made[0] for r in c.outs]
    assert outs[0] > 0 and outs[1:] == [0, CHAIN_STOPPED, CHAIN_STOPPED] and eng.record(1)[2] & 4
    assert eng.record(1)[4] == len(xs.blocks[0].data)
    eng.reset([1])
    xs2 = XStream("after the reset", "hand", 8192, [XBlock(b.off, b.data) for b in xs.blocks])
    bad, made, _ = drive_x(eng, rs, [xs2], rng, mode="none", ids=[1], absent=0.0, check_state=eng.state_is)
    assert not bad and all(r > 0 for c in made[0] for r in c.outs)


def test_walks_alternate_on_one_record(sim, rs):
    """calls of the existing walk (the source follows its history) and of the new one alternate on one record: the bytes are ONE
    LZ4_stream_t's, whichever walk takes a call"""
    data = book1()
    rng = random.Random(75)
    for trial in range(12):
        pieces = cut_pieces(data, rng, 16, 0, 3000)
        offs, pos = [], 0
        for k, p in enumerate(pieces):     # contiguous, but every fourth block jumps to a place of its own further up
            if k and k % 4 == 0:
                pos += 5000
            offs.append(pos); pos += len(p)
        xs = XStream("alternating %d" % trial, "contig", pos + 16, [XBlock(o, p) for o, p in zip(offs, pieces)])
        ref = RefX(rs, xs)
        eng = SimX(sim, 1)
        k = 0
        while k < len(pieces):
            c = ref.next_call(k + 1)
            jump = k and k % 4 == 0
            if jump or (k % 2 == 0 and k % 4 != 1):
                pk = PackedX([c], rng)
                dst, out, cons = eng.call([0], pk)
                assert not pk.check([xs.name], dst, out, cons), (trial, k)
            else:
                # the existing call: the stream's history directly in front of the source, as the arena has it
                s = ref.win_off + offs[k]
                cap = bound(len(pieces[k]))
                dst, out, cons = eng.call_prefix([0], c.arena, [s], [c.hist_len], [len(pieces[k])], [0, 1], cap + 16, [8], [cap])
                assert c.hist_end in (s, 0) and int(out[0]) == c.outs[0] and dst[8:8 + c.outs[0]] == c.by[0], (trial, k)
            assert eng.state_is(0, c.state), (trial, k, eng.record(0), c.state)
            k += 1
        assert eng.oob == 0
        ref.close()


def overlapping_streams(rng, n_streams):
    """a block, then a block whose source begins INSIDE the first one and runs past its end (rule 2 trims only a source that ends inside
    its history): external-dictionary mode against a history whose second half the block's own bytes have replaced.  Small alphabets,
    so that buckets collide and short matches abound"""
    out = []
    for t in range(n_streams):
        alpha = bytes(rng.sample(range(256), rng.choice((2, 3, 4, 8))))
        text = lambda n: bytes(rng.choice(alpha) for _ in range(n))
        n0 = rng.randrange(200, 1500)
        s1 = rng.randrange(1, n0 - 12)       # (not 0: a source that begins exactly where its history does is the header's exception)
        blocks = [XBlock(0, text(n0)), XBlock(s1, text(rng.randrange(n0 - s1, 2500))), XBlock(3000, text(300))]
        out.append(XStream("overlap #%d" % t, "hand", 8192, blocks))
    return out


def test_source_written_over_its_history(sim, rs):
    """the history is read as it is NOW, as liblz4's compare of the candidate bytes does: a table entry's fingerprint was taken from
    the bytes that were there when it was made (FastCore's alias_hi).  (With the rule switched off, a developer build of this
    simulator fails this test in its first streams.)"""
    rng = random.Random(76)
    streams = overlapping_streams(rng, 300)
    eng = SimX(sim, len(streams))
    bad, made, _ = drive_x(eng, rs, streams, rng, mode="every", absent=0.0, check_state=eng.state_is)
    assert eng.oob == 0 and not bad, (len(bad), bad[:5])
