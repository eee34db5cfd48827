"""Shared pieces of the tests of lz4hip_compress_fast_stream_ext_batch (test_cxstream_hostsim.py, test_cxstream_abi.py,
test_gpu_cxstream.py): compress streams whose sources land anywhere.  Every expected value is the reference library's: ONE LZ4_stream_t
per stream (dstream_common.RefStream's handle on liblz4 1.9.3) runs over an encoder buffer of the stream's layout, block by block, and
the engine is given the same buffer as it stands at the end of each call.

A call is a snapshot: all of its blocks are read from one image of the caller's memory.  The reference compresses block after block
while the producer overwrites its ring, so a call ends in front of the first block whose bytes would land on anything an earlier block
of the same call reads (its source or the history it can reach): RefX.next_call cuts there whatever the caller asked for, and in front
of every block of the save-area layout, whose caller moves the history between two blocks.

The layouts (offsets relative to the stream's window):
  contig     blocks back to back
  two4096    two alternating buffers of 4096 bytes       two16   of 16 bytes, blocks of 0 .. 16
  save       a 64 KB save area + a block area: before every block the last 64 KB go to the save area through LZ4_saveDict
  ring73727  a ring of 65535 + 2 x 4096 bytes that wraps to 0 when the next block does not fit
  ring8192   blocks of up to 1500 bytes: the overlap trim at every wrap          ring3000   the trim leaves nothing
  ring200000 blocks of up to 60000 bytes: jumps with 64 KB of history
  dict7 / dict4096 / dict70000   contiguous blocks of a fresh stream whose dictionary lies elsewhere: in front of the window, behind it,
             or directly in front of it (`lead`)"""
import ctypes as C
import random

import numpy as np

from cchain_common import CHAIN_STOPPED, bound
from conftest import calgary
from dstream_common import RefStream, cut_pieces, ring_place

GUARD = 128
OFF_CUR, OFF_DICT, OFF_DSIZE = 16384, 16392, 16408   # LZ4_stream_t_internal, 1.9.3: currentOffset, dictionary, dictSize


def book1():
    return calgary("book1")


class XBlock:
    def __init__(self, off, data, cap=None, src_len=None):
        self.off, self.data = int(off), bytes(data)
        self.cap = bound(len(self.data)) if cap is None else int(cap)
        self.src_len = len(self.data) if src_len is None else int(src_len)


class XStream:
    """one stream: its window's length, its blocks, its dictionary (side: 'front' / 'back' of the window behind a guard, or 'lead':
    directly in front of it) and the save area's size (layout `save`)"""

    def __init__(self, name, layout, win_len, blocks, dictionary=None, side="front", save_area=0):
        self.name, self.layout, self.win_len, self.blocks = name, layout, int(win_len), blocks
        self.dictionary, self.side, self.save_area = dictionary, side, save_area


def placed(name, layout, win_len, pieces, place, **kw):
    blocks, pos = [], 0
    for k, p in enumerate(pieces):
        off = place(k, len(p), pos)
        assert 0 <= off and off + len(p) <= win_len, (name, k, off, len(p))
        blocks.append(XBlock(off, p))
        pos = off + len(p)
    return XStream(name, layout, win_len, blocks, **kw)


LAYOUTS = ("contig", "two4096", "two16", "save", "ring73727", "ring8192", "ring3000", "ring200000", "dict7", "dict4096", "dict70000")
JUMP_LAYOUTS = ("two4096", "ring73727", "ring8192", "ring3000")


def make_xstream(layout, rng, data, tag="", n_blocks=None):
    name = "%s %s" % (layout, tag)
    if layout == "contig":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(4, 30), 0, 4096)
        return placed(name, layout, sum(map(len, p)) + 16, p, lambda k, n, pos: pos)
    if layout == "two4096":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(4, 30), 0, 4096)
        return placed(name, layout, 8192, p, lambda k, n, pos: (k & 1) * 4096)
    if layout == "two16":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(8, 60), 0, 16)
        return placed(name, layout, 32, p, lambda k, n, pos: (k & 1) * 16)
    if layout == "save":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(4, 40), 1, 4096)
        return placed(name, layout, 65536 + 4096, p, lambda k, n, pos: 65536, save_area=65536)
    if layout == "ring73727":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(50, 90), 0, 4096)
        return placed(name, layout, 73727, p, ring_place(73727))
    if layout in ("ring8192", "ring3000"):
        ring = int(layout[4:])
        p = cut_pieces(data, rng, n_blocks or rng.randrange(10, 40), 0, 1500)
        return placed(name, layout, ring, p, ring_place(ring))
    if layout == "ring200000":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(10, 14), 20000, 60000)
        return placed(name, layout, 200000, p, ring_place(200000))
    if layout.startswith("dict"):
        size = int(layout[4:])
        o = rng.randrange(0, len(data) - size - 1)
        p = cut_pieces(data, rng, n_blocks or rng.randrange(3, 20), 0, 4096)
        if size >= 4096:      # (the first block starts with bytes of the dictionary's tail: a match over the joint)
            p[0] = data[o + size - 40:o + size - 10] + p[0]
        return placed(name, layout, sum(map(len, p)) + 16, p, lambda k, n, pos: pos, dictionary=data[o:o + size],
                      side=rng.choice(("front", "back", "lead")))
    raise ValueError(layout)


class XCall:
    """one call's share of a stream, as the reference did it: blocks [k0, k1); where the history ends (an arena offset) and how much of
    it there is; the arena as it stands behind the call; per block the reference's result and bytes; the stream's currentOffset and
    min(dictSize, 65536) behind the call (None once the stream has stopped)"""


class RefX:
    """ONE LZ4_stream_t of the reference library over an arena [guard | dictionary | guard | window | guard | dictionary | guard]"""

    def __init__(self, rs, xs):
        self.L, self.xs = rs.L, xs
        L = self.L
        L.LZ4_saveDict.restype = C.c_int
        d = xs.dictionary or b""
        front = d if xs.side in ("front", "lead") else b""
        back = d if xs.side == "back" else b""
        gap = 0 if xs.side == "lead" else GUARD
        self.win_off = GUARD + len(front) + gap
        self.dict_end = GUARD + len(front) if front else self.win_off + xs.win_len + GUARD + len(back)
        self.size = self.win_off + xs.win_len + GUARD + len(back) + GUARD
        self.buf = C.create_string_buffer(bytes([0xA5]) * self.size, self.size)
        self.base = C.addressof(self.buf)
        if d:
            C.memmove(self.base + self.dict_end - len(d), d, len(d))
        self.st = L.LZ4_createStream()
        if d:
            L.LZ4_loadDict(self.st, self.base + self.dict_end - len(d), len(d))
        self.k, self.alive = 0, True

    def close(self):
        if self.st:
            self.L.LZ4_freeStream(self.st)
            self.st = None

    def fields(self):
        cur = C.c_uint32.from_address(self.st + OFF_CUR).value
        dptr = C.c_uint64.from_address(self.st + OFF_DICT).value
        dsz = C.c_uint32.from_address(self.st + OFF_DSIZE).value
        return cur, (dptr + dsz - self.base if dsz else 0), dsz

    def window(self):
        """(win_off, win_len) for the next call: a `lead` dictionary joins the window once the history has grown out of it"""
        d = len(self.xs.dictionary or b"")
        if self.xs.side == "lead" and self.k:
            return self.win_off - d, self.xs.win_len + d
        return self.win_off, self.xs.win_len

    def next_call(self, want_end):
        L, xs = self.L, self.xs
        c = XCall()
        c.k0 = self.k
        c.win, c.blk_base = self.window(), self.win_off
        _, de, dsz = self.fields()
        if self.k == 0 and xs.dictionary:
            c.hist_end, c.hist_len = self.dict_end, len(xs.dictionary)
        else:
            c.hist_end, c.hist_len = de, min(dsz, 65536)
        if xs.save_area and self.k and self.alive:
            keep = min(xs.save_area, 65536, dsz)
            assert L.LZ4_saveDict(self.st, self.base + self.win_off + xs.save_area - keep, keep) == keep
            c.hist_end, c.hist_len = (self.win_off + xs.save_area, keep) if keep else (0, 0)
        read, c.outs, c.by = [], [], []
        while self.k < want_end:
            b = xs.blocks[self.k]
            s, n = self.win_off + b.off, len(b.data)
            if self.k > c.k0 and (xs.save_area or any(s < hi and s + n > lo for lo, hi in read)):
                break
            if self.alive:
                _, de, dl = self.fields()
                if dl < 4 and de != s:
                    dl = 0
                if de - dl < s + n < de:
                    dl = min(de - (s + n), 65536)
                    dl = 0 if dl < 4 else dl
                dl = min(dl, 65536)
                if dl:
                    read.append((de - dl, de))
            read.append((s, s + n))
            C.memmove(self.base + s, b.data, n)
            if not self.alive:
                c.outs.append(CHAIN_STOPPED); c.by.append(b"")
            else:
                if b.src_len < 0 or b.cap < 0:
                    r = 0
                else:
                    dst = C.create_string_buffer(max(b.cap, 1) + 8)
                    r = L.LZ4_compress_fast_continue(self.st, self.base + s, dst, b.src_len, b.cap, 1)
                    assert 0 <= r <= b.cap
                c.outs.append(r)
                c.by.append(dst.raw[:r] if r else b"")
                if r == 0:
                    self.alive = False
            self.k += 1
        c.k1 = self.k
        c.blocks = xs.blocks[c.k0:c.k1]
        c.consumed = sum(len(b.data) for b, r in zip(c.blocks, c.outs) if r > 0)
        c.arena = self.buf.raw
        cur, _, dsz = self.fields()
        c.state = (cur, min(dsz, 65536)) if self.alive else None
        return c


class PackedX:
    """one engine call: every stream's arena side by side in src (offsets shifted), every block's slot in dst between guards"""

    def __init__(self, calls, rng, fill=0x5A):
        self.fill, self.calls = fill, calls
        src, dst = bytearray(), bytearray(b"\xA5" * GUARD)
        self.src_off, self.src_len, self.first, self.hist_end, self.hist_len = [], [], [0], [], []
        self.win_off, self.win_len, self.dst_off, self.dst_cap = [], [], [], []
        for c in calls:
            src += b"\xA5" * rng.randrange(4)
            base = len(src)
            src += c.arena
            self.hist_end.append(base + c.hist_end if c.hist_len else 0); self.hist_len.append(c.hist_len)
            self.win_off.append(base + c.win[0]); self.win_len.append(c.win[1])
            for b in c.blocks:
                dst += b"\xA5" * rng.randrange(4)
                self.src_off.append(base + c.blk_base + b.off)
                self.src_len.append(b.src_len); self.dst_off.append(len(dst)); self.dst_cap.append(b.cap)
                dst += bytes([fill]) * max(b.cap, 0) + b"\xA5" * GUARD
            self.first.append(len(self.src_len))
        self.src, self.dst = bytes(src) + b"\xA5" * 8, dst
        self.n_blocks, self.n_chains = len(self.src_len), len(calls)

    def arrays(self):
        a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
        return (a64(self.src_off), a32(self.src_len), a32(self.first, np.uint32), a64(self.hist_end), a32(self.hist_len), a64(self.win_off), a64(self.win_len),
                a64(self.dst_off), a32(self.dst_cap))

    def check(self, names, dst, out_len, consumed):
        bad = []
        dst = bytes(dst)
        assert len(dst) == len(self.dst)
        if dst[:GUARD] != b"\xA5" * GUARD:
            bad.append(("front guard written",))
        for t, (name, c) in enumerate(zip(names, self.calls)):
            b0, b1 = self.first[t], self.first[t + 1]
            got = [int(v) for v in out_len[b0:b1]]
            if got != c.outs or int(consumed[t]) != c.consumed:
                bad.append((name, "values", c.k0, got[:8], c.outs[:8], int(consumed[t]), c.consumed))
                continue
            for i in range(b0, b1):
                o, cap, r = self.dst_off[i], max(self.dst_cap[i], 0), max(c.outs[i - b0], 0)
                if dst[o:o + r] != c.by[i - b0]:
                    bad.append((name, "bytes of block", c.k0 + i - b0))
                    break
                if dst[o + r:o + cap] != bytes([self.fill]) * (cap - r) and c.outs[i - b0] != 0:
                    bad.append((name, "written past the result", c.k0 + i - b0))
                    break
                if dst[o - 1:o] != b"\xA5" or dst[o + cap:o + cap + GUARD] != b"\xA5" * GUARD:
                    bad.append((name, "guard written", c.k0 + i - b0))
                    break
        return bad


def cut_plan(n, mode, rng):
    """where the caller wants its calls to end: 'every' block boundary, 'random' ones, 'none' (one call, cut only where it must be)"""
    if mode == "every":
        return list(range(1, n + 1))
    if mode == "none" or n < 2:
        return [n]
    return sorted(rng.sample(range(1, n), min(n - 1, rng.randrange(1, 6)))) + [n]


def drive_x(engine, rs, streams, rng, mode="random", ids=None, absent=0.3, check_state=None, keep=None):
    """every stream on its own engine stream, call by call; in every round each unfinished stream takes part with probability
    1 - absent.  check_state(id, state): called behind every call with the reference's (currentOffset, held).  -> (mismatches, per
    stream the calls made, rounds)"""
    ids = list(range(len(streams))) if ids is None else list(ids)
    refs = [RefX(rs, xs) for xs in streams]
    plans = [cut_plan(len(xs.blocks), mode, rng) for xs in streams]
    made = [[] for _ in streams]
    bad, rounds = [], 0
    while any(r.k < len(xs.blocks) for r, xs in zip(refs, streams)):
        todo = [i for i, (r, xs) in enumerate(zip(refs, streams)) if r.k < len(xs.blocks)]
        now = [i for i in todo if rng.random() >= absent] or todo[:1]
        calls = []
        for i in now:
            want = next(e for e in plans[i] if e > refs[i].k)
            calls.append(refs[i].next_call(want))
            made[i].append(calls[-1])
        pk = PackedX(calls, rng)
        dst, out, cons = engine.call([ids[i] for i in now], pk)
        bad += [(rounds,) + b for b in pk.check([streams[i].name for i in now], dst, out, cons)]
        if check_state:
            for i, c in zip(now, calls):
                if c.state is not None and not check_state(ids[i], c.state):
                    bad.append((rounds, streams[i].name, "state", c.k1, c.state))
        if keep is not None:
            keep.append((rounds, now, pk, [int(v) for v in out[:pk.n_blocks]], dst))
        rounds += 1
        if len(bad) > 20:
            break
    for r in refs:
        r.close()
    return bad, made, rounds


def prefix_chain_bytes(rs, xs):
    """what the reference's prefix-mode chain gives for the same pieces laid back to back (and the same dictionary)"""
    pieces = [b.data for b in xs.blocks]
    flat = placed(xs.name + " flat", "contig", sum(map(len, pieces)) + 16, pieces, lambda k, n, pos: pos, dictionary=xs.dictionary, side="lead" if xs.dictionary else "front")
    r = RefX(rs, flat)
    c = r.next_call(len(flat.blocks))
    assert c.k1 == len(flat.blocks)
    r.close()
    return c.by


def jump_share(rs, streams, made):
    """-> (blocks whose bytes differ from the prefix-mode chain's, blocks) over these streams"""
    differ = total = 0
    for xs, calls in zip(streams, made):
        flat = prefix_chain_bytes(rs, xs)
        got = [x for c in calls for x in c.by]
        differ += sum(a != b for a, b in zip(got, flat))
        total += len(got)
    return differ, total


u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8
EXT_ARGTYPES = [C.c_void_p] * 15 + [C.c_uint32, C.c_uint32]


class DevX:
    """a set of n resident streams behind the C ABI, driven through lz4hip_compress_fast_stream_ext_batch"""

    def __init__(self, amd, n):
        self.amd, self.l, self.n = amd, amd.lib(), n
        self.h = C.c_void_p(None)
        assert self.l.lz4hip_cstreams_create(n, C.byref(self.h)) == 0, self.l.lz4hip_last_error()

    def call(self, ids, pk, expect=0):
        sid = np.ascontiguousarray(ids, dtype=np.uint32)
        src = C.create_string_buffer(pk.src, len(pk.src))
        dst = C.create_string_buffer(bytes(pk.dst), len(pk.dst))
        so, sl, cf, he, hl, wo, wl, do, dc = pk.arrays()
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        f = self.l.lz4hip_compress_fast_stream_ext_batch
        f.argtypes, f.restype = EXT_ARGTYPES, C.c_int
        rc = f(self.h, sid.ctypes.data, C.addressof(src), so.ctypes.data, sl.ctypes.data, cf.ctypes.data, he.ctypes.data, hl.ctypes.data, wo.ctypes.data,
               wl.ctypes.data, C.addressof(dst), do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains)
        assert rc == expect, (rc, self.l.lz4hip_last_error())
        assert src.raw == pk.src
        return dst.raw, out, cons

    def reset(self, ids=None):
        if ids is None:
            assert self.l.lz4hip_cstreams_reset(self.h, None, 0) == 0
        else:
            assert self.l.lz4hip_cstreams_reset(self.h, (u32 * len(ids))(*ids), len(ids)) == 0, self.l.lz4hip_last_error()

    def consumed(self, first=0, n=None):
        n = self.n - first if n is None else n
        cons, stop = (u64 * max(n, 1))(), (u8 * max(n, 1))()
        assert self.l.lz4hip_cstreams_consumed(self.h, first, n, cons, stop) == 0, self.l.lz4hip_last_error()
        return list(cons[:n]), list(stop[:n])

    def close(self):
        if self.h:
            self.l.lz4hip_cstreams_free(self.h)
            self.h = C.c_void_p(None)


# ---- the hand-built cases ----
def hand_built(rng, data):
    """-> [XStream]: the joints, the dropped histories and the small blocks of the issue's list"""
    out = []
    # a block that begins with the bytes of its dictionary's tail: the match runs from the dictionary's end into the block's start
    for d in range(1, 21):
        first = data[5000:5600]
        tail = first[-d - 30:]
        second = tail + tail[:d] * 3 + data[9000:9200]      # repeats the tail, then the bytes that followed it in the block itself
        out.append(XStream("joint %d" % d, "hand", 4096, [XBlock(2000, first), XBlock(0, second), XBlock(len(second), data[9200:9300] + first[:50])]))
        second = first[-d:] + first[:40] + data[9000:9100]
        out.append(XStream("joint short %d" % d, "hand", 4096, [XBlock(2000, first), XBlock(100, second)]))
    # a 0-byte block at a jump drops the history: the block behind it would have matched it
    one = data[20000:21000]
    out.append(XStream("zero at a jump", "hand", 8192, [XBlock(0, one), XBlock(4096, b""), XBlock(4096, one[100:900]), XBlock(2000, one[:500])]))
    out.append(XStream("zero in place", "hand", 8192, [XBlock(0, one), XBlock(1000, b""), XBlock(1000, one[100:900])]))
    # blocks of 1 .. 12 bytes at jumps, between blocks that match each other
    for n in range(1, 13):
        out.append(XStream("small %d at jumps" % n, "hand", 8192, [XBlock(0, one), XBlock(4096, one[50:50 + n]), XBlock(2000, one[30:700]),
                                                                   XBlock(6000, one[:n]), XBlock(6000 + n, one[200:600]), XBlock(3000, one[:300])]))
    # a history of 1, 3 and 4 bytes at a jump, and in place
    for h in (1, 3, 4):
        out.append(XStream("history %d at a jump" % h, "hand", 8192, [XBlock(0, one), XBlock(4096, one[:h]), XBlock(2000, one[:h] + one[:600])]))
        out.append(XStream("history %d in place" % h, "hand", 8192, [XBlock(0, one), XBlock(4096, one[:h]), XBlock(4096 + h, one[:h] + one[:600])]))
        out.append(XStream("first blocks of %d" % h, "hand", 8192, [XBlock(100, one[:h]), XBlock(100 + h, one[h:2 * h]), XBlock(4096, one[:600]), XBlock(100 + 2 * h, one[:700])]))
    # a stream whose WHOLE history is 4 .. 7 bytes (8 and 12: beside them) at a jump: the lower bound is index 0, the empty buckets name
    # the stream's first byte, and the block repeats the stream's first four bytes at probed positions -- liblz4 takes that match into a
    # history shorter than any load but a 4-byte one.  The history above the block and below it: a read past either piece shows
    for h in (4, 5, 6, 7, 8, 12):
        head = data[1000:1000 + h]
        body = b"Q" + head[:4] + data[2000:2010] + head[:4] + data[3000:3040] + head + data[3100:3120]
        out.append(XStream("whole history %d above" % h, "hand", 4096, [XBlock(2000, head), XBlock(0, body), XBlock(len(body), head[:4] + data[3000:3030])]))
        out.append(XStream("whole history %d below" % h, "hand", 4096, [XBlock(0, head), XBlock(2000, body), XBlock(3000, body[:50])]))
        out.append(XStream("whole history %d in two" % h, "hand", 4096, [XBlock(0, head[:2]), XBlock(2, head[2:]), XBlock(2000, body)]))
    return out


def capacity_case(rs, data, short=1):
    """a capacity one short of the output at a jump: the result is 0 and the stream stops"""
    one = data[30000:31000]
    xs = XStream("cap short at a jump", "hand", 8192, [XBlock(0, one), XBlock(4096, one[100:900] + data[40000:40200]), XBlock(2000, one[:500]), XBlock(6000, one[:100])])
    r = RefX(rs, xs)
    c = r.next_call(2)
    r.close()
    xs.blocks[1] = XBlock(4096, xs.blocks[1].data, cap=c.outs[1] - short)
    return xs
