"""Shared pieces of the resident-stream compressor tests (test_cstream_hostsim.py, test_cstream_abi.py, test_gpu_cstream.py): ONE
LZ4_stream_t of the reference library per stream through ctypes (LZ4_createStream / LZ4_loadDict / LZ4_compress_fast_continue /
LZ4_saveDict), the Life record (what a stream is given call by call), the case set, and the driver that cuts lives into calls, lays
each call out and checks what came back.  The expected value of every case is what the reference library returns and writes -- never
this project's output."""
import ctypes as C
import random

import numpy as np

from cchain_common import CHAIN_STOPPED, CChain, RefCChain, book1, bound

GUARD = 128
FULL = None    # a call's prefix: everything the stream holds, at most 64 KB (the caller left the data in place)


class Call:
    """one call's share of a stream: blocks = [(source bytes, dst_cap)]; prefix = the chain_prefix_len the caller passes: FULL, or a
    number -- for a fresh stream the bytes LZ4_loadDict gets, for a running one LZ4_saveDict's size; lens: src_len where it is not
    len(source)"""

    def __init__(self, blocks, prefix=FULL, lens=None):
        self.blocks = [(bytes(s), int(c)) for s, c in blocks]
        self.prefix = prefix
        self.lens = list(lens) if lens is not None else [len(s) for s, _ in self.blocks]

    @property
    def data(self):
        return b"".join(s for s, _ in self.blocks)


class Life:
    """one stream from its creation (or reset) on: `history` = the bytes a fresh stream loads (LZ4_loadDict), calls = [Call]"""

    def __init__(self, name, calls, history=b""):
        self.name, self.calls, self.history = name, list(calls), bytes(history)

    def untruncated(self):
        return all(c.prefix is FULL for c in self.calls)

    def as_chain(self):
        """the same blocks as ONE chain of lz4hip_compress_fast_chain_batch (only where no call cuts the history)"""
        blocks = [b for c in self.calls for b in c.blocks]
        return CChain(self.name, blocks, self.history, [n for c in self.calls for n in c.lens])


def life_of(name, data, sizes, cuts, history=b"", caps=None):
    """data cut into blocks of the given sizes (capacity: the bound, or caps[i]); cuts = the block indexes at which a new call starts"""
    blocks, o = [], 0
    for i, n in enumerate(sizes):
        blocks.append((data[o:o + n], caps[i] if caps else bound(n)))
        o += n
    assert o == len(data), (name, o, len(data))
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(blocks))) + [len(blocks)]
    return Life(name, [Call(blocks[a:b]) for a, b in zip(edges, edges[1:])], history)


class RefStream:
    """ONE LZ4_stream_t of the reference library, fed call by call.  A running stream's next call goes through LZ4_saveDict(size) into a
    buffer of its own with the call's source directly behind the saved bytes -- with prefix FULL the saved size is everything the stream
    holds (at most 64 KB), which compresses as data left in place does (test_cstream_hostsim.py checks that against the reference
    too).  `held` = the bytes the stream holds (liblz4's dictionary, dictSize of them), which is what the caller has to put in front
    of the next call's source."""

    def __init__(self, rc, history=b""):
        self.L, self.st = rc.L, rc.L.LZ4_createStream()
        self.L.LZ4_saveDict.restype = C.c_int
        self.L.LZ4_saveDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.fresh, self.alive, self.history = True, True, bytes(history)
        self.held, self.buf, self.consumed = b"", None, 0

    def close(self):
        if self.st:
            self.L.LZ4_freeStream(self.st)
            self.st = None

    def front(self, call):
        """-> (the bytes the caller lays in front of the call's source, chain_prefix_len).  A number larger than what the stream holds
        is filled up with bytes that are none of the stream's"""
        if self.fresh:
            return self.history, len(self.history)
        if call.prefix is FULL:
            h = self.held[-65536:]
            return h, len(h)
        h = self.held[-call.prefix:] if call.prefix else b""
        return bytes([0xC3]) * (call.prefix - len(h)) + h, call.prefix

    def run(self, call):
        """-> (out_len per block, consumed by this call, [bytes per block]) of the reference for this call"""
        L = self.L
        n = len(call.blocks)
        if not self.alive:
            return [CHAIN_STOPPED] * n, 0, [b""] * n
        data = call.data
        if self.fresh:
            P = len(self.history)
            buf = C.create_string_buffer(GUARD + P + len(data) + GUARD)
            base = C.addressof(buf) + GUARD
            C.memmove(base, self.history + data, P + len(data))
            if P > 0:
                L.LZ4_loadDict(self.st, base, P)
            k = 0 if P < 8 else min(P, 65536)
            self.held = self.history[len(self.history) - k:]
            self.fresh = False
            start = base + P
        else:
            want = 65536 if call.prefix is FULL else call.prefix
            buf = C.create_string_buffer(GUARD + 65536 + len(data) + GUARD)
            base = C.addressof(buf) + GUARD
            k = L.LZ4_saveDict(self.st, base, min(want, 65536))
            assert k == min(want, 65536, len(self.held)), (k, want, len(self.held))
            assert C.string_at(base, k) == (self.held[-k:] if k else b"")
            self.held = self.held[-k:] if k else b""
            C.memmove(base + k, data, len(data))
            start = base + k
        self.buf = buf          # (the stream points into it until the next call)
        outs, by, pos = [], [], 0
        for (s, cap), sl in zip(call.blocks, call.lens):
            if not self.alive:
                outs.append(CHAIN_STOPPED); by.append(b"")
                continue
            if sl < 0 or cap < 0:
                r = 0
            else:
                dst = C.create_string_buffer(max(cap, 1) + 8)
                r = L.LZ4_compress_fast_continue(self.st, start + pos, dst, sl, cap, 1)
                assert 0 <= r <= cap
            outs.append(r)
            if r == 0:
                self.alive = False
                by.append(b"")
            else:
                by.append(dst.raw[:r])
                pos += sl
        self.held += data[:pos]
        self.consumed += pos
        return outs, pos, by


# ---- the case set ----
def content(rng, O, n, kind=None):
    """n bytes of one of the kinds: text of the committed corpus, the synthetic generator, incompressible, a short
    period"""
    b = book1()
    kind = rng.randrange(4) if kind is None else kind
    if kind == 0:
        o = rng.randrange(len(b) - n)
        return b[o:o + n]
    if kind == 1:
        return O.gen_block(n, rng.randrange(10000), litmax=rng.choice([4, 38, 200]), win=rng.choice([64, 300, 4096, 65535]))
    if kind == 2:
        return rng.randbytes(n)
    p = rng.randbytes(rng.randrange(1, 40))
    return (p * (n // len(p) + 1))[:n]


def block_size(rng, top):
    k = rng.random()
    if k < 0.08:
        return 0
    if k < 0.22:
        return rng.randrange(1, 13)
    if k < 0.30:
        return rng.choice([13, 14, 15, 16, 64, 65])
    if k < 0.85:
        return rng.randrange(17, min(top, 3000) + 1)
    return rng.randrange(17, top + 1)


def random_life(rng, O, name, n_blocks, top, history=b"", every_boundary=False, same_kind=None):
    """n_blocks blocks of 0 .. top bytes; every block of a stream continues one piece of content or starts another, so that later blocks
    find matches in earlier ones; cut into calls at every block boundary or at random ones"""
    sizes = [block_size(rng, top) for _ in range(n_blocks)]
    total = sum(sizes)
    data = bytearray()
    while len(data) < total:
        n = min(total - len(data), rng.randrange(1, 30000))
        piece = content(rng, O, n, same_kind)
        if data and rng.random() < 0.3:        # a copy of something seen before, somewhere inside
            o = rng.randrange(len(data))
            piece = (bytes(data[o:o + n]) + piece)[:n]
        data += piece
    if every_boundary:
        cuts = range(1, n_blocks)
    else:
        cuts = sorted(rng.sample(range(1, n_blocks), min(n_blocks - 1, rng.randrange(0, 7)))) if n_blocks > 1 else []
    return life_of(name, bytes(data), sizes, cuts, history)


def truncation_lives(rng, O):
    """running streams whose kept history the caller cuts (LZ4_saveDict with a smaller size): every size of the list, on a stream that
    holds less than 64 KB, one that holds more, and one that began with a loaded dictionary; then the stream goes on with everything"""
    b = book1()
    out = []
    for k in (0, 3, 7, 8, 1000, 65535, 65536, 70000, 200000):
        for tag, first, hist in (("small", [700, 5, 900], b""), ("large", [20000] * 4, b""), ("dict", [3000, 3000], b[50000:53000])):
            o = rng.randrange(1000, 90000)
            n1 = sum(first)
            d = b[o:o + n1 + 9000]
            c1 = Call([(d[a:a + n], bound(n)) for a, n in zip(np.cumsum([0] + first[:-1]).tolist(), first)])
            # (the second call repeats bytes of the first: what is found depends on what was kept)
            again = d[200:1200] + d[n1:n1 + 2000] + d[n1 - 600:n1] + d[n1 + 2000:n1 + 3000]
            c2 = Call([(again[:2500], bound(2500)), (again[2500:], bound(len(again) - 2500))], prefix=k)
            c3 = Call([(d[n1 + 3000:n1 + 6000] + d[100:400], bound(3300))])
            out.append(Life("kept %d on a %s stream" % (k, tag), [c1, c2, c3], hist))
    return out


def small_first_lives(rng, O):
    """first calls made of blocks under 13 bytes only: the table is built in a later call, with all, some or none of the stream's first
    bytes still in front of the source"""
    b = book1()
    out = []
    for k, (first, hist) in enumerate((([1], b""), ([2, 1], b""), ([3], b""), ([4], b""), ([12, 12, 12], b""), ([0, 0], b""), ([5, 0, 7], b""), ([12], b[:5]),
                                       ([3, 3], b[:8]), ([12, 1], b[:3000]), ([2], b[:70000]))):
        for prefix in (FULL, 0, 2, 100):
            o = 3000 * k + 777
            d = b[o:o + 5000]
            n1 = sum(first)
            cuts1 = np.cumsum([0] + first[:-1]).tolist()
            c1 = Call([(d[a:a + n], bound(n)) for a, n in zip(cuts1, first)])
            c2 = Call([(d[n1:n1 + 6], bound(6))], prefix=prefix if prefix is FULL else min(prefix, 100))
            rest = d[:n1] * 3 + d[n1 + 6:n1 + 900] + d[:40]
            c3 = Call([(rest, bound(len(rest))), (d[:300], bound(300))], prefix=prefix)
            out.append(Life("small first %r hist %d kept %r" % (first, len(hist), prefix), [c1, c2, c3], hist))
    return out


def prefix_lives(rng, O):
    """fresh streams that load 0, 1, 7, 8, 1000, 65536 and 70000 bytes, cut into calls"""
    b = book1()
    out = []
    for P in (0, 1, 7, 8, 1000, 65536, 70000):
        for sizes, cuts in (([1000] * 6, (1, 2, 3, 4, 5)), ([5, 0, 13, 300, 12, 2000], (2, 4)), ([4096] * 20, (7, 13))):
            o = 70000 + 1000 * (P % 13)
            out.append(life_of("fresh, %d loaded, %r..." % (P, sizes[:3]), b[o:o + sum(sizes)], sizes, cuts, history=b[o - P:o]))
    return out


def capacity_lives(rc, rng, O):
    """a block that does not fit in the first, a middle and the last call; a negative src_len and dst_cap; the calls behind the stop"""
    b = book1()
    out = []
    sizes = [800, 900, 1000, 1100, 1200, 700]
    for at in range(6):
        for how in ("cap - 1", "cap 0", "cap -1", "src_len -1"):
            o = 1000 * at + 31
            lf = life_of("%s at block %d" % (how, at), b[o:o + sum(sizes)], sizes, (2, 4))
            ref = RefStream(rc)
            exact = [r for c in lf.calls for r in ref.run(c)[0]]
            ref.close()
            call = lf.calls[at // 2]
            s, cap = call.blocks[at % 2]
            if how == "src_len -1":
                call.lens[at % 2] = -1
            else:
                call.blocks[at % 2] = (s, {"cap - 1": exact[at] - 1, "cap 0": 0, "cap -1": -1}[how])
            out.append(lf)
    return out


def case_set(rc, rng, O, n_random=260):
    """every life of the CPU test"""
    lives = []
    for i in range(n_random):
        nb = rng.choice([1, 2, 3, 5, 8, 20, 40]) if i % 9 else rng.choice([100, 150])
        top = 20000 if nb <= 20 else (3000 if nb <= 40 else 1500)
        hist = b""
        if i % 5 == 0:
            P = rng.choice([1, 7, 8, 9, 500, 5000, 65536, 70000])
            o = rng.randrange(70000, 150000)
            hist = book1()[o - P:o]
        lives.append(random_life(rng, O, "random %d" % i, nb, top, hist, every_boundary=(i % 3 == 0)))
    # histories that pass 64 KB: across calls, inside a call
    lives.append(random_life(rng, O, "150 x up to 2000, text", 150, 2000, same_kind=0, every_boundary=True))
    lives.append(life_of("book1 40 x 4096", book1()[5000:5000 + 40 * 4096], [4096] * 40, range(3, 40, 3)))
    lives.append(life_of("book1 5 x 30000", book1()[:150000], [30000] * 5, (1, 2, 3, 4)))
    lives.append(life_of("book1 70000 + 70000", book1()[:140000], [70000] * 2, (1,)))
    lives.append(life_of("incompressible 6 x 4096", rng.randbytes(6 * 4096), [4096] * 6, (1, 3)))
    lives.append(life_of("empty only", b"", [0, 0, 0], (1, 2)))
    return lives + prefix_lives(rng, O) + truncation_lives(rng, O) + small_first_lives(rng, O) + capacity_lives(rc, rng, O)


# ---- the driver ----
class Engine:
    """what runs a call: the lane simulator on host state, or the C ABI on a set of device streams.  call(ids, P) gets the stream ids
    (ascending) and a PackedCall and returns (dst, out_len, chain_consumed); reset(ids) makes those streams fresh"""

    def call(self, ids, pk):
        raise NotImplementedError

    def reset(self, ids):
        raise NotImplementedError


u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


class DevEngine(Engine):
    """a set of n resident streams behind the C ABI"""

    def __init__(self, amd, n):
        self.amd, self.l, self.n = amd, amd.lib(), n
        self.h = C.c_void_p(None)
        assert self.l.lz4hip_cstreams_create(n, C.byref(self.h)) == 0, self.l.lz4hip_last_error()
        assert self.l.lz4hip_cstreams_count(self.h) == n

    def call(self, ids, pk, expect=0):
        sid = np.ascontiguousarray(ids, dtype=np.uint32)
        src = C.create_string_buffer(pk.src, len(pk.src))
        dst = C.create_string_buffer(bytes(pk.dst), len(pk.dst))
        cso, pre, sl, cf, do, dc = pk.arrays()
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        rc = self.l.lz4hip_compress_fast_stream_batch(self.h, P(sid, u32), src, P(cso, u64), pre.ctypes.data, P(sl, i32), P(cf, u32), dst, P(do, u64),
                                                      P(dc, i32), P(out, i32), P(cons, u64), pk.n_blocks, pk.n_chains)
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


class PackedCall:
    """one call's chains laid out: every chain's front bytes and source in src with GUARD bytes of 0xA5 around them (and a pad of 0..3
    bytes, so that addresses are odd as often as not), every block's slot of max(dst_cap, 0) bytes in dst, filled, between guards"""

    def __init__(self, parts, rng, fill=0x5A):
        self.fill = fill
        src = bytearray(b"\xA5" * GUARD)
        dst = bytearray(b"\xA5" * GUARD)
        self.chain_src_off, self.prefix, self.src_len, self.chain_first, self.dst_off, self.dst_cap = [], [], [], [0], [], []
        for front, plen, call in parts:
            src += b"\xA5" * rng.randrange(4)
            assert len(front) == plen
            src += front
            self.chain_src_off.append(len(src)); self.prefix.append(plen)
            src += call.data + b"\xA5" * GUARD
            for (s, cap), sl in zip(call.blocks, call.lens):
                dst += b"\xA5" * rng.randrange(4)
                self.src_len.append(sl); self.dst_off.append(len(dst)); self.dst_cap.append(cap)
                dst += bytes([fill]) * max(cap, 0) + b"\xA5" * GUARD
            self.chain_first.append(len(self.src_len))
        self.src, self.dst = bytes(src), dst
        self.n_blocks, self.n_chains = len(self.src_len), len(parts)

    def arrays(self):
        a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
        return (a64(self.chain_src_off), a32(self.prefix), a32(self.src_len), a32(self.chain_first, np.uint32), a64(self.dst_off), a32(self.dst_cap))

    def check(self, names, dst, out_len, consumed, want):
        """what the call left against the reference's results: the values, the bytes produced, and every byte the call must not have
        written -- the guards, what lies past a result, a stopped block's slot"""
        bad = []
        dst = bytes(dst)
        assert len(dst) == len(self.dst)
        if dst[:GUARD] != b"\xA5" * GUARD:
            bad.append(("front guard written",))
        for c, (name, (outs, done, by)) in enumerate(zip(names, want)):
            b0, b1 = self.chain_first[c], self.chain_first[c + 1]
            got = [int(v) for v in out_len[b0:b1]]
            if got != outs or int(consumed[c]) != done:
                bad.append((name, "values", got[:8], outs[:8], int(consumed[c]), done))
                continue
            for i in range(b0, b1):
                o, cap, r = self.dst_off[i], max(self.dst_cap[i], 0), max(outs[i - b0], 0)
                if dst[o:o + r] != by[i - b0]:
                    bad.append((name, "bytes of block", i - b0))
                    break
                if dst[o + r:o + cap] != bytes([self.fill]) * (cap - r) and outs[i - b0] != 0:
                    bad.append((name, "written past the result", i - b0))
                    break
                if dst[o - 1:o] != b"\xA5" or dst[o + cap:o + cap + GUARD] != b"\xA5" * GUARD:
                    bad.append((name, "guard written", i - b0))
                    break
        return bad


def drive(engine, rc, lives, rng, absent=0.5, ids=None, keep=None):
    """every life on its own stream (ids[i], ascending; default 0 .. n - 1), call by call: in every round each unfinished stream takes
    part with probability 1 - absent.  -> (mismatches, per life the reference's results [(outs, consumed, bytes)] call by call, rounds).
    keep: a list that receives (round, ids, PackedCall, out_len) of every call (the round-trip test reads it)"""
    ids = list(range(len(lives))) if ids is None else list(ids)
    refs = [RefStream(rc, lf.history) for lf in lives]
    nxt = [0] * len(lives)
    results = [[] for _ in lives]
    bad, rounds = [], 0
    while any(nxt[i] < len(lf.calls) for i, lf in enumerate(lives)):
        todo = [i for i, lf in enumerate(lives) if nxt[i] < len(lf.calls)]
        now = [i for i in todo if rng.random() >= absent] or todo[:1]
        parts, want = [], []
        for i in now:
            call = lives[i].calls[nxt[i]]
            front, plen = refs[i].front(call)
            parts.append((front, plen, call))
            want.append(refs[i].run(call))
            results[i].append(want[-1])
            nxt[i] += 1
        pk = PackedCall(parts, rng)
        dst, out, cons = engine.call([ids[i] for i in now], pk)
        bad += [(rounds,) + b for b in pk.check([lives[i].name for i in now], dst, out, cons, want)]
        if keep is not None:
            keep.append((rounds, [ids[i] for i in now], now, pk, [int(v) for v in out[:pk.n_blocks]], dst))
        rounds += 1
    for r in refs:
        r.close()
    return bad, results, rounds


def chain_equals_stream(rc, life, result):
    """the one-call chain of the reference (a fresh stream, every block in one go) gives what the stream gave call by call"""
    outs, done, by = rc.compress(life.as_chain())
    s_outs = [r for c in result for r in c[0]]
    s_by = [x for c in result for x in c[2]]
    return outs == s_outs and by == s_by and done == sum(c[1] for c in result)


__all__ = ["CHAIN_STOPPED", "Call", "DevEngine", "Engine", "FULL", "GUARD", "Life", "PackedCall", "RefCChain", "RefStream", "bound", "capacity_lives", "case_set",
           "chain_equals_stream", "drive", "life_of", "prefix_lives", "random_life", "small_first_lives", "truncation_lives"]
