"""Shared pieces of the tests of the accelerated linked-block compressors (test_caccel_hostsim.py, test_caccel_abi.py,
test_gpu_caccel.py): lz4hip_compress_fast_chain_accel_batch, lz4hip_compress_fast_stream_accel_batch and
lz4hip_compress_fast_stream_ext_accel_batch.  Every expected value is the reference library's own LZ4_compress_fast_continue on ONE
LZ4_stream_t per chain or stream.  cchain_common.py, cstream_common.py and cxstream_common.py drive that call with a literal 1; here the
same drivers run over a handle on the library whose LZ4_compress_fast_continue gets the acceleration of an AccelPlan in the place of
that 1, so layouts, records and checks are theirs and only the last argument differs.

An AccelPlan is the acceleration of every call of a run, in order: plan.now is what the NEXT call -- the reference's and the engine's --
runs at; an engine calls plan.step() behind each of its calls (the drivers compute the reference's results of a round in front of the
engine's call of that round)."""
import ctypes as C
import os
import random

import numpy as np

from cchain_common import CHAIN_STOPPED, CChain, CPacked, RefCChain, book1, bound, chain_of
from conftest import GOLD
import cstream_common as S
import cxstream_common as X
import dstream_common as D

ACCELS = (2, 3, 8, 64, 65537)
CLAMPED = ((0, 1), (-7, 1), (70000, 65537), (1 << 30, 65537))
OFF_CUR, OFF_DSIZE = X.OFF_CUR, X.OFF_DSIZE


class AccelPlan:
    def __init__(self, pattern):
        self.pattern, self.k, self.used = tuple(pattern), 0, []

    @property
    def now(self):
        return self.pattern[self.k % len(self.pattern)]

    def step(self):
        self.used.append(self.now)
        self.k += 1


class AccelLib:
    """the reference library with the plan's acceleration as LZ4_compress_fast_continue's last argument (the drivers pass 1)"""

    def __init__(self, lib, plan):
        self._lib, self.plan = lib, plan

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def LZ4_compress_fast_continue(self, st, src, dst, n, cap, one):
        assert one == 1
        return self._lib.LZ4_compress_fast_continue(st, src, dst, n, cap, self.plan.now)


class RefAccelChain(RefCChain):
    """cchain_common.RefCChain (and what cstream_common.RefStream takes) at the plan's acceleration"""

    def __init__(self, ref, plan=None):
        super().__init__(ref)
        self.plan = plan or AccelPlan((1,))
        self.L = AccelLib(self.L, self.plan)

    def at(self, accel):
        self.plan.pattern, self.plan.k = (accel,), 0
        return self


class RefAccelX(D.RefStream):
    """what cxstream_common.RefX takes, at the plan's acceleration"""

    def __init__(self, ref, plan):
        super().__init__(ref)
        self.plan = plan
        self.L = AccelLib(self.L, plan)


def gold(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def datasets():
    """short miss runs, long miss runs (k passes 64 and the step grows), long matches, zeros, one miss run from start to end"""
    return {"book1": book1()[:200000], "geo": gold("geo_65536.bin"), "pic": gold("pic_65536.bin"), "zeros": bytes(65536),
            "random": random.Random(4242).randbytes(65536)}


def chain_cases():
    """-> [CChain], every capacity the bound: per data set the first sizes that probe (13 .. 20), blocks of 1 .. 12 bytes between bigger
    ones, 1000, 4096 and 65536 bytes; book1: the 200000-byte chain in 4 KiB blocks (history passes 64 KB) and prefixes of 7, 8, 4096, 65536
    and more than 65536 bytes"""
    out = []
    for name, d in datasets().items():
        out.append(chain_of(name + " 13..20", d[100:100 + sum(range(13, 21))], list(range(13, 21))))
        sizes = [1000, 1, 2, 1500, 12, 3, 700, 5, 11, 0, 2000, 7, 13, 4, 900]
        out.append(chain_of(name + " small between", d[3000:3000 + sum(sizes)], sizes))
        out.append(chain_of(name + " 16 x 1000", d[7000:23000], [1000] * 16))
        out.append(chain_of(name + " 64 x 1000", d[:64000], [1000] * 64))
        out.append(chain_of(name + " 16 x 4096", d[:65536], [4096] * 16))
        out.append(chain_of(name + " 1 x 65536", d[:65536], [65536]))
    b = book1()
    out.append(chain_of("book1 200000 in 4 KiB blocks", b[:200000], [4096] * 48 + [200000 - 48 * 4096]))
    out.append(chain_of("book1 2 x 65536", b[40000:40000 + 131072], [65536] * 2))
    g = gold("geo_65536.bin")
    for P in (7, 8, 4096, 65536, 70000):
        out.append(chain_of("book1 prefix %d, 6 x 1000" % P, b[80000:86000], [1000] * 6, history=b[80000 - P:80000]))
        out.append(chain_of("book1 prefix %d, 4 x 4096" % P, b[90000:90000 + 16384], [4096] * 4, history=b[90000 - P:90000]))
        out.append(chain_of("book1 prefix %d, small first" % P, b[99000:99000 + 2330], [5, 0, 13, 300, 12, 2000], history=b[99000 - P:99000]))
        if P <= 4096:
            out.append(chain_of("geo prefix %d, 8 x 1000" % P, g[8000:16000], [1000] * 8, history=g[8000 - P:8000]))
    return out


def tight_cases(rc, chains, accel):
    """one byte short of the reference's result AT THIS ACCELERATION on a middle block: the chain stops there"""
    out = []
    rc.at(accel)
    for ch in chains:
        sizes = rc.compress(ch)[0]
        m = len(ch.blocks) // 2
        while m < len(ch.blocks) and sizes[m] < 2:
            m += 1
        if m < len(ch.blocks):
            out.append(ch.with_caps(lambda i, c: sizes[i] - 1 if i == m else c, "cap - 1 at %d (acceleration %d)" % (m, accel)))
    return out


def is_book1_big(ch):
    return ch.name.startswith("book1")


def differing_share(want_a, want_1, chains):
    """-> (blocks whose reference bytes at the acceleration differ from the reference's acceleration-1 bytes of the same block of the same
    chain, blocks) over book1 blocks of 1000 bytes and more that both runs compressed"""
    differ = total = 0
    for ch, (oa, _, ba), (o1, _, b1) in zip(chains, want_a, want_1):
        if not is_book1_big(ch):
            continue
        for (s, _), ra, r1, xa, x1 in zip(ch.blocks, oa, o1, ba, b1):
            if len(s) >= 1000 and ra > 0 and r1 > 0:
                total += 1
                differ += xa != x1
    return differ, total


def state_of(st):
    """(currentOffset, min(dictSize, 64 KB)) of the reference's LZ4_stream_t (1.9.3's LZ4_stream_t_internal)"""
    return C.c_uint32.from_address(st + OFF_CUR).value, min(C.c_uint32.from_address(st + OFF_DSIZE).value, 65536)


def drive_lives(engine, rc, lives, rng, absent=0.5, ids=None, keep=None):
    """cstream_common.drive with the record check: behind every call the engine's record of every stream that took part and still runs
    holds the reference stream's currentOffset and min(dictSize, 64 KB) (engine.state_is).  The acceleration of a round is rc.plan.now;
    the engine steps the plan.  -> (mismatches, per life the reference's results call by call, rounds)"""
    ids = list(range(len(lives))) if ids is None else list(ids)
    refs = [S.RefStream(rc, lf.history) for lf in lives]
    nxt = [0] * len(lives)
    results = [[] for _ in lives]
    bad, rounds = [], 0
    while any(nxt[i] < len(lf.calls) for i, lf in enumerate(lives)):
        todo = [i for i, lf in enumerate(lives) if nxt[i] < len(lf.calls)]
        now = [i for i in todo if rng.random() >= absent] or todo[:1]
        parts, want, states = [], [], []
        for i in now:
            call = lives[i].calls[nxt[i]]
            front, plen = refs[i].front(call)
            parts.append((front, plen, call))
            want.append(refs[i].run(call))
            states.append(state_of(refs[i].st) if refs[i].alive else None)
            results[i].append(want[-1])
            nxt[i] += 1
        pk = S.PackedCall(parts, rng)
        accel = rc.plan.now
        dst, out, cons = engine.call([ids[i] for i in now], pk)
        bad += [(rounds, accel) + b for b in pk.check([lives[i].name for i in now], dst, out, cons, want)]
        for i, st in zip(now, states):
            if st is not None and not engine.state_is(ids[i], st):
                bad.append((rounds, accel, lives[i].name, "record", st))
        if keep is not None:
            keep.append((rounds, [ids[i] for i in now], now, pk, [int(v) for v in out[:pk.n_blocks]], dst))
        rounds += 1
        if len(bad) > 20:
            break
    for r in refs:
        r.close()
    return bad, results, rounds


# ---- the engines behind the C ABI ----
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


def chain_accel_call(L, pk, accel, prefix=True):
    """lz4hip_compress_fast_chain_accel_batch on a CPacked -> (status, dst, out_len, chain_consumed)"""
    a64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    a32 = lambda v, t=np.int32: np.ascontiguousarray(v, dtype=t)
    cso, pre, sl, cf = a64(pk.chain_src_off), a32(pk.prefix), a32(pk.src_len), a32(pk.chain_first, np.uint32)
    do, dc = a64(pk.dst_off), a32(pk.dst_cap)
    out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
    src = C.create_string_buffer(pk.src, len(pk.src))
    dst = C.create_string_buffer(bytes(pk.dst), len(pk.dst))
    f = L.lz4hip_compress_fast_chain_accel_batch
    f.argtypes, f.restype = [C.c_void_p] * 10 + [C.c_uint32, C.c_uint32, C.c_int], C.c_int
    rc = f(C.addressof(src), cso.ctypes.data, pre.ctypes.data if prefix else None, sl.ctypes.data, cf.ctypes.data, C.addressof(dst), do.ctypes.data,
           dc.ctypes.data, out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains, accel)
    assert src.raw == pk.src
    return rc, dst.raw, out, cons


def stream_call(l, h, ids, pk, accel, existing=False, expect=0):
    """one call on the set h through lz4hip_compress_fast_stream_accel_batch at `accel`, or (existing, acceleration 1) through
    lz4hip_compress_fast_stream_batch -> (dst, out_len, chain_consumed)"""
    sid = np.ascontiguousarray(ids, dtype=np.uint32)
    src = C.create_string_buffer(pk.src, len(pk.src))
    dst = C.create_string_buffer(bytes(pk.dst), len(pk.dst))
    cso, pre, sl, cf, do, dc = pk.arrays()
    out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
    args = [h, sid.ctypes.data, C.addressof(src), cso.ctypes.data, pre.ctypes.data, sl.ctypes.data, cf.ctypes.data, C.addressof(dst), do.ctypes.data,
            dc.ctypes.data, out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains]
    if existing:
        assert accel == 1
        f = l.lz4hip_compress_fast_stream_batch
        f.argtypes, f.restype = [C.c_void_p] * 12 + [C.c_uint32, C.c_uint32], C.c_int
    else:
        f = l.lz4hip_compress_fast_stream_accel_batch
        f.argtypes, f.restype = [C.c_void_p] * 12 + [C.c_uint32, C.c_uint32, C.c_int], C.c_int
        args.append(accel)
    rc = f(*args)
    assert rc == expect, (rc, l.lz4hip_last_error())
    assert src.raw == pk.src
    return dst.raw, out, cons


class DevAccel(S.DevEngine):
    """a set of n resident streams behind the C ABI: every call goes through lz4hip_compress_fast_stream_accel_batch at plan.now, or --
    every other call at acceleration 1 -- through the existing lz4hip_compress_fast_stream_batch"""

    def __init__(self, amd, n, plan):
        super().__init__(amd, n)
        self.plan, self.ones = plan, 0

    def call(self, ids, pk, expect=0):
        accel = self.plan.now
        self.ones += accel == 1
        res = stream_call(self.l, self.h, ids, pk, accel, existing=(accel == 1 and self.ones & 1), expect=expect)
        self.plan.step()
        return res

    def state_is(self, i, state):
        """(the record lives on the device: what the C ABI shows of it is lz4hip_cstreams_consumed, which the tests check)"""
        return True


class DevAccelX(X.DevX):
    """the same set driven through lz4hip_compress_fast_stream_ext_accel_batch at plan.now, or -- every other call at acceleration 1 --
    through the existing lz4hip_compress_fast_stream_ext_batch"""

    def __init__(self, amd, n, plan):
        super().__init__(amd, n)
        self.plan, self.ones = plan, 0

    def call(self, ids, pk, expect=0):
        accel = self.plan.now
        if accel == 1:
            self.ones += 1
            if self.ones & 1:
                self.plan.step()
                return super().call(ids, pk, expect)
        sid = np.ascontiguousarray(ids, dtype=np.uint32)
        src = C.create_string_buffer(pk.src, len(pk.src))
        dst = C.create_string_buffer(bytes(pk.dst), len(pk.dst))
        so, sl, cf, he, hl, wo, wl, do, dc = pk.arrays()
        out, cons = np.full(max(pk.n_blocks, 1), 12345, np.int32), np.full(max(pk.n_chains, 1), 12345, np.uint64)
        f = self.l.lz4hip_compress_fast_stream_ext_accel_batch
        f.argtypes, f.restype = X.EXT_ARGTYPES + [C.c_int], C.c_int
        rc = f(self.h, sid.ctypes.data, C.addressof(src), so.ctypes.data, sl.ctypes.data, cf.ctypes.data, he.ctypes.data, hl.ctypes.data, wo.ctypes.data,
               wl.ctypes.data, C.addressof(dst), do.ctypes.data, dc.ctypes.data, out.ctypes.data, cons.ctypes.data, pk.n_blocks, pk.n_chains, accel)
        assert rc == expect, (rc, self.l.lz4hip_last_error())
        assert src.raw == pk.src
        self.plan.step()
        return dst.raw, out, cons

    def call_prefix(self, ids, pk, expect=0):
        """the prefix-mode entry points on the SAME set (the blocks follow their history): lz4hip_compress_fast_stream_accel_batch at
        plan.now, or -- every other call at acceleration 1 -- the existing lz4hip_compress_fast_stream_batch"""
        accel = self.plan.now
        self.prefix_ones = getattr(self, "prefix_ones", 0) + (accel == 1)
        res = stream_call(self.l, self.h, ids, pk, accel, existing=(accel == 1 and self.prefix_ones & 1), expect=expect)
        self.plan.step()
        return res


# ---- one small well-formed call per entry point (the argument-error tests) ----
NAMES = {"lz4hip_compress_fast_chain_accel_batch": "lz4hip_compress_fast_chain_batch",
         "lz4hip_compress_fast_stream_accel_batch": "lz4hip_compress_fast_stream_batch",
         "lz4hip_compress_fast_stream_ext_accel_batch": "lz4hip_compress_fast_stream_ext_batch"}


class ChainCall:
    """one well-formed call of the chain entry: two chains of 2 + 1 blocks"""

    def __init__(self):
        self.src = C.create_string_buffer(b"abcdefgh" * 8, 64)
        self.dst = C.create_string_buffer(b"\x07" * 256, 256)
        self.cso, self.pre = (u64 * 2)(4, 40), (i32 * 2)(4, 0)
        self.sl, self.first = (i32 * 3)(10, 10, 16), (u32 * 3)(0, 2, 3)
        self.doff, self.dc = (u64 * 3)(0, 64, 128), (i32 * 3)(40, 40, 40)
        self.out, self.cons = (i32 * 3)(5, 5, 5), (u64 * 2)(9, 9)

    def args(self, accel=None, **kw):
        a = dict(src=self.src, cso=self.cso, pre=self.pre, sl=self.sl, first=self.first, dst=self.dst, doff=self.doff, dc=self.dc, out=self.out,
                 cons=self.cons, n_blocks=3, n_chains=2)
        a.update(kw)
        v = [a[k] for k in ("src", "cso", "pre", "sl", "first", "dst", "doff", "dc", "out", "cons", "n_blocks", "n_chains")]
        return v if accel is None else v + [accel]

    def untouched(self):
        return self.dst.raw == b"\x07" * 256 and list(self.out) == [5, 5, 5] and list(self.cons) == [9, 9]


class StreamCall:
    """one well-formed call of the resident-stream entry apart from its set: streams 0 and 1 with 2 + 1 blocks"""
    ORDER = ("set", "ids", "src", "cso", "pre", "sl", "first", "dst", "doff", "dc", "out", "cons", "n_blocks", "n_chains")

    def __init__(self):
        c = ChainCall()
        self.v = dict(set=None, ids=(u32 * 2)(0, 1), src=c.src, cso=c.cso, pre=c.pre, sl=c.sl, first=c.first, dst=c.dst, doff=c.doff, dc=c.dc, out=c.out,
                      cons=c.cons, n_blocks=3, n_chains=2)
        self.untouched = c.untouched

    def args(self, accel=None, **kw):
        a = dict(self.v)
        a.update(kw)
        v = [a[k] for k in self.ORDER]
        return v if accel is None else v + [accel]


class ExtCall(StreamCall):
    """the same for the entry whose sources land anywhere: stream 0 in the window [8, 40) without a history, stream 1 in [40, 72) behind 4
    bytes that end at 48"""
    ORDER = ("set", "ids", "src", "src_off", "sl", "first", "hist_end", "hist_len", "win_off", "win_len", "dst", "doff", "dc", "out", "cons", "n_blocks", "n_chains")

    def __init__(self):
        super().__init__()
        self.v.update(src=C.create_string_buffer(bytes(range(96)), 96), src_off=(u64 * 3)(8, 30, 60), sl=(i32 * 3)(4, 4, 4), hist_end=(u64 * 2)(0, 48),
                      hist_len=(i32 * 2)(0, 4), win_off=(u64 * 2)(8, 40), win_len=(u64 * 2)(32, 32))


def overlapping_streams(rng, n_streams):
    """a block, then a block whose source begins INSIDE the first one and runs past its end (liblz4's trim catches only a source that ends
    inside its history): external-dictionary mode against a history whose second half the block's own bytes have replaced.  Small
    alphabets, so that buckets collide and short matches abound.  (The generator of tests/test_cxstream_hostsim.py, restated: test
    modules do not import each other.)"""
    out = []
    for t in range(n_streams):
        alpha = bytes(rng.sample(range(256), rng.choice((2, 3, 4, 8))))
        text = lambda n: bytes(rng.choice(alpha) for _ in range(n))
        n0 = rng.randrange(200, 1500)
        s1 = rng.randrange(1, n0 - 12)       # (not 0: a source that begins exactly where its history does is the header's exception)
        blocks = [X.XBlock(0, text(n0)), X.XBlock(s1, text(rng.randrange(n0 - s1, 2500))), X.XBlock(3000, text(300))]
        out.append(X.XStream("overlap #%d" % t, "hand", 8192, blocks))
    return out
