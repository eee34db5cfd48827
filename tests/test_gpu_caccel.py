"""The accelerated linked-block compressors on the device (lz4hip_compress_fast_chain_accel_batch, lz4hip_compress_fast_stream_accel_batch,
lz4hip_compress_fast_stream_ext_accel_batch: compress_fast_chain_accel_cu_kernel, compress_fast_stream_accel_cu_kernel,
compress_fast_xstream_accel_cu_kernel) against the reference library's LZ4_compress_fast_continue on ONE LZ4_stream_t per chain or stream
at the same accelerations (tests/caccel_common.py); every slot lies between guard bytes.  The existing entry points take the calls at
acceleration 1 in turn with the new ones, on the same sets."""
import ctypes as C
import importlib
import io
import random
import struct
import threading

import numpy as np
import pytest

import cstream_common as S
import cxstream_common as X
from caccel_common import AccelPlan, DevAccel, DevAccelX, RefAccelChain, RefAccelX, chain_accel_call, chain_cases, drive_lives, tight_cases
from cchain_common import CHAIN_STOPPED, CPacked, batched_linked_frame, book1, bound, chain_of
from support import run_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rc(ref):
    return RefAccelChain(ref)


@pytest.fixture(scope="module")
def chains():
    return chain_cases()


def decode_chains(amd, pk, dst, out):
    """every chain that ran to its end back through lz4hip_decompress_safe_chain_batch, behind its history -> the decoded sources"""
    src, so, sl, caps, first, dbuf, cdo, cdc, pre, names = bytearray(), [], [], [], [0], bytearray(), [], [], [], []
    for c, ch in enumerate(pk.chains):
        b0, b1 = pk.chain_first[c], pk.chain_first[c + 1]
        if any(int(out[i]) <= 0 for i in range(b0, b1)):
            continue
        hist = ch.history[-65536:]
        dbuf += hist
        cdo.append(len(dbuf)); cdc.append(len(ch.data)); pre.append(len(hist)); names.append(ch)
        dbuf += bytes(len(ch.data))
        for i in range(b0, b1):
            so.append(len(src)); sl.append(int(out[i])); caps.append(pk.src_len[i])
            src += dst[pk.dst_off[i]:pk.dst_off[i] + int(out[i])]
        first.append(len(so))
    got, dn = amd.LZ4HIPBatch.decompressSafeChain(bytes(src), so, sl, caps, first, dbuf, cdo, cdc, pre)
    assert list(got) == caps and list(dn) == cdc
    for ch, o, n in zip(names, cdo, cdc):
        assert bytes(dbuf[o:o + n]) == ch.data, ch.name
    return len(names)


@pytest.mark.parametrize("accel", [2, 8, 65537])
def test_chains(amd, rc, chains, accel):
    """the simulator test's chains (the 200000-byte chain once) and their tight twins, at least 64 per call: bytes, values, consumed
    sizes, guards; every chain that ran to its end goes back through the chain decoder to its source"""
    part = list(chains) + tight_cases(rc, [c for c in chains if len(c.data) <= 70000 and len(c.blocks) > 1], accel)
    assert len(part) >= 64 and sum(c.name.startswith("book1 200000") for c in part) == 1
    want = [rc.at(accel).compress(c) for c in part]
    pk = CPacked(part)
    status, dst, out, cons = chain_accel_call(amd.lib(), pk, accel)
    assert status == 0, amd.lib().lz4hip_last_error()
    bad = pk.check(dst, out, cons, want)
    assert not bad, (accel, len(bad), bad[:5])
    assert decode_chains(amd, pk, dst, out) >= 40
    # the Python layer's keyword is the same call
    d2 = bytearray(pk.dst)
    o2, c2 = amd.LZ4HIPBatch.compressFastChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, d2, pk.dst_off, pk.dst_cap, pk.prefix, acceleration=accel)
    assert bytes(d2) == dst and list(o2) == [int(v) for v in out[:pk.n_blocks]] and list(c2) == [int(v) for v in cons[:pk.n_chains]]


def test_clamps(amd, rc, chains):
    """acceleration 0 gives the bytes of lz4hip_compress_fast_chain_batch, 70000 those of acceleration 65537"""
    part = [c for c in chains if c.name in ("book1 16 x 4096", "geo 16 x 1000", "book1 prefix 4096, 6 x 1000", "pic 16 x 4096")]
    pk = CPacked(part)
    L = amd.lib()
    plain = bytearray(pk.dst)
    o1, c1 = amd.LZ4HIPBatch.compressFastChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, plain, pk.dst_off, pk.dst_cap, pk.prefix)
    res = {a: chain_accel_call(L, pk, a) for a in (0, -7, 1, 70000, 1 << 30, 65537)}
    assert all(r[0] == 0 for r in res.values())
    for a in (0, -7, 1):
        assert res[a][1] == bytes(plain) and [int(v) for v in res[a][2][:pk.n_blocks]] == list(o1), a
    for a in (70000, 1 << 30):
        assert res[a][1] == res[65537][1] and list(res[a][2]) == list(res[65537][2]), a
    assert res[65537][1] != bytes(plain)
    assert not pk.check(res[0][1], res[0][2], res[0][3], [rc.at(1).compress(c) for c in part])
    assert not pk.check(res[70000][1], res[70000][2], res[70000][3], [rc.at(65537).compress(c) for c in part])


def recut(life, rng, lo=2, hi=6):
    blocks = [b for c in life.calls for b in c.blocks]
    k = min(len(blocks), rng.randrange(lo, hi + 1))
    cuts = sorted(rng.sample(range(1, len(blocks)), k - 1)) if k > 1 else []
    edges = [0] + cuts + [len(blocks)]
    life.calls = [S.Call(blocks[a:b]) for a, b in zip(edges, edges[1:])]
    return life


def test_resident_streams(amd, rc, O):
    """64 streams in 2 .. 6 calls at changing accelerations, the new and the existing entry point alternating on one set;
    lz4hip_cstreams_consumed; then a stop by a tight capacity and a reset after it"""
    rng = random.Random(171)
    b = book1()
    lives = [recut(S.random_life(rng, O, "stream %d" % i, rng.randrange(8, 30), 3000, history=(b[9000 - P:9000] if (P := (0, 0, 5, 3000)[i % 4]) else b"")), rng)
             for i in range(62)]
    lives.append(recut(S.life_of("150 x 2 KiB", b[4321:4321 + 150 * 2048], [2048] * 150, ()), rng))
    lives.append(recut(S.life_of("book1 20 x 4096", b[100000:100000 + 20 * 4096], [4096] * 20, ()), rng))
    assert len(lives) == 64 and all(2 <= len(l.calls) <= 6 for l in lives)
    plan = rc.plan
    plan.pattern, plan.k, plan.used = (8, 1, 64, 1, 2, 3), 0, []
    eng = DevAccel(amd, 70, plan)
    try:
        ids = sorted(random.Random(172).sample(range(70), 64))
        bad, results, rounds = drive_lives(eng, rc, lives, random.Random(173), absent=0.5, ids=ids)
        assert not bad, (len(bad), bad[:5])
        assert rounds >= 6 and {1, 2, 3, 8, 64} <= set(plan.used) and eng.ones >= 2
        cons, stop = eng.consumed()
        for i, lf in zip(ids, lives):
            assert cons[i] == sum(len(c.data) for c in lf.calls) and not stop[i], lf.name
        assert all(cons[i] == 0 for i in range(70) if i not in ids)
        # a capacity one byte short of the reference's result at acceleration 8 stops the stream; a reset makes it fresh
        free = [i for i in range(70) if i not in ids][:2]
        plan.pattern, plan.k = (8,), 0
        probe = S.RefStream(rc)
        exact = probe.run(S.Call([(b[:1000], bound(1000)), (b[1000:2000], bound(1000))]))[0]
        probe.close()
        tight = S.Life("tight", [S.Call([(b[:1000], bound(1000)), (b[1000:2000], exact[1] - 1), (b[2000:3000], bound(1000))]), S.Call([(b[3000:4000], bound(1000))])])
        beside = S.life_of("beside it", b[7000:11000], [1000] * 4, (2,))
        plan.pattern, plan.k = (8, 3), 0
        bad, results, _ = drive_lives(eng, rc, [tight, beside], random.Random(174), absent=0.0, ids=free)
        assert not bad, bad
        assert [r for c in results[0] for r in c[0]] == [exact[0], 0, CHAIN_STOPPED, CHAIN_STOPPED]
        assert eng.consumed(free[0], 1) == ([1000], [1]) and eng.consumed(free[1], 1) == ([4000], [0])
        eng.reset([free[0]])
        assert eng.consumed(free[0], 1) == ([0], [0])
        plan.pattern, plan.k = (2, 1), 0
        bad, results, _ = drive_lives(eng, rc, [S.life_of("after the reset", b[:4000], [1000] * 4, (2,))], random.Random(175), absent=0.0, ids=free[:1])
        assert not bad and all(r > 0 for c in results[0] for r in c[0])
    finally:
        eng.close()


@pytest.mark.parametrize("layout,pattern", [("two4096", (3, 1, 64)), ("ring73727", (64, 3, 1)), ("dict4096", (3, 64, 1, 1))])
def test_ext_streams(amd, ref, layout, pattern):
    """64 streams per layout at accelerations 3 and 64, lz4hip_compress_fast_stream_ext_accel_batch and the existing
    lz4hip_compress_fast_stream_ext_batch alternating on one set (the prefix-mode entry points join them in
    test_prefix_and_ext_entry_points_alternate_on_one_set); all 64 ring and two-buffer streams go back through DecodeStreams into windows
    of the same layout"""
    rng = random.Random(181 + len(layout))
    data = book1()
    n = 64
    streams = [X.make_xstream(layout, rng, data, "#%d" % t) for t in range(n)]
    plan = AccelPlan(pattern)
    rs = RefAccelX(ref, plan)
    eng = DevAccelX(amd, n + 2, plan)
    try:
        ids = sorted(rng.sample(range(n + 2), n))
        keep = []
        bad, made, rounds = X.drive_x(eng, rs, streams, rng, mode="random", ids=ids, keep=keep)
        assert not bad, (len(bad), bad[:5])
        assert {3, 64, 1} <= set(plan.used) and eng.ones >= 2
        cons, stop = eng.consumed()
        assert [cons[i] for i in ids] == [sum(len(b.data) for b in xs.blocks) for xs in streams] and not any(stop)
    finally:
        eng.close()
    if layout in ("ring73727", "two4096"):
        # back through the stream decoder: every stream's blocks into a window of the same layout, block k of every stream in one call
        sel = list(range(n))
        ds = amd.DecodeStreams(len(sel))
        win = streams[0].win_len
        back = bytearray(len(sel) * win)
        nb = max(len(streams[i].blocks) for i in sel)
        for k in range(nb):
            now = [j for j, i in enumerate(sel) if k < len(streams[i].blocks)]
            comp = [[x for c in made[sel[j]] for x in c.by][k] for j in now]
            blk = [streams[sel[j]].blocks[k] for j in now]
            src = b"".join(comp)
            so = np.concatenate([[0], np.cumsum([len(x) for x in comp])[:-1]]).astype(np.uint64).tolist()
            r = ds.decompress(now, src, so, [len(x) for x in comp], list(range(len(now) + 1)), back, [j * win + b.off for j, b in zip(now, blk)],
                              [len(b.data) for b in blk], [j * win for j in now], [win] * len(now))
            assert list(r) == [len(b.data) for b in blk], k
            for j, b in zip(now, blk):
                assert bytes(back[j * win + b.off:j * win + b.off + len(b.data)]) == b.data, (streams[sel[j]].name, k)


def test_prefix_and_ext_entry_points_alternate_on_one_set(amd, ref):
    """64 streams of 16 blocks, back to back but for every fourth block, which jumps to a place of its own: the jumps and some of the
    blocks that follow their history go through lz4hip_compress_fast_stream_ext_accel_batch / lz4hip_compress_fast_stream_ext_batch, the
    other blocks that follow their history through lz4hip_compress_fast_stream_accel_batch / lz4hip_compress_fast_stream_batch -- all
    four entry points on the SAME streams, one block of every stream per call, the acceleration changing from call to call.  The bytes
    are ONE LZ4_stream_t's"""
    from dstream_common import cut_pieces
    data = book1()
    rng = random.Random(193)
    n = 64
    plan = AccelPlan((8, 1, 64, 2, 1, 3))
    rs = RefAccelX(ref, plan)
    streams, offsets = [], []
    for t in range(n):
        pieces = cut_pieces(data, rng, 16, 1, 3000)
        offs, pos = [], 0
        for k, p in enumerate(pieces):
            if k and k % 4 == 0:
                pos += 5000
            offs.append(pos); pos += len(p)
        streams.append(X.XStream("alternating %d" % t, "contig", pos + 16, [X.XBlock(o, p) for o, p in zip(offs, pieces)]))
        offsets.append(offs)
    refs = [X.RefX(rs, xs) for xs in streams]
    eng = DevAccelX(amd, n, plan)
    kinds = []
    try:
        for k in range(16):
            calls = [r.next_call(k + 1) for r in refs]
            assert all(c.k1 == k + 1 for c in calls)
            jump = k and k % 4 == 0
            if jump or (k % 2 == 0 and k % 4 != 1):
                pk = X.PackedX(calls, rng)
                dst, out, cons = eng.call(list(range(n)), pk)
                bad = pk.check([xs.name for xs in streams], dst, out, cons)
                kinds.append("ext")
            else:
                parts = []
                for r, c, xs, offs in zip(refs, calls, streams, offsets):
                    s = r.win_off + offs[k]
                    assert c.hist_end in (s, 0)
                    blk = xs.blocks[k]
                    parts.append((c.arena[s - c.hist_len:s], c.hist_len, S.Call([(blk.data, blk.cap)])))
                pk = S.PackedCall(parts, rng)
                dst, out, cons = eng.call_prefix(list(range(n)), pk)
                bad = pk.check([xs.name for xs in streams], dst, out, cons, [(c.outs, c.consumed, c.by) for c in calls])
                kinds.append("prefix")
            assert not bad, (k, kinds[-1], len(bad), bad[:5])
        assert kinds.count("ext") >= 6 and kinds.count("prefix") >= 6 and {1, 2, 3, 8, 64} <= set(plan.used) and eng.ones >= 2 and eng.prefix_ones >= 2
        # (both kinds of call ran at acceleration 1 -- through the existing entry point and through the new one -- and above it)
        by_kind = {(kd, a > 1) for kd, a in zip(kinds, plan.used)}
        assert by_kind == {("ext", False), ("ext", True), ("prefix", False), ("prefix", True)}, sorted(by_kind)
        cons, stop = eng.consumed()
        assert cons == [sum(len(b.data) for b in xs.blocks) for xs in streams] and not any(stop)
    finally:
        eng.close()
        for r in refs:
            r.close()


def test_3000_streams_three_calls_of_one_block_at_8(amd, rc, monkeypatch):
    """the host call with 1 MiB chunks (LZ4HIP_HOST_CHUNK_MB=1, read per call): 3000 streams x 1 KiB are three chunks in the first call
    and, with every stream's history in front of its block, six and nine in the second and third; more streams than resident wavefronts,
    every stream in every call, acceleration 8.  A chunk launched at another acceleration, a slot taken from the wrong chain of a later
    chunk, a table carried into the next stream a wavefront draws, or a state saved to the wrong slot changes bytes"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    n = 3000
    rng = random.Random(191)
    b = book1()
    noise = rng.randbytes(1 << 19)
    datas = []
    for i in range(n):
        o = (i * 113) % 600000
        own = noise[i * 160:i * 160 + 160]
        d0 = (own + b[o:o + 1024])[:1024]
        d1 = (d0[40:200] + b[o + 2000:o + 3024])[:1024]
        d2 = (d1[:120] + own[::-1] + d0[100:260] + b[o + 4000:o + 5024])[:1024]
        datas.append((d0, d1, d2))
    L = rc.at(8).L
    want = []
    for i in range(n):
        buf = C.create_string_buffer(b"".join(datas[i]), 3072)
        st = L.LZ4_createStream()
        res = []
        for k in range(3):
            d = C.create_string_buffer(bound(1024))
            r = L.LZ4_compress_fast_continue(st, C.addressof(buf) + 1024 * k, d, 1024, bound(1024), 1)      # (the handle passes 8)
            res.append(d.raw[:r])
        L.LZ4_freeStream(st)
        want.append(res)
    with amd.CompressStreams(n) as streams:
        ids = np.arange(n, dtype=np.uint32)
        for k in range(3):
            hist = [b"".join(d[:k]) for d in datas]
            src = b"".join(h + d[k] for h, d in zip(hist, datas))
            lens = np.full(n, 1024, np.int32)
            pre = np.array([len(h) for h in hist], np.int32)
            cso = (np.cumsum(np.concatenate([[0], (lens + pre)[:-1]])) + pre).astype(np.uint64)
            caps = np.full(n, bound(1024), np.int32)
            do = np.concatenate([[0], np.cumsum(caps + 3)[:-1]]).astype(np.uint64)
            dst = bytearray(b"\xA5" * int(np.sum(caps + 3)))
            out, cons = streams.compress(ids, src, cso, lens, np.arange(n + 1, dtype=np.uint32), dst, do, caps, pre, acceleration=8)
            assert list(cons) == list(lens) and len(src) > (2 + 3 * k) << 20      # (several chunks of 1 MiB)
            wrong = [i for i in range(n) if out[i] != len(want[i][k]) or bytes(dst[int(do[i]):int(do[i]) + int(out[i])]) != want[i][k]]
            assert not wrong, (k, len(wrong), wrong[:8])
        cons, stop = streams.consumed()
        assert cons == [3072] * n and not any(stop)


def test_threads(amd, ref, O):
    """two host threads on two sets, each at its own changing accelerations"""
    res = {}

    def work(key, pattern, seed):
        try:
            rng = random.Random(seed)
            rcx = RefAccelChain(ref, AccelPlan(pattern))
            lives = [S.random_life(rng, O, "%s %d" % (key, i), rng.randrange(3, 9), 2000, every_boundary=True) for i in range(12)]
            eng = DevAccel(amd, 12, rcx.plan)
            try:
                res[key] = drive_lives(eng, rcx, lives, rng, absent=0.3)[0]
            finally:
                eng.close()
        except BaseException as e:      # (an assertion in a thread is a failure of the test)
            res[key] = [("exception", repr(e))]
    th = [threading.Thread(target=work, args=("a", (8, 1, 2), 1)), threading.Thread(target=work, args=("b", (64, 3, 1), 2))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res == {"a": [], "b": []}, {k: v[:3] for k, v in res.items()}


def test_set_divided_over_device_entries():
    """the set's streams divided over the engine's devices, and accelerated calls sharded at those boundaries: device 0 listed twice"""
    assert "caccel multidev ok" in run_child("caccel_multidev_child.py", 2, timeout=120)


@pytest.mark.parametrize("stream_state", [False, True])
def test_frame_writer(amd, rc, port, stream_state):
    """LZ4FrameOutputStream(linkedBlocks=True, acceleration=8) on 300 KB of book1 in 64 KiB blocks: LZ4FrameInputStream(linkedBlocks=True)
    reads it back, and each block's payload is the reference stream's bytes at acceleration 8; with and without streamState"""
    F = importlib.import_module("lz4-java_amd.streams")
    data = book1()[20000:20000 + 300000]
    sink = io.BytesIO()
    w = F.LZ4FrameOutputStream(sink, 4, -1, linkedBlocks=True, acceleration=8, streamState=stream_state)
    w.write(data)
    w.close()
    frame = sink.getvalue()
    assert F.LZ4FrameInputStream(io.BytesIO(frame), linkedBlocks=True).read() == data
    sizes = [65536] * 4 + [300000 - 4 * 65536]
    outs, done, by = rc.at(8).compress(chain_of("frame", data, sizes))
    assert done == len(data) and by != rc.at(1).compress(chain_of("frame", data, sizes))[2]
    pos, payloads = 7, []
    while True:
        (word,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        if word == 0:
            break
        payloads.append(frame[pos:pos + (word & 0x7FFFFFFF)])
        pos += word & 0x7FFFFFFF
    assert payloads == by
    assert frame == batched_linked_frame(rc.at(8), port.xxh32, data, 4, 10 ** 6)
    # the default is the frame it was
    sink = io.BytesIO()
    w = F.LZ4FrameOutputStream(sink, 4, -1, linkedBlocks=True, streamState=stream_state)
    w.write(data)
    w.close()
    assert sink.getvalue() == batched_linked_frame(rc.at(1), port.xxh32, data, 4, 10 ** 6) != frame


def test_helper_programs(rc, port, tmp_path):
    """tests/cpp/caccel_mirror_test.cpp (LZ4HIPBatch::compressFastChain, CompressStreams::compress in two calls and compressAt of
    host/lz4hip.hpp at an acceleration, which must agree; the frame writer twin with acceleration(8)) and tests/jni_stub/fake_jni_caccel.c
    (the three accelerated natives over the fake JNIEnv): values and bytes are the reference's at that acceleration"""
    import subprocess
    from cchain_common import cchain_file
    from support import build_fake_jni, build_mirror
    b = book1()
    ch = chain_of("helper", b[30100:30100 + 9000], [1000, 2000, 13, 5, 3000, 2982], history=b[30000:30100])
    (tmp_path / "c.bin").write_bytes(cchain_file(ch))
    exe = build_mirror("caccel_mirror_test", tmp_path, werror=True)
    jni = build_fake_jni("fake_jni_caccel", tmp_path)
    for accel in (8, 65537):
        outs, done, by = rc.at(accel).compress(ch)
        line = " ".join(str(r) for r in outs) + " | %d" % done
        out = subprocess.check_output([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin"), str(accel)], timeout=120).decode()
        assert out.split() == line.split() and (tmp_path / "o.bin").read_bytes() == b"".join(by), accel
        out = subprocess.check_output([jni, str(tmp_path / "c.bin"), str(tmp_path), str(accel)], timeout=120).decode()
        assert "checks ok" in out, out
        assert (tmp_path / "caccel.txt").read_text().split() == line.split() and (tmp_path / "caccel.out").read_bytes() == b"".join(by), accel
    data = b[20000:20000 + 300000]
    (tmp_path / "d.bin").write_bytes(data)
    want = batched_linked_frame(rc.at(8), port.xxh32, data, 4, 10 ** 6)
    for state in (0, 1):
        subprocess.check_output([exe, "--frame", str(tmp_path / "d.bin"), str(tmp_path / "f.bin"), "8", str(state)], timeout=120)
        assert (tmp_path / "f.bin").read_bytes() == want, state


def test_argument_errors_with_a_live_set(amd):
    """against a set that exists, the accelerated stream entries refuse what their twins refuse, with the twins' message: a NULL array,
    ids that are >= n_streams or do not ascend, a source outside its window; nothing is written, no stream is touched; then the
    well-formed call goes through"""
    from support import E_ARG
    from caccel_common import ExtCall, NAMES, StreamCall
    l = amd.lib()
    h = C.c_void_p(None)
    assert l.lz4hip_cstreams_create(2, C.byref(h)) == 0, l.lz4hip_last_error()
    u = lambda *v: (C.c_uint32 * len(v))(*v)
    try:
        for name, c, kws in (("lz4hip_compress_fast_stream_accel_batch", StreamCall(), [{"out": None}, {"ids": u(0, 2)}, {"ids": u(1, 1)}, {"first": u(0, 3, 2)}]),
                             ("lz4hip_compress_fast_stream_ext_accel_batch", ExtCall(),
                              [{"cons": None}, {"ids": u(2, 3)}, {"ids": u(1, 0)}, {"src_off": (C.c_uint64 * 3)(8, 37, 60)}])):
            f, twin = getattr(l, name), getattr(l, NAMES[name])
            for kw in kws:
                assert twin(*c.args(set=h, **kw)) == E_ARG, (name, kw)
                msg = l.lz4hip_last_error()
                assert f(*c.args(8, set=h, **kw)) == E_ARG and l.lz4hip_last_error() == msg, (name, kw, msg)
            assert c.untouched()
            cons, stop = (C.c_uint64 * 2)(), (C.c_uint8 * 2)()
            assert l.lz4hip_cstreams_consumed(h, 0, 2, cons, stop) == 0 and list(cons) == [0, 0] and list(stop) == [0, 0]
            assert f(*c.args(8, set=h)) == 0, l.lz4hip_last_error()
            assert all(r > 0 for r in c.v["out"])
            assert l.lz4hip_cstreams_reset(h, None, 0) == 0
    finally:
        l.lz4hip_cstreams_free(h)
