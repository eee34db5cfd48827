"""The resident-stream compressor on the device (lz4hip_cstreams_* / lz4hip_compress_fast_stream_batch, compress_fast_stream_cu_kernel)
against ONE LZ4_stream_t of the reference library per stream (tests/cstream_common.py) and against lz4hip_compress_fast_chain_batch on
the same blocks in one call; every slot lies between 128 guard bytes at odd addresses."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

from cchain_common import CPacked, book1
from cstream_common import (CHAIN_STOPPED, Call, DevEngine, PackedCall, RefCChain, RefStream, bound, drive, life_of, random_life, small_first_lives,
                            truncation_lives)
from support import E_ARG, run_child

pytestmark = pytest.mark.gpu
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


def chain_call(amd, pk):
    """lz4hip_compress_fast_chain_batch on a cchain_common.CPacked -> (dst, out, consumed)"""
    dst = bytearray(pk.dst)
    out, cons = amd.LZ4HIPBatch.compressFastChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, dst, pk.dst_off, pk.dst_cap, pk.prefix)
    return bytes(dst), out, cons


def recut(life, rng, lo=2, hi=6):
    """the life's blocks cut into lo .. hi calls at random block boundaries"""
    blocks = [b for c in life.calls for b in c.blocks]
    k = min(len(blocks), rng.randrange(lo, hi + 1))
    cuts = sorted(rng.sample(range(1, len(blocks)), k - 1)) if k > 1 else []
    edges = [0] + cuts + [len(blocks)]
    life.calls = [Call(blocks[a:b]) for a, b in zip(edges, edges[1:])]
    return life


@pytest.fixture(scope="module")
def sixty_four(rc, O):
    """64 streams: 60 of 8 .. 40 blocks of 0 .. 3000 bytes, four of 150 x 2 KiB (their history passes 64 KB), in 2 .. 6 calls each"""
    rng = random.Random(71)
    lives = [recut(random_life(rng, O, "stream %d" % i, rng.randrange(8, 41), 3000, history=(book1()[9000 - P:9000] if (P := (0, 0, 5, 3000)[i % 4]) else b"")), rng)
             for i in range(60)]
    b = book1()
    for i in range(4):
        o = 100000 * i + 4321
        lives.insert(16 * i, recut(life_of("150 x 2 KiB %d" % i, b[o:o + 150 * 2048], [2048] * 150, ()), rng))
    return lives


def test_64_streams_against_the_reference_and_the_one_call_chain(amd, rc, sixty_four):
    """half of the unfinished streams absent from every call; then the same blocks through lz4hip_compress_fast_chain_batch in one call;
    then every stream back through lz4hip_decompress_safe_chain_batch across the same call cuts"""
    lives = sixty_four
    assert len(lives) == 64 and all(2 <= len(l.calls) <= 6 for l in lives)
    eng = DevEngine(amd, 70)
    try:
        ids = sorted(random.Random(72).sample(range(70), 64))
        bad, results, rounds = drive(eng, rc, lives, random.Random(73), absent=0.5, ids=ids)
        assert not bad, (len(bad), bad[:5])
        assert rounds >= 6
        cons, stop = eng.consumed()
        for i, lf in zip(ids, lives):
            assert cons[i] == sum(len(c.data) for c in lf.calls) and not stop[i], lf.name
        assert all(cons[i] == 0 for i in range(70) if i not in ids)
    finally:
        eng.close()
    # the one-call chain on the same blocks gives the same values and bytes
    want = [([r for c in res for r in c[0]], sum(c[1] for c in res), [x for c in res for x in c[2]]) for res in results]
    pk = CPacked([lf.as_chain() for lf in lives])
    dst, out, done = chain_call(amd, pk)
    assert not pk.check(dst, out, done, want)
    # back through the chain decoder, call by call: round r decodes every stream's r-th call behind what it has decoded so far
    decoded = [bytearray(lf.history) for lf in lives]
    for r in range(max(len(l.calls) for l in lives)):
        now = [i for i, l in enumerate(lives) if r < len(l.calls)]
        src, so, sl, caps, first, dbuf, cdo, cdc, pre = bytearray(), [], [], [], [0], bytearray(), [], [], []
        for i in now:
            call, (outs, done_i, by) = lives[i].calls[r], results[i][r]
            hist = bytes(decoded[i][-65536:])
            dbuf += hist
            cdo.append(len(dbuf)); cdc.append(len(call.data)); pre.append(len(hist))
            dbuf += bytes(len(call.data))
            for (s, cap), x in zip(call.blocks, by):
                so.append(len(src)); sl.append(len(x)); caps.append(len(s))
                src += x
            first.append(len(so))
        got, dn = amd.LZ4HIPBatch.decompressSafeChain(bytes(src), so, sl, caps, first, dbuf, cdo, cdc, pre)
        assert list(got) == caps and list(dn) == cdc
        for i, o, n in zip(now, cdo, cdc):
            assert bytes(dbuf[o:o + n]) == lives[i].calls[r].data, (lives[i].name, r)
            decoded[i] += dbuf[o:o + n]


def test_every_third_of_120_streams_in_1_mib_chunks(amd, rc, monkeypatch):
    """the host call with 1 MiB chunks (LZ4HIP_HOST_CHUNK_MB=1, read per call): 40 chains on the streams 0, 3, 6 .. 117 of a set of 120,
    so that a chain's slot is never its index in the call, let alone in its chunk; two calls of 16 x 4 KiB per stream (2.5 MiB of source:
    three chunks in the first call, more in the second, which has every stream's 64 KiB of history in front).  A slot taken from the wrong
    chain of a second or third chunk continues another stream's text: bytes, return values and the set's own count all say so"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    b = book1()
    ids = list(range(0, 120, 3))
    lives = [life_of("stream %d" % i, b[5000 * i + 7:5000 * i + 7 + 32 * 4096], [4096] * 32, (16,)) for i in ids]
    assert len(lives) == 40 and all(len(l.calls) == 2 and len(l.calls[0].data) == 65536 for l in lives)
    eng = DevEngine(amd, 120)
    try:
        bad, _, rounds = drive(eng, rc, lives, random.Random(78), absent=0.0, ids=ids)
        assert not bad, (len(bad), bad[:5])
        assert rounds == 2
        assert eng.consumed() == ([32 * 4096 if i % 3 == 0 else 0 for i in range(120)], [0] * 120)
    finally:
        eng.close()


def test_6000_streams_three_calls_of_one_block(amd, rc):
    """more streams than resident wavefronts, every stream in every call: a table carried into the next stream a wavefront draws, or a
    state saved to the wrong slot, changes bytes.  Stream i repeats in call k what it -- and nobody else -- saw in the calls before"""
    n = 6000
    rng = random.Random(74)
    b = book1()
    noise = rng.randbytes(1 << 20)
    sizes = [[rng.randrange(300, 1501) for _ in range(3)] for _ in range(n)]
    datas = []
    for i in range(n):
        o = (i * 113) % 600000
        own = noise[i * 160:i * 160 + 160]                        # distinct per stream
        d0 = (own + b[o:o + 1500])[:sizes[i][0]]
        d1 = (d0[40:200] + b[o + 2000:o + 3500])[:sizes[i][1]]   # found only in the stream's own history
        d2 = (d1[:120] + own[::-1] + d0[100:260] + b[o + 4000:o + 5500])[:sizes[i][2]]
        datas.append((d0, d1, d2))
    # the reference: one stream each, the three blocks in place
    L = rc.L
    want = []
    for i in range(n):
        buf = C.create_string_buffer(b"".join(datas[i]), sum(sizes[i]))
        st = L.LZ4_createStream()
        o, res = 0, []
        for k in range(3):
            d = C.create_string_buffer(bound(sizes[i][k]))
            r = L.LZ4_compress_fast_continue(st, C.addressof(buf) + o, d, sizes[i][k], bound(sizes[i][k]), 1)
            res.append(d.raw[:r]); o += sizes[i][k]
        L.LZ4_freeStream(st)
        want.append(res)
    assert sum(len(w[1]) < 0.9 * s[1] for w, s in zip(want, sizes)) > n // 2     # (the second call does find the first)
    with amd.CompressStreams(n) as streams:
        assert len(streams) == n
        ids = np.arange(n, dtype=np.uint32)
        for k in range(3):
            hist = [b"".join(d[:k]) for d in datas]
            src = b"".join(h + d[k] for h, d in zip(hist, datas))
            lens = np.array([s[k] for s in sizes], np.int32)
            pre = np.array([len(h) for h in hist], np.int32)
            cso = (np.cumsum(np.concatenate([[0], (lens + pre)[:-1]])) + pre).astype(np.uint64)
            caps = np.array([bound(int(v)) for v in lens], np.int32)
            do = np.concatenate([[0], np.cumsum(caps + 3)[:-1]]).astype(np.uint64)
            dst = bytearray(b"\xA5" * int(np.sum(caps + 3)))
            out, cons = streams.compress(ids, src, cso, lens, np.arange(n + 1, dtype=np.uint32), dst, do, caps, pre)
            assert list(cons) == list(lens)
            wrong = [i for i in range(n) if out[i] != len(want[i][k]) or bytes(dst[int(do[i]):int(do[i]) + int(out[i])]) != want[i][k]]
            assert not wrong, (k, len(wrong), wrong[:8])
            assert all(dst[int(do[i]) + int(out[i]):int(do[i]) + int(caps[i]) + 3].count(0xA5) == int(caps[i]) + 3 - int(out[i]) for i in range(0, n, 97))
        cons, stop = streams.consumed()
        assert cons == [sum(s) for s in sizes] and not any(stop)


def test_truncated_histories_and_small_first_calls(amd, rc, O):
    """the CPU file's LZ4_saveDict list on the device: kept histories of 0, 3, 7, 8, 1000, 65535, 65536 and more than the stream holds, and
    first calls made of blocks under 13 bytes only"""
    rng = random.Random(75)
    sel = truncation_lives(rng, O) + small_first_lives(rng, O)
    eng = DevEngine(amd, len(sel))
    try:
        bad, results, _ = drive(eng, rc, sel, rng, absent=0.0)
        assert not bad, (len(bad), bad[:5])
    finally:
        eng.close()


def test_stops_resets_and_ids(amd, rc):
    """a block that does not fit stops its stream; LZ4HIP_CHAIN_STOPPED in later calls; reset of a subset; consumed / stopped as
    reported; a call that names a strict subset leaves the others untouched, and they continue correctly afterwards; the id errors"""
    b = book1()
    rng = random.Random(76)
    blocks = lambda o, n=4: [(b[o + 1000 * i:o + 1000 * (i + 1)], bound(1000)) for i in range(n)]
    eng = DevEngine(amd, 5)
    ref = [RefStream(rc) for _ in range(5)]
    try:
        def both(ids, calls):
            parts, want = [], []
            for i, c in zip(ids, calls):
                front, plen = ref[i].front(c)
                parts.append((front, plen, c)); want.append(ref[i].run(c))
            pk = PackedCall(parts, rng)
            dst, out, cons = eng.call(ids, pk)
            assert not pk.check(["stream %d" % i for i in ids], dst, out, cons, want)
            return out, cons
        out, cons = both([0, 1, 2, 4], [Call(blocks(0)), Call([(b[5000:6000], 10)] + blocks(6000, 2)), Call(blocks(9000)), Call(blocks(30000, 2))])
        assert list(out[4:7]) == [0, CHAIN_STOPPED, CHAIN_STOPPED] and int(cons[1]) == 0
        assert eng.consumed() == ([4000, 0, 4000, 0, 2000], [0, 1, 0, 0, 0])
        out, cons = both([1, 2], [Call(blocks(7000)), Call(blocks(13000))])          # 0 and 4 are not named
        assert list(out[:4]) == [CHAIN_STOPPED] * 4 and int(cons[0]) == 0
        assert eng.consumed(1, 2) == ([0, 8000], [1, 0])
        eng.reset([1, 3])
        ref[1].close(); ref[1] = RefStream(rc)
        out, cons = both([0, 1, 4], [Call(blocks(4000)), Call(blocks(7000)), Call(blocks(32000, 3))])
        assert all(r > 0 for r in out[:11])
        assert eng.consumed() == ([8000, 4000, 8000, 0, 5000], [0] * 5)
        eng.reset()
        assert eng.consumed() == ([0] * 5, [0] * 5)
        # the ids: not ascending, repeated, out of range -- argument errors, nothing written, no stream touched
        pk = PackedCall([(b"", 0, Call(blocks(0, 1))), (b"", 0, Call(blocks(1000, 1)))], rng)
        for ids in ([1, 0], [2, 2], [0, 5]):
            dst, out, cons = eng.call(ids, pk, expect=E_ARG)
            assert b"stream_id" in eng.l.lz4hip_last_error() and dst == bytes(pk.dst) and list(out[:2]) == [12345] * 2
        assert eng.consumed() == ([0] * 5, [0] * 5)
    finally:
        eng.close()
        for r in ref:
            r.close()


def test_argument_errors_with_a_live_set(amd):
    """every argument error of lz4hip_compress_fast_stream_batch against a set that exists: a NULL where a pointer is required (the
    prefix array is optional), a chain_first that is not ascending from 0 to n_blocks, a prefix that is negative or longer than the
    chain's offset, ids that are not strictly ascending or are >= n_streams -- LZ4HIP_E_ARG each, nothing written, no stream touched;
    then the well-formed call goes through"""
    from test_cstream_abi import Call as AbiCall
    eng = DevEngine(amd, 2)
    try:
        l, c = eng.l, AbiCall(eng.h)
        f = l.lz4hip_compress_fast_stream_batch
        err = lambda: l.lz4hip_last_error()
        for name in ("set", "ids", "src", "cso", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "cons"):
            assert f(*c.args(**{name: None})) == E_ARG and b"null" in err().lower(), name
        for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
            assert f(*c.args(first=(u32 * 3)(*first))) == E_ARG and b"chain_first" in err(), first
        assert f(*c.args(n_chains=0)) == E_ARG
        for pre in ((1, 4), (0, 13), (0, -1)):
            assert f(*c.args(prefix=(i32 * 2)(*pre))) == E_ARG and b"chain_prefix_len" in err(), pre
        for ids in ((1, 1), (1, 0), (0, 2), (2, 3)):
            assert f(*c.args(ids=(u32 * 2)(*ids))) == E_ARG and b"stream_id" in err(), ids
        assert c.untouched() and eng.consumed() == ([0, 0], [0, 0])
        assert f(*c.args(n_blocks=0, n_chains=0)) == 0 and c.untouched()           # the empty call
        assert f(*c.args(prefix=None, cso=(u64 * 2)(0, 8))) == 0                      # the optional array
        assert list(c.out) == [5, 5, 5] and list(c.cons) == [8, 4] and eng.consumed() == ([8, 4], [0, 0])
    finally:
        eng.close()


def test_threads(amd, rc, O):
    """two sets from two host threads, and one set from two threads (serialised): every stream as the reference's"""
    rng = random.Random(77)
    def lives(tag, n):
        return [random_life(rng, O, "%s %d" % (tag, i), rng.randrange(3, 9), 2000, every_boundary=True) for i in range(n)]
    a, bb, c0, c1 = lives("a", 12), lives("b", 12), lives("c0", 8), lives("c1", 8)
    ea, eb, ec = DevEngine(amd, 12), DevEngine(amd, 12), DevEngine(amd, 16)
    res = {}
    def work(key, eng, ls, ids, seed):
        try:
            res[key] = drive(eng, rc, ls, random.Random(seed), absent=0.3, ids=ids)[0]
        except BaseException as e:      # (an assertion in a thread is a failure of the test)
            res[key] = [("exception", repr(e))]
    try:
        th = [threading.Thread(target=work, args=("a", ea, a, None, 1)), threading.Thread(target=work, args=("b", eb, bb, None, 2)),
              threading.Thread(target=work, args=("c0", ec, c0, list(range(0, 16, 2)), 3)), threading.Thread(target=work, args=("c1", ec, c1, list(range(1, 16, 2)), 4))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert res == {"a": [], "b": [], "c0": [], "c1": []}, {k: v[:3] for k, v in res.items()}
    finally:
        for e in (ea, eb, ec):
            e.close()


def test_set_divided_over_device_entries():
    """the set's streams divided over the engine's devices, and calls sharded at those boundaries: device 0 listed three times"""
    assert "cstream multidev ok" in run_child("cstream_multidev_child.py", 3, timeout=120)


def test_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    assert "cstream multidev ok" in run_child("cstream_multidev_child.py", 0, timeout=120)


def test_cstream_cpp_mirror(rc, tmp_path):
    """CompressStreams of host/lz4hip.hpp: a stream cut into two calls against the mirror's one-call chain (inside the program) and
    against the reference (here), with and without a loaded prefix, and with a block that does not fit"""
    import subprocess
    from cchain_common import chain_of, cchain_file
    from support import build_mirror
    exe = build_mirror("cstream_mirror_test", tmp_path, werror=True)
    b = book1()
    chains = [chain_of("plain", b[3000:3000 + 9 * 700], [700] * 9), chain_of("prefix", b[9000:9000 + 6 * 1000], [1000] * 6, history=b[6000:9000]),
              chain_of("mixed", b[500:500 + 1330], [5, 0, 13, 300, 12, 1000])]
    chains.append(chains[0].with_caps(lambda i, c: 10 if i == 6 else c, "cap 10 at 6"))
    for ch in chains:
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 0, (ch.name, p.returncode, p.stderr)
        outs, done, by = rc.compress(ch)
        assert p.stdout.decode().split() == [str(r) for r in outs] + ["|", str(done)], (ch.name, p.stdout)
        assert (tmp_path / "o.bin").read_bytes() == b"".join(by), ch.name


def test_frame_writer_with_stream_state(amd, rc, port):
    """LZ4FrameOutputStream(linkedBlocks=True, streamState=True): one stream per frame, so the frame is what ONE LZ4_stream_t writes
    block after block, for batchBlocks 1, 3 and 64 and with flush() calls on block boundaries in between; LZ4FrameInputStream reads it
    back; without streamState the bytes are the parent's (every batch a fresh LZ4_loadDict chain)"""
    import importlib
    import io
    from cchain_common import batched_linked_frame
    S = importlib.import_module("lz4-java_amd.streams")
    B = S.FLG.Bits
    data = book1()[20000:20000 + 9 * 65536 + 12345]
    block_id, bs = 4, 65536
    want = batched_linked_frame(rc, port.xxh32, data, block_id, 10 ** 6, block_checksum=True, content_checksum=True)   # one batch = one stream
    frames = {}
    for batch, flush_every in ((1, 0), (3, 0), (64, 0), (3, 2), (64, 5)):
        sink = io.BytesIO()
        w = S.LZ4FrameOutputStream(sink, block_id, -1, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, batchBlocks=batch, linkedBlocks=True, streamState=True)
        for k, a in enumerate(range(0, len(data), bs)):
            w.write(data[a:a + bs])
            if flush_every and (k + 1) % flush_every == 0:
                w.flush()
        w.close()
        frames[(batch, flush_every)] = sink.getvalue()
        assert sink.getvalue() == want, (batch, flush_every)
    assert S.LZ4FrameInputStream(io.BytesIO(want), linkedBlocks=True).read() == data
    for batch in (1, 3):
        sink = io.BytesIO()
        w = S.LZ4FrameOutputStream(sink, block_id, -1, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, batchBlocks=batch, linkedBlocks=True)
        for a in range(0, len(data), bs):
            w.write(data[a:a + bs])
        w.close()
        assert sink.getvalue() == batched_linked_frame(rc, port.xxh32, data, block_id, batch, block_checksum=True, content_checksum=True) != want
    with pytest.raises(ValueError):
        S.LZ4FrameOutputStream(io.BytesIO(), block_id, streamState=True)
    with pytest.raises(ValueError):
        S.LZ4FrameOutputStream(io.BytesIO(), block_id, linkedBlocks=True, level=9, streamState=True)


def test_cpp_frame_writer_with_stream_state(rc, port, tmp_path):
    """host/lz4hip_streams.hpp: LZ4FrameOutputStream(linkedBlocks = true) with streamState(true) writes the frame of ONE stream for
    batchBlocks 1, 3 and 64 and with flush() on block boundaries; the program reads it back through LZ4FrameInputStream"""
    import subprocess
    from cchain_common import batched_linked_frame
    from support import build_mirror
    exe = build_mirror("cstream_mirror_test", tmp_path, werror=True)
    data = book1()[40000:40000 + 7 * 65536 + 4321]
    (tmp_path / "d.bin").write_bytes(data)
    want = batched_linked_frame(rc, port.xxh32, data, 4, 10 ** 6, block_checksum=True, content_checksum=True)
    for batch, flush_every in ((1, 0), (3, 0), (64, 0), (3, 2), (64, 5)):
        p = subprocess.run([exe, "--frame", str(tmp_path / "d.bin"), str(tmp_path / "f.lz4"), "4", str(batch), str(flush_every)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 0, (batch, flush_every, p.stderr.decode()[-2000:])
        assert (tmp_path / "f.lz4").read_bytes() == want, (batch, flush_every)


def test_cstream_jni_program(rc, tmp_path):
    """tests/jni_stub/fake_jni_cstream.c: the JNI shim's resident-stream natives over the fake JNIEnv -- a stream cut into two calls
    against the reference's ONE stream, with and without a loaded prefix, small blocks first, and a block that does not fit"""
    import subprocess
    from cchain_common import chain_of, cchain_file
    from support import build_fake_jni
    exe = build_fake_jni("fake_jni_cstream", tmp_path)
    b = book1()
    chains = [chain_of("plain", b[3000:3000 + 9 * 700], [700] * 9), chain_of("prefix", b[9000:9000 + 6 * 1000], [1000] * 6, history=b[6000:9000]),
              chain_of("short prefix", b[500:500 + 4 * 900], [900] * 4, history=b[495:500]), chain_of("mixed", b[500:500 + 1330], [5, 0, 13, 300, 12, 1000])]
    chains.append(chains[0].with_caps(lambda i, c: 10 if i == 6 else c, "cap 10 at 6"))
    for ch in chains:
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        out = subprocess.check_output([exe, str(tmp_path / "c.bin"), str(tmp_path)], timeout=60).decode()
        assert "checks ok" in out, (ch.name, out)
        outs, done, by = rc.compress(ch)
        assert (tmp_path / "cstream.txt").read_text().split() == [str(r) for r in outs] + ["|", str(done)], ch.name
        assert (tmp_path / "cstream.out").read_bytes() == b"".join(by), ch.name
