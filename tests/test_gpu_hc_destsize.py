"""HC compress to a target size on the GPU (-m gpu): every layer of LZ4_compress_HC_destSize -- hc_build_kernel +
hc_parse_dest_kernel through the host batch, the device batch with and without a caller's workspace, coalesced single calls, the
multi-device host path, the Python factory, the C++ mirror and the JNI shim -- checked byte for byte, and consumed size for consumed
size, against the reference library's own LZ4_compress_HC_destSize (oracle.ref_path())."""
import ctypes as C
import random
import subprocess
import threading

import numpy as np
import pytest

from conftest import calgary, rnd_inputs
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
_u8p = C.POINTER(C.c_uint8)
GUARD = 0xA5
CHAIN_LEVELS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
OPT_LEVELS = (10, 11, 12, 13)


def bound(n):
    return n + n // 255 + 16 if 0 <= n <= 0x7E000000 else 0


@pytest.fixture(scope="module")
def lz4hcdest(ref):
    """(src, target, level) -> (ret, consumed, bytes) of the reference library's LZ4_compress_HC_destSize; one state per thread"""
    lib = C.CDLL(ref.path)
    f = lib.LZ4_compress_HC_destSize
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int, C.c_int]
    lib.LZ4_sizeofStateHC.restype = C.c_int
    size = lib.LZ4_sizeofStateHC() + 64
    tls = threading.local()

    def run(v, t, level):
        if not hasattr(tls, "state"):
            tls.state = C.create_string_buffer(size)
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int(len(v))
        r = f((C.addressof(tls.state) + 15) & ~15, bytes(v), out, C.byref(sz), t, level)
        return r, sz.value, bytes(out[:max(r, 0)])
    return run


def c_host_batch(amd, inputs, pairs, level, gap=32):
    """lz4hip_compress_hc_dest_size_batch straight through the C ABI (targets <= 0 included): every (input index, target) pair is one
    block reading the input's single copy; every slot is followed by `gap` guard bytes -> (out, consumed, dst, offsets)"""
    l = amd.lib()
    offs = np.concatenate([[0], np.cumsum([len(v) for v in inputs])[:-1]]).astype(np.uint64)
    src = b"".join(inputs) + b"\0"
    n = len(pairs)
    so = np.array([offs[i] for i, _ in pairs], dtype=np.uint64)
    sl = np.array([len(inputs[i]) for i, _ in pairs], dtype=np.int32)
    ts = np.array([t for _, t in pairs], dtype=np.int32)
    do = np.concatenate([[0], np.cumsum([max(t, 0) + gap for _, t in pairs])[:-1]]).astype(np.uint64)
    dst = bytearray([GUARD]) * (int(do[-1]) + max(pairs[-1][1], 0) + gap)
    out, cons = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    dp = (C.c_uint8 * len(dst)).from_buffer(dst)
    u64, i32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    rc = l.lz4hip_compress_hc_dest_size_batch(src, u64(so), i32(sl), dp, u64(do), i32(ts), i32(out), i32(cons), n, level)
    assert rc == 0, l.lz4hip_last_error()
    return out, cons, dst, do


def check_batch(amd, lz4hcdest, inputs, pairs, level, gap=32):
    out, cons, dst, do = c_host_batch(amd, inputs, pairs, level, gap)
    streams, sizes = [], []
    for k, (i, t) in enumerate(pairs):
        want = lz4hcdest(inputs[i], t, level)
        o = int(do[k])
        assert (int(out[k]), int(cons[k])) == want[:2], (level, k, len(inputs[i]), t, int(out[k]), int(cons[k]), want[:2])
        assert bytes(dst[o:o + int(out[k])]) == want[2], (level, k, len(inputs[i]), t)
        # the guard bytes behind the target-sized slot (and the unused rest of the slot) are untouched
        assert dst[o + int(out[k]):o + max(t, 0) + gap] == bytearray([GUARD]) * (max(t, 0) + gap - int(out[k])), ("guard", level, k, t)
        if out[k] > 0:
            streams.append(want[2]); sizes.append((i, int(cons[k])))
    # every output decodes (lz4hip_decompress_safe_batch) to exactly the consumed prefix of its input
    so = np.concatenate([[0], np.cumsum([len(s) for s in streams])[:-1]]).astype(np.uint64)
    caps = np.array([c for _, c in sizes], dtype=np.int32)
    dof = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    back = bytearray(int(caps.sum()) + 1)
    r = amd.LZ4HIPBatch.decompressSafe(b"".join(streams), so, np.array([len(s) for s in streams], dtype=np.int32), back, dof, caps)
    for k, (i, c) in enumerate(sizes):
        assert int(r[k]) == c and bytes(back[int(dof[k]):int(dof[k]) + c]) == inputs[i][:c], (level, k, c)
    return out, cons


def fuzz_pairs(ref, O, corpus, level):
    """mixed sizes and targets for one level: lengths 0 .. 13 at every target 0 .. 20, a seeded mixed bag of inputs (up to 70,000
    bytes at levels 0 .. 9, up to 16 KiB at the optimal-parser levels) at the targets around every edge"""
    rng = random.Random(100 + level)
    inputs, pairs = [], []
    book1 = corpus["book1[:200000]"]

    def add(v, ts):
        inputs.append(v)
        pairs.extend((len(inputs) - 1, t) for t in ts)

    def edge(v, n_random=2):
        dl, b = len(ref.compress_hc(v, level)), bound(len(v))
        return sorted({1, 5, 6, 12, 13, 18, dl - 16, dl - 1, dl, dl + 1, dl + 16, b, b + 9} | {rng.randrange(1, b + 3) for _ in range(n_random)})
    for n in range(0, 14):
        for v in (book1[9000:9000 + n], bytes(n)):
            add(v, range(-1, 21))
    opt = level >= 10
    for v in rnd_inputs(O, corpus, 200 + level, 60 if opt else 150, max_n=16384 if opt else 70000):
        add(v, edge(v))
    for v in (bytes(16384 if opt else 65547), O.gen_block(16384 if opt else 65536, level), rng.randbytes(9000)):
        add(v, edge(v, 4) + [4096])
    return inputs, pairs


@pytest.mark.parametrize("level", CHAIN_LEVELS + OPT_LEVELS)
def test_host_batch_fuzz(amd, ref, lz4hcdest, O, corpus, level):
    """one host batch per level of mixed sizes and targets: sizes, consumed sizes, bytes, the gaps between the slots, decodes"""
    inputs, pairs = fuzz_pairs(ref, O, corpus, level)
    assert len(pairs) > (1400 if level >= 10 else 2500), len(pairs)
    check_batch(amd, lz4hcdest, inputs, pairs, level)


def test_big_blocks_and_65547_boundary(amd, lz4hcdest, O):
    """1 MiB and 4 MiB App. F blocks, text across the 65546 / 65547 boundary, at levels 1, 4 and 9"""
    book1 = calgary("book1")
    inputs = [O.gen_block(1 << 20, 1, win=4096), O.gen_block(1 << 20, 2), O.gen_block(4 << 20, 3, win=4096), book1[:700000],
              book1[:65546], book1[:65547], book1[:65548], O.gen_block(65547, 5), bytes(65547)]
    pairs = []
    for i, v in enumerate(inputs):
        for t in (1, 17, 4096, 16384, 1 << 18, len(v) // 3, bound(len(v)) - 1, bound(len(v))):
            pairs.append((i, t))
    for level in (1, 4, 9):
        check_batch(amd, lz4hcdest, inputs, pairs, level)


def test_large_targets_are_the_plain_hc_bytes(amd, O, corpus):
    """targets >= compressBound(n): the bytes of lz4hip_compress_hc_batch, all of the input consumed (levels 1 and 9; level 10 on
    the inputs of at most 16 KiB)"""
    every = rnd_inputs(O, corpus, 24, 200) + [O.gen_block(65536, i) for i in range(8)] + [calgary("book1")[:300000]]
    for level in (1, 9, 10):
        inputs = every if level < 10 else [v for v in every if len(v) <= 16384]
        assert len(inputs) > 100
        pairs = [(i, bound(len(v)) + k) for i, v in enumerate(inputs) for k in (0, 7)]
        caps = [bound(len(v)) for v in inputs]
        so = np.concatenate([[0], np.cumsum([len(v) for v in inputs])[:-1]]).astype(np.uint64)
        fdo = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
        out, cons, dst, do = c_host_batch(amd, inputs, pairs, level)
        fdst = bytearray(int(sum(caps)) + 1)
        fout = amd.LZ4HIPBatch.compressHC(b"".join(inputs), so, np.array([len(v) for v in inputs], dtype=np.int32), fdst, fdo,
                                          np.array(caps, dtype=np.int32), level)
        for k, (i, _) in enumerate(pairs):
            assert int(out[k]) == int(fout[i]) and int(cons[k]) == len(inputs[i]), (level, k, len(inputs[i]))
            assert dst[int(do[k]):int(do[k]) + int(out[k])] == fdst[int(fdo[i]):int(fdo[i]) + int(fout[i])], (level, k)


def test_device_batch_4096_blocks(amd, lz4hcdest, O):
    """the device batch on 4,096 x 64 KiB blocks (App. F and text) at 16 KiB targets, level 9, through _batch_dev_ws (which must not
    synchronise: it returns while earlier work of the stream is still running) and through _batch_dev: every size and consumed
    count against the reference, the bytes of 64 sampled blocks, the guard bytes between the slots"""
    import torch
    book1 = calgary("book1")
    n, T, G, level = 4096, 16384, 64, 9
    blocks = [O.gen_block(65536, i) if i % 4 else book1[(i * 977) % (len(book1) - 65536):][:65536] for i in range(n)]
    dev = torch.device("cuda:0")
    src = torch.frombuffer(bytearray(b"".join(blocks)), dtype=torch.uint8).to(dev)
    so = torch.arange(n, dtype=torch.int64, device=dev) * 65536
    sl = torch.full((n,), 65536, dtype=torch.int32, device=dev)
    do = torch.arange(n, dtype=torch.int64, device=dev) * (T + G)
    ts = torch.full((n,), T, dtype=torch.int32, device=dev)
    want = [lz4hcdest(b, T, level) for b in blocks]
    sample = set(random.Random(9).sample(range(n), 64))

    def fresh():
        return (torch.full((n * (T + G),), GUARD, dtype=torch.uint8, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev),
                torch.full((n,), -7, dtype=torch.int32, device=dev))

    def verify(dst, out, cons, what):
        h, r, c = dst.cpu().numpy().tobytes(), out.cpu().tolist(), cons.cpu().tolist()
        for i in range(n):
            assert (r[i], c[i]) == want[i][:2], (what, i, r[i], c[i], want[i][:2])
            o = i * (T + G)
            if i in sample:
                assert h[o:o + r[i]] == want[i][2], (what, i)
            assert h[o + r[i]:o + T + G] == bytes([GUARD]) * (T + G - r[i]), ("guard", what, i)

    dst, out, cons = fresh()
    amd.DeviceBatch.compress_hc_dest_size(src, so, sl, dst, do, ts, out, cons, level)     # (warms the allocator: the workspace tensor)
    torch.cuda.synchronize()
    verify(dst, out, cons, "_ws")
    # _ws does not synchronise: with one launch in flight, a second call returns before the first one's event has fired
    dst1, out1, cons1 = fresh()
    dst2, out2, cons2 = fresh()
    torch.cuda.synchronize()
    amd.DeviceBatch.compress_hc_dest_size(src, so, sl, dst1, do, ts, out1, cons1, level)
    ev = torch.cuda.Event()
    ev.record()
    amd.DeviceBatch.compress_hc_dest_size(src, so, sl, dst2, do, ts, out2, cons2, level)
    still_running = not ev.query()
    torch.cuda.synchronize()
    assert still_running, "lz4hip_compress_hc_dest_size_batch_dev_ws waited for the stream"
    verify(dst2, out2, cons2, "_ws second")
    dst3, out3, cons3 = fresh()
    amd.DeviceBatch.compress_hc_dest_size_sync(src, so, sl, dst3, do, ts, out3, cons3, level)
    torch.cuda.synchronize()
    verify(dst3, out3, cons3, "_batch_dev")
    # a workspace that is too small for the span is refused, nothing runs
    L = amd.lib()
    out4 = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    rc = L.lz4hip_compress_hc_dest_size_batch_dev_ws(src.data_ptr(), so.data_ptr(), sl.data_ptr(), dst3.data_ptr(), do.data_ptr(), ts.data_ptr(),
                                                     out4.data_ptr(), cons3.data_ptr(), n, level, 0, torch.cuda.current_stream(dev).cuda_stream,
                                                     n * 65536, ws.data_ptr(), 4096)
    torch.cuda.synchronize()
    assert rc == -3 and b"workspace too small" in L.lz4hip_last_error() and out4.cpu().tolist() == [-7] * n


def test_concurrent_single_calls(amd, ref, lz4hcdest):
    """8 threads: HC destSize single calls at four levels interleaved with plain lz4hip_compress_hc single calls; coalescing keeps
    levels and operations apart"""
    l = amd.lib()
    book1 = calgary("book1")
    data = [book1[o:o + 32768] for o in range(0, 8 * 32768, 32768)]
    jobs = [(kind, v, t, lv) for v in data for kind, t, lv in (("dest", 4096, 1), ("dest", 9000, 9), ("dest", 1, 4), ("dest", 5000, 10),
                                                              ("dest", 4096, 9), ("hc", 0, 9))] * 2
    random.Random(13).shuffle(jobs)
    barrier = threading.Barrier(8)
    errors = []

    def worker(k):
        barrier.wait()
        for kind, v, t, lv in jobs[k::8]:
            if kind == "dest":
                out = (C.c_uint8 * t)()
                sz = C.c_int32(len(v))
                r = l.lz4hip_compress_hc_dest_size(v, C.byref(sz), out, t, lv)
                want = lz4hcdest(v, t, lv)
                if (r, sz.value, bytes(out[:max(r, 0)])) != want:
                    errors.append(("dest", t, lv, r, sz.value, want[:2]))
            else:
                cap = bound(len(v))
                out = (C.c_uint8 * cap)()
                r = l.lz4hip_compress_hc(v, len(v), out, cap, lv)
                if r <= 0 or bytes(out[:r]) != ref.compress_hc(v, lv):
                    errors.append(("hc", r))
    th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:10]


def test_single_call_edge_cases(amd, lz4hcdest):
    """the liblz4 edge cases through the single call: targets < 1 and bad sizes leave *src_size alone, the empty block, inputs below
    LZ4_minLength, the level clamp"""
    l = amd.lib()
    v = calgary("book1")[:5000]
    for level in (-5, 0, 1, 9, 10, 12, 13, 99):
        for n, t in ((5000, 0), (5000, -3), (0, 1), (0, 20), (12, 1), (12, 5), (12, 13), (12, 40), (13, 14), (5000, 6), (5000, 13), (5000, 5000),
                     (5000, 6000)):
            out = (C.c_uint8 * max(t, 1))()
            sz = C.c_int32(n)
            r = l.lz4hip_compress_hc_dest_size(v[:n], C.byref(sz), out, t, level)
            want = lz4hcdest(v[:n], t, level)
            assert (r, sz.value, bytes(out[:max(r, 0)])) == want, (level, n, t, r, sz.value, want[:2])
    sz = C.c_int32(-1)
    assert l.lz4hip_compress_hc_dest_size(v, C.byref(sz), (C.c_uint8 * 10)(), 10, 9) == 0 and sz.value == -1


def test_python_factory(amd, lz4hcdest, O):
    f = amd.LZ4Factory.hipInstance()
    v = O.gen_block(65536, 7)
    for level in (1, 9, 11):
        c = f.highCompressor(level)
        dst = bytearray(b"\xEE" * 5000)
        w, consumed = c.compressDestSize(v, 0, len(v), dst, 100, 4096)
        want = lz4hcdest(v, 4096, level)
        assert (w, consumed) == want[:2] and bytes(dst[100:100 + w]) == want[2]
        assert dst[:100] == b"\xEE" * 100 and dst[100 + w:] == b"\xEE" * (len(dst) - 100 - w)
        assert f.safeDecompressor().decompress(bytes(dst[100:100 + w]), consumed) == v[:consumed]
        out, cons = amd.LZ4HIPBatch.compressHCDestSize(v * 2, [0, 65536], [65536, 65536], bytearray(9000), [0, 4096], [4096, 4096], level)
        assert out == [w, w] and cons == [consumed, consumed]


def test_cpp_mirror(lz4hcdest, tmp_path):
    """tests/cpp/hc_destsize_mirror_test.cpp: LZ4HCHIPCompressor::compressDestSize of host/lz4hip.hpp, against the reference"""
    exe = build_mirror("hc_destsize_mirror_test", tmp_path)
    v = calgary("book1")[7000:90000]
    (tmp_path / "in.bin").write_bytes(v)
    for t, level in ((100, 9), (4096, 1), (30000, 9), (4096, 10)):
        p = subprocess.run([exe, str(tmp_path / "in.bin"), str(t), str(tmp_path / "out.bin"), str(level)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        w, consumed = map(int, p.stdout.decode().split())
        want = lz4hcdest(v, t, level)
        assert (w, consumed) == want[:2] and (tmp_path / "out.bin").read_bytes() == want[2], (t, level)


def test_jni_hc_dest_size_full_scenarios(lz4hcdest, tmp_path):
    """the shim's new natives over the fake JNIEnv (tests/jni_stub/fake_jni_hc_destsize.c): arrays, direct buffers, NULL arrays, a
    destination that cannot be pinned, the batch native; the stream and consumed size are the reference's"""
    exe = build_fake_jni("fake_jni_hc_destsize", tmp_path)
    v = calgary("book1")[100000:165536]
    (tmp_path / "in.bin").write_bytes(v)
    for level in (9, 4):
        out = subprocess.check_output([exe, str(tmp_path / "in.bin"), "16384", str(tmp_path), str(level)], timeout=300).decode()
        assert "checks ok" in out and "no device" not in out, out
        want = lz4hcdest(v, 16384, level)
        w, consumed = map(int, (tmp_path / "dest.txt").read_text().split())
        assert (w, consumed) == want[:2] and (tmp_path / "dest.bin").read_bytes() == want[2], level


def test_multidevice_host_path():
    """lz4hip_init([0, 0]) in a child process: a ragged HC destSize batch across the device boundary, at level 9"""
    assert "hc destsize multidev ok D=2" in run_child("hc_destsize_multidev_child.py", "2", "9", timeout=900)
