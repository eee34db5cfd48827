"""Compress to a target size on the GPU (-m gpu): every layer of LZ4_compress_destSize -- compress_fast_dest_cu_kernel through the
host batch, the device batch, coalesced single calls, the multi-device host path, the Python factory, the C++ mirror and the JNI
shim -- checked byte for byte, and consumed size for consumed size, against the reference library's own LZ4_compress_destSize
(oracle.ref_path())."""
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


def bound(n):
    return n + n // 255 + 16 if 0 <= n <= 0x7E000000 else 0


@pytest.fixture(scope="module")
def lz4dest(ref):
    """(src, target) -> (ret, consumed, bytes) of the reference library's LZ4_compress_destSize"""
    f = C.CDLL(ref.path).LZ4_compress_destSize
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int]

    def run(v, t):
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int(len(v))
        r = f(bytes(v), out, C.byref(sz), t)
        return r, sz.value, bytes(out[:max(r, 0)])
    return run


def c_host_batch(amd, inputs, pairs, gap=32):
    """lz4hip_compress_dest_size_batch straight through the C ABI (targets <= 0 included): every (input index, target) pair is one
    block reading the input's single copy; every slot is followed by `gap` guard bytes -> (out, consumed, slot bytes, dst, offsets)"""
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
    rc = l.lz4hip_compress_dest_size_batch(src, u64(so), i32(sl), dp, u64(do), i32(ts), i32(out), i32(cons), n)
    assert rc == 0, l.lz4hip_last_error()
    return out, cons, dst, do


def check_batch(amd, lz4dest, inputs, pairs, gap=32):
    out, cons, dst, do = c_host_batch(amd, inputs, pairs, gap)
    streams, sizes = [], []
    for k, (i, t) in enumerate(pairs):
        want = lz4dest(inputs[i], t)
        o = int(do[k])
        assert (int(out[k]), int(cons[k])) == want[:2], (k, len(inputs[i]), t, int(out[k]), int(cons[k]), want[:2])
        assert bytes(dst[o:o + int(out[k])]) == want[2], (k, len(inputs[i]), t)
        # the guard bytes behind the target-sized slot (and the unused rest of the slot) are untouched
        assert dst[o + int(out[k]):o + max(t, 0) + gap] == bytearray([GUARD]) * (max(t, 0) + gap - int(out[k])), ("guard", k, t)
        if out[k] > 0:
            streams.append(want[2]); sizes.append((i, int(cons[k])))
    # every output decodes (lz4hip_decompress_safe_batch) to exactly the consumed prefix of its input
    so = np.concatenate([[0], np.cumsum([len(s) for s in streams])[:-1]]).astype(np.uint64)
    caps = np.array([c for _, c in sizes], dtype=np.int32)
    dof = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    back = bytearray(int(caps.sum()) + 1)
    r = amd.LZ4HIPBatch.decompressSafe(b"".join(streams), so, np.array([len(s) for s in streams], dtype=np.int32), back, dof, caps)
    for k, (i, c) in enumerate(sizes):
        assert int(r[k]) == c and bytes(back[int(dof[k]):int(dof[k]) + c]) == inputs[i][:c], (k, c)
    return out, cons


def fuzz_pairs(ref, O, corpus):
    """the (input, target) pairs of tests/test_destsize_hostsim.py, in one list"""
    rng = random.Random(11)
    inputs, pairs = [], []
    book1 = corpus["book1[:200000]"]

    def add(v, ts):
        inputs.append(v)
        pairs.extend((len(inputs) - 1, t) for t in ts)

    def edge(v, n_random=3):
        dl, b = len(ref.compress_fast(v)), bound(len(v))
        return sorted({1, 5, 6, 11, 12, 17, dl - 1, dl, dl + 1, b - 1, b} | {rng.randrange(1, b + 3) for _ in range(n_random)})
    for n in list(range(0, 41)) + [100, 1000]:
        for v in (book1[5000:5000 + n], O.gen_block(n, n, litmax=4, win=8)):
            add(v, range(-1, bound(n) + 3))
    for v in rnd_inputs(O, corpus, 23, 1500):
        add(v, edge(v))
    for name in ("book1", "geo", "pic"):
        data = calgary(name)
        for o in range(0, len(data) - 65536 + 1, 65536 * 2):
            v = data[o:o + 65536]
            add(v, edge(v, 2) + [4096, 16384, 32768])
    for n in (13, 100, 1000, 4096, 65535, 65536, 65547):
        for v in (bytes(n), bytes(rng.choice((0x41, 0x42)) for _ in range(n))):
            add(v, edge(v, 6) + list(range(1, 40)))
    for v in (book1[:65547], O.gen_block(70000, 4), book1, O.gen_block(200000, 9, win=4096), bytes(70000)):
        add(v, edge(v, 4) + [1000, 4096, 65536])
    return inputs, pairs


def test_host_batch_fuzz(amd, ref, lz4dest, O, corpus):
    """one host batch of every (input, target) pair of the CPU fuzz: sizes, consumed sizes, bytes, guards, decodes"""
    inputs, pairs = fuzz_pairs(ref, O, corpus)
    assert len(pairs) > 20000
    check_batch(amd, lz4dest, inputs, pairs)


def test_target_at_least_bound_is_the_fast_path(amd, O, corpus):
    """targets >= compressBound(n): the bytes of lz4hip_compress_fast, all of the input consumed"""
    inputs = rnd_inputs(O, corpus, 24, 300) + [O.gen_block(65536, i) for i in range(8)] + [calgary("book1")[:300000]]
    pairs = [(i, bound(len(v)) + k) for i, v in enumerate(inputs) for k in (0, 7)]
    out, cons, dst, do = c_host_batch(amd, inputs, pairs)
    caps = [bound(len(v)) for v in inputs]
    so = np.concatenate([[0], np.cumsum([len(v) for v in inputs])[:-1]]).astype(np.uint64)
    fdo = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    fdst = bytearray(int(sum(caps)) + 1)
    fout = amd.LZ4HIPBatch.compress(b"".join(inputs), so, np.array([len(v) for v in inputs], dtype=np.int32), fdst, fdo, np.array(caps, dtype=np.int32))
    for k, (i, _) in enumerate(pairs):
        assert int(out[k]) == int(fout[i]) and int(cons[k]) == len(inputs[i]), (k, len(inputs[i]))
        assert dst[int(do[k]):int(do[k]) + int(out[k])] == fdst[int(fdo[i]):int(fdo[i]) + int(fout[i])], k


def test_big_blocks_and_table_boundary(amd, lz4dest, O):
    """4 MiB App. F blocks, a 16 MiB block, and the byU16 / byU32 boundary at 65546 / 65547 bytes"""
    book1 = calgary("book1")
    inputs = [O.gen_block(4 << 20, 1, win=4096), O.gen_block(4 << 20, 2), O.gen_block(16 << 20, 3, win=4096),
              book1[:65546], book1[:65547], O.gen_block(65546, 5), O.gen_block(65547, 5), bytes(65546), bytes(65547)]
    pairs = []
    for i, v in enumerate(inputs):
        for t in (1, 17, 4096, 16384, 1 << 20, len(v) // 2, bound(len(v)) - 1):
            pairs.append((i, t))
    check_batch(amd, lz4dest, inputs, pairs)


def test_device_batch_4096_blocks(amd, lz4dest, O):
    """the device batch on 4,096 x 64 KiB blocks (App. F and text) at 16 KiB targets: every size and consumed count against the
    reference, the bytes of 64 sampled blocks, the guard bytes between the slots"""
    import torch
    book1 = calgary("book1")
    n, T, G = 4096, 16384, 64
    blocks = [O.gen_block(65536, i) if i % 4 else book1[(i * 977) % (len(book1) - 65536):][:65536] for i in range(n)]
    dev = torch.device("cuda:0")
    src = torch.frombuffer(bytearray(b"".join(blocks)), dtype=torch.uint8).to(dev)
    so = torch.arange(n, dtype=torch.int64, device=dev) * 65536
    sl = torch.full((n,), 65536, dtype=torch.int32, device=dev)
    do = torch.arange(n, dtype=torch.int64, device=dev) * (T + G)
    ts = torch.full((n,), T, dtype=torch.int32, device=dev)
    dst = torch.full((n * (T + G),), GUARD, dtype=torch.uint8, device=dev)
    out = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cons = torch.full((n,), -7, dtype=torch.int32, device=dev)
    amd.DeviceBatch.compress_dest_size(src, so, sl, dst, do, ts, out, cons)
    torch.cuda.synchronize()
    h, r, c = dst.cpu().numpy().tobytes(), out.cpu().tolist(), cons.cpu().tolist()
    sample = set(random.Random(9).sample(range(n), 64))
    for i, b in enumerate(blocks):
        want = lz4dest(b, T)
        assert (r[i], c[i]) == want[:2], (i, r[i], c[i], want[:2])
        o = i * (T + G)
        if i in sample:
            assert h[o:o + r[i]] == want[2], i
        assert h[o + r[i]:o + T + G] == bytes([GUARD]) * (T + G - r[i]), ("guard", i)


def test_concurrent_single_calls(amd, lz4dest):
    """8 threads: destSize single calls interleaved with plain lz4hip_compress_fast single calls; coalescing keeps them apart"""
    l = amd.lib()
    book1 = calgary("book1")
    data = [book1[o:o + 65536] for o in range(0, 8 * 65536, 65536)]
    jobs = [(kind, v, t) for v in data for kind, t in (("dest", 4096), ("dest", 20000), ("dest", 1), ("fast", 0))] * 3
    random.Random(13).shuffle(jobs)
    barrier = threading.Barrier(8)
    errors = []

    def worker(k):
        barrier.wait()
        for kind, v, t in jobs[k::8]:
            if kind == "dest":
                out = (C.c_uint8 * t)()
                sz = C.c_int32(len(v))
                r = l.lz4hip_compress_dest_size(v, C.byref(sz), out, t)
                want = lz4dest(v, t)
                if (r, sz.value, bytes(out[:max(r, 0)])) != want:
                    errors.append(("dest", t, r, sz.value, want[:2]))
            else:
                cap = bound(len(v))
                out = (C.c_uint8 * cap)()
                r = l.lz4hip_compress_fast(v, len(v), out, cap)
                if r <= 0 or bytes(out[:r]) != lz4dest(v, cap)[2]:
                    errors.append(("fast", r))
    th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:10]


def test_single_call_edge_cases(amd, lz4dest):
    """the liblz4 edge cases through the single call: targets <= 0 and bad sizes leave *src_size alone, the empty block, tiny inputs"""
    l = amd.lib()
    v = calgary("book1")[:5000]
    for n, t in ((5000, 0), (5000, -3), (0, 1), (0, 20), (12, 1), (12, 5), (12, 13), (12, 40), (5000, 6), (5000, 5000), (5000, 6000)):
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int32(n)
        r = l.lz4hip_compress_dest_size(v[:n], C.byref(sz), out, t)
        want = lz4dest(v[:n], t)
        assert (r, sz.value, bytes(out[:max(r, 0)])) == want, (n, t)
    sz = C.c_int32(-1)
    assert l.lz4hip_compress_dest_size(v, C.byref(sz), (C.c_uint8 * 10)(), 10) == 0 and sz.value == -1


def test_python_factory(amd, lz4dest, O):
    f = amd.LZ4Factory.hipInstance()
    c = f.fastCompressor()
    v = O.gen_block(65536, 7)
    dst = bytearray(b"\xEE" * 5000)
    w, consumed = c.compressDestSize(v, 0, len(v), dst, 100, 4096)
    want = lz4dest(v, 4096)
    assert (w, consumed) == want[:2] and bytes(dst[100:100 + w]) == want[2]
    assert dst[:100] == b"\xEE" * 100 and dst[100 + w:] == b"\xEE" * (len(dst) - 100 - w)
    assert f.safeDecompressor().decompress(bytes(dst[100:100 + w]), consumed) == v[:consumed]
    out, cons = amd.LZ4HIPBatch.compressDestSize(v * 2, [0, 65536], [65536, 65536], bytearray(9000), [0, 4096], [4096, 4096])
    assert out == [w, w] and cons == [consumed, consumed]
    with pytest.raises(NotImplementedError):
        f.fastCompressor(acceleration=8).compressDestSize(v, 0, len(v), bytearray(4096), 0, 4096)


def test_cpp_mirror(lz4dest, tmp_path):
    """tests/cpp/destsize_mirror_test.cpp: LZ4HIPCompressor::compressDestSize of host/lz4hip.hpp, against the reference"""
    exe = build_mirror("destsize_mirror_test", tmp_path)
    v = calgary("book1")[7000:90000]
    (tmp_path / "in.bin").write_bytes(v)
    for t in (100, 4096, 30000):
        p = subprocess.run([exe, str(tmp_path / "in.bin"), str(t), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        w, consumed = map(int, p.stdout.decode().split())
        want = lz4dest(v, t)
        assert (w, consumed) == want[:2] and (tmp_path / "out.bin").read_bytes() == want[2], t


def test_jni_dest_size_full_scenarios(lz4dest, tmp_path):
    """the shim's new natives over the fake JNIEnv (tests/jni_stub/fake_jni_destsize.c): arrays, direct buffers, NULL arrays, a
    destination that cannot be pinned, the batch native; the stream and consumed size are the reference's"""
    exe = build_fake_jni("fake_jni_destsize", tmp_path)
    v = calgary("book1")[100000:165536]
    (tmp_path / "in.bin").write_bytes(v)
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), "16384", str(tmp_path)], timeout=300).decode()
    assert "checks ok" in out and "no device" not in out, out
    want = lz4dest(v, 16384)
    w, consumed = map(int, (tmp_path / "dest.txt").read_text().split())
    assert (w, consumed) == want[:2] and (tmp_path / "dest.bin").read_bytes() == want[2]


def test_multidevice_host_path():
    """lz4hip_init([0, 0]) in a child process: a ragged destSize batch across the device boundary"""
    assert "destsize multidev ok D=2" in run_child("destsize_multidev_child.py", "2", timeout=900)
