"""Accelerated fast compress on the GPU (-m gpu): every layer of LZ4_compress_fast(..., acceleration) -- compress_fast_accel_cu_kernel
through the host batch, the device batch, coalesced single calls, the multi-device host path, the Python factory and the JNI shim --
checked byte for byte against the reference library's own LZ4_compress_fast (oracle.ref_path())."""
import ctypes as C
import random
import subprocess
import threading

import numpy as np
import pytest

from conftest import ROOT, calgary, rnd_inputs
from support import build_fake_jni, run_child

pytestmark = pytest.mark.gpu
_u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lz4fast(ref):
    """(src, cap, acceleration) -> (ret, bytes) of the reference library's LZ4_compress_fast"""
    f = C.CDLL(ref.path).LZ4_compress_fast
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_int]
    memo = {}

    def run(v, cap, a):
        key = (v, cap, a)
        if key not in memo:
            out = (C.c_uint8 * max(cap, 1))()
            r = f(bytes(v), out, len(v), cap, a)
            memo[key] = (r, bytes(out[:max(r, 0)]))
        return memo[key]
    return run


def bound(n):
    return n + n // 255 + 16


def host_batch(amd, blocks, caps, a, fn="compress"):
    so = np.concatenate([[0], np.cumsum([len(b) for b in blocks])[:-1]]).astype(np.uint64)
    do = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    dst = bytearray(int(sum(caps)) + 1)
    if fn == "compress":
        out = amd.LZ4HIPBatch.compress(b"".join(blocks), so, np.array([len(b) for b in blocks], dtype=np.int32), dst, do,
                                       np.array(caps, dtype=np.int32), acceleration=a)
    else:   # the plain fast path, for comparison
        out = amd.LZ4HIPBatch.compress(b"".join(blocks), so, np.array([len(b) for b in blocks], dtype=np.int32), dst, do,
                                       np.array(caps, dtype=np.int32))
    return [int(x) for x in out], [bytes(dst[int(o):int(o) + max(int(r), 0)]) for o, r in zip(do, out)]


def test_host_batch_fuzz(amd, lz4fast, O, corpus):
    """~1500 mixed inputs x several accelerations x {full, tight, one byte short} capacities, one host batch per acceleration"""
    inputs = rnd_inputs(O, corpus, 41, 1500) + list(corpus.values())
    for a in (2, 3, 8, 17, 64, 1000, 65537, 70000):
        blocks, caps, want = [], [], []
        for v in inputs:
            er, _ = lz4fast(v, bound(len(v)), a)
            for cap in (bound(len(v)), er, max(0, er - 1)):
                blocks.append(v); caps.append(cap); want.append(lz4fast(v, cap, a))
        out, got = host_batch(amd, blocks, caps, a)
        for i, (r, b) in enumerate(zip(out, got)):
            assert r == want[i][0] and (r <= 0 or b == want[i][1]), (a, len(blocks[i]), caps[i], r, want[i][0])


def test_device_batch_mixed_sizes_with_guards(amd, lz4fast, O):
    """one _dev batch: 64 KiB App. F blocks, text slices, byU32 blocks of 1 MiB, 4 MiB and 5 MiB + 123; every destination slot sits
    between guard bytes that must not change"""
    import torch
    book1 = calgary("book1")
    rng = random.Random(12)
    blocks = [O.gen_block(65536, i) for i in range(40)]
    for _ in range(40):
        n = rng.choice([65536, 65546, 65547, 30000, 13, 12, 0, 100000])
        o = rng.randrange(len(book1) - n)
        blocks.append(book1[o:o + n])
    blocks += [O.gen_block(1 << 20, 1, win=4096), O.gen_block(4 << 20, 2, win=4096), O.gen_block((5 << 20) + 123, 3, win=4096), book1]
    G = 256
    for a in (2, 8, 64):
        want = [lz4fast(b, bound(len(b)), a) for b in blocks]
        caps = [bound(len(b)) if i % 5 else max(0, want[i][0] - 1) for i, b in enumerate(blocks)]
        so = np.concatenate([[0], np.cumsum([len(b) for b in blocks])[:-1]]).astype(np.int64)
        do, p = [], G
        for c in caps:
            do.append(p); p += c + G
        dev = torch.device("cuda:0")
        src = torch.frombuffer(bytearray(b"".join(blocks) + b"\0"), dtype=torch.uint8).to(dev)
        dst = torch.full((p,), 0xA5, dtype=torch.uint8, device=dev)
        out = torch.full((len(blocks),), -7, dtype=torch.int32, device=dev)
        amd.DeviceBatch.compress_fast(src, torch.tensor(so, device=dev), torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev),
                                      dst, torch.tensor(do, dtype=torch.int64, device=dev), torch.tensor(caps, dtype=torch.int32, device=dev), out,
                                      acceleration=a)
        torch.cuda.synchronize()
        h, r = dst.cpu().numpy().tobytes(), out.cpu().tolist()
        end = 0
        for i, b in enumerate(blocks):
            exp = want[i][0] if caps[i] >= want[i][0] else 0
            assert r[i] == exp, (a, i, len(b), caps[i], r[i], exp)
            if r[i] > 0:
                assert h[do[i]:do[i] + r[i]] == want[i][1], (a, i)
            assert h[end:do[i]] == b"\xA5" * (do[i] - end), ("guard in front of slot", a, i)
            end = do[i] + caps[i]
        assert h[end:] == b"\xA5" * (len(h) - end)


def test_acceleration_one_and_below_is_the_fast_path(amd, O, corpus):
    """after clamping, acceleration <= 1 is lz4hip_compress_fast_batch: identical results and bytes"""
    blocks = rnd_inputs(O, corpus, 42, 300) + [O.gen_block(65536, i) for i in range(8)]
    caps = [bound(len(b)) for b in blocks]
    base = host_batch(amd, blocks, caps, 1, fn="fast")
    for a in (1, 0, -5, -(2 ** 31)):
        assert host_batch(amd, blocks, caps, a) == base, a


def test_concurrent_single_calls_keep_their_acceleration(amd, lz4fast):
    """threads issue single calls with different accelerations at once: coalescing must never hand one caller another value's bytes"""
    book1 = calgary("book1")
    data = [book1[o:o + 65536] for o in range(0, 8 * 65536, 65536)]
    accels = (1, 2, 4, 8, 16, 64)
    for v in data[:2]:
        assert len({lz4fast(v, bound(len(v)), a)[1] for a in accels}) == len(accels)   # every value gives other bytes
    comps = {a: amd.LZ4HIPCompressor(acceleration=a) for a in accels}
    jobs = [(a, v) for _ in range(3) for a in accels for v in data]
    random.Random(13).shuffle(jobs)
    barrier = threading.Barrier(16)
    errors = []

    def worker(k):
        barrier.wait()
        for a, v in jobs[k::16]:
            try:
                got = comps[a].compress(v)
                if got != lz4fast(v, bound(len(v)), a)[1]:
                    errors.append((a, len(v)))
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append((a, repr(e)))
    th = [threading.Thread(target=worker, args=(k,)) for k in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:10]


def test_multidevice_host_path():
    """lz4hip_init([0, 0]) in a child process: a ragged accelerated batch across the device boundary"""
    assert "accel multidev ok D=2" in run_child("accel_multidev_child.py", "2", timeout=900)


def test_factory_accelerated_compressor_round_trips(amd, lz4fast, O):
    f = amd.LZ4Factory.hipInstance()
    assert f.fastCompressor() is f.fastCompressor(acceleration=1)    # the no-argument accessor still hands out the singleton
    c = f.fastCompressor(acceleration=8)
    for v in (O.gen_block(65536, 5), calgary("book1")[:200000], b"abcd      abcdefghij"):
        s = c.compress(v)
        assert s == lz4fast(v, bound(len(v)), 8)[1]
        assert f.safeDecompressor().decompress(s, len(v)) == v
    with pytest.raises(amd.LZ4Exception):
        v = O.gen_block(65536, 6)
        c.compress(v, 0, len(v), bytearray(100), 0, 100)


def test_jni_accel_native_full_scenarios(lz4fast, tmp_path):
    """the shim's new native over the fake JNIEnv (tests/jni_stub/fake_jni_accel.c): arrays, direct buffers, NULL arrays, a heap
    buffer without an address, a destination that cannot be pinned, too small a destination, the batch op; the streams of
    accelerations 1 and 8 are the reference's"""
    exe = build_fake_jni("fake_jni_accel", tmp_path)
    v = calgary("book1")[100000:165536]
    inp = tmp_path / "in.bin"
    inp.write_bytes(v)
    out = subprocess.check_output([exe, str(inp), str(tmp_path)], timeout=300).decode()
    assert "checks ok" in out and "no device" not in out, out
    for a in (1, 8):
        assert (tmp_path / ("accel_%d.bin" % a)).read_bytes() == lz4fast(v, bound(len(v)), a)[1], a
