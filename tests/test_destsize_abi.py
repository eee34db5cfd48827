"""No-GPU checks of compress-to-a-target-size (LZ4_compress_destSize): its three C-ABI entry points are declared, exported and bound,
fail LOUDLY without a device (no CPU fallback), report NULL and length errors and leave *src_size untouched on failure; the Python,
C++, shard.py and JNI layers carry the new calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_compress_dest_size_batch", "lz4hip_compress_dest_size_batch_dev", "lz4hip_compress_dest_size")


def test_dest_size_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    # the batch shapes of the fast path plus the consumed-size array
    fast = amd.C_ABI["lz4hip_compress_fast_batch"][1]
    assert amd.C_ABI["lz4hip_compress_dest_size_batch"][1] == fast[:7] + [fast[6]] + fast[7:]
    dev = amd.C_ABI["lz4hip_compress_fast_batch_dev"][1]
    assert amd.C_ABI["lz4hip_compress_dest_size_batch_dev"][1] == dev[:7] + [C.c_void_p] + dev[7:]
    assert amd.C_ABI["lz4hip_compress_dest_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int])


def test_null_src_size_is_an_argument_error(amd):
    """a NULL src_size is LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG), device or not, and says so"""
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert l.lz4hip_compress_dest_size(src, None, dst, 30) == LIB_ERROR(E_ARG)
    assert b"src_size" in l.lz4hip_last_error()


def test_dest_size_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 128)()
    so, sl, do, ts = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(40), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(30)
    out, cons = (C.c_int32 * 1)(7), (C.c_int32 * 1)(9)
    assert l.lz4hip_compress_dest_size_batch(src, so, sl, dst, do, ts, out, cons, 1) == E_NO_DEVICE
    assert l.lz4hip_compress_dest_size_batch_dev(src, so, sl, dst, do, ts, out, cons, 1, 0, None) == E_NO_DEVICE
    assert (out[0], cons[0]) == (7, 9)
    for n, t in ((40, 30), (0, 1), (-1, 10), (40, 0), (40, -5)):   # (liblz4's own zero cases included: no answer without a device)
        size = C.c_int32(n)
        assert l.lz4hip_compress_dest_size(src, C.byref(size), dst, t) == LIB_ERROR(E_NO_DEVICE)
        assert size.value == n   # untouched on failure
    assert b"no HIP device" in l.lz4hip_last_error()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPCompressor().compressDestSize(b"hello hello hello hello", 0, 23, bytearray(20), 0, 20)
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.compressDestSize(b"x" * 40, [0], [40], bytearray(100), [0], [30])
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPCompressor(acceleration=0).compressDestSize(b"abc", 0, 3, bytearray(8), 0, 8)   # (0 acts as 1: allowed)


def test_dest_size_batch_null_arrays_without_device(amd):
    """without a device the status is LZ4HIP_E_NO_DEVICE before any pointer is looked at; the empty batch is fine"""
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    assert l.lz4hip_compress_dest_size_batch(None, None, None, None, None, None, None, None, 1) == E_NO_DEVICE


def test_dest_size_python_layer(amd):
    c = amd.LZ4HIPCompressor()
    with pytest.raises(NotImplementedError):                       # liblz4 has no accelerated destSize
        amd.LZ4HIPCompressor(acceleration=8).compressDestSize(b"abcdef", 0, 6, bytearray(100), 0, 100)
    with pytest.raises(IndexError):                                # the argument checks of compress()
        c.compressDestSize(b"abcdef", 2, 10, bytearray(100), 0, 100)
    with pytest.raises(IndexError):
        c.compressDestSize(b"abcdef", 0, 6, bytearray(10), 5, 20)
    with pytest.raises(ValueError):
        c.compressDestSize(b"abcdef", 0, 6, bytearray(10), 0, -1)
    with pytest.raises(amd.ReadOnlyBufferException):
        c.compressDestSize(b"abcdef", 0, 6, b"\0" * 100, 0, 100)
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.compressDestSize(b"abc", [2], [5], bytearray(10), [0], [10])
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.compressDestSize(b"abc", [0], [3], bytearray(10), [4], [10])
    with pytest.raises(ValueError):
        amd.LZ4HIPBatch.compressDestSize(b"abc", [0], [3], bytearray(10), [0, 1], [10])
    assert callable(amd.DeviceBatch.compress_dest_size)


def test_shard_dest_size_gathers_both_arrays():
    """shard.compress_dest_size_sharded in one process (world 1): the codec's two arrays come back as they are"""
    import torch
    from importlib import import_module
    shard = import_module("lz4-java_amd.shard")
    calls = []

    def codec(b0, b1):
        calls.append((b0, b1))
        return torch.arange(b0, b1, dtype=torch.int32), torch.arange(b0, b1, dtype=torch.int32) * 2
    (b0, b1), sizes, cons = shard.compress_dest_size_sharded(codec, 7)
    assert (b0, b1) == (0, 7) and calls == [(0, 7)]
    assert sizes.tolist() == list(range(7)) and cons.tolist() == [2 * i for i in range(7)]


def _gloo_rank(rank, world, port, n_blocks, q):
    import torch
    import torch.distributed as dist
    from importlib import import_module
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = import_module("lz4-java_amd.shard")

        def codec(b0, b1):   # a fake codec: block i "writes" 1000 + i bytes and "consumes" 5000 + 3 i
            idx = torch.arange(b0, b1, dtype=torch.int32)
            return 1000 + idx, 5000 + 3 * idx
        rng, sizes, cons = shard.compress_dest_size_sharded(codec, n_blocks)
        q.put((rank, rng, sizes.tolist(), cons.tolist()))
    finally:
        dist.destroy_process_group()


def test_shard_dest_size_gloo_world_2():
    """a gloo world of 2 with an uneven block count: each rank runs its contiguous range, both arrays are all-gathered in block order"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    n_blocks = 11
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, n_blocks, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [(0, 5), (5, 11)]
    for _, _, sizes, cons in res:
        assert sizes == [1000 + i for i in range(n_blocks)] and cons == [5000 + 3 * i for i in range(n_blocks)]


def test_cpp_mirror_dest_size_builds(tmp_path):
    """host/lz4hip.hpp: LZ4HIPCompressor::compressDestSize(src, srcOff, int& srcLen, dest, destOff, target); loud without a device,
    srcLen untouched; an accelerated compressor throws std::logic_error"""
    cpp = tmp_path / "dest_mirror.cpp"
    cpp.write_text(r'''
#include "lz4-java_amd/host/lz4hip.hpp"
#include <cstdio>
#include <stdexcept>
using namespace net::jpountz;
int main() {
  const lz4::LZ4HIPCompressor c, accel(8);
  const bytes in(1000, 'a');
  bytes out(100);
  int len = 1000;
  try { (void)accel.compressDestSize(in, 0, len, out, 0, 100); return 4; } catch (const std::logic_error&) {}
  try { int bad = 2000; (void)c.compressDestSize(in, 0, bad, out, 0, 100); return 5; } catch (const std::out_of_range&) {}
  try {
    const int w = c.compressDestSize(in, 0, len, out, 0, 100);
    std::printf("%d %d\n", w, len);
    return 0;
  } catch (const lz4::LZ4Exception&) { std::printf("%d\n", len); return 3; }
}
''')
    exe = build_mirror("dest_mirror", tmp_path, src=cpp)
    if no_device():
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        assert p.returncode == 3 and p.stdout.decode().strip() == "1000"   # loud failure, srcLen untouched


def test_jni_dest_size_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch / LZ4HIPCompressor and defined in the shim; over the fake
    JNIEnv (tests/jni_stub/fake_jni_destsize.c) NULL arrays are argument errors and without a device every call fails loudly"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_compress_dest_size\s*\(", java)
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchDestSize\s*\(", java)
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_batch\(int op, int level, ByteBuffer src, long\[\] srcOff, int\[\] srcLen,\s+ByteBuffer dest, "
                     r"long\[\] destOff, int\[\] destCap, int\[\] outLen, int nBlocks\);", java)
    assert "LZ4HIPJNI.LZ4HIP_batchDestSize(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_compress_dest_size(" in open(os.path.join(jdir, "LZ4HIPCompressor.java")).read()
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1dest_1size" in shim
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDestSize" in shim
    exe = build_fake_jni("fake_jni_destsize", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
