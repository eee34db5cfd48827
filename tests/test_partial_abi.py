"""No-GPU checks of the partial decoder (LZ4_decompress_safe_partial): its three C-ABI entry points are declared, exported and bound,
fail LOUDLY without a device (no CPU fallback), report NULL arrays as argument errors, and the Python, C++ and JNI layers carry the new
calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_decompress_safe_partial_batch", "lz4hip_decompress_safe_partial_batch_dev", "lz4hip_decompress_safe_partial")


def test_partial_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    # the safe batch's shapes plus the target array in front of the capacities
    safe = amd.C_ABI["lz4hip_decompress_safe_batch"][1]
    assert amd.C_ABI["lz4hip_decompress_safe_partial_batch"][1] == safe[:5] + [safe[5]] + safe[5:]
    dev = amd.C_ABI["lz4hip_decompress_safe_batch_dev"][1]
    assert amd.C_ABI["lz4hip_decompress_safe_partial_batch_dev"][1] == dev[:5] + [C.c_void_p] + dev[5:]
    assert amd.C_ABI["lz4hip_decompress_safe_partial"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int])
    # the new kernels exist in the fat binary under their names (the profiles look kernels up by name)
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "decode_partial_kernel" in syms and "decode_partial_deep_kernel" in syms


def test_partial_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(*([0x10, 0x61] + [0] * 62)), (C.c_uint8 * 128)()
    so, sl, do = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_uint64 * 1)(0)
    tl, dc, out = (C.c_int32 * 1)(1), (C.c_int32 * 1)(100), (C.c_int32 * 1)(7)
    assert l.lz4hip_decompress_safe_partial_batch(src, so, sl, dst, do, tl, dc, out, 1) == E_NO_DEVICE
    assert l.lz4hip_decompress_safe_partial_batch_dev(src, so, sl, dst, do, tl, dc, out, 1, 0, None) == E_NO_DEVICE
    assert out[0] == 7
    for n, t, c in ((2, 1, 100), (0, 5, 5), (2, 0, 0), (-1, 10, 10), (2, -1, 10), (2, 10, -1)):   # (liblz4's own trivial cases included)
        assert l.lz4hip_decompress_safe_partial(src, n, dst, t, c) == LIB_ERROR(E_NO_DEVICE)
    assert b"no HIP device" in l.lz4hip_last_error()
    assert bytes(dst) == bytes(128)   # nothing written
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4Factory.hipInstance()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4SafeDecompressor().decompressPartial(b"\x10a", 0, 2, bytearray(20), 0, 1)
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.decompressSafePartial(b"\x10a", [0], [2], bytearray(20), [0], [1], [20])


def test_partial_batch_null_arrays(amd):
    """without a device the status is LZ4HIP_E_NO_DEVICE before any pointer is looked at; the empty batch is fine; on a device NULL
    arrays are LZ4HIP_E_ARG"""
    l = amd.lib()
    if no_device():
        assert l.lz4hip_decompress_safe_partial_batch(None, None, None, None, None, None, None, None, 1) == E_NO_DEVICE
        assert l.lz4hip_decompress_safe_partial_batch_dev(None, None, None, None, None, None, None, None, 1, 0, None) == E_NO_DEVICE
    else:
        so, sl, do, tl, dc, out = ((C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(1), (C.c_int32 * 1)(8),
                                   (C.c_int32 * 1)(7))
        src, dst = (C.c_uint8 * 8)(), (C.c_uint8 * 8)()
        args = [src, so, sl, dst, do, tl, dc, out]
        for k in range(len(args)):
            a = list(args)
            a[k] = None
            assert l.lz4hip_decompress_safe_partial_batch(*a, 1) == E_ARG, k
        assert out[0] == 7
    assert l.lz4hip_decompress_safe_partial_batch(None, None, None, None, None, None, None, None, 0) in (0, E_NO_DEVICE)


def test_partial_python_layer(amd):
    d = amd.LZ4SafeDecompressor()
    with pytest.raises(IndexError):                                # the argument checks of decompress()
        d.decompressPartial(b"abcdef", 2, 10, bytearray(100), 0, 5)
    with pytest.raises(IndexError):
        d.decompressPartial(b"abcdef", 0, 6, bytearray(10), 5, 3, 20)
    with pytest.raises(amd.ReadOnlyBufferException):
        d.decompressPartial(b"abcdef", 0, 6, b"\0" * 100, 0, 5)
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.decompressSafePartial(b"abc", [2], [5], bytearray(10), [0], [4], [10])
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.decompressSafePartial(b"abc", [0], [3], bytearray(10), [4], [4], [10])
    with pytest.raises(ValueError):
        amd.LZ4HIPBatch.decompressSafePartial(b"abc", [0], [3], bytearray(10), [0], [4, 5], [10])
    assert callable(amd.DeviceBatch.decompress_safe_partial)


def test_cpp_mirror_partial_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4SafeDecompressor::decompressPartial(src, srcOff, srcLen, dest, destOff, targetLen, maxDestLen) builds;
    tests/cpp/partial_mirror_test.cpp exits 3 (loud library failure) without a device"""
    exe = build_mirror("partial_mirror_test", tmp_path)
    if no_device():
        stream = tmp_path / "s.bin"
        stream.write_bytes(b"\x10a")
        p = subprocess.run([exe, str(stream), "10", "10", str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr


def test_jni_partial_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch / LZ4HIPSafeDecompressor and defined in the shim; over the
    fake JNIEnv (tests/jni_stub/fake_jni_partial.c) NULL arrays are argument errors and without a device every call fails loudly"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_decompress_safe_partial\s*\(", java)
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchSafePartial\s*\(", java)
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_decompress_safe\(byte\[\] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,\s+"
                     r"byte\[\] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen\);", java)
    assert "LZ4HIPJNI.LZ4HIP_batchSafePartial(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    safe = open(os.path.join(jdir, "LZ4HIPSafeDecompressor.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_decompress_safe_partial(" in safe
    assert len(re.findall(r"public (final )?int decompressPartial\((byte\[\]|ByteBuffer) src", safe)) == 2
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe_1partial" in shim
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafePartial" in shim
    exe = build_fake_jni("fake_jni_partial", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
