"""No-GPU checks of the decoded-size query: its three C-ABI entry points are declared, exported and bound, fail LOUDLY without a
device (no CPU fallback), report NULL arrays as argument errors and accept the empty batch, the Python wrappers do their range checks
before any call, and the C++ and JNI layers carry the new calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_decompressed_size_batch", "lz4hip_decompressed_size_batch_dev", "lz4hip_decompressed_size")


def test_size_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    # the safe batch's shapes without the destination buffer and its offsets
    safe = amd.C_ABI["lz4hip_decompress_safe_batch"][1]
    assert amd.C_ABI["lz4hip_decompressed_size_batch"][1] == safe[:3] + safe[5:]
    dev = amd.C_ABI["lz4hip_decompress_safe_batch_dev"][1]
    assert amd.C_ABI["lz4hip_decompressed_size_batch_dev"][1] == dev[:3] + dev[5:]
    assert amd.C_ABI["lz4hip_decompressed_size"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int])
    assert re.search(r"int\s+lz4hip_decompressed_size_batch\s*\(const uint8_t\* src, const uint64_t\* src_off, const int32_t\* src_len,\s*"
                     r"const int32_t\* dst_cap, int32_t\* out_len, uint32_t n_blocks\);", h)
    assert re.search(r"int\s+lz4hip_decompressed_size\s*\(const uint8_t\* src, int src_len, int dst_cap\);", h)
    # the new kernel exists in the fat binary under its name (the profiles look kernels up by name)
    assert "decode_size_kernel" in subprocess.check_output(["strings", so]).decode(errors="replace")


def test_size_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src = (C.c_uint8 * 64)(*([0x10, 0x61] + [0] * 62))
    so, sl, dc, out = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_int32 * 1)(100), (C.c_int32 * 1)(7)
    assert l.lz4hip_decompressed_size_batch(src, so, sl, dc, out, 1) == E_NO_DEVICE
    assert l.lz4hip_decompressed_size_batch_dev(src, so, sl, dc, out, 1, 0, None) == E_NO_DEVICE
    assert out[0] == 7
    for n, c in ((2, 100), (0, 5), (1, 0), (-1, 10), (2, -1)):   # (liblz4's own trivial cases included: no answer without a device)
        assert l.lz4hip_decompressed_size(src, n, c) == LIB_ERROR(E_NO_DEVICE)
    assert b"no HIP device" in l.lz4hip_last_error()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4SafeDecompressor().decompressedLength(b"\x10a", 0, 2, 20)
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.decompressedLengths(b"\x10a", [0], [2], [20])
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.decompressSafeSized(b"\x10a", [0], [2], [20])


def test_size_batch_null_arrays_and_empty_batch(amd):
    """without a device the status is LZ4HIP_E_NO_DEVICE before any pointer is looked at; the empty batch is fine; on a device NULL
    arrays are LZ4HIP_E_ARG"""
    l = amd.lib()
    if no_device():
        assert l.lz4hip_decompressed_size_batch(None, None, None, None, None, 1) == E_NO_DEVICE
        assert l.lz4hip_decompressed_size_batch_dev(None, None, None, None, None, 1, 0, None) == E_NO_DEVICE
    else:
        so, sl, dc, out = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_int32 * 1)(8), (C.c_int32 * 1)(7)
        src = (C.c_uint8 * 8)()
        args = [src, so, sl, dc, out]
        for k in range(len(args)):
            a = list(args)
            a[k] = None
            assert l.lz4hip_decompressed_size_batch(*a, 1) == E_ARG, k
            assert l.lz4hip_decompressed_size_batch_dev(*a, 1, 0, None) == E_ARG, k
        assert out[0] == 7
    assert l.lz4hip_decompressed_size_batch(None, None, None, None, None, 0) in (0, E_NO_DEVICE)
    assert l.lz4hip_decompressed_size_batch_dev(None, None, None, None, None, 0, 0, None) in (0, E_NO_DEVICE)


def test_size_python_layer_checks_before_any_call(amd, monkeypatch):
    """the range checks of decompress() run first: with a library that would fail the test on ANY call, the errors are the checks'"""
    class Trap:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    monkeypatch.setattr(amd, "lib", lambda: Trap())
    d = amd.LZ4SafeDecompressor()
    with pytest.raises(IndexError):
        d.decompressedLength(b"abcdef", 2, 10, 100)
    with pytest.raises(IndexError):
        d.decompressedLength(b"abcdef", -1, 3, 100)
    with pytest.raises(ValueError):
        d.decompressedLength(b"abcdef", 0, -1, 100)
    with pytest.raises(ValueError):
        d.decompressedLength(b"abcdef", 0, 6, -1)
    B = amd.LZ4HIPBatch
    for f in (B.decompressedLengths, B.decompressSafeSized):
        with pytest.raises(IndexError):
            f(b"abc", [2], [5], [10])
        with pytest.raises(ValueError):
            f(b"abc", [0], [3], [4, 5])
        with pytest.raises(ValueError):
            f(b"abc", [0], [3], [-4])
    assert callable(amd.DeviceBatch.decoded_size)


def test_cpp_mirror_size_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4SafeDecompressor::decompressedLength and LZ4HIPBatch::decompressedLengths / decompressSafeSized build;
    tests/cpp/size_mirror_test.cpp exits 3 (loud library failure) without a device"""
    exe = build_mirror("size_mirror_test", tmp_path)
    if no_device():
        stream = tmp_path / "s.bin"
        stream.write_bytes(b"\x10a")
        p = subprocess.run([exe, str(stream), "10", str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr


def test_jni_size_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch / LZ4HIPSafeDecompressor and defined in the shim; over the
    fake JNIEnv (tests/jni_stub/fake_jni_size.c) NULL arrays are argument errors, malloc / free balance, and without a device every
    call fails loudly"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_decompressed_length\s*\(byte\[\] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen, int maxDestLen\);", java)
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchDecompressedLengths\s*\(", java)
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_decompress_safe\(byte\[\] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,\s+"
                     r"byte\[\] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen\);", java)
    assert "LZ4HIPJNI.LZ4HIP_batchDecompressedLengths(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    safe = open(os.path.join(jdir, "LZ4HIPSafeDecompressor.java")).read()
    assert safe.count("LZ4HIPJNI.LZ4HIP_decompressed_length(") == 2
    assert len(re.findall(r"public (final )?int decompressedLength\((byte\[\]|ByteBuffer) src", safe)) == 2
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompressed_1length" in shim
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDecompressedLengths" in shim
    exe = build_fake_jni("fake_jni_size", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
