"""No-GPU checks of HC compress-to-a-target-size (LZ4_compress_HC_destSize): its four C-ABI entry points are declared, exported and
bound, hc_parse_dest_kernel is in the fat binary, every entry fails LOUDLY without a device (no CPU fallback) and writes nothing,
NULL and length errors are reported and *src_size stays untouched on failure; the Python, C++ and JNI layers carry the new calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_compress_hc_dest_size_batch", "lz4hip_compress_hc_dest_size_batch_dev", "lz4hip_compress_hc_dest_size_batch_dev_ws",
       "lz4hip_compress_hc_dest_size")


def test_hc_dest_size_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    assert "lz4hip_compress_hc_dest_size*" in h.split("#ifndef LZ4HIP_H")[0]   # the header's opening table
    # the shapes of the HC entries plus the consumed-size array
    hc = amd.C_ABI["lz4hip_compress_hc_batch"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dest_size_batch"][1] == hc[:7] + [hc[6]] + hc[7:]
    dev = amd.C_ABI["lz4hip_compress_hc_batch_dev"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dest_size_batch_dev"][1] == dev[:7] + [C.c_void_p] + dev[7:]
    ws = amd.C_ABI["lz4hip_compress_hc_batch_dev_ws"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dest_size_batch_dev_ws"][1] == ws[:7] + [C.c_void_p] + ws[7:]
    assert amd.C_ABI["lz4hip_compress_hc_dest_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int])


def test_hc_parse_dest_kernel_is_in_the_fat_binary():
    """the gfx950 kernel behind the entry points is compiled into liblz4hip.so, next to the two kernels it is built from"""
    blob = open(os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so"), "rb").read()
    for k in (b"hc_parse_dest_kernel", b"hc_parse_kernel", b"hc_build_kernel"):
        assert re.search(rb"_ZN6lz4hip\d+" + k, blob), k
    assert b"gfx950" in blob


def test_null_src_size_is_an_argument_error(amd):
    """a NULL src_size is LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG), device or not, at every level, and says so"""
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    for level in (0, 1, 9, 12, 13):
        assert l.lz4hip_compress_hc_dest_size(src, None, dst, 30, level) == LIB_ERROR(E_ARG)
        assert b"src_size" in l.lz4hip_last_error()


def test_hc_dest_size_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 128)(*([0xA5] * 128))
    so, sl, do, ts = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(40), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(30)
    out, cons = (C.c_int32 * 1)(7), (C.c_int32 * 1)(9)
    ws = (C.c_uint8 * 4096)()
    for level in (1, 9, 10, 12):
        assert l.lz4hip_compress_hc_dest_size_batch(src, so, sl, dst, do, ts, out, cons, 1, level) == E_NO_DEVICE
        assert l.lz4hip_compress_hc_dest_size_batch_dev(src, so, sl, dst, do, ts, out, cons, 1, level, 0, None) == E_NO_DEVICE
        assert l.lz4hip_compress_hc_dest_size_batch_dev_ws(src, so, sl, dst, do, ts, out, cons, 1, level, 0, None, 64, ws, 4096) == E_NO_DEVICE
        assert (out[0], cons[0]) == (7, 9)
        for n, t in ((40, 30), (0, 1), (-1, 10), (40, 0), (40, -5)):   # (liblz4's own zero cases included: no answer without a device)
            size = C.c_int32(n)
            assert l.lz4hip_compress_hc_dest_size(src, C.byref(size), dst, t, level) == LIB_ERROR(E_NO_DEVICE)
            assert size.value == n   # untouched on failure
        assert b"no HIP device" in l.lz4hip_last_error()
    assert bytes(dst) == b"\xa5" * 128   # nothing was written
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HCHIPCompressor(9).compressDestSize(b"hello hello hello hello", 0, 23, bytearray(20), 0, 20)
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.compressHCDestSize(b"x" * 40, [0], [40], bytearray(100), [0], [30], 9)


def test_hc_dest_size_batch_null_arrays_without_device(amd):
    """without a device the status is LZ4HIP_E_NO_DEVICE before any pointer is looked at"""
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    assert l.lz4hip_compress_hc_dest_size_batch(None, None, None, None, None, None, None, None, 1, 9) == E_NO_DEVICE
    assert l.lz4hip_compress_hc_dest_size_batch_dev(None, None, None, None, None, None, None, None, 1, 9, 0, None) == E_NO_DEVICE
    assert l.lz4hip_compress_hc_dest_size_batch_dev_ws(None, None, None, None, None, None, None, None, 1, 9, 0, None, 0, None, 0) == E_NO_DEVICE


def test_hc_dest_size_is_described_once_in_the_op_table():
    """csrc/api.cpp: one Op for the operation, and the op predicates are what route it (no entry point compares ops itself)"""
    api = open(os.path.join(ROOT, "lz4-java_amd", "csrc", "api.cpp")).read()
    assert re.search(r"enum Op \{[^}]*OP_COMPRESS_HC_DEST[^}]*\}", api)
    for pred in ("op_compresses", "op_has_consumed", "op_uses_hc_ws"):
        assert re.search(r"constexpr bool %s\(Op op\) \{[^}]*OP_COMPRESS_HC_DEST[^}]*\}" % pred, api), pred
    body = api.split("// ---- host-pointer path")[1]
    assert len(re.findall(r"c\.op == OP_COMPRESS_HC_DEST", body)) == 1   # combiner_for: the per-level combiners


def test_hc_dest_size_python_layer(amd):
    c = amd.LZ4HCHIPCompressor(9)
    with pytest.raises(IndexError):                                # the argument checks of compress()
        c.compressDestSize(b"abcdef", 2, 10, bytearray(100), 0, 100)
    with pytest.raises(IndexError):
        c.compressDestSize(b"abcdef", 0, 6, bytearray(10), 5, 20)
    with pytest.raises(ValueError):
        c.compressDestSize(b"abcdef", 0, 6, bytearray(10), 0, -1)
    with pytest.raises(amd.ReadOnlyBufferException):
        c.compressDestSize(b"abcdef", 0, 6, b"\0" * 100, 0, 100)
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.compressHCDestSize(b"abc", [2], [5], bytearray(10), [0], [10], 9)
    with pytest.raises(IndexError):
        amd.LZ4HIPBatch.compressHCDestSize(b"abc", [0], [3], bytearray(10), [4], [10], 9)
    with pytest.raises(ValueError):
        amd.LZ4HIPBatch.compressHCDestSize(b"abc", [0], [3], bytearray(10), [0, 1], [10], 9)
    assert callable(amd.DeviceBatch.compress_hc_dest_size) and callable(amd.DeviceBatch.compress_hc_dest_size_sync)
    assert amd.LZ4Factory.hipInstance is not None and hasattr(amd.LZ4HCHIPCompressor, "compressDestSize")


def test_cpp_mirror_hc_dest_size_builds(tmp_path):
    """host/lz4hip.hpp: LZ4HCHIPCompressor::compressDestSize(src, srcOff, int& srcLen, dest, destOff, target), through
    tests/cpp/hc_destsize_mirror_test.cpp; loud without a device (exit code 3)"""
    exe = build_mirror("hc_destsize_mirror_test", tmp_path)
    if no_device():
        (tmp_path / "in.bin").write_bytes(b"to be or not to be, that is the question " * 40)
        p = subprocess.run([exe, str(tmp_path / "in.bin"), "100", str(tmp_path / "out.bin"), "9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)
        assert not (tmp_path / "out.bin").exists()


def test_jni_hc_dest_size_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch / LZ4HCHIPCompressor and defined in the shim; over the fake
    JNIEnv (tests/jni_stub/fake_jni_hc_destsize.c) NULL arrays are argument errors and without a device every call fails loudly"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_compressHC_dest_size\s*\(", java)
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchHCDestSize\s*\(", java)
    # the existing destSize natives keep their signatures
    assert re.search(r"static native int LZ4HIP_compress_dest_size\(byte\[\] srcArray, ByteBuffer srcBuffer, int srcOff, int\[\] srcSize,\s+"
                     r"byte\[\] destArray, ByteBuffer destBuffer, int destOff, int targetDestSize\);", java)
    assert "LZ4HIPJNI.LZ4HIP_batchHCDestSize(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    hcj = open(os.path.join(jdir, "LZ4HCHIPCompressor.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_compressHC_dest_size(" in hcj
    assert len(re.findall(r"public int compressDestSize\(", hcj)) == 2    # arrays and buffers
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compressHC_1dest_1size" in shim
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCDestSize" in shim
    exe = build_fake_jni("fake_jni_hc_destsize", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
