"""No-GPU checks of the dictionary HC compressor (LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream): its C-ABI entry points
are declared, exported and bound; a handle that never compresses lives and dies as before and still answers its size; every compress
fails LOUDLY without a device (no CPU fallback) and before any pointer is looked at; and the Python, C++ and JNI layers carry the new
calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from dict_common import book1
from support import E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_compress_hc_dict_batch", "lz4hip_compress_hc_dict_batch_dev", "lz4hip_compress_hc_dict_batch_dev_ws", "lz4hip_compress_hc_dict")


def test_hcdict_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    # the HC batch's shapes plus the handle (behind the level; in front of (device, stream) for the device forms)
    hc = amd.C_ABI["lz4hip_compress_hc_batch"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dict_batch"][1] == hc + [C.c_void_p]
    dev = amd.C_ABI["lz4hip_compress_hc_batch_dev"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dict_batch_dev"][1] == dev[:9] + [C.c_void_p] + dev[9:]
    ws = amd.C_ABI["lz4hip_compress_hc_batch_dev_ws"][1]
    assert amd.C_ABI["lz4hip_compress_hc_dict_batch_dev_ws"][1] == ws[:9] + [C.c_void_p] + ws[9:]
    assert amd.C_ABI["lz4hip_compress_hc_dict"] == (C.c_int, amd.C_ABI["lz4hip_compress_hc"][1] + [C.c_void_p])
    # the header no longer says that there is no HC dictionary compressor
    assert "no HC dictionary compressor" not in h
    # the new kernels exist in the fat binary under their names (the profiles look kernels up by name)
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    for k in ("hc_dict_image_kernel", "hc_build_dict_kernel", "hc_parse_dict_kernel"):
        assert k in syms, k


def test_hcdict_handle_lifetime_without_a_compress(amd):
    """a handle that never compresses is created, sized and freed as before -- at every length around the 4-byte and 64 KB rules"""
    l = amd.lib()
    b = book1()
    for n in (0, 1, 3, 4, 5, 65535, 65536, 65537, 100000):
        out = C.c_void_p(None)
        assert l.lz4hip_dict_create(b[:max(n, 1)], n, C.byref(out)) == 0 and out
        assert l.lz4hip_dict_size(out) == n
        l.lz4hip_dict_free(out)


def test_hcdict_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(*range(64)), (C.c_uint8 * 128)()
    so, sl, do = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(20), (C.c_uint64 * 1)(0)
    dc, out = (C.c_int32 * 1)(100), (C.c_int32 * 1)(7)
    ws = (C.c_uint8 * 4096)()
    h = C.c_void_p(None)
    assert l.lz4hip_dict_create(b"0123456789", 10, C.byref(h)) == 0
    for level in (0, 1, 9, 12, 13):
        assert l.lz4hip_compress_hc_dict_batch(src, so, sl, dst, do, dc, out, 1, level, h) == E_NO_DEVICE
        assert l.lz4hip_compress_hc_dict_batch_dev(src, so, sl, dst, do, dc, out, 1, level, h, 0, None) == E_NO_DEVICE
        assert l.lz4hip_compress_hc_dict_batch_dev_ws(src, so, sl, dst, do, dc, out, 1, level, h, 0, None, 64, ws, 4096) == E_NO_DEVICE
    assert l.lz4hip_compress_hc_dict_batch(None, None, None, None, None, None, None, 1, 9, None) == E_NO_DEVICE   # (before any pointer is looked at)
    assert l.lz4hip_compress_hc_dict_batch_dev(None, None, None, None, None, None, None, 1, 9, None, 0, None) == E_NO_DEVICE
    assert l.lz4hip_compress_hc_dict_batch_dev_ws(None, None, None, None, None, None, None, 1, 9, None, 0, None, 0, None, 0) == E_NO_DEVICE
    assert out[0] == 7
    for n, c, hh in ((20, 100, h), (0, 5, h), (20, 0, h), (-1, 10, h), (20, -1, h), (20, 100, None)):
        assert l.lz4hip_compress_hc_dict(src, n, dst, c, 9, hh) == LIB_ERROR(E_NO_DEVICE)
    assert b"no HIP device" in l.lz4hip_last_error()
    assert bytes(dst) == bytes(128)   # nothing written
    assert l.lz4hip_dict_size(h) == 10   # (the handle's size still answers)
    l.lz4hip_dict_free(h)                # (a handle whose compress failed frees like any other)
    with amd.LZ4Dictionary(b"0123456789") as d:
        with pytest.raises(amd.LZ4HIPError):
            amd.LZ4HCHIPCompressor(9).compressWithDict(d, b"abcdefgh" * 4)
        with pytest.raises(amd.LZ4HIPError):
            amd.LZ4HIPBatch.compressHCDict(b"abcdefgh" * 4, [0], [32], bytearray(64), [0], [64], d, 9)
        assert len(d) == 10
    assert l.lz4hip_compress_hc_dict_batch(None, None, None, None, None, None, None, 0, 9, None) in (0, E_NO_DEVICE)


def test_hcdict_python_layer_checks(amd):
    c = amd.LZ4HCHIPCompressor(9)
    with amd.LZ4Dictionary(b"0123456789") as h:
        with pytest.raises(IndexError):                                # the argument checks of compress()
            c.compressWithDict(h, b"abcdef", 2, 10, bytearray(100), 0)
        with pytest.raises(IndexError):
            c.compressWithDict(h, b"abcdef", 0, 6, bytearray(10), 5, 20)
        with pytest.raises(amd.ReadOnlyBufferException):
            c.compressWithDict(h, b"abcdef", 0, 6, b"\0" * 100, 0)
        with pytest.raises(IndexError):
            amd.LZ4HIPBatch.compressHCDict(b"abc", [2], [5], bytearray(10), [0], [10], h)
        with pytest.raises(IndexError):
            amd.LZ4HIPBatch.compressHCDict(b"abc", [0], [3], bytearray(10), [4], [10], h, 3)
        with pytest.raises(ValueError):
            amd.LZ4HIPBatch.compressHCDict(b"abc", [0], [3], bytearray(10), [0], [4, 5], h)
    with pytest.raises(AssertionError):                                # a closed dictionary
        c.compressWithDict(h, b"abcdef")
    assert callable(amd.DeviceBatch.compress_hc_dict) and callable(amd.DeviceBatch.compress_hc_dict_sync)


def test_cpp_mirror_hcdict_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4HCHIPCompressor::compressWithDict and LZ4HIPBatch::compressHCDict build; tests/cpp/hcdict_mirror_test.cpp
    passes its argument checks and exits 3 (loud library failure) without a device"""
    exe = build_mirror("hcdict_mirror_test", tmp_path)
    if no_device():
        (tmp_path / "d.bin").write_bytes(b"0123456789")
        (tmp_path / "s.bin").write_bytes(b"abcdefgh" * 8)
        p = subprocess.run([exe, str(tmp_path / "d.bin"), str(tmp_path / "s.bin"), str(tmp_path / "o.bin"), "9"], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_hcdict_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HCHIPCompressor / LZ4HIPBatch and defined in the shim; over the fake
    JNIEnv (tests/jni_stub/fake_jni_hcdict.c) NULL arguments and a 0 handle are argument errors and every compress fails loudly
    without a device"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    for sig in (r"static\s+native\s+int\s+LZ4HIP_compress_hc_dict\s*\(long dict, int level,",
                r"static\s+native\s+int\s+LZ4HIP_batchCompressHCDict\s*\(long dict, int level,"):
        assert re.search(sig, java), sig
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_batchCompressDict\(long dict, ByteBuffer src, long\[\] srcOff, int\[\] srcLen, ByteBuffer dest, long\[\] destOff,\s+"
                     r"int\[\] destCap, int\[\] outLen, int nBlocks\);", java)
    assert "LZ4HIPJNI.LZ4HIP_batchCompressHCDict(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    comp = open(os.path.join(jdir, "LZ4HCHIPCompressor.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_compress_hc_dict(" in comp
    assert len(re.findall(r"public int compressWithDict\(LZ4HIPDictionary dict, (byte\[\]|ByteBuffer) src", comp)) == 2
    for name in ("compress_1hc_1dict", "batchCompressHCDict"):
        assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1" + name in shim, name
    exe = build_fake_jni("fake_jni_hcdict", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
