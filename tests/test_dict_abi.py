"""No-GPU checks of the dictionary decoder (LZ4_decompress_safe_usingDict): its C-ABI entry points are declared, exported and bound;
argument errors come first for the handle calls; a handle lives without a device (created, sized, freed) while every decode against it
fails LOUDLY there (no CPU fallback); dict_len == 0 is the plain decoder by the reference's own word; and the Python, C++ and JNI
layers carry the new calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from dict_common import RefDict, book1
from support import E_ARG, E_NO_DEVICE, LIB_ERROR, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_dict_create", "lz4hip_dict_size", "lz4hip_dict_free", "lz4hip_decompress_safe_dict_batch",
       "lz4hip_decompress_safe_dict_batch_dev", "lz4hip_decompress_safe_dict")


def test_dict_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    assert "typedef struct lz4hip_dict lz4hip_dict;" in h
    # the safe batch's shapes plus the handle / plus the dictionary's device pointer and length in front of (device, stream)
    safe = amd.C_ABI["lz4hip_decompress_safe_batch"][1]
    assert amd.C_ABI["lz4hip_decompress_safe_dict_batch"][1] == safe + [C.c_void_p]
    dev = amd.C_ABI["lz4hip_decompress_safe_batch_dev"][1]
    assert amd.C_ABI["lz4hip_decompress_safe_dict_batch_dev"][1] == dev[:8] + [C.c_void_p, C.c_int] + dev[8:]
    assert amd.C_ABI["lz4hip_decompress_safe_dict"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p])
    # the new kernels exist in the fat binary under their names (the profiles look kernels up by name)
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "decode_dict_kernel" in syms and "decode_dict_deep_kernel" in syms


def test_dict_handle_arguments_and_lifetime(amd):
    """NULL and a negative length are LZ4HIP_E_ARG whether or not a device exists; a handle keeps the TRUE length; freeing NULL is fine"""
    l = amd.lib()
    out = C.c_void_p(None)
    assert l.lz4hip_dict_create(None, 4, C.byref(out)) == E_ARG and not out
    assert l.lz4hip_dict_create(None, 0, C.byref(out)) == E_ARG and not out
    assert l.lz4hip_dict_create(b"abcd", -1, C.byref(out)) == E_ARG and not out
    assert l.lz4hip_dict_create(b"abcd", 4, None) == E_ARG
    assert b"null" in l.lz4hip_last_error()
    assert l.lz4hip_dict_size(None) == E_ARG
    l.lz4hip_dict_free(None)
    b = book1()
    for n in (0, 1, 4096, 65536, 65537, 300000):
        assert l.lz4hip_dict_create(b[:max(n, 1)], n, C.byref(out)) == 0 and out
        assert l.lz4hip_dict_size(out) == n
        l.lz4hip_dict_free(out)
        out = C.c_void_p(None)
    with amd.LZ4Dictionary(b[:1000]) as d:
        assert len(d) == 1000
    with pytest.raises(AssertionError):
        len(d)
    d.close()   # (twice is fine)


def test_dict_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    src, dst = (C.c_uint8 * 64)(*([0x10, 0x61] + [0] * 62)), (C.c_uint8 * 128)()
    so, sl, do = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_uint64 * 1)(0)
    dc, out = (C.c_int32 * 1)(100), (C.c_int32 * 1)(7)
    h = C.c_void_p(None)
    assert l.lz4hip_dict_create(b"0123456789", 10, C.byref(h)) == 0
    assert l.lz4hip_decompress_safe_dict_batch(src, so, sl, dst, do, dc, out, 1, h) == E_NO_DEVICE
    assert l.lz4hip_decompress_safe_dict_batch(None, None, None, None, None, None, None, 1, None) == E_NO_DEVICE   # (before any pointer is looked at)
    assert l.lz4hip_decompress_safe_dict_batch_dev(src, so, sl, dst, do, dc, out, 1, src, 10, 0, None) == E_NO_DEVICE
    assert l.lz4hip_decompress_safe_dict_batch_dev(None, None, None, None, None, None, None, 1, None, -1, 0, None) == E_NO_DEVICE
    assert out[0] == 7
    for n, c, hh in ((2, 100, h), (0, 5, h), (2, 0, h), (-1, 10, h), (2, -1, h), (2, 100, None)):
        assert l.lz4hip_decompress_safe_dict(src, n, dst, c, hh) == LIB_ERROR(E_NO_DEVICE)
    assert b"no HIP device" in l.lz4hip_last_error()
    assert bytes(dst) == bytes(128)   # nothing written
    l.lz4hip_dict_free(h)
    with amd.LZ4Dictionary(b"0123456789") as d:
        with pytest.raises(amd.LZ4HIPError):
            amd.LZ4SafeDecompressor().decompressWithDict(d, b"\x10a", 0, 2, bytearray(20), 0)
        with pytest.raises(amd.LZ4HIPError):
            amd.LZ4HIPBatch.decompressSafeDict(b"\x10a", [0], [2], bytearray(20), [0], [20], d)
    assert l.lz4hip_decompress_safe_dict_batch(None, None, None, None, None, None, None, 0, None) in (0, E_NO_DEVICE)


def test_dict_len_0_equals_the_plain_decoders_reference_value(ref):
    """the reference's LZ4_decompress_safe_usingDict with dictSize 0 returns what its LZ4_decompress_safe returns -- valid, cut and
    damaged streams, tight and roomy capacities: the value the engine's dict_len == 0 path (the plain decoder) is held to"""
    import random
    rd = RefDict(ref)
    b = book1()
    rng = random.Random(6)
    n = 0
    for v in (b[:300], b[1000:5096], b[300000:370000], b"abcd      abcdefghij", b""):
        s = ref.compress_fast(v)
        forms = [s, s[:len(s) // 2], s[:-1]] + [bytes(x if rng.random() > 0.01 else rng.randrange(256) for x in s) for _ in range(10)]
        for t in forms:
            for cap in (0, max(len(v) - 1, 0), len(v), len(v) + 1, len(v) + 100):
                r, by = rd.decode(t, cap, b"")
                assert r == rd.plain(t, cap), (len(v), len(t), cap)
                if t is s and cap >= len(v):
                    assert (r, by) == (len(v), v)
                n += 1
    assert n == 5 * 13 * 5


def test_dict_python_layer_checks(amd):
    d = amd.LZ4SafeDecompressor()
    with amd.LZ4Dictionary(b"0123456789") as h:
        with pytest.raises(IndexError):                                # the argument checks of decompress()
            d.decompressWithDict(h, b"abcdef", 2, 10, bytearray(100), 0)
        with pytest.raises(IndexError):
            d.decompressWithDict(h, b"abcdef", 0, 6, bytearray(10), 5, 20)
        with pytest.raises(amd.ReadOnlyBufferException):
            d.decompressWithDict(h, b"abcdef", 0, 6, b"\0" * 100, 0)
        with pytest.raises(IndexError):
            amd.LZ4HIPBatch.decompressSafeDict(b"abc", [2], [5], bytearray(10), [0], [10], h)
        with pytest.raises(IndexError):
            amd.LZ4HIPBatch.decompressSafeDict(b"abc", [0], [3], bytearray(10), [4], [10], h)
        with pytest.raises(ValueError):
            amd.LZ4HIPBatch.decompressSafeDict(b"abc", [0], [3], bytearray(10), [0], [4, 5], h)
    assert callable(amd.DeviceBatch.decompress_safe_dict)


def test_cpp_mirror_dict_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4Dictionary, LZ4SafeDecompressor::decompressWithDict and LZ4HIPBatch::decompressSafeDict build;
    tests/cpp/dict_mirror_test.cpp passes its argument checks and exits 3 (loud library failure) without a device"""
    exe = build_mirror("dict_mirror_test", tmp_path)
    if no_device():
        (tmp_path / "d.bin").write_bytes(b"0123456789")
        (tmp_path / "s.bin").write_bytes(b"\x10a")
        p = subprocess.run([exe, str(tmp_path / "d.bin"), str(tmp_path / "s.bin"), "10", str(tmp_path / "o.bin")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr


def test_jni_dict_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPDictionary / LZ4HIPBatch / LZ4HIPSafeDecompressor and defined in
    the shim; over the fake JNIEnv (tests/jni_stub/fake_jni_dict.c) NULL arguments are argument errors, a handle lives without a
    device and every decode fails loudly there"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    for sig in (r"static\s+native\s+long\s+LZ4HIP_dictCreate\s*\(", r"static\s+native\s+int\s+LZ4HIP_dictSize\s*\(",
                r"static\s+native\s+void\s+LZ4HIP_dictFree\s*\(", r"static\s+native\s+int\s+LZ4HIP_decompress_safe_dict\s*\(",
                r"static\s+native\s+int\s+LZ4HIP_batchSafeDict\s*\("):
        assert re.search(sig, java), sig
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_decompress_safe\(byte\[\] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,\s+"
                     r"byte\[\] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen\);", java)
    dic = open(os.path.join(jdir, "LZ4HIPDictionary.java")).read()
    assert re.search(r"public final class LZ4HIPDictionary implements Closeable", dic)
    for call in ("LZ4HIPJNI.LZ4HIP_dictCreate(", "LZ4HIPJNI.LZ4HIP_dictSize(", "LZ4HIPJNI.LZ4HIP_dictFree("):
        assert call in dic, call
    assert "LZ4HIPJNI.LZ4HIP_batchSafeDict(" in open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    safe = open(os.path.join(jdir, "LZ4HIPSafeDecompressor.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_decompress_safe_dict(" in safe
    assert len(re.findall(r"public (final )?int decompressWithDict\(LZ4HIPDictionary dict, (byte\[\]|ByteBuffer) src", safe)) == 2
    for name in ("dictCreate", "dictSize", "dictFree", "decompress_1safe_1dict", "batchSafeDict"):
        assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1" + name in shim, name
    exe = build_fake_jni("fake_jni_dict", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
