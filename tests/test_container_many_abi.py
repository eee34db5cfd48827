"""No-GPU checks of the many-container read call: the two C-ABI entry points are declared, exported and bound; every argument error
is said before a device is looked for; the call of no items is fine; a well-formed call fails LOUDLY without a device; the bound call
equals lz4hip_container_decode_bound item by item on the case list (hostile headers size nothing); the header's new section says what
the call promises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import container_many_common as cm
from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, no_device

NEW = ("lz4hip_container_decode_many_bound", "lz4hip_container_decode_many")
HEAD = (r"int kind, const uint8_t\* bodies, const uint64_t\* body_off, const uint64_t\* body_len,\s*const uint32_t\* max_block, "
        r"const uint8_t\* flags, uint32_t n_items, uint32_t n_max,\s*")


@pytest.fixture(scope="module")
def case_list(ref, corpus):
    return cm.cases(ref, corpus)


def test_many_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert s in exported and s in amd.C_ABI and hasattr(amd.lib(), s), s
    assert not [s for s in exported if "container_decode_many" in s and s.endswith("_dev")]
    assert re.search(r"int lz4hip_container_decode_many_bound\(" + HEAD + r"uint32_t\* item_blocks, uint64_t\* item_dst_bytes\);", h)
    assert re.search(r"int lz4hip_container_decode_many\(" + HEAD + r"uint8_t\* dst, uint64_t dst_cap, uint64_t\* item_dst_off, uint32_t\* item_first, "
                     r"int32_t\* sizes,\s*uint32_t sizes_cap, uint64_t\* info\);", h)
    u64p, u32p, u8p, i32p = (C.POINTER(t) for t in (C.c_uint64, C.c_uint32, C.c_uint8, C.c_int32))
    head = [C.c_int, C.c_void_p, u64p, u64p, u32p, u8p, C.c_uint32, C.c_uint32]
    assert amd.C_ABI[NEW[0]] == (C.c_int, head + [u32p, u64p])
    assert amd.C_ABI[NEW[1]] == (C.c_int, head + [u8p, C.c_uint64, u64p, u32p, i32p, C.c_uint32, u64p])
    strings = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "container_walk_many_kernel" in strings and "container_verdict_many_kernel" in strings
    assert callable(amd.LZ4HIPBatch.containerDecodeMany)


def test_many_header_section(amd):
    h = " ".join(open(os.path.join(ROOT, "include", "lz4hip.h")).read().replace("*", " ").split())
    for sentence in ("The contract is the existing call, item by item",
                     "bit 0 of flags[c] means the frame has block checksums, and items with and without them may be mixed in one call",
                     "Delivered blocks lie back to back, item after item",
                     "item_dst_off[n_items] is the total written, and nothing at or behind it is written",
                     "An item that stops for any reason changes nothing about any other item",
                     "LZ4HIP_E_ARG is said before a device is looked for",
                     "n_items == 0 is LZ4HIP_OK with item_dst_off[0] = item_first[0] = 0",
                     "Device memory is sized by what the bodies hold and never by n_max x max_block",
                     "An item of thousands of blocks walks slowly there",
                     "Out of scope: writing many containers per call; device-pointer forms; mixing kinds in one call; sharding items over several "
                     "devices; linked-block frames inside the many-call; a parallel walk inside one item."):
        assert sentence in h, sentence


def _call(L, kind, pk, n_max, dst_cap, sizes_cap, null=None, bound_null=None):
    n = pk.n
    dst, sizes, info = np.zeros(max(dst_cap, 1), np.uint8), np.zeros(max(sizes_cap, 1), np.int32), np.zeros(5 * n + 1, np.uint64)
    doff, first = np.full(n + 1, 9, np.uint64), np.full(n + 1, 9, np.uint32)
    args = list(pk.head(kind, n_max)) + [cm._p(dst, C.c_uint8), dst_cap, cm._p(doff, C.c_uint64), cm._p(first, C.c_uint32), cm._p(sizes, C.c_int32),
                                         sizes_cap, cm._p(info, C.c_uint64)]
    if null is not None:
        args[null] = None
    return L.lz4hip_container_decode_many(*args), doff, first


def test_many_argument_errors_come_before_the_device_check(amd, ref, corpus):
    """every LZ4HIP_E_ARG case, on a machine without a device too: it is said before a device is looked for"""
    L = amd.lib()
    text = corpus["book1[:200000]"]
    items = [("a", 0, cm.frame_body(ref, [text[:3000]], True), 65536, True), ("b", 0, cm.frame_body(ref, [text[:500], text[:70]], False), 65536, False)]
    pk = cm.Packed(items)
    nb, need = cm.bound_many(L, 0, pk, 8)
    assert list(nb) == [1, 2] and list(need) == [65536, 65536 + 70]
    cap, scap = int(need.sum()), int(nb.sum())
    good = _call(L, 0, pk, 8, cap, scap)[0]
    assert good == (E_NO_DEVICE if no_device() else 0), (good, L.lz4hip_last_error())
    if no_device():
        assert b"no HIP device" in L.lz4hip_last_error()
    for kind in (-1, 2):
        assert _call(L, kind, pk, 8, cap, scap)[0] == E_ARG and b"kind" in L.lz4hip_last_error()
        assert L.lz4hip_container_decode_many_bound(*pk.head(kind, 8), cm._p(nb, C.c_uint32), cm._p(need, C.c_uint64)) == E_ARG
    for k in (1, 2, 3, 4, 5, 8, 10, 11, 12, 14):      # bodies, body_off, body_len, max_block, flags, dst, item_dst_off, item_first, sizes, info
        assert _call(L, 0, pk, 8, cap, scap, null=k)[0] == E_ARG, k
        assert b"null pointer" in L.lz4hip_last_error(), k
    for n_max in (0, 1 << 31):
        assert _call(L, 0, pk, n_max, cap, scap)[0] == E_ARG and b"2^31 - 1" in L.lz4hip_last_error()
    for mb in (0, 1 << 31):
        bad = cm.Packed(items); bad.mb[1] = mb
        assert _call(L, 0, bad, 8, cap, scap)[0] == E_ARG and b"2^31 - 1" in L.lz4hip_last_error()
        assert L.lz4hip_container_decode_many_bound(*bad.head(0, 8), cm._p(nb, C.c_uint32), cm._p(need, C.c_uint64)) == E_ARG
    for fl in (2, 3, 0x80):
        bad = cm.Packed(items); bad.fl[0] = fl
        assert _call(L, 0, bad, 8, cap, scap)[0] == E_ARG and b"bit 0" in L.lz4hip_last_error()
    assert _call(L, 0, pk, 8, cap - 1, scap)[0] == E_ARG and b"dst_cap" in L.lz4hip_last_error() and b"sizes_cap" not in L.lz4hip_last_error()
    assert _call(L, 0, pk, 8, cap, scap - 1)[0] == E_ARG and b"sizes_cap" in L.lz4hip_last_error() and b"dst_cap" not in L.lz4hip_last_error()


def test_many_call_of_no_items(amd):
    L = amd.lib()
    pk = cm.Packed([])
    rc, doff, first = _call(L, 1, pk, 4, 0, 0)
    assert rc == 0 and doff[0] == 0 and first[0] == 0
    doff, first = np.full(1, 9, np.uint64), np.full(1, 9, np.uint32)
    assert L.lz4hip_container_decode_many(0, None, None, None, None, None, 0, 4, None, 0, cm._p(doff, C.c_uint64), cm._p(first, C.c_uint32), None, 0, None) == 0
    assert doff[0] == 0 and first[0] == 0
    assert L.lz4hip_container_decode_many_bound(0, None, None, None, None, None, 0, 4, None, None) == 0
    assert amd.LZ4HIPBatch.containerDecodeMany(0, [], [], 4, []) == []


@pytest.mark.parametrize("n_max", [1, 2, 64])
def test_many_bound_equals_the_single_bound_item_by_item(amd, case_list, n_max):
    L = amd.lib()
    for kind in (cm.FRAME, cm.LZ4BLOCK):
        items = cm.of_kind(case_list, kind)
        assert len(items) > 300
        nb, need = cm.bound_many(L, kind, cm.Packed(items, pad=3), n_max)
        for i, (name, _, body, mb, cks) in enumerate(items):
            one_nb, one_need = C.c_uint32(7), C.c_uint64(7)
            buf = (C.c_uint8 * max(len(body), 1)).from_buffer_copy(body or b"\0")
            assert L.lz4hip_container_decode_bound(kind, 1 if cks else 0, buf, len(body), mb, n_max, C.byref(one_nb), C.byref(one_need)) == 0
            assert (int(nb[i]), int(need[i])) == (one_nb.value, one_need.value), name


def test_cpp_mirror_many_builds_and_fails_loudly(tmp_path, case_list):
    """host/lz4hip_streams.hpp: BatchEngine::containerDecodeMany builds (-Werror); tests/cpp/container_many_mirror_test.cpp exits 3
    (loud library failure) without a device"""
    from support import build_mirror
    exe = build_mirror("container_many_mirror_test", tmp_path, werror=True)
    if no_device():
        (tmp_path / "c.bin").write_bytes(cm.case_file(cm.of_kind(case_list, cm.FRAME)[:5], 4))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)
        # readFrames of the C++ mirror: the frame header's checksum is the first thing that needs the device
        import struct
        frame = bytes.fromhex("04224d186040") + b"\x82" + b"\0\0\0\0"
        (tmp_path / "s.bin").write_bytes(struct.pack("<IQ", 1, len(frame)) + frame)
        p = subprocess.run([exe, "--streams", "0", "4", str(tmp_path / "s.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stdout, p.stderr)


def test_jni_many_natives_declared_and_checked_without_device(tmp_path):
    """the natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim, which type-checks; over the fake
    JNIEnv (tests/jni_stub/fake_jni_container_many.c) NULL and short arrays are argument errors, the bound native needs no device,
    malloc / free balance, and without a device the read fails loudly"""
    from support import build_fake_jni, typecheck_jni_shim
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static native int LZ4HIP_containerDecodeMany\(int kind, ByteBuffer bodies, long\[\] bodyOff, long\[\] bodyLen, int\[\] maxBlock, "
                     r"int\[\] flags,\s+int nItems, int nMax, ByteBuffer dest, long destOff, long destCap, long\[\] itemDstOff, int\[\] itemFirst, "
                     r"int\[\] sizes, long\[\] info\);", java)
    assert re.search(r"static native int LZ4HIP_containerDecodeManyBound\(", java)
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_containerDecode\(int kind, int flags, ByteBuffer src, long srcOff, long len, int maxBlock, int nMax,\s+"
                     r"ByteBuffer dest, long destOff, long destCap, int\[\] sizes, long\[\] info\);", java)
    assert "LZ4HIPJNI.LZ4HIP_containerDecodeMany(" in batch and "LZ4HIPJNI.LZ4HIP_containerDecodeManyBound(" in batch
    assert re.search(r"public static void containerDecodeMany\(int kind, ByteBuffer bodies,", batch)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeMany(" in shim and "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeManyBound(" in shim
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_container_many", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out


def test_many_hostile_headers_size_nothing(amd, case_list):
    L = amd.lib()
    items = [c for c in case_list if c[0] == "lz4block-hostile-5k"] * 3
    assert len(items) == 3 and 5000 < len(items[0][2]) < 6000
    nb, need = cm.bound_many(L, cm.LZ4BLOCK, cm.Packed(items), 256)
    assert list(nb) == [0, 0, 0] and list(need) == [0, 0, 0]
