"""No-GPU checks of the linked-block decoder (LZ4_decompress_safe_continue over chains): its C-ABI entry points are declared, exported
and bound; every argument error is LZ4HIP_E_ARG and is said BEFORE a device is looked for; a well-formed call fails loudly without a
device (no CPU fallback) and writes nothing; LZ4HIP_CHAIN_STOPPED cannot collide with a liblz4 value; the Python, C++ and JNI layers
carry the call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from chain_common import CHAIN_STOPPED
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_decompress_safe_chain_batch", "lz4hip_decompress_safe_chain_batch_dev")
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


class Call:
    """one well-formed call: two chains of 2 + 1 blocks (each block the stream 0x10 'a'), the second behind 4 bytes of history"""

    def __init__(self):
        self.src = (u8 * 64)(*([0x10, 0x61] * 3))
        self.src_off, self.src_len = (u64 * 3)(0, 2, 4), (i32 * 3)(2, 2, 2)
        self.stored, self.dst_cap = (u8 * 3)(0, 0, 0), (i32 * 3)(8, 8, 8)
        self.first = (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 64)(*([7] * 64))
        self.cdo, self.ccap, self.prefix = (u64 * 2)(0, 36), (u64 * 2)(16, 8), (i32 * 2)(0, 4)
        self.out, self.cout = (i32 * 3)(7, 7, 7), (u64 * 2)(9, 9)
        self.n_blocks, self.n_chains = 3, 2

    def args(self, **kw):
        a = dict(src=self.src, src_off=self.src_off, src_len=self.src_len, stored=self.stored, dst_cap=self.dst_cap, first=self.first, dst=self.dst,
                 cdo=self.cdo, ccap=self.ccap, prefix=self.prefix, out=self.out, cout=self.cout, n_blocks=self.n_blocks, n_chains=self.n_chains)
        a.update(kw)
        return [a[k] for k in ("src", "src_off", "src_len", "stored", "dst_cap", "first", "dst", "cdo", "ccap", "prefix", "out", "cout", "n_blocks", "n_chains")]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and list(self.cout) == [9, 9] and bytes(self.dst) == bytes([7] * 64)


def test_chain_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    host, dev = amd.C_ABI[NEW[0]][1], amd.C_ABI[NEW[1]][1]
    assert len(host) == 14 and len(dev) == 16 and dev[-2:] == [C.c_int, C.c_void_p] and host[-2:] == [C.c_uint32, C.c_uint32]
    # the marker is LZ4HIP_LIB_ERROR of a status of its own: below every liblz4 result, inside the library-error band
    assert re.search(r"LZ4HIP_E_CHAIN_STOPPED\s*=\s*-6\b", h)
    assert re.search(r"#define\s+LZ4HIP_CHAIN_STOPPED\s+LZ4HIP_LIB_ERROR\(LZ4HIP_E_CHAIN_STOPPED\)", h)
    assert CHAIN_STOPPED == -2 ** 31 + 6 == amd.LZ4HIPBatch.CHAIN_STOPPED and CHAIN_STOPPED < -2 ** 31 + 64
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "decode_chain_kernel" in syms


def test_chain_argument_errors_come_before_the_device(amd):
    """every argument error of the issue, device or not: a NULL where a pointer is required, a chain_first that is not ascending from 0
    to n_blocks, a prefix that is negative or longer than the chain's offset into dst; nothing is written"""
    l = amd.lib()
    c = Call()
    for name in ("src", "src_off", "src_len", "dst_cap", "first", "dst", "cdo", "ccap", "out", "cout"):
        assert l.lz4hip_decompress_safe_chain_batch(*c.args(**{name: None})) == E_ARG, name
        assert b"null" in l.lz4hip_last_error()
        assert l.lz4hip_decompress_safe_chain_batch_dev(*(c.args(**{name: None}) + [0, None])) == E_ARG, name
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert l.lz4hip_decompress_safe_chain_batch(*c.args(first=(u32 * 3)(*first))) == E_ARG, first
        assert b"chain_first" in l.lz4hip_last_error()
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(n_chains=0)) == E_ARG          # 3 blocks in no chain
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(prefix=(i32 * 2)(1, 4))) == E_ARG   # chain 0 starts at dst + 0
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(prefix=(i32 * 2)(0, 37))) == E_ARG
    assert b"chain_prefix_len" in l.lz4hip_last_error()
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(prefix=(i32 * 2)(0, -1))) == E_ARG
    assert c.untouched()


def test_chain_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    c = Call()
    assert l.lz4hip_decompress_safe_chain_batch(*c.args()) == E_NO_DEVICE
    assert b"no HIP device" in l.lz4hip_last_error()
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(stored=None, prefix=None)) == E_NO_DEVICE   # (the two optional arrays)
    assert l.lz4hip_decompress_safe_chain_batch_dev(*(c.args() + [0, None])) == E_NO_DEVICE
    assert l.lz4hip_decompress_safe_chain_batch(*c.args(n_blocks=0, n_chains=0)) in (0, E_NO_DEVICE)
    assert c.untouched()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.decompressSafeChain(b"\x10a", [0], [2], [8], [0, 1], bytearray(20), [0], [8])


def test_chain_python_layer_checks(amd):
    f = amd.LZ4HIPBatch.decompressSafeChain
    with pytest.raises(IndexError):
        f(b"\x10a", [1], [2], [8], [0, 1], bytearray(20), [0], [8])                  # the stream leaves src
    with pytest.raises(IndexError):
        f(b"\x10a", [0], [2], [8], [0, 1], bytearray(20), [16], [8])                 # the region leaves dst
    with pytest.raises(IndexError):
        f(b"\x10a", [0], [2], [8], [0, 1], bytearray(20), [4], [8], [5])             # the history lies in front of dst
    with pytest.raises(ValueError):
        f(b"\x10a", [0], [2], [8], [0, 1], bytearray(20), [4], [8], [-1])
    with pytest.raises(ValueError):
        f(b"\x10a", [0], [2], [-8], [0, 1], bytearray(20), [4], [8])
    with pytest.raises(ValueError):
        f(b"\x10a", [0], [2], [8, 8], [0, 1], bytearray(20), [0], [8])               # per-block arrays differ
    with pytest.raises(ValueError):
        f(b"\x10a", [0], [2], [8], [0, 1, 1], bytearray(20), [0], [8])               # per-chain arrays differ
    for first in ([1, 1], [0, 0], [0, 2]):
        with pytest.raises(ValueError):
            f(b"\x10a", [0], [2], [8], first, bytearray(20), [0], [8])
    with pytest.raises(ValueError):
        f(b"\x10a", [0], [2], [8], [0, 1], bytearray(20), [0], [8], None, [0, 0])    # stored[] of the wrong length
    with pytest.raises(amd.ReadOnlyBufferException):
        f(b"\x10a", [0], [2], [8], [0, 1], b"\0" * 20, [0], [8])
    assert callable(amd.DeviceBatch.decompress_safe_chain)


def test_cpp_mirror_chain_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4HIPBatch::decompressSafeChain builds; tests/cpp/chain_mirror_test.cpp passes its argument checks and exits 3
    (loud library failure) without a device; host/lz4hip_streams.hpp carries the linkedBlocks switch"""
    from chain_common import Chain, chain_file
    exe = build_mirror("chain_mirror_test", tmp_path)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip_streams.hpp")).read()
    assert re.search(r"size_t batchBlocks = 64,\s+bool linkedBlocks = false\)", hpp)
    if no_device():
        (tmp_path / "c.bin").write_bytes(chain_file(Chain("two", [(b"\x10a", False, 8), (b"\x10b", False, 8)], history=b"0123")))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_chain_native_declared_and_checked_without_device(tmp_path):
    """the new native is declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim; over the fake JNIEnv
    (tests/jni_stub/fake_jni_chain.c) NULL arguments and a bad chainFirst are argument errors and a well-formed call fails loudly
    without a device, nothing leaked or left pinned"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchSafeChain\s*\(", java)
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_batchSafeChain(" in batch and re.search(r"public static void decompressSafeChain\(ByteBuffer src", batch)
    assert re.search(r"public static final int CHAIN_STOPPED = Integer\.MIN_VALUE \+ 6;", batch)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeChain" in shim
    # the existing natives keep their signatures
    assert re.search(r"static native int LZ4HIP_batchSafeDict\(long dict, ByteBuffer src, long\[\] srcOff, int\[\] srcLen, ByteBuffer dest, long\[\] destOff,", java)
    exe = build_fake_jni("fake_jni_chain", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
