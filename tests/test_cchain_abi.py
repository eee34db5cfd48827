"""No-GPU checks of the linked-block compressor (LZ4_compress_fast_continue over chains): its C-ABI entry points are declared, exported
and bound; every argument error is LZ4HIP_E_ARG and is said BEFORE a device is looked for; a well-formed call fails loudly without a
device (no CPU fallback) and writes nothing; the Python layer checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from cchain_common import CHAIN_STOPPED
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, no_device

NEW = ("lz4hip_compress_fast_chain_batch", "lz4hip_compress_fast_chain_batch_dev")
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


class Call:
    """one well-formed call: two chains of 2 + 1 blocks of 4 bytes, the second behind 4 bytes of history"""

    def __init__(self):
        self.src = (u8 * 64)(*range(64))
        self.cso, self.prefix = (u64 * 2)(0, 12), (i32 * 2)(0, 4)
        self.src_len, self.first = (i32 * 3)(4, 4, 4), (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 64)(*([7] * 64))
        self.dst_off, self.dst_cap = (u64 * 3)(0, 20, 40), (i32 * 3)(20, 20, 20)
        self.out, self.cons = (i32 * 3)(7, 7, 7), (u64 * 2)(9, 9)
        self.n_blocks, self.n_chains = 3, 2

    def args(self, **kw):
        a = dict(src=self.src, cso=self.cso, prefix=self.prefix, src_len=self.src_len, first=self.first, dst=self.dst, dst_off=self.dst_off,
                 dst_cap=self.dst_cap, out=self.out, cons=self.cons, n_blocks=self.n_blocks, n_chains=self.n_chains)
        a.update(kw)
        return [a[k] for k in ("src", "cso", "prefix", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "cons", "n_blocks", "n_chains")]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and list(self.cons) == [9, 9] and bytes(self.dst) == bytes([7] * 64)


def test_cchain_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    host, dev = amd.C_ABI[NEW[0]][1], amd.C_ABI[NEW[1]][1]
    assert len(host) == 12 and len(dev) == 14 and dev[-2:] == [C.c_int, C.c_void_p] and host[-2:] == [C.c_uint32, C.c_uint32]
    assert CHAIN_STOPPED == -2 ** 31 + 6 == amd.LZ4HIPBatch.CHAIN_STOPPED
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "compress_fast_chain_cu_kernel" in syms
    # the chain decoder no longer calls the compressing side out of scope; the compressor's own list is in the header
    assert "out of scope: linked-block compression" not in h
    for word in ("acceleration above 1", "LZ4_saveDict", "not contiguous", "LZ4_attach_dictionary", "an HC form"):
        assert word in h, word


def test_cchain_argument_errors_come_before_the_device(amd):
    """every argument error of the contract, device or not: a NULL where a pointer is required, a chain_first that is not ascending from 0
    to n_blocks, a prefix that is negative or longer than the chain's offset into src; nothing is written"""
    l = amd.lib()
    c = Call()
    for name in ("src", "cso", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "cons"):
        assert l.lz4hip_compress_fast_chain_batch(*c.args(**{name: None})) == E_ARG, name
        assert b"null" in l.lz4hip_last_error().lower()
        assert l.lz4hip_compress_fast_chain_batch_dev(*(c.args(**{name: None}) + [0, None])) == E_ARG, name
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert l.lz4hip_compress_fast_chain_batch(*c.args(first=(u32 * 3)(*first))) == E_ARG, first
        assert b"chain_first" in l.lz4hip_last_error()
    assert l.lz4hip_compress_fast_chain_batch(*c.args(n_chains=0)) == E_ARG          # 3 blocks in no chain
    assert l.lz4hip_compress_fast_chain_batch(*c.args(prefix=(i32 * 2)(1, 4))) == E_ARG   # chain 0 starts at src + 0
    assert l.lz4hip_compress_fast_chain_batch(*c.args(prefix=(i32 * 2)(0, 13))) == E_ARG
    assert b"chain_prefix_len" in l.lz4hip_last_error()
    assert l.lz4hip_compress_fast_chain_batch(*c.args(prefix=(i32 * 2)(0, -1))) == E_ARG
    assert c.untouched()


def test_cchain_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    c = Call()
    assert l.lz4hip_compress_fast_chain_batch(*c.args()) == E_NO_DEVICE
    assert b"no HIP device" in l.lz4hip_last_error()
    assert l.lz4hip_compress_fast_chain_batch(*c.args(prefix=None)) == E_NO_DEVICE   # (the optional array)
    assert l.lz4hip_compress_fast_chain_batch_dev(*(c.args() + [0, None])) == E_NO_DEVICE
    assert l.lz4hip_compress_fast_chain_batch(*c.args(n_blocks=0, n_chains=0)) in (0, E_NO_DEVICE)
    assert c.untouched()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.compressFastChain(b"abcd", [0], [4], [0, 1], bytearray(20), [0], [20])


def test_cchain_python_layer_checks(amd):
    f = amd.LZ4HIPBatch.compressFastChain
    with pytest.raises(IndexError):
        f(b"abcd", [1], [4], [0, 1], bytearray(20), [0], [20])                   # the source leaves src
    with pytest.raises(IndexError):
        f(b"abcdefgh", [0], [4, 5], [0, 2], bytearray(40), [0, 20], [20, 20])    # the chain's second block does
    with pytest.raises(IndexError):
        f(b"abcd", [0], [4], [0, 1], bytearray(20), [4], [20])                   # the slot leaves dst
    with pytest.raises(IndexError):
        f(b"abcdefgh", [4], [4], [0, 1], bytearray(20), [0], [20], [5])          # the history lies in front of src
    with pytest.raises(ValueError):
        f(b"abcdefgh", [4], [4], [0, 1], bytearray(20), [0], [20], [-1])
    with pytest.raises(ValueError):
        f(b"abcd", [0], [-4], [0, 1], bytearray(20), [0], [20])
    with pytest.raises((ValueError, IndexError)):
        f(b"abcd", [0], [4], [0, 1], bytearray(20), [0], [-20])
    with pytest.raises(ValueError):
        f(b"abcd", [0], [4], [0, 1], bytearray(20), [0, 0], [20])                # per-block arrays differ
    with pytest.raises(ValueError):
        f(b"abcd", [0], [4], [0, 1, 1], bytearray(20), [0], [20])                # per-chain arrays differ
    with pytest.raises(ValueError):
        f(b"abcd", [0], [4], [0, 1], bytearray(20), [0], [20], [0, 0])
    for first in ([1, 1], [0, 0], [0, 2]):
        with pytest.raises(ValueError):
            f(b"abcd", [0], [4], first, bytearray(20), [0], [20])
    with pytest.raises(amd.ReadOnlyBufferException):
        f(b"abcd", [0], [4], [0, 1], b"\0" * 20, [0], [20])
    assert callable(amd.DeviceBatch.compress_fast_chain)


def test_cpp_mirror_cchain_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4HIPBatch::compressFastChain builds (-Werror); tests/cpp/cchain_mirror_test.cpp passes its argument checks and
    exits 3 (loud library failure) without a device; host/lz4hip_streams.hpp carries the writer's linkedBlocks switch"""
    from cchain_common import chain_of, cchain_file
    exe = build_mirror("cchain_mirror_test", tmp_path, werror=True)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip_streams.hpp")).read()
    assert re.search(r"size_t batchBlocks = 64, bool linkedBlocks = false\)\s+: out_\(out\)", hpp)
    if no_device():
        (tmp_path / "c.bin").write_bytes(cchain_file(chain_of("two", b"abcdefgh" * 5, [20, 20], history=b"0123")))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_cchain_native_declared_and_checked_without_device(tmp_path):
    """the new native is declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim; over the fake JNIEnv
    (tests/jni_stub/fake_jni_cchain.c) NULL arguments and a bad chainFirst are argument errors and a well-formed call fails loudly
    without a device, nothing leaked or left pinned"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchFastChain\s*\(", java)
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_batchFastChain(" in batch and re.search(r"public static void compressFastChain\(ByteBuffer src", batch)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastChain" in shim
    # the existing chain native keeps its signature
    assert re.search(r"static native int LZ4HIP_batchSafeChain\(ByteBuffer src, long\[\] srcOff, int\[\] srcLen, int\[\] stored,", java)
    from support import typecheck_jni_shim
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_cchain", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
