"""No-GPU checks of the HC linked-block compressor (LZ4_compress_HC_continue over chains): its C-ABI entry point is declared,
exported and bound; every argument error is LZ4HIP_E_ARG and is said BEFORE a device is looked for; a well-formed call fails loudly
without a device (no CPU fallback) and writes nothing; the "hc_chain_segment" knob checks its range; the Python layer checks its
arguments."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, no_device, typecheck_jni_shim

NEW = ("lz4hip_compress_hc_chain_batch",)
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


class Call:
    """one well-formed call: two chains of 2 + 1 blocks of 4 bytes, the second behind 4 bytes of history"""
    ORDER = ("src", "cso", "prefix", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "n_blocks", "n_chains", "level")

    def __init__(self):
        self.src = (u8 * 64)(*range(64))
        self.cso, self.prefix = (u64 * 2)(0, 12), (i32 * 2)(0, 4)
        self.src_len, self.first = (i32 * 3)(4, 4, 4), (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 64)(*([7] * 64))
        self.dst_off, self.dst_cap = (u64 * 3)(0, 20, 40), (i32 * 3)(20, 20, 20)
        self.out = (i32 * 3)(7, 7, 7)
        self.n_blocks, self.n_chains, self.level = 3, 2, 9

    def args(self, **kw):
        a = {k: getattr(self, k) for k in self.ORDER}
        a.update(kw)
        return [a[k] for k in self.ORDER]

    def forms(self, l, **kw):
        """the entry point on these arrays -> (its status,)"""
        return (l.lz4hip_compress_hc_chain_batch(*self.args(**kw)),)

    def untouched(self):
        return list(self.out) == [7, 7, 7] and bytes(self.dst) == bytes([7] * 64)


def test_hcchain_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    host = amd.C_ABI[NEW[0]][1]
    assert len(host) == 12 and host[-3:] == [C.c_uint32, C.c_uint32, C.c_int]
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    for k in ("hc_chain_layout_kernel", "hc_build_chain_kernel", "hc_parse_chain_kernel"):
        assert k in syms, k
    # the header says what differs from the fast chain, and the fast chain no longer calls an HC form out of scope
    doc = h[h.index("COMPRESS CHAINS OF LINKED BLOCKS AT AN HC LEVEL"):h.index("int lz4hip_compress_hc_chain_batch(")]
    for word in ("DOES NOT END ITS CHAIN", "No\n *     LZ4HIP_CHAIN_STOPPED exists", "LZ4_saveDictHC", "LZ4_attach_HC_dictionary", "favorDecSpeed", "destSize", "hc_chain_segment", "device-pointer forms", "ONE chain"):
        assert word in doc, word
    fast = h[h.index("int lz4hip_decompress_safe_chain_batch("):h.index("int lz4hip_compress_fast_chain_batch(")]
    assert "LZ4_attach_dictionary; an HC form" not in fast
    assert callable(amd.LZ4HIPBatch.compressHCChain)


def test_hcchain_argument_errors_come_before_the_device(amd):
    """every argument error of the contract, device or not: a NULL where a pointer is required (everything but chain_prefix_len), a
    chain_first that is not ascending from 0 to n_blocks, a prefix that is negative or longer than the chain's offset into src; nothing
    is written"""
    l = amd.lib()
    c = Call()
    for name in ("src", "cso", "src_len", "first", "dst", "dst_off", "dst_cap", "out"):
        assert c.forms(l, **{name: None}) == (E_ARG,), name
        assert b"null" in l.lz4hip_last_error().lower()
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert l.lz4hip_compress_hc_chain_batch(*c.args(first=(u32 * 3)(*first))) == E_ARG, first
        assert b"chain_first" in l.lz4hip_last_error()
    assert l.lz4hip_compress_hc_chain_batch(*c.args(n_chains=0)) == E_ARG          # 3 blocks in no chain
    assert l.lz4hip_compress_hc_chain_batch(*c.args(prefix=(i32 * 2)(1, 4))) == E_ARG   # chain 0 starts at src + 0
    assert l.lz4hip_compress_hc_chain_batch(*c.args(prefix=(i32 * 2)(0, 13))) == E_ARG
    assert b"chain_prefix_len" in l.lz4hip_last_error()
    assert l.lz4hip_compress_hc_chain_batch(*c.args(prefix=(i32 * 2)(0, -1))) == E_ARG
    assert c.untouched()


def test_hcchain_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    c = Call()
    assert c.forms(l) == (E_NO_DEVICE,)
    assert b"no HIP device" in l.lz4hip_last_error()
    assert c.forms(l, prefix=None) == (E_NO_DEVICE,)     # (the optional array)
    for level in (-5, 0, 13, 100):                                                # (levels are clamped, never refused)
        assert c.forms(l, level=level)[0] == E_NO_DEVICE
    assert l.lz4hip_compress_hc_chain_batch(*c.args(n_blocks=0, n_chains=0)) in (0, E_NO_DEVICE)
    assert c.untouched()
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.compressHCChain(b"abcd", [0], [4], [0, 1], bytearray(20), [0], [20])


def test_hc_chain_segment_knob_range(amd):
    """4096 .. 2^30, settable without a device (host state)"""
    for v in (4096, 65536, 1 << 30, 4097, 1 << 20):
        amd.set_option("hc_chain_segment", v)
    for v in (4095, 0, -1, (1 << 30) + 1, 2 ** 31 - 1):
        with pytest.raises(amd.LZ4HIPError):
            amd.set_option("hc_chain_segment", v)
    assert b"hc_chain_segment" in amd.lib().lz4hip_last_error()
    amd.set_option("hc_chain_segment", 1 << 20)


def test_hcchain_is_described_once_in_the_op_table():
    """csrc/api.cpp: one Op for the operation -- a compressor, using the chain workspace, taking chain arrays, whose chains do not stop --
    and the op predicates are what route it"""
    api = open(os.path.join(ROOT, "lz4-java_amd", "csrc", "api.cpp")).read()
    assert re.search(r"enum Op \{[^}]*OP_COMPRESS_HC_CHAIN[^}]*\}", api)
    for pred in ("op_compresses", "op_uses_hc_ws", "op_takes_cchain"):
        assert re.search(r"constexpr bool %s\(Op op\) \{[^}]*OP_COMPRESS_HC_CHAIN[^}]*\}" % pred, api), pred
    assert not re.search(r"constexpr bool op_chain_stops\(Op op\) \{[^}]*OP_COMPRESS_HC_CHAIN[^}]*\}", api)
    assert len(re.findall(r"\bint cchain_host_shard\(", api)) == 1          # the two chain compressors share their host path


def test_hcchain_python_layer_checks(amd):
    f = amd.LZ4HIPBatch.compressHCChain
    with pytest.raises(IndexError):
        f(b"abcd", [1], [4], [0, 1], bytearray(20), [0], [20])                   # the source leaves src
    with pytest.raises(IndexError):
        f(b"abcdefgh", [0], [4, 5], [0, 2], bytearray(40), [0, 20], [20, 20])    # the chain's second block does
    with pytest.raises(IndexError):
        f(b"abcd", [0], [4], [0, 1], bytearray(20), [4], [20])                   # the slot leaves dst
    with pytest.raises(IndexError):
        f(b"abcdefgh", [4], [4], [0, 1], bytearray(20), [0], [20], [5], 9)       # the history lies in front of src
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
    for first in ([1, 1], [0, 0], [0, 2]):
        with pytest.raises(ValueError):
            f(b"abcd", [0], [4], first, bytearray(20), [0], [20])
    with pytest.raises(amd.ReadOnlyBufferException):
        f(b"abcd", [0], [4], [0, 1], b"\0" * 20, [0], [20])


def test_cpp_mirror_hcchain_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: LZ4HIPBatch::compressHCChain builds (-Werror); tests/cpp/hcchain_mirror_test.cpp passes its argument checks and
    exits 3 (loud library failure) without a device; host/lz4hip_streams.hpp carries the writer's level as a trailing constructor
    argument of a second constructor (the first keeps its signature) and says what the level changes"""
    from cchain_common import chain_of, cchain_file
    exe = build_mirror("hcchain_mirror_test", tmp_path, werror=True)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip_streams.hpp")).read()
    assert re.search(r"size_t batchBlocks = 64, bool linkedBlocks = false\)\s+: out_\(out\)", hpp)
    assert re.search(r"size_t batchBlocks, bool linkedBlocks, int level\)", hpp)
    assert "do not depend on batchBlocks" in hpp
    if no_device():
        (tmp_path / "c.bin").write_bytes(cchain_file(chain_of("two", b"abcdefgh" * 5, [20, 20], history=b"0123")))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin"), "9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_hcchain_native_declared_and_checked_without_device(tmp_path):
    """the new native is declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim; over the fake JNIEnv
    (tests/jni_stub/fake_jni_hcchain.c) NULL arguments and a bad chainFirst are argument errors and a well-formed call fails loudly
    without a device, nothing leaked or left pinned"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchHCChain\s*\(", java)
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    assert "LZ4HIPJNI.LZ4HIP_batchHCChain(" in batch and re.search(r"public static void compressHCChain\(ByteBuffer src", batch)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCChain" in shim
    # the fast chain's native keeps its signature
    assert re.search(r"static native int LZ4HIP_batchFastChain\(ByteBuffer src, long\[\] chainSrcOff, int\[\] chainPrefixLen, int\[\] srcLen, int\[\] chainFirst,", java)
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_hcchain", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
