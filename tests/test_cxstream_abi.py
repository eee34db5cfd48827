"""No-GPU checks of lz4hip_compress_fast_stream_ext_batch (resident compress streams whose sources land anywhere): the entry point is
declared, exported and bound in Python, C++ and Java; every argument error of its contract is LZ4HIP_E_ARG and is said BEFORE a device
is looked for, with nothing written; a well-formed call fails loudly without a device (no CPU fallback); the header says the contract
and declares no device-pointer form; the staging arithmetic agrees with a naive restatement under the sanitizers; the Python layer
checks its arguments."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, build_sanitized, no_device, typecheck_jni_shim
from test_dstream_abi import DEVICE_ENTRY_POINTS

u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8
NAME = "lz4hip_compress_fast_stream_ext_batch"


class Call:
    """one well-formed call apart from its set: streams 0 and 1 with 2 + 1 blocks of 4 bytes; stream 0 in the window [8, 40) without a
    history, stream 1 in [40, 72) behind 4 bytes that end at 48, inside its window"""
    ORDER = ("set", "ids", "src", "src_off", "src_len", "first", "hist_end", "hist_len", "win_off", "win_len", "dst", "dst_off", "dst_cap", "out", "cons",
             "n_blocks", "n_chains")
    POINTERS = ORDER[1:15]

    def __init__(self, set_=None):
        self.set = set_
        self.ids = (u32 * 2)(0, 1)
        self.src = (u8 * 96)(*range(96))
        self.src_off, self.src_len, self.first = (u64 * 3)(8, 30, 60), (i32 * 3)(4, 4, 4), (u32 * 3)(0, 2, 3)
        self.hist_end, self.hist_len = (u64 * 2)(0, 48), (i32 * 2)(0, 4)
        self.win_off, self.win_len = (u64 * 2)(8, 40), (u64 * 2)(32, 32)
        self.dst = (u8 * 64)(*([7] * 64))
        self.dst_off, self.dst_cap = (u64 * 3)(0, 20, 40), (i32 * 3)(20, 20, 20)
        self.out, self.cons = (i32 * 3)(7, 7, 7), (u64 * 2)(9, 9)
        self.n_blocks, self.n_chains = 3, 2

    def args(self, **kw):
        a = {k: getattr(self, k) for k in self.ORDER}
        a.update(kw)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and list(self.cons) == [9, 9] and bytes(self.dst) == bytes([7] * 64)


def header():
    return open(os.path.join(ROOT, "include", "lz4hip.h")).read()


def stream_file(win_len, calls, blocks):
    """the file of tests/cpp/cxstream_mirror_test.cpp and tests/jni_stub/fake_jni_cxstream.c: calls = [(end block, hist_end relative to
    the window, hist_len)], blocks = [(off, bytes, cap)]"""
    q = lambda *v: struct.pack("<%dq" % len(v), *v)
    out = q(win_len, len(blocks), len(calls))
    for c in calls:
        out += q(*c)
    for off, data, cap in blocks:
        out += q(off, len(data), cap)
    return out + b"".join(d for _, d, _ in blocks)


def test_symbol_declared_exported_and_bound(amd):
    h = header()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    assert re.search(r"\bint\s+%s\s*\(\s*lz4hip_cstreams\s*\*\s*set,\s*const uint32_t\s*\*\s*stream_id," % NAME, h)
    assert NAME in exported and NAME in amd.C_ABI and hasattr(amd.lib(), NAME)
    assert len(amd.C_ABI[NAME][1]) == 17
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "compress_fast_xstream_cu_kernel" in syms and "compress_fast_stream_cu_kernel" in syms
    assert callable(amd.CompressStreams.compressAt) and callable(amd.LZ4HIPBatch.compressFastStreamAt)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip.hpp")).read()
    assert "LZ4HIPBatch::Chains compressAt(" in hpp and NAME + "(" in hpp
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchFastStreamAt\s*\(long set, int\[\] streamId, ByteBuffer src, long\[\] srcOff,", java)
    assert "public void compressAt(int[] streamId, ByteBuffer src, long[] srcOff" in batch and "LZ4HIPJNI.LZ4HIP_batchFastStreamAt(" in batch
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAt" in shim and NAME + "(" in shim


def test_header_says_the_contract_and_declares_no_device_pointer_form():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    names = re.findall(r"\b(lz4hip_[a-z0-9_]+)\s*\(", code)
    assert not [s for s in names if "_dev" in s and ("cstream" in s or "stream_ext" in s or "fast_stream" in s)]
    assert sorted(set(s for s in names if re.search(r"_dev(_ws)?$", s))) == sorted(DEVICE_ENTRY_POINTS)
    i = h.index("COMPRESS STREAMS WHOSE SOURCES LAND ANYWHERE")
    text = " ".join(h[i:h.index("int " + NAME, i)].replace("*", " ").split())
    for word in ("THE SAME CONTRACT", "in any interleaving", "external-dictionary mode", "min(chain_hist_len[c], 65536, what the stream holds)", "LZ4_saveDict",
                 "LZ4_loadDict does", "lz4hip_compress_fast_dict", "D_len < 4 and D_end != s", "the source overlaps its own history", "D_end == s: prefix mode",
                 "goes on at the block's start", "a block of 0 bytes at a jump drops the history", "A CALL IS A SNAPSHOT", "0x7E000000", "LZ4HIP_CHAIN_STOPPED",
                 "wholly inside the window or wholly outside it", "stays contiguous with it", "windows of different streams may overlap",
                 "Destination slots may not overlap", "ALL pointers are required", "a source outside its window", "straddles a window edge",
                 "a negative chain_hist_len", "LZ4HIP_E_NO_DEVICE", "compress_fast_xstream_cu_kernel", "wave-uniform",
                 "out of scope: device-pointer forms", "far-offset and stream-contract tables", "acceleration above 1", "LZ4_attach_dictionary", "an HC form",
                 "streams past the index limit"):
        assert word in text, word
    # the two lists stay, with the pointers to this call
    assert "sources that are not contiguous; LZ4_attach_dictionary" in h and "the external-dictionary mode (a source that does not follow its" in h
    flat = " ".join(h.replace("*", " ").split())
    assert "(No longer out of scope: sources that are not contiguous, on a resident stream, is lz4hip_compress_fast_stream_ext_batch, below.)" in flat
    assert "(No longer out of scope: the external-dictionary mode is lz4hip_compress_fast_stream_ext_batch, below.)" in flat


def test_argument_errors_come_before_the_device(amd):
    """every LZ4HIP_E_ARG case of the contract that does not depend on the set, device or not: the library checks them BEFORE the set, so
    without one (a NULL set is the last error it can report here) the message says which check spoke; nothing is written"""
    l = amd.lib()
    c = Call()
    f = getattr(l, NAME)
    f.argtypes, f.restype = amd.C_ABI[NAME][1], C.c_int
    err = lambda: l.lz4hip_last_error().lower()
    assert f(*c.args()) == E_ARG and b"null stream set" in err()
    for name in Call.POINTERS:            # all pointers are required
        assert f(*c.args(**{name: None})) == E_ARG, name
        assert b"null pointer" in err() and b"stream set" not in err(), name
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert f(*c.args(first=(u32 * 3)(*first))) == E_ARG and b"chain_first" in err(), first
    assert f(*c.args(n_chains=0)) == E_ARG and b"chain_first" in err()               # 3 blocks in no chain
    for ids in ((1, 1), (1, 0)):
        assert f(*c.args(ids=(u32 * 2)(*ids))) == E_ARG and b"strictly ascending" in err(), ids
    # a source outside its window: in front of it, over its end, behind it; a negative length's offset counts too
    for off, ln in (((7, 30, 60), (4, 4, 4)), ((8, 37, 60), (4, 4, 4)), ((8, 30, 39), (4, 4, 4)), ((8, 30, 69), (4, 4, 4)), ((8, 30, 73), (4, 4, 0)),
                    ((8, 41, 60), (4, -1, 4))):
        assert f(*c.args(src_off=(u64 * 3)(*off), src_len=(i32 * 3)(*ln))) == E_ARG and b"outside its stream's window" in err(), (off, ln)
    assert f(*c.args(win_off=(u64 * 2)(8, 2 ** 64 - 4))) == E_ARG
    # a history piece that straddles a window edge (its start, its end); one longer than its end offset; a negative length
    for he, hl in (((0, 42), (0, 4)), ((0, 74), (0, 4)), ((10, 48), (4, 4))):
        assert f(*c.args(hist_end=(u64 * 2)(*he), hist_len=(i32 * 2)(*hl))) == E_ARG and b"straddles" in err(), (he, hl)
    assert f(*c.args(hist_end=(u64 * 2)(0, 3), hist_len=(i32 * 2)(0, 4))) == E_ARG and b"reaches in front of src" in err()
    assert f(*c.args(hist_len=(i32 * 2)(0, -1))) == E_ARG and b"negative chain_hist_len" in err()
    assert f(*c.args(n_blocks=0, n_chains=0)) == E_ARG and b"null stream set" in err()   # the empty call still needs its set
    # what is NOT an argument error gets as far as the set: a history that ends exactly where the window begins or begins where it
    # ends, one far away, an empty one with any end, a negative length inside the window, a 0-byte block at the window's end
    for kw in (dict(hist_end=(u64 * 2)(0, 40)), dict(hist_end=(u64 * 2)(0, 76)), dict(hist_end=(u64 * 2)(0, 6)), dict(hist_end=(u64 * 2)(0, 90), hist_len=(i32 * 2)(0, 6)),
               dict(hist_end=(u64 * 2)(77, 48)), dict(src_len=(i32 * 3)(4, -1, 4)), dict(src_off=(u64 * 3)(8, 30, 72), src_len=(i32 * 3)(4, 4, 0))):
        assert f(*c.args(**kw)) == E_ARG and b"null stream set" in err(), kw
    assert c.untouched()


def test_fails_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    f = getattr(l, NAME)
    f.argtypes, f.restype = amd.C_ABI[NAME][1], C.c_int
    # no set can exist here (lz4hip_cstreams_create is LZ4HIP_E_NO_DEVICE), and a set is read only once a device is there: the empty
    # call on a handle that is none is well formed and gets as far as the device
    h = C.c_void_p(None)
    assert l.lz4hip_cstreams_create(4, C.byref(h)) == E_NO_DEVICE and not h
    c = Call(C.cast(C.create_string_buffer(256), C.c_void_p))
    assert f(*c.args(n_blocks=0, n_chains=0, first=(u32 * 1)(0))) == E_NO_DEVICE and b"no HIP device" in l.lz4hip_last_error()
    assert c.untouched()
    with pytest.raises(amd.LZ4HIPError):
        amd.CompressStreams(4)


def test_python_layer_checks(amd):
    class FakeSet:
        def __len__(self):
            return 2

        def _handle(self):
            raise AssertionError("the checks come first")
    f = lambda ids, *a: amd.LZ4HIPBatch.compressFastStreamAt(FakeSet(), ids, *a)
    ok = (b"abcdefgh", [0, 4], [4, 4], [0, 1, 2], [0, 0], [0, 0], [0, 4], [4, 4], bytearray(40), [0, 20], [20, 20])
    def bad(exc, ids=(0, 1), **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        with pytest.raises(exc):
            f(list(ids), *a)
    bad(ValueError, ids=(0, 0))
    bad(ValueError, ids=(1, 0))
    bad(ValueError, ids=(0, 2))                     # two streams exist
    bad(ValueError, a1=[0])                         # per-block arrays differ
    bad(ValueError, a4=[0])                         # per-chain arrays differ
    bad(ValueError, a3=[0, 2])                      # chainFirst
    bad(amd.ReadOnlyBufferException, a8=b"\0" * 40)
    with pytest.raises(AssertionError):             # (the well-formed call reaches the handle)
        f([0, 1], *ok)


def test_staging_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/cxstream_staging_test.cpp: the history piece against the window, the used hull, its place in the device image, the
    pieces apart, the metadata layout and the argument errors against a naive restatement -- host code alone, address and
    undefined-behaviour sanitizers, a program of its own"""
    exe = build_sanitized("cxstream_staging_test", tmp_path)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "cxstream staging ok: 203000 cases" in out, out


def test_cpp_mirror_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: CompressStreams::compressAt builds (-Werror); tests/cpp/cxstream_mirror_test.cpp exits 3 (loud library failure)
    without a device"""
    exe = build_mirror("cxstream_mirror_test", tmp_path, werror=True)
    if no_device():
        (tmp_path / "s.bin").write_bytes(stream_file(64, [(1, 0, 0), (2, 20, 20)], [(0, b"abcdefgh" * 2 + b"abcd", 40), (32, b"abcdefgh" * 2, 40)]))
        p = subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_native_checked_without_device(tmp_path):
    """over the fake JNIEnv (tests/jni_stub/fake_jni_cxstream.c) a 0 handle is an argument error with nothing pinned, and without a
    device no set can be made, loudly, nothing leaked; the existing stream native keeps its signature"""
    java = open(os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4", "LZ4HIPJNI.java")).read()
    assert re.search(r"static native int LZ4HIP_batchFastStream\(long set, int\[\] streamId, ByteBuffer src, long\[\] chainSrcOff, int\[\] chainPrefixLen,", java)
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_cxstream", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
