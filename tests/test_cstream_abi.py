"""No-GPU checks of the resident-stream compressor (lz4hip_cstreams_* and lz4hip_compress_fast_stream_batch): the entry points are
declared, exported and bound; every argument error is LZ4HIP_E_ARG and is said BEFORE a device is looked for, with nothing written; a
set cannot be created and a well-formed call fails loudly without a device (no CPU fallback); the header names what is out of scope
and declares no device-pointer form; the Python layer checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, no_device

NEW = ("lz4hip_cstreams_create", "lz4hip_cstreams_count", "lz4hip_cstreams_reset", "lz4hip_cstreams_consumed", "lz4hip_cstreams_free",
       "lz4hip_compress_fast_stream_batch")
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


class Call:
    """one well-formed call apart from its set: two chains of 2 + 1 blocks of 4 bytes for streams 0 and 1, the second behind 4 bytes"""

    def __init__(self, set_=None):
        self.set = set_
        self.ids = (u32 * 2)(0, 1)
        self.src = (u8 * 64)(*range(64))
        self.cso, self.prefix = (u64 * 2)(0, 12), (i32 * 2)(0, 4)
        self.src_len, self.first = (i32 * 3)(4, 4, 4), (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 64)(*([7] * 64))
        self.dst_off, self.dst_cap = (u64 * 3)(0, 20, 40), (i32 * 3)(20, 20, 20)
        self.out, self.cons = (i32 * 3)(7, 7, 7), (u64 * 2)(9, 9)
        self.n_blocks, self.n_chains = 3, 2

    def args(self, **kw):
        a = dict(set=self.set, ids=self.ids, src=self.src, cso=self.cso, prefix=self.prefix, src_len=self.src_len, first=self.first, dst=self.dst,
                 dst_off=self.dst_off, dst_cap=self.dst_cap, out=self.out, cons=self.cons, n_blocks=self.n_blocks, n_chains=self.n_chains)
        a.update(kw)
        return [a[k] for k in ("set", "ids", "src", "cso", "prefix", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "cons", "n_blocks", "n_chains")]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and list(self.cons) == [9, 9] and bytes(self.dst) == bytes([7] * 64)


def test_cstream_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, h), s
        assert s in exported and s in amd.C_ABI, s
        assert hasattr(amd.lib(), s)
    chain = amd.C_ABI["lz4hip_compress_fast_chain_batch"][1]
    assert amd.C_ABI["lz4hip_compress_fast_stream_batch"][1] == [C.c_void_p, C.POINTER(u32)] + chain
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "compress_fast_stream_cu_kernel" in syms and "compress_fast_chain_cu_kernel" in syms
    assert callable(amd.CompressStreams) and callable(amd.LZ4HIPBatch.compressFastStream)


def test_header_names_the_scope_and_declares_no_device_pointer_form():
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert not [s for s in re.findall(r"\b(lz4hip_[a-z0-9_]+)\s*\(", code) if "_dev" in s and ("cstream" in s or "fast_stream" in s)]
    i = h.index("COMPRESS STREAMS THAT ARE CONTINUED BY ANY NUMBER OF CALLS")
    text = " ".join(h[i:h.index("typedef struct lz4hip_cstreams", i)].replace("*", " ").split())
    for word in ("out of scope: a device-pointer form", "acceleration above 1", "the external-dictionary mode", "LZ4_attach_dictionary", "an HC form",
                 "streams longer than the index limit", "JUST UNDER 2 GiB BETWEEN RESETS", "32 KB table image", "65536 streams are about 2 GiB",
                 "LZ4HIP_E_NOMEM", "STRICTLY ASCENDING", "NOT a reset", "serialised", "before lz4hip_shutdown()"):
        assert word in text, word
    # the chain call's list stays, with the pointer to this call
    assert "LZ4_saveDict and resuming a stream's exact state across calls" in h
    assert re.search(r"No longer out of scope: resuming a stream's exact state across calls, LZ4_saveDict\s+\*?\s*included, is lz4hip_compress_fast_stream_batch, below", h)


def test_cstream_argument_errors_come_before_the_device(amd):
    """every argument error of the contract that does not depend on the set, device or not: the library checks them BEFORE the set, so
    without one (a NULL set is the last error it can report here) the message says which check spoke -- a NULL where a pointer is
    required, a chain_first that is not ascending from 0 to n_blocks, a prefix that is negative or longer than the chain's offset, ids
    that are not strictly ascending; nothing is written.  The ids against n_streams need a set: tests/test_gpu_cstream.py, which
    repeats all of these with a live one"""
    l = amd.lib()
    c = Call()
    f = l.lz4hip_compress_fast_stream_batch
    err = lambda: l.lz4hip_last_error().lower()
    assert f(*c.args()) == E_ARG and b"null stream set" in err()
    for name in ("ids", "src", "cso", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "cons"):
        assert f(*c.args(**{name: None})) == E_ARG, name
        assert b"null pointer" in err() and b"stream set" not in err(), name
    assert f(*c.args(prefix=None)) == E_ARG and b"null stream set" in err()          # (the optional array)
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert f(*c.args(first=(u32 * 3)(*first))) == E_ARG and b"chain_first" in err(), first
    assert f(*c.args(n_chains=0)) == E_ARG and b"chain_first" in err()               # 3 blocks in no chain
    assert f(*c.args(prefix=(i32 * 2)(1, 4))) == E_ARG and b"chain_prefix_len" in err()   # chain 0 starts at src + 0
    assert f(*c.args(prefix=(i32 * 2)(0, 13))) == E_ARG and b"chain_prefix_len" in err()
    assert f(*c.args(prefix=(i32 * 2)(0, -1))) == E_ARG and b"chain_prefix_len" in err()
    for ids in ((1, 1), (1, 0)):
        assert f(*c.args(ids=(u32 * 2)(*ids))) == E_ARG and b"strictly ascending" in err(), ids
    assert f(*c.args(n_blocks=0, n_chains=0)) == E_ARG and b"null stream set" in err()   # the empty call still needs its set
    assert l.lz4hip_cstreams_create(4, None) == E_ARG
    h = C.c_void_p(None)
    assert l.lz4hip_cstreams_create(0, C.byref(h)) == E_ARG and not h
    assert l.lz4hip_cstreams_count(None) == E_ARG
    assert l.lz4hip_cstreams_reset(None, None, 0) == E_ARG
    assert l.lz4hip_cstreams_consumed(None, 0, 0, None, None) == E_ARG
    l.lz4hip_cstreams_free(None)
    assert c.untouched()


def test_cstream_entry_points_fail_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    h = C.c_void_p(None)
    assert l.lz4hip_cstreams_create(4, C.byref(h)) == E_NO_DEVICE and not h
    assert b"no HIP device" in l.lz4hip_last_error()
    with pytest.raises(amd.LZ4HIPError):
        amd.CompressStreams(4)


def test_cstream_python_layer_checks(amd):
    class FakeSet:
        def __len__(self):
            return 2

        def _handle(self):
            raise AssertionError("the checks come first")
    f = lambda ids, *a: amd.LZ4HIPBatch.compressFastStream(FakeSet(), ids, *a)
    with pytest.raises(ValueError):
        f([0, 0], b"abcdefgh", [0, 4], [4, 4], [0, 1, 2], bytearray(40), [0, 20], [20, 20])     # not strictly ascending
    with pytest.raises(ValueError):
        f([1, 0], b"abcdefgh", [0, 4], [4, 4], [0, 1, 2], bytearray(40), [0, 20], [20, 20])
    with pytest.raises(ValueError):
        f([2], b"abcd", [0], [4], [0, 1], bytearray(20), [0], [20])                             # two streams exist
    with pytest.raises(ValueError):
        f([0, 1], b"abcd", [0], [4], [0, 1], bytearray(20), [0], [20])                          # per-chain arrays differ
    with pytest.raises(IndexError):
        f([0], b"abcd", [1], [4], [0, 1], bytearray(20), [0], [20])                             # the source leaves src
    with pytest.raises(IndexError):
        f([0], b"abcdefgh", [4], [4], [0, 1], bytearray(20), [0], [20], [5])                    # the history lies in front of src
    with pytest.raises(amd.ReadOnlyBufferException):
        f([0], b"abcd", [0], [4], [0, 1], b"\0" * 20, [0], [20])
    with pytest.raises(ValueError):
        amd.CompressStreams(0)


def test_staging_layout_is_the_chain_calls_plus_slots(tmp_path):
    """host_staging.h: CChainMeta without slots is the layout it was; with slots the array lies behind chain_first, among the inputs"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "lz4-java_amd/csrc/host_staging.h"\n#include <stdio.h>\nint main() {\n'
                   '  const staging::CChainMeta a(7, 3), b(7, 3, false), c(7, 3, true);\n'
                   '  if (a.l.total != b.l.total || a.l.upload != b.l.upload || a.l.results != b.l.results || a.consumed.off != b.consumed.off || a.slot.n) return 1;\n'
                   '  if (c.slot.n != 3 || c.slot.off != c.first.off + 16 || c.slot.off + 12 > c.consumed.off || c.l.upload != c.l.total) return 2;\n'
                   '  puts("layout ok");\n  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-I" + ROOT, str(src), "-o", str(exe)])
    assert b"layout ok" in subprocess.check_output([str(exe)])


def test_cpp_mirror_cstream_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: CompressStreams builds (-Werror); tests/cpp/cstream_mirror_test.cpp exits 3 (loud library failure) without a
    device"""
    from cchain_common import chain_of, cchain_file
    from support import build_mirror
    exe = build_mirror("cstream_mirror_test", tmp_path, werror=True)
    if no_device():
        (tmp_path / "c.bin").write_bytes(cchain_file(chain_of("two", b"abcdefgh" * 5, [20, 20], history=b"0123")))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_cstream_natives_declared_and_checked_without_device(tmp_path):
    """the new natives are declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim; over the fake JNIEnv
    (tests/jni_stub/fake_jni_cstream.c) a 0 handle is an argument error with nothing pinned, and without a device no set can be made,
    loudly, nothing leaked"""
    from support import build_fake_jni, typecheck_jni_shim
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    for native in ("cstreamsCreate", "cstreamsCount", "cstreamsFree", "cstreamsReset", "cstreamsConsumed", "batchFastStream"):
        assert re.search(r"static\s+native\s+(int|long|void)\s+LZ4HIP_%s\s*\(" % native, java), native
        assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1%s" % native in shim, native
        assert "LZ4HIPJNI.LZ4HIP_%s(" % native in batch, native
    assert re.search(r"public static void compressFastStream\(CompressStreams streams, int\[\] streamId, ByteBuffer src", batch)
    assert "public static final class CompressStreams implements java.io.Closeable" in batch
    # the chain native keeps its signature
    assert re.search(r"static native int LZ4HIP_batchFastChain\(ByteBuffer src, long\[\] chainSrcOff, int\[\] chainPrefixLen, int\[\] srcLen, int\[\] chainFirst,", java)
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_cstream", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
