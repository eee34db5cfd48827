"""No-GPU checks of the stream decoder (lz4hip_decompress_safe_stream_batch): the entry point is declared, exported and bound in Python,
C++ and Java; every argument error of its contract is LZ4HIP_E_ARG and is said BEFORE a device is looked for, with nothing written; a
well-formed call fails loudly without a device (no CPU fallback); the header says the contract and still declares exactly the device
entry points it did; the staging arithmetic agrees with a naive restatement under the sanitizers; the Python layer checks its
arguments."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, build_sanitized, no_device, typecheck_jni_shim

u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8
NAME = "lz4hip_decompress_safe_stream_batch"
# the device entry points the header declared before this call existed
DEVICE_ENTRY_POINTS = """lz4hip_compress_dest_size_batch_dev lz4hip_compress_fast_accel_batch_dev lz4hip_compress_fast_batch_dev
lz4hip_compress_fast_chain_batch_dev lz4hip_compress_fast_dict_batch_dev lz4hip_compress_hc_batch_dev lz4hip_compress_hc_batch_dev_ws
lz4hip_compress_hc_dest_size_batch_dev lz4hip_compress_hc_dest_size_batch_dev_ws lz4hip_compress_hc_dict_batch_dev
lz4hip_compress_hc_dict_batch_dev_ws lz4hip_container_blocks_dev lz4hip_container_decode_dev lz4hip_dbg_compress_fast_profile_dev
lz4hip_decompress_fast_batch_dev
lz4hip_decompress_safe_batch_dev lz4hip_decompress_safe_chain_batch_dev lz4hip_decompress_safe_dict_batch_dev
lz4hip_decompress_safe_partial_batch_dev lz4hip_decompressed_size_batch_dev lz4hip_gen_blocks_dev lz4hip_xxh32_batch_dev
lz4hip_xxh64_batch_dev lz4hip_xxh_stream_update_dev""".split()


class Call:
    """one well-formed call: two streams of 2 + 1 blocks; stream 0 fresh in the window [8, 72), stream 1 in [80, 144) behind a prefix of
    4 bytes that ends at 96 and an external dictionary of 6 bytes that ends at 200, outside the window"""

    def __init__(self):
        self.state = (u64 * 8)(0, 0, 0, 0, 96, 4, 200, 6)
        self.src = (u8 * 64)(*([0x10, 97] * 32))
        self.src_off, self.src_len, self.first = (u64 * 3)(0, 2, 4), (i32 * 3)(2, 2, 2), (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 256)(*([7] * 256))
        self.dst_off, self.dst_cap = (u64 * 3)(8, 40, 96), (i32 * 3)(16, 32, 48)
        self.win_off, self.win_len = (u64 * 2)(8, 80), (u64 * 2)(64, 64)
        self.out = (i32 * 3)(7, 7, 7)
        self.n_blocks, self.n_chains = 3, 2

    ORDER = ("state", "src", "src_off", "src_len", "first", "dst", "dst_off", "dst_cap", "win_off", "win_len", "out", "n_blocks", "n_chains")

    def args(self, **kw):
        a = {k: getattr(self, k) for k in self.ORDER}
        a.update(kw)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and bytes(self.dst) == bytes([7] * 256) and list(self.state) == [0, 0, 0, 0, 96, 4, 200, 6]


def header():
    return open(os.path.join(ROOT, "include", "lz4hip.h")).read()


def test_dstream_symbol_declared_exported_and_bound(amd):
    h = header()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    assert re.search(r"\bint\s+%s\s*\(\s*lz4hip_dstream_state\s*\*\s*state" % NAME, h)
    assert re.search(r"typedef struct lz4hip_dstream_state \{ uint64_t prefix_end, prefix_len, ext_end, ext_len; \} lz4hip_dstream_state;", h)
    assert NAME in exported and NAME in amd.C_ABI and hasattr(amd.lib(), NAME)
    assert len(amd.C_ABI[NAME][1]) == 13
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "decode_stream_kernel" in syms and "decode_chain_kernel" in syms
    assert callable(amd.DecodeStreams) and callable(amd.LZ4HIPBatch.decompressSafeStream)
    for m in ("set", "reset", "state", "decompress"):
        assert callable(getattr(amd.DecodeStreams, m))
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip.hpp")).read()
    assert "class DecodeStreams" in hpp and "static std::vector<int32_t> decompressSafeStream(" in hpp and NAME + "(" in hpp


def test_header_says_the_contract_and_declares_the_device_entry_points_it_did():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(s for s in re.findall(r"\b(lz4hip_[a-z0-9_]+)\s*\(", code) if re.search(r"_dev(_ws)?$", s)))
    assert not [s for s in re.findall(r"\b(lz4hip_[a-z0-9_]+)\s*\(", code) if "_dev" in s and "stream_batch" in s]
    assert declared == sorted(DEVICE_ENTRY_POINTS), set(declared) ^ set(DEVICE_ENTRY_POINTS)
    i = h.index("DECODE STREAMS WHOSE BLOCKS LAND ANYWHERE")
    text = " ".join(h[i:h.index("typedef struct lz4hip_dstream_state", i)].replace("*", " ").split())
    for word in ("LZ4_decompress_safe_forceExtDict", "LZ4_decompress_safe_doubleDict", "LZ4_setStreamDecode(sd, dst + p, n) is {p + n, n, 0, 0}",
                 "BEFORE decoding", "continues at the start of the prefix", "LZ4HIP_CHAIN_STOPPED", "THE WINDOW", "uploaded once per staged chunk",
                 "stays contiguous with the window", "Windows of different streams must not overlap", "control flow never depends on copied bytes",
                 "the bytes of matches that read the overlapped part are unspecified", "nothing outside the slot is written",
                 "nothing outside window and history pieces is read", "65535 + 2 x maxBlock", "65536 + 14 + maxBlock", "store-exact, strictly in-order",
                 "follow-up", "out of scope: a device-pointer form", "stored blocks", "fast and partial decoders in stream form",
                 "LZ4_decoderRingBufferSize", "said before a device is looked for", "LZ4HIP_E_NO_DEVICE", "there is no handle"):
        assert word in text, word
    # the chain call's list stays, with the pointer to this call
    assert "ring-buffer destinations that wrap" in h
    assert re.search(r"No longer\s+\*\s+out of scope: dictionaries elsewhere, destinations that wrap or alternate and save areas are\s+\*\s+"
                     r"lz4hip_decompress_safe_stream_batch, below", h)


def test_dstream_argument_errors_come_before_the_device(amd):
    """every LZ4HIP_E_ARG case of the contract, device or not: a NULL where a pointer is required (every pointer is), a chain_first that
    is not ascending from 0 to n_blocks, a slot outside its window, a history piece that straddles a window edge, a history longer than
    its end offset; nothing is written, the state stays"""
    l = amd.lib()
    c = Call()
    f = getattr(l, NAME)
    err = lambda: l.lz4hip_last_error().lower()
    for name in Call.ORDER[:11]:
        assert f(*c.args(**{name: None})) == E_ARG, name
        assert b"null pointer" in err(), name
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert f(*c.args(first=(u32 * 3)(*first))) == E_ARG and b"chain_first" in err(), first
    assert f(*c.args(n_chains=0)) == E_ARG and b"chain_first" in err()               # 3 blocks in no stream
    for off, cap in (((7, 40, 96), (16, 32, 48)), ((8, 40, 96), (16, 33, 48)), ((8, 40, 145), (16, 32, 0)), ((8, 40, 79), (16, 32, 1)),
                     ((8, 40, 96), (16, 32, 49))):
        assert f(*c.args(dst_off=(u64 * 3)(*off), dst_cap=(i32 * 3)(*cap))) == E_ARG and b"outside its stream's window" in err(), (off, cap)
    assert f(*c.args(win_off=(u64 * 2)(8, 2 ** 64 - 4))) == E_ARG
    for st in ((0, 0, 0, 0, 82, 4, 200, 6), (0, 0, 0, 0, 146, 4, 200, 6), (0, 0, 0, 0, 96, 4, 82, 6), (0, 0, 0, 0, 96, 4, 145, 6), (10, 4, 0, 0, 96, 4, 200, 6)):
        assert f(*c.args(state=(u64 * 8)(*st))) == E_ARG and b"straddles" in err(), st
    for st in ((0, 0, 0, 0, 96, 97, 200, 6), (0, 0, 0, 0, 96, 4, 5, 6), (3, 4, 0, 0, 96, 4, 200, 6)):
        assert f(*c.args(state=(u64 * 8)(*st))) == E_ARG and b"reaches in front of dst" in err(), st
    assert c.untouched()
    # what is NOT an argument error: a history that ends exactly where the window begins or begins where it ends, one far away, an
    # empty history with any end, a negative length (the kernel's -1) -- these get as far as the device
    for st in ((0, 0, 0, 0, 80, 4, 200, 6), (0, 0, 0, 0, 96, 4, 150, 6), (0, 0, 0, 0, 96, 4, 80, 6), (5, 0, 77, 0, 96, 4, 200, 6)):
        rc = f(*c.args(state=(u64 * 8)(*st)))
        assert rc == (E_NO_DEVICE if no_device() else 0), (st, rc, l.lz4hip_last_error())
    if no_device():
        assert f(*c.args(src_len=(i32 * 3)(2, -1, 2))) == E_NO_DEVICE


def test_dstream_fails_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    c = Call()
    assert getattr(l, NAME)(*c.args()) == E_NO_DEVICE and b"no HIP device" in l.lz4hip_last_error()
    assert c.untouched()
    assert getattr(l, NAME)(*c.args(n_blocks=0, n_chains=0)) == E_NO_DEVICE
    with pytest.raises(amd.LZ4HIPError):
        amd.DecodeStreams(1).decompress([0], b"\x10a", [0], [2], [0, 1], bytearray(64), [8], [16], [8], [32])


def test_dstream_python_layer_checks(amd):
    f = amd.LZ4HIPBatch.decompressSafeStream
    ok = ([(0, 0, 0, 0)], b"\x10a", [0], [2], [0, 1], bytearray(64), [8], [16], [8], [32])
    def bad(exc, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        with pytest.raises(exc):
            f(*a)
    bad(ValueError, a3=[2, 2])                      # per-block arrays differ
    bad(ValueError, a8=[8, 8])                      # per-stream arrays differ
    bad(ValueError, a4=[0, 2])                      # chainFirst
    bad(IndexError, a2=[1])                         # the source leaves src
    bad(IndexError, a6=[60])                        # the slot leaves dst
    bad(IndexError, a9=[60])                        # the window leaves dst
    bad(IndexError, a0=[(3, 4, 0, 0)])              # a history longer than its end
    bad(IndexError, a0=[(8, 4, 70, 4)])             # a history behind the buffer
    bad(amd.ReadOnlyBufferException, a5=b"\0" * 64)
    with pytest.raises(ValueError):
        amd.DecodeStreams(0)
    ds = amd.DecodeStreams(3)
    ds.set(1, 40, 8)
    assert ds.state() == [(0, 0, 0, 0), (40, 8, 0, 0), (0, 0, 0, 0)] and len(ds) == 3
    with pytest.raises(IndexError):
        ds.set(2, 4, 8)
    with pytest.raises(ValueError):
        ds.decompress([1, 1], b"\x10a" * 2, [0, 2], [2, 2], [0, 1, 2], bytearray(64), [8, 40], [16, 16], [8, 40], [16, 16])
    ds.reset([1])
    assert ds.state([1]) == [(0, 0, 0, 0)]


def test_dstream_staging_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/dstream_staging_test.cpp: window, lead-room and piece placement, the device states and the way back, the argument
    errors and the joined runs against a naive restatement -- host code alone, address and undefined-behaviour sanitizers"""
    exe = build_sanitized("dstream_staging_test", tmp_path)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "dstream staging ok: 205000 cases" in out, out


def test_cpp_mirror_dstream_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp: DecodeStreams builds (-Werror); tests/cpp/dstream_mirror_test.cpp exits 3 (loud library failure) without a
    device"""
    from dstream_common import Block, Stream, stream_file
    exe = build_mirror("dstream_mirror_test", tmp_path, werror=True)
    if no_device():
        s = Stream("two", "a", 64, [Block(b"\x10a", 0, 8), Block(b"\x10b", 1, 8)], True)
        (tmp_path / "s.bin").write_bytes(stream_file(s, [1, 2]))
        p = subprocess.run([exe, str(tmp_path / "s.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_dstream_native_declared_and_checked_without_device(tmp_path):
    """the new native is declared in LZ4HIPJNI.java, used by LZ4HIPBatch.java and defined in the shim; over the fake JNIEnv
    (tests/jni_stub/fake_jni_dstream.c) every argument error is said with nothing pinned, and without a device the call fails loudly,
    nothing leaked, the state as it was"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchSafeStream\s*\(long\[\] state, ByteBuffer src,", java)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStream" in shim and "LZ4HIPJNI.LZ4HIP_batchSafeStream(" in batch
    assert re.search(r"public static void decompressSafeStream\(long\[\] state, ByteBuffer src", batch)
    assert "public static final class DecodeStreams" in batch
    for m in ("public void set(int streamId, long prefixEnd, long prefixLen)", "public void reset(int[] streamId)", "public long[] state(int streamId)",
              "public void decompress(int[] streamId, ByteBuffer src"):
        assert m in batch, m
    # the chain native keeps its signature
    assert re.search(r"static native int LZ4HIP_batchSafeChain\(ByteBuffer src, long\[\] srcOff, int\[\] srcLen, int\[\] stored, int\[\] destCap, int\[\] chainFirst,", java)
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_dstream", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
