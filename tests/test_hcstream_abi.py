"""No-GPU checks of lz4hip_compress_hc_stream_batch (HC streams whose sources land anywhere) and its two state edits: the entry points
are declared, exported and bound in Python; every argument error of the contract is LZ4HIP_E_ARG and is said BEFORE a device is looked
for, with nothing written; a well-formed call fails loudly without a device (no CPU fallback); lz4hip_hcstream_load_dict and
lz4hip_hcstream_save_dict leave what the reference library's own fields say after LZ4_loadDictHC and LZ4_saveDictHC; the header says
the contract, its exceptions and its out-of-scope list; the staging arithmetic agrees with a naive restatement under the sanitizers (a
stand-alone program: nothing is loaded into Python)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from hcstream_common import Op, RefHCStream, Script, block, same_state, script_file
from support import E_ARG, E_NO_DEVICE, build_fake_jni, build_mirror, build_sanitized, no_device, typecheck_jni_shim
from test_dstream_abi import DEVICE_ENTRY_POINTS

u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8
NAME = "lz4hip_compress_hc_stream_batch"


class Call:
    """one well-formed call: stream 0 fresh with two blocks of 4 bytes, stream 1 behind a prefix of 4 bytes that ends at 48 and an external
    dictionary of 6 that ends at 80, one block"""
    ORDER = ("state", "src", "src_off", "src_len", "first", "dst", "dst_off", "dst_cap", "out", "n_blocks", "n_chains", "level")
    POINTERS = ORDER[:9]

    def __init__(self):
        self.state = (u64 * 10)(0, 0, 0, 0, 0, 48, 4, 80, 6, 10)
        self.src = (u8 * 96)(*range(96))
        self.src_off, self.src_len, self.first = (u64 * 3)(8, 30, 48), (i32 * 3)(4, 4, 4), (u32 * 3)(0, 2, 3)
        self.dst = (u8 * 64)(*([7] * 64))
        self.dst_off, self.dst_cap = (u64 * 3)(0, 20, 40), (i32 * 3)(20, 20, 20)
        self.out = (i32 * 3)(7, 7, 7)
        self.n_blocks, self.n_chains, self.level = 3, 2, 9

    def args(self, **kw):
        a = {k: getattr(self, k) for k in self.ORDER}
        a.update(kw)
        return [a[k] for k in self.ORDER]

    def untouched(self):
        return list(self.out) == [7, 7, 7] and bytes(self.dst) == bytes([7] * 64) and list(self.state) == [0, 0, 0, 0, 0, 48, 4, 80, 6, 10]


def header():
    return open(os.path.join(ROOT, "include", "lz4hip.h")).read()


def test_symbols_declared_exported_and_bound(amd):
    h = header()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    assert re.search(r"\bint\s+%s\s*\(\s*lz4hip_hcstream_state\s*\*\s*state,\s*const uint8_t\s*\*\s*src," % NAME, h)
    assert "typedef struct lz4hip_hcstream_state { uint64_t prefix_end, prefix_len, ext_end, ext_len, index; } lz4hip_hcstream_state;" in h
    for s in (NAME, "lz4hip_hcstream_load_dict", "lz4hip_hcstream_save_dict"):
        assert s in exported and s in amd.C_ABI and hasattr(amd.lib(), s), s
    assert len(amd.C_ABI[NAME][1]) == 12 and amd.C_ABI[NAME][1][-3:] == [C.c_uint32, C.c_uint32, C.c_int]
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    assert "hc_build_stream_kernel" in syms and "hc_parse_stream_kernel" in syms
    assert callable(amd.LZ4HIPBatch.compressHCStream)
    for m in ("loadDict", "saveDict", "compress", "state", "reset"):
        assert callable(getattr(amd.CompressStreamsHC, m)), m


def test_header_says_the_contract_and_declares_no_device_pointer_form():
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    names = re.findall(r"\b(lz4hip_[a-z0-9_]+)\s*\(", code)
    assert not [s for s in names if "_dev" in s and "hc_stream" in s]
    assert sorted(set(s for s in names if re.search(r"_dev(_ws)?$", s))) == sorted(DEVICE_ENTRY_POINTS)
    i = h.index("COMPRESS HC STREAMS WHOSE SOURCES LAND ANYWHERE")
    text = " ".join(h[i:h.index("int " + NAME, i)].replace("*", " ").split())
    for word in ("THE CONTRACT", "ONE LZ4_streamHC_t", "LZ4_resetStreamHC_fast", "however the blocks are cut into calls", "THE STATE is plain host data",
                 "no handle and no device memory between calls", "All zero is a fresh stream", "never of compressed results", "s != prefix_end (a jump)",
                 "ext_len = ext_end - min(s + n, ext_end), and under 4 bytes it becomes 0", "prefix_len += n, prefix_end = s + n, index += n",
                 "last 65535 bytes of external dictionary ++ prefix", "goes on at the prefix's start", "stops at the start of the piece the match lies in",
                 "last three positions of every contiguous run that a jump ended", "A RESULT OF 0 DOES NOT END THE STREAM",
                 "the engine's rule for src_len[i] < 0 or > 0x7E000000", "step 1 alone is applied, nothing is consumed", "LZ4_loadDictHC as a state edit",
                 "{dict_end, min(dict_len, 65536), 0, 0, min(dict_len, 65536)}", "lz4hip_compress_hc_dict", "LZ4_saveDictHC as a state edit",
                 "kept = min(k, 65536), below 4 it is 0, then min(kept, prefix_len)", "A CALL IS A SNAPSHOT", "LEVELS 1..9", "LEVELS 10..12", "stale entry",
                 "never matches", "NOT SERIAL", "only while the prefix is shorter than 65535 bytes", "hc_parse_stream_kernel", "hc_build_stream_kernel",
                 "shards over the initialised devices at stream boundaries", "Slots must not overlap", "said before a device is looked for",
                 "65536 + index would pass 2^31", "LZ4HIP_E_NO_DEVICE",
                 "out of scope: device-pointer forms; LZ4_attach_HC_dictionary; LZ4_compress_HC_continue_destSize; favorDecSpeed; the 2 GiB reload"):
        assert word in text, word
    flat = " ".join(h.replace("*", " ").split())
    assert "(No longer out of scope: LZ4_saveDictHC and sources that are not contiguous are lz4hip_compress_hc_stream_batch, below.)" in flat


def test_argument_errors_come_before_the_device(amd):
    """every LZ4HIP_E_ARG case of the contract, device or not; nothing is written"""
    l = amd.lib()
    f = getattr(l, NAME)
    f.argtypes, f.restype = amd.C_ABI[NAME][1], C.c_int
    c = Call()
    for name in Call.POINTERS:            # all pointers are required
        assert f(*c.args(**{name: None})) == E_ARG, name
        assert b"null" in l.lz4hip_last_error().lower() and c.untouched(), name
    for first in ((1, 2, 3), (0, 2, 2), (0, 2, 4), (0, 3, 2), (0, 4, 3)):
        assert f(*c.args(first=(u32 * 3)(*first))) == E_ARG, first
        assert b"chain_first" in l.lz4hip_last_error() and c.untouched()
    assert f(*c.args(n_chains=0)) == E_ARG and c.untouched()          # 3 blocks in no stream
    for st, word in (((0, 0, 0, 0, 0, 48, 49, 80, 6, 10), b"prefix_len"), ((0, 0, 0, 0, 0, 48, 4, 80, 81, 10), b"ext_len"),
                     ((0, 0, 0, 0, (1 << 31) - 65536 - 7, 48, 4, 80, 6, 10), b"2 GiB"), ((0, 0, 0, 0, 0, 48, 4, 80, 6, (1 << 31) - 65536 - 3), b"2 GiB")):
        c2 = Call()
        c2.state = (u64 * 10)(*st)
        assert f(*c2.args()) == E_ARG, st
        assert word in l.lz4hip_last_error(), (st, l.lz4hip_last_error())
        assert list(c2.out) == [7, 7, 7] and bytes(c2.dst) == bytes([7] * 64) and list(c2.state) == list(st)
    # exactly at the limit is fine: the next error is the missing device, or none at all
    c3 = Call()
    c3.state = (u64 * 10)(0, 0, 0, 0, (1 << 31) - 65536 - 8, 48, 4, 80, 6, 10)
    assert f(*c3.args()) != E_ARG
    # the two helpers
    st = (u64 * 5)()
    assert l.lz4hip_hcstream_load_dict(None, 10, 5) == E_ARG and l.lz4hip_hcstream_save_dict(None, 10, 5) == E_ARG
    assert l.lz4hip_hcstream_load_dict(st, 4, 5) == E_ARG and list(st) == [0] * 5


def test_well_formed_call_fails_loudly_without_a_device(amd):
    if not no_device():
        pytest.skip("a device is present: tests/test_gpu_hcstream.py runs the call")
    l = amd.lib()
    f = getattr(l, NAME)
    f.argtypes, f.restype = amd.C_ABI[NAME][1], C.c_int
    c = Call()
    assert f(*c.args()) == E_NO_DEVICE and c.untouched()
    assert f(*c.args(n_blocks=0, n_chains=0)) == E_NO_DEVICE
    with pytest.raises(amd.LZ4HIPError):
        amd.CompressStreamsHC(1).compress([0], bytes(64), [0], [10], [0, 1], bytearray(64), [0], [40])


def test_cpp_mirror_builds_and_fails_loudly_without_a_device(tmp_path):
    """the C++ twin (CompressStreamsHC of host/lz4hip.hpp) compiles warning-free and links against the C ABI; without a device its call
    fails loudly"""
    exe = build_mirror("hcstream_mirror_test", tmp_path, werror=True)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip.hpp")).read()
    assert "class CompressStreamsHC" in hpp and NAME + "(" in hpp and "lz4hip_hcstream_save_dict(" in hpp and "lz4hip_hcstream_load_dict(" in hpp
    if no_device():
        sc = Script("t", 100, [block(10, bytes(range(40)))])
        (tmp_path / "s.bin").write_bytes(script_file(sc, 9))
        assert subprocess.call([exe, str(tmp_path / "s.bin"), str(tmp_path / "o.bin")], stderr=subprocess.DEVNULL) == 3


def test_java_twin_and_jni_shim():
    """LZ4HIPBatch.CompressStreamsHC and compressHCStream are declared over the native LZ4HIP_batchHCStream, which the shim exports and
    hands to the C ABI; the shim type-checks against the stub jni.h; its entry RUNS over the fake JNIEnv (tests/jni_stub/
    fake_jni_hcstream.c): a NULL array, buffer or state is LZ4HIP_E_ARG with nothing left pinned, and without a device the call fails loudly"""
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static\s+native\s+int\s+LZ4HIP_batchHCStream\s*\(long\[\] state, ByteBuffer src, long\[\] srcOff,", java)
    assert "public static final class CompressStreamsHC" in batch and "LZ4HIPJNI.LZ4HIP_batchHCStream(" in batch
    for m in ("public void loadDict(int streamId, long dictEnd, long dictLen)", "public int saveDict(int streamId, long bufOff, int k)",
              "public void compress(int[] streamId, ByteBuffer src, long[] srcOff", "public static void compressHCStream(long[] state, ByteBuffer src"):
        assert m in batch, m
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCStream" in shim and NAME + "(" in shim
    typecheck_jni_shim()


def test_jni_shim_runs_over_the_fake_jnienv_without_a_device(tmp_path):
    if not no_device():
        pytest.skip("a device is present: tests/test_gpu_hcstream.py runs the program")
    exe = build_fake_jni("fake_jni_hcstream", tmp_path)
    out = subprocess.check_output([exe, "--no-gpu"]).decode()
    assert "checks ok" in out, out


def test_helpers_against_the_references_fields(amd, ref):
    """lz4hip_hcstream_load_dict and lz4hip_hcstream_save_dict leave the state that the reference's own fields show behind LZ4_loadDictHC and
    LZ4_saveDictHC: dictionaries of 0 .. 70000 bytes; k = 0, 3, 4, 100, 4096, 65536, 70000 and a negative one behind prefixes shorter
    and longer than k"""
    rr = RefHCStream(ref)
    l = amd.lib()
    data = bytes(range(256)) * 300
    n = 0
    for dlen in (0, 1, 3, 4, 100, 65535, 65536, 65537, 70000):
        sc = Script("load %d" % dlen, 80000, [Op("L", 100 + dlen, n=dlen)], [(100, data[:dlen])])
        want = rr.run(sc, 9)[0][1]
        st = (u64 * 5)(9, 9, 9, 9, 9)
        assert l.lz4hip_hcstream_load_dict(st, 100 + dlen, dlen) == 0
        assert same_state(tuple(st), want) and tuple(st)[2:4] == (0, 0), (dlen, tuple(st), want)
        n += 1
    for plen in (0, 2, 50, 5000, 66000):
        for k in (-5, 0, 3, 4, 100, 4096, 65536, 70000):
            ops = [block(70000, data[:7]), block(1000, data[:plen]), Op("S", 200000, k=k)]
            sc = Script("save %d %d" % (plen, k), 280000, ops)
            res = rr.run(sc, 9)
            st = (u64 * 5)(*res[1][3])
            kept = l.lz4hip_hcstream_save_dict(st, 200000, k)
            assert kept == res[2][1] and same_state(tuple(st), res[2][2]) and st[3] == 0, (plen, k, kept, tuple(st), res[2])
            n += 1
    assert n == 49


def test_python_layer_checks_its_arguments(amd):
    B = amd.LZ4HIPBatch
    src, dst = bytes(100), bytearray(100)
    fresh = [(0, 0, 0, 0, 0)]
    for kw in (dict(srcOff=[90], srcLen=[20]), dict(srcOff=[-1], srcLen=[4]), dict(srcOff=[101], srcLen=[-1]), dict(dstOff=[90], dstCap=[20]),
               dict(chainFirst=[0]), dict(srcLen=[1, 2]), dict(state=[(200, 4, 0, 0, 4)]), dict(state=[(10, 0, 300, 4, 4)]), dict(state=[(-1, 0, 0, 0, 0)])):
        a = dict(state=fresh, src=src, srcOff=[0], srcLen=[10], chainFirst=[0, 1], dst=dst, dstOff=[0], dstCap=[40])
        a.update(kw)
        with pytest.raises((IndexError, ValueError)):
            B.compressHCStream(a["state"], a["src"], a["srcOff"], a["srcLen"], a["chainFirst"], a["dst"], a["dstOff"], a["dstCap"])
    with pytest.raises(amd.ReadOnlyBufferException):
        B.compressHCStream(fresh, src, [0], [10], [0, 1], bytes(100), [0], [40])
    hs = amd.CompressStreamsHC(3, 12)
    assert len(hs) == 3 and hs.level == 12 and hs.state() == [(0, 0, 0, 0, 0)] * 3
    hs.loadDict(1, 70000, 66000)
    assert hs.state([1]) == [(70000, 65536, 0, 0, 65536)]
    assert hs.saveDict(1, 5, 100) == 100 and hs.state([1]) == [(105, 100, 0, 0, 65536)]
    with pytest.raises(IndexError):
        hs.loadDict(0, 5, 6)
    with pytest.raises(ValueError):
        hs.compress([1, 1], src, [0, 0], [1, 1], [0, 1, 2], dst, [0, 50], [40, 40])
    hs.reset([1])
    assert hs.state() == [(0, 0, 0, 0, 0)] * 3
    with pytest.raises(ValueError):
        amd.CompressStreamsHC(0)


def test_staging_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/hcstream_staging_test.cpp: the state machine and the linear image against a naive restatement, as a stand-alone program
    built with the address and undefined-behaviour sanitizers"""
    exe = build_sanitized("hcstream_staging_test", tmp_path)
    out = subprocess.check_output([exe]).decode()
    assert "hcstream staging ok" in out, out
