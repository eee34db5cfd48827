"""The accelerated linked-block compressors, the layers that need no GPU: the three C entry points (lz4hip_compress_fast_chain_accel_batch,
lz4hip_compress_fast_stream_accel_batch, lz4hip_compress_fast_stream_ext_accel_batch) are declared, exported and bound; their argument
errors and their failure without a device are their acceleration-1 twins'; the Python keywords, the frame writer's checks, the C++ mirror
and the JNI shim."""
import ctypes as C
import inspect
import io
import os
import re
import struct
import subprocess

import pytest

from caccel_common import NAMES, ChainCall, ExtCall, StreamCall
from cchain_common import book1, bound, cchain_file, chain_of
from support import E_ARG, E_NO_DEVICE, ROOT, build_fake_jni, build_mirror, no_device, typecheck_jni_shim

u64, i32, u32 = C.c_uint64, C.c_int32, C.c_uint32
KERNELS = ("compress_fast_chain_accel_cu_kernel", "compress_fast_stream_accel_cu_kernel", "compress_fast_xstream_accel_cu_kernel")


def header():
    return open(os.path.join(ROOT, "include", "lz4hip.h")).read()


def test_symbols_declared_exported_and_bound(amd):
    h = header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    syms = subprocess.check_output(["strings", so]).decode(errors="replace")
    for name, twin in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        twin_decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % twin, code)
        assert decl and twin_decl, name
        norm = lambda s: " ".join(s.split())
        assert norm(decl.group(1)) == norm(twin_decl.group(1)) + ", int acceleration", name      # the twin's list plus the trailing argument
        assert name in exported and name in amd.C_ABI and hasattr(amd.lib(), name)
        assert amd.C_ABI[name][1] == amd.C_ABI[twin][1] + [C.c_int]
        assert name + "_dev" not in code
    for k in KERNELS:
        assert k in syms, k
    i = h.index("LINKED BLOCKS WITH AN ACCELERATION")
    text = " ".join(h[i:h.index("int lz4hip_compress_fast_chain_accel_batch", i)].replace("*", " ").split())
    for word in ("ONE acceleration per call", "< 1 -> 1, > 65537", "acceleration 1 IS the twin", "acceleration << 6", "any mix of the six entry points",
                 "NO device-pointer", "a per-block acceleration array", "lz4hip_compress_fast_dict", "LZ4_attach_dictionary", "lean and window-parallel",
                 "lz4 --fast=N", "profiles/caccel_kernel_diff.txt"):
        assert word in text, word
    assert "- out of scope: acceleration above 1" not in " ".join(h.replace("*", " ").split())


def test_argument_errors_are_the_twins(amd):
    """every argument error of the chain entry, with the twin's status and message, before a device is looked for; a NULL set for the two
    stream entries"""
    l = amd.lib()
    f, twin = l.lz4hip_compress_fast_chain_accel_batch, l.lz4hip_compress_fast_chain_batch
    c = ChainCall()
    cases = [{k: None} for k in ("src", "cso", "sl", "first", "dst", "doff", "dc", "out", "cons")]
    cases += [{"first": (u32 * 3)(*v)} for v in ((1, 2, 3), (0, 2, 2), (0, 3, 2))] + [{"pre": (i32 * 2)(*v)} for v in ((5, 0), (0, -1), (0, 41))]
    for kw in cases:
        for accel in (0, 8, 70000):
            assert f(*c.args(accel, **kw)) == E_ARG, kw
            msg = l.lz4hip_last_error()
            assert twin(*c.args(**kw)) == E_ARG and l.lz4hip_last_error() == msg, kw
    assert c.untouched()


def test_stream_argument_errors_are_the_twins(amd):
    """the argument errors of the two stream entries that need no set (the library checks them in front of it): the accelerated entry
    answers with its twin's status and its twin's message, at any acceleration -- NULL pointers, a chain_first that does not ascend to
    n_blocks, ids that do not ascend, a prefix longer than the chain's offset, a source outside its window, a history piece that
    straddles a window edge or is negative; a well-formed call gets as far as the missing set.  Nothing is written"""
    l = amd.lib()
    u = lambda *v: (u32 * len(v))(*v)
    common = [{"first": u(1, 2, 3)}, {"first": u(0, 3, 2)}, {"n_chains": 0}, {"ids": u(1, 1)}, {"ids": u(1, 0)}, {}]
    cases = {"lz4hip_compress_fast_stream_accel_batch": (StreamCall(), [{k: None} for k in ("ids", "src", "cso", "sl", "first", "dst", "doff", "dc", "out", "cons")]
                                                         + common + [{"pre": (i32 * 2)(5, 0)}, {"pre": (i32 * 2)(0, -1)}]),
             "lz4hip_compress_fast_stream_ext_accel_batch": (ExtCall(), [{k: None} for k in ExtCall.ORDER[1:15]] + common
                                                             + [{"src_off": (u64 * 3)(7, 30, 60)}, {"src_off": (u64 * 3)(8, 37, 60)}, {"win_off": (u64 * 2)(8, 2 ** 64 - 4)},
                                                                {"hist_end": (u64 * 2)(0, 42)}, {"hist_end": (u64 * 2)(0, 3)}, {"hist_len": (i32 * 2)(0, -1)}])}
    for name, (c, kws) in cases.items():
        f, twin = getattr(l, name), getattr(l, NAMES[name])
        seen = set()
        for kw in kws:
            assert twin(*c.args(**kw)) == E_ARG, (name, kw)
            msg = l.lz4hip_last_error()
            seen.add(msg)
            for accel in (0, 8, 70000):
                assert f(*c.args(accel, **kw)) == E_ARG and l.lz4hip_last_error() == msg, (name, kw, accel, msg)
        assert len(seen) >= 5 and any(b"stream set" in m.lower() for m in seen), (name, seen)     # (the cases reach different checks; the last is the set's)
        assert c.untouched()


def test_fails_loudly_without_device(amd):
    if not no_device():
        pytest.skip("a GPU is present")
    l = amd.lib()
    c = ChainCall()
    for accel in (-7, 1, 2, 65537, 1 << 30):
        assert l.lz4hip_compress_fast_chain_accel_batch(*c.args(accel)) == E_NO_DEVICE and b"no HIP device" in l.lz4hip_last_error()
        msg = l.lz4hip_last_error()
        assert l.lz4hip_compress_fast_chain_batch(*c.args()) == E_NO_DEVICE and l.lz4hip_last_error() == msg
    assert c.untouched()
    d = bytearray(64)
    with pytest.raises(amd.LZ4HIPError):
        amd.LZ4HIPBatch.compressFastChain(b"abcdefgh" * 4, [0], [32], [0, 1], d, [0], [64], acceleration=8)
    with pytest.raises(amd.LZ4HIPError):
        amd.CompressStreams(2)


def test_python_keywords_exist(amd):
    for fn in (amd.LZ4HIPBatch.compressFastChain, amd.LZ4HIPBatch.compressFastStream, amd.LZ4HIPBatch.compressFastStreamAt, amd.CompressStreams.compress,
               amd.CompressStreams.compressAt):
        p = inspect.signature(fn).parameters
        assert "acceleration" in p and p["acceleration"].default == 1 and list(p)[-1] == "acceleration", fn


def test_frame_writer_checks_and_default(ref, port, O):
    """acceleration needs linkedBlocks and no level; at the default the writer calls its engine exactly as before -- an engine that does
    not know the keyword still serves it -- and every byte is what it was; an engine that knows it gets it"""
    import importlib
    from caccel_common import RefAccelChain
    from cchain_common import RefCChain, batched_linked_frame, oracle_cchain_engine
    from streams_common import OracleEngine
    F = importlib.import_module("lz4-java_amd.streams")
    with pytest.raises(ValueError):
        F.LZ4FrameOutputStream(io.BytesIO(), 4, acceleration=8)
    with pytest.raises(ValueError):
        F.LZ4FrameOutputStream(io.BytesIO(), 4, linkedBlocks=True, level=9, acceleration=8)
    data = book1()[:200000]
    rc = RefCChain(ref)
    sink = io.BytesIO()
    w = F.LZ4FrameOutputStream(sink, 4, -1, linkedBlocks=True, engine=oracle_cchain_engine(OracleEngine, rc, port=port, O=O))   # (no keyword there)
    w.write(data)
    w.close()
    assert sink.getvalue() == batched_linked_frame(rc, port.xxh32, data, 4, 10 ** 6)
    ra = RefAccelChain(ref)
    eng = oracle_cchain_engine(OracleEngine, ra, port=port, O=O)
    plain = eng.compressFastChain

    def with_keyword(*a, acceleration=1):
        ra.at(acceleration)
        try:
            return plain(*a)
        finally:
            ra.at(1)
    eng.compressFastChain = with_keyword
    sink = io.BytesIO()
    w = F.LZ4FrameOutputStream(sink, 4, -1, linkedBlocks=True, acceleration=8, engine=eng)
    w.write(data)
    w.close()
    want = batched_linked_frame(ra.at(8), port.xxh32, data, 4, 10 ** 6)
    assert sink.getvalue() == want and want != batched_linked_frame(ra.at(1), port.xxh32, data, 4, 10 ** 6)


def test_cpp_mirror_builds_and_fails_loudly(tmp_path):
    """host/lz4hip.hpp and lz4hip_streams.hpp build with the acceleration parameter (-Werror); tests/cpp/caccel_mirror_test.cpp exits 3
    (loud library failure) without a device"""
    exe = build_mirror("caccel_mirror_test", tmp_path, werror=True)
    hpp = open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip.hpp")).read()
    for name in NAMES:
        assert name + "(" in hpp, name
    assert "void acceleration(int a)" in open(os.path.join(ROOT, "lz4-java_amd", "host", "lz4hip_streams.hpp")).read()
    if no_device():
        b = book1()
        (tmp_path / "c.bin").write_bytes(cchain_file(chain_of("c", b[100:4100], [1000] * 4, history=b[:100])))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin"), "8"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 3 and b"no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_jni_shim_and_java_overloads(tmp_path):
    typecheck_jni_shim()
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    for native, name in (("batchFastChainAccel", "lz4hip_compress_fast_chain_accel_batch"), ("batchFastStreamAccel", "lz4hip_compress_fast_stream_accel_batch"),
                         ("batchFastStreamAtAccel", "lz4hip_compress_fast_stream_ext_accel_batch")):
        assert re.search(r"static\s+native\s+int\s+LZ4HIP_%s\s*\([^;]*int acceleration\);" % native, java), native
        assert "LZ4HIPJNI.LZ4HIP_%s(" % native in batch
        assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1%s" % native in shim and name + "(" in shim
    assert len(re.findall(r"public static void compressFastChain\(", batch)) == 2 and len(re.findall(r"public void compressAt\(", batch)) == 2
    assert re.search(r"public void compress\(int\[\] streamId,[^)]*long\[\] chainConsumed, int acceleration\)", batch)
    exe = build_fake_jni("fake_jni_caccel", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
