"""The HC linked-block compressor (LZ4_compress_HC_continue over chains, liblz4's prefix mode) on the GPU against the reference library's
own stream compressor: the case set of tests/hcchain_common.py through lz4hip_compress_hc_chain_batch, a call or two per level; the
same with the build cut into segments of 4096 and 65536 positions; one chain of 256 x 4096 bytes, the single-stream case the design is
for; the same call repeated; the Python class, the C++ mirror, the JNI shim, the frame writer and the multi-device path.  Guard bytes
(0xA5) lie around every slot and around every chain's region, and what every call produced goes back through the chain decoder and is
compared with the source."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from cchain_common import GUARD, book1, cchain_file, chain_of
from hcchain_common import BIG_LEVELS, CLAMPS, LEVELS, HCPacked, RefHCChain, case_set, expected, hc_linked_frame, is_small
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def rc(ref):
    return RefHCChain(ref)


@pytest.fixture(scope="module")
def chains(rc):
    return case_set(rc)


def chains_at(chains, level):
    """the set at `level`: every chain at 9 and 10, the chains of up to 20 000 bytes at the other levels and the two clamps"""
    return chains if level in BIG_LEVELS else [c for c in chains if is_small(c)]


def host_abi_call(amd, pk, level, with_prefix=True):
    """the C ABI's call as it is (the Python layer refuses negative lengths and capacities) -> (dst, out)"""
    dst = bytearray(pk.dst)
    arr = lambda t, v: (t * max(len(v), 1))(*v)
    out = (C.c_int32 * max(pk.n_blocks, 1))()
    dbuf = (C.c_uint8 * len(dst)).from_buffer(dst)
    r = amd.lib().lz4hip_compress_hc_chain_batch(pk.src, arr(C.c_uint64, pk.chain_src_off), arr(C.c_int32, pk.prefix) if with_prefix else None,
                                                 arr(C.c_int32, pk.src_len), arr(C.c_uint32, pk.chain_first), C.addressof(dbuf), arr(C.c_uint64, pk.dst_off),
                                                 arr(C.c_int32, pk.dst_cap), out, pk.n_blocks, pk.n_chains, level)
    assert r == 0, amd.lib().lz4hip_last_error()
    del dbuf
    return dst, list(out)[:pk.n_blocks]


def decode_back(amd, pk, dst, out):
    """what the call produced through the chain decoder (LZ4HIPBatch.decompressSafeChain).  A block that failed leaves a hole and the
    blocks behind it still refer to its source, so every run of blocks that succeeded is a chain of the decoder's, behind the last
    64 KB of what lies in front of the run in the compressor's chain"""
    src_off, src_len, dst_cap, first, cdo, ccap, pre, runs = [], [], [], [0], [], [], [], []
    buf = bytearray(b"\xA5" * GUARD)
    for c in range(pk.n_chains):
        lo, at = pk.chain_src_off[c] - pk.prefix[c], pk.chain_src_off[c]
        i, b1 = pk.chain_first[c], pk.chain_first[c + 1]
        while i < b1:
            if out[i] <= 0:
                at += max(pk.src_len[i], 0)
                i += 1
                continue
            start = at
            while i < b1 and out[i] > 0:
                src_off.append(pk.dst_off[i]); src_len.append(out[i]); dst_cap.append(pk.src_len[i])
                at += pk.src_len[i]
                i += 1
            P = min(start - lo, 65536)
            first.append(len(src_off))
            buf += pk.src[start - P:start]
            cdo.append(len(buf)); ccap.append(at - start); pre.append(P); runs.append((c, start))
            buf += b"\x33" * (at - start) + b"\xA5" * GUARD
    if not src_off:
        return
    r, cout = amd.LZ4HIPBatch.decompressSafeChain(bytes(dst), src_off, src_len, dst_cap, first, buf, cdo, ccap, pre)
    assert list(r) == dst_cap and list(cout) == ccap, "the decoder's values"
    for k, (c, start) in enumerate(runs):
        assert bytes(buf[cdo[k]:cdo[k] + ccap[k]]) == pk.src[start:start + ccap[k]], ("round trip", pk.chains[c].name)


def run_set(amd, rc, chains, level, what, with_prefix=True):
    """one call: values and bytes are the reference's; only the bytes produced came back -- every other byte of the caller's buffer is as
    it was, the slot of a block that failed included; what was produced decodes to the source"""
    pk = HCPacked(chains)
    dst, out = host_abi_call(amd, pk, level, with_prefix)
    bad = pk.check(dst, out, expected(rc, chains, level))
    assert not bad, (what, level, len(bad), bad[:5])
    for i in range(pk.n_blocks):
        o, cap, r = pk.dst_off[i], max(pk.dst_cap[i], 0), max(out[i], 0)
        assert dst[o + r:o + cap] == bytes([pk.fill]) * (cap - r), i
    decode_back(amd, pk, dst, out)


@pytest.mark.parametrize("level", LEVELS + tuple(a for a, _ in CLAMPS))
def test_hcchain_set(amd, rc, chains, level):
    """the set at one level in ONE call (one launch of the three kernels per device), and every second chain again: the same scratch
    and workspace, reused.  Only the last 64 KB of a history are uploaded: a 70000-byte prefix still gives the reference's bytes"""
    sel = chains_at(chains, level)
    assert len(sel) >= (400 if level in BIG_LEVELS else 300)
    assert any(len(c.history) == 70000 for c in sel) or level not in BIG_LEVELS
    run_set(amd, rc, sel, level, "whole set")
    run_set(amd, rc, sel[::2], level, "every second chain")


@pytest.mark.parametrize("seg", (4096, 65536))
def test_hcchain_segments(amd, rc, chains, seg):
    """the same bytes with the build cut every 4096 and every 65536 positions: cuts inside blocks, on block boundaries and less than
    64 KB from a chain's start"""
    try:
        amd.set_option("hc_chain_segment", seg)
        for level in (9, 10, 3):
            run_set(amd, rc, chains_at(chains, level), level, "segments of %d" % seg)
    finally:
        amd.set_option("hc_chain_segment", 1 << 20)


def test_hcchain_single_long_chain(amd, rc):
    """one chain of 256 x 4096 bytes of book1 (wrapped around) at level 9 behind 1000 bytes of history: the single-stream case -- 256
    blocks parsed at once, the build in two segments at 1 MiB and in 17 at 65536"""
    b = book1()
    data = (b * 3)[700000:700000 + 1000 + 256 * 4096]
    ch = chain_of("256 x 4096", data[1000:], [4096] * 256, history=data[:1000])
    run_set(amd, rc, [ch], 9, "single chain")
    try:
        amd.set_option("hc_chain_segment", 65536)
        run_set(amd, rc, [ch], 9, "single chain, 17 segments")
    finally:
        amd.set_option("hc_chain_segment", 1 << 20)
    # what the form is for, by the reference: the linked blocks are well under the same blocks compressed alone
    linked = sum(rc.compress(ch, 9)[0])
    alone = sum(rc.compress(chain_of("alone", s, [4096]), 9)[0][0] for s, _ in ch.blocks)
    assert linked < 0.8 * alone, (linked, alone)


def test_hcchain_same_call_twice_and_prefix_null(amd, rc, chains):
    """one short chain, the same call 40 times in one process -- with the prefix array and without it: with the layout's scratch
    allocated per launch, every call behind a process's first gave every block the chain's first bytes one time in three"""
    ch = next(c for c in chains if c.name == "book1 16 x 5 cap - 1 at 8")
    for k in range(40):   # (it showed in a third of the calls behind the first)
        run_set(amd, rc, [ch], 9, "call %d" % k, with_prefix=k % 2 == 0)
    sel = [c for c in chains if not c.history and is_small(c)][:150]
    run_set(amd, rc, sel, 9, "zeros", with_prefix=True)
    run_set(amd, rc, sel, 9, "NULL", with_prefix=False)


def test_hcchain_in_small_chunks(amd, rc, chains, monkeypatch):
    """1 MiB chunks (LZ4HIP_HOST_CHUNK_MB=1, read per call): the set is staged in several chunks through one buffer set, each with a
    workspace for its own packed source; the zero chain and the 3 x 65536 chain are a good part of a chunk each"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    pk = HCPacked(chains)
    assert pk.span > 3 << 20
    dst, out = host_abi_call(amd, pk, 9)
    bad = pk.check(dst, out, expected(rc, chains, 9))
    assert not bad, (len(bad), bad[:5])


def test_hcchain_python_class(amd, rc, chains):
    """LZ4HIPBatch.compressHCChain on a handful of chains (lists and numpy arrays), and the empty call"""
    sel = [c for c in chains if min(c.lens + [0]) >= 0 and min([cap for _, cap in c.blocks] + [0]) >= 0 and is_small(c)][::9][:40]
    assert any(c.history for c in sel) and any(0 in rc.compress(c, 9)[0] for c in sel)
    pk = HCPacked(sel)
    want = expected(rc, sel, 9)
    dst = bytearray(pk.dst)
    out = amd.LZ4HIPBatch.compressHCChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, dst, pk.dst_off, pk.dst_cap, pk.prefix, 9)
    assert isinstance(out, list) and not pk.check(dst, out, want)
    dst = bytearray(pk.dst)
    out = amd.LZ4HIPBatch.compressHCChain(pk.src, np.array(pk.chain_src_off, dtype=np.uint64), np.array(pk.src_len, dtype=np.int32),
                                          np.array(pk.chain_first, dtype=np.uint32), dst, np.array(pk.dst_off, dtype=np.uint64),
                                          np.array(pk.dst_cap, dtype=np.int32), np.array(pk.prefix, dtype=np.int32), level=0)   # (level 0 means 9)
    assert out.dtype == np.int32 and not pk.check(dst, out.tolist(), want)
    assert amd.LZ4HIPBatch.compressHCChain(b"", [], [], [0], bytearray(1), [], []) == []


def program_cases(rc, chains):
    """four chains for the C++ and JNI programs, which start a process per chain (their layers refuse negative lengths and capacities,
    as the Python layer does): mixed block sizes with empty and short blocks, a history, a block that fails in the middle, a pattern"""
    ok = [c for c in chains if min(c.lens + [0]) >= 0 and min([cap for _, cap in c.blocks] + [0]) >= 0 and c.blocks and len(c.data) + len(c.history) <= 20000]
    first = lambda cond: next(c for c in ok if cond(c))
    picks = [first(lambda c: c.name == "book1 mixed"), first(lambda c: c.history and len(c.blocks) >= 3),
             first(lambda c: 0 in rc.compress(c, 9)[0][:-1]), first(lambda c: c.name.startswith("pattern") and len(c.blocks) >= 3)]
    assert len({id(c) for c in picks}) == 4
    return picks


def test_hcchain_cpp_mirror(rc, chains, tmp_path):
    """tests/cpp/hcchain_mirror_test.cpp: LZ4HIPBatch::compressHCChain of host/lz4hip.hpp, two chains per call"""
    exe = build_mirror("hcchain_mirror_test", tmp_path)
    for k, ch in enumerate(program_cases(rc, chains)):
        level = (9, 4, 10, 9)[k]
        outs, by = rc.compress(ch, level)
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin"), str(level)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert p.stdout.decode().split() == [str(o) for o in outs], ch.name
        assert (tmp_path / "o.bin").read_bytes() == b"".join(by), ch.name


def test_hcchain_jni_program(rc, chains, tmp_path):
    """tests/jni_stub/fake_jni_hcchain.c: the JNI shim's LZ4HIP_batchHCChain over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_hcchain", tmp_path)
    for k, ch in enumerate(program_cases(rc, chains)):
        level = (9, 1, 12, 9)[k]
        outs, by = rc.compress(ch, level)
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path), str(level)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and b"checks ok" in p.stdout, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert (tmp_path / "hcchain.txt").read_text().split() == [str(o) for o in outs], ch.name
        assert (tmp_path / "hcchain.out").read_bytes() == b"".join(by), ch.name


def test_hcchain_frame_writer_with_the_engine(amd, rc, port, tmp_path):
    """LZ4FrameOutputStream(linkedBlocks=True, level=9) with HIPEngine, in Python and through host/lz4hip_streams.hpp: batchBlocks 1, 3
    and 64 write the same frame, the frame assembled from the reference, and this project's readers read it back"""
    import importlib
    import io
    import random
    S = importlib.import_module("lz4-java_amd.streams")
    b = book1()
    data = b[:200000] + random.Random(9).randbytes(100000) + b[250000:340000]
    B = S.FLG.Bits
    want = hc_linked_frame(rc, port.xxh32, data, 4, 9, block_checksum=True, content_checksum=True)
    for batch in (1, 3, 64):
        sink = io.BytesIO()
        w = S.LZ4FrameOutputStream(sink, 4, -1, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, batchBlocks=batch, linkedBlocks=True, level=9)
        for a in range(0, len(data), 100000):
            w.write(data[a:a + 100000])
        w.close()
        assert sink.getvalue() == want, batch
    assert S.LZ4FrameInputStream(io.BytesIO(want), linkedBlocks=True).read() == data
    exe = build_mirror("hcchain_mirror_test", tmp_path)
    (tmp_path / "d.bin").write_bytes(data)
    for batch in (1, 3, 64):
        p = subprocess.run([exe, "--frame", str(tmp_path / "d.bin"), str(tmp_path / "f.lz4"), "4", str(batch), "9"], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (batch, p.stderr.decode()[-2000:])
        assert (tmp_path / "f.lz4").read_bytes() == want, batch


def test_hcchain_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 2): the host call takes the multi-device branch (whole chains per listed device)"""
    assert "hcchain multidev ok D=2" in run_child("hcchain_multidev_child.py", "2", "repeat", timeout=600)


def test_hcchain_multidev_host_path_two_gpus():
    """two different devices: chains are split at chain boundaries only, each device compressing whole chains"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "hcchain multidev ok D=2" in run_child("hcchain_multidev_child.py", "2", "distinct", timeout=600)
