"""The linked-block compressor (LZ4_compress_fast_continue over chains, liblz4's prefix mode) on the GPU against the reference library's
own stream compressor: the whole case set of tests/cchain_common.py through the device call in one launch, again in launches of 1 and
of 33 chains, 6000 short chains (more chains than wavefront slots: every wavefront draws several, and every distinct chain appears at
several places in the order), the optional array, untrusted arrays, the host call with prefixes, the Python layer, eight threads and
the multi-device host path.  Guard bytes (0xA5) lie around every slot and around every chain's source, and every device test feeds what
was produced to lz4hip_decompress_safe_chain_batch_dev and compares with the source."""
import ctypes as C
import random
import subprocess
import threading

import numpy as np
import pytest

from cchain_common import (CHAIN_STOPPED, CChain, CPacked, GUARD, RefCChain, batched_linked_frame, book1, bound, case_set, cchain_file, chain_of, expected,
                           stops_early)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


@pytest.fixture(scope="module")
def cases(rc):
    """the chains and the reference's (out_len, chain_consumed, bytes per block) for each, computed once"""
    chains = case_set(rc, random.Random(41))
    return chains, expected(rc, chains)


def device_call(amd, pk, with_prefix=True):
    """-> (dst bytes, out, consumed, src bytes as the device holds them afterwards, the device tensors for a second call)"""
    import torch
    dev = torch.device("cuda", 0)
    d_src = torch.frombuffer(bytearray(pk.src), dtype=torch.uint8).to(dev)
    d_dst = torch.frombuffer(bytearray(pk.dst), dtype=torch.uint8).to(dev)
    i64 = lambda v: torch.tensor(np.asarray(v, dtype=np.int64), device=dev)
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32), device=dev)
    out = torch.full((max(pk.n_blocks, 1),), -12345, dtype=torch.int32, device=dev)
    cons = torch.full((max(pk.n_chains, 1),), -1, dtype=torch.int64, device=dev)
    amd.DeviceBatch.compress_fast_chain(d_src, i64(pk.chain_src_off), i32(pk.src_len), i32(pk.chain_first), d_dst, i64(pk.dst_off), i32(pk.dst_cap),
                                        out, cons, i32(pk.prefix) if with_prefix else None)
    torch.cuda.synchronize()
    assert d_src.cpu().numpy().tobytes() == pk.src, "the source was written"
    return d_dst.cpu().numpy().tobytes(), out.cpu().tolist()[:pk.n_blocks], cons.cpu().tolist()[:pk.n_chains], d_dst


def decode_back(amd, pk, d_dst, out, cons, prefix=None):
    """what the call produced through lz4hip_decompress_safe_chain_batch_dev: per chain the blocks that succeeded, decoded behind the
    chain's history into a region of exactly the consumed bytes, compared with the source"""
    import torch
    dev = torch.device("cuda", 0)
    prefix = pk.prefix if prefix is None else prefix
    src_off, src_len, dst_cap, first, cdo, ccap, pre = [], [], [], [0], [], [], []
    buf = bytearray(b"\xA5" * GUARD)
    for c in range(pk.n_chains):
        b0, b1 = pk.chain_first[c], pk.chain_first[c + 1]
        for i in range(b0, b1):
            if out[i] <= 0:
                break
            src_off.append(pk.dst_off[i]); src_len.append(out[i]); dst_cap.append(pk.src_len[i])
        first.append(len(src_off))
        P, o = prefix[c], pk.chain_src_off[c]
        buf += pk.src[o - P:o]
        cdo.append(len(buf)); ccap.append(cons[c]); pre.append(P)
        buf += b"\x33" * cons[c] + b"\xA5" * GUARD
    nb, nc = len(src_off), pk.n_chains
    d_out = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    i64 = lambda v: torch.tensor(np.asarray(v, dtype=np.int64), device=dev)
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32), device=dev)
    r = torch.full((max(nb, 1),), -12345, dtype=torch.int32, device=dev)
    cout = torch.full((max(nc, 1),), -1, dtype=torch.int64, device=dev)
    if nb == 0:
        return
    amd.DeviceBatch.decompress_safe_chain(d_dst, i64(src_off or [0]), i32(src_len or [0]), i32(dst_cap or [0]), i32(first), d_out, i64(cdo), i64(ccap), r, cout,
                                          i32(pre))
    torch.cuda.synchronize()
    back = d_out.cpu().numpy().tobytes()
    assert r.cpu().tolist()[:nb] == dst_cap and cout.cpu().tolist()[:nc] == list(cons), "the decoder's values"
    for c in range(nc):
        o = pk.chain_src_off[c]
        assert back[cdo[c]:cdo[c] + cons[c]] == pk.src[o:o + cons[c]], ("round trip", pk.chains[c].name)


def run_device(amd, chains, want, what, with_prefix=True):
    pk = CPacked(chains)
    dst, out, cons, d_dst = device_call(amd, pk, with_prefix)
    bad = pk.check(dst, out, cons, want)
    assert not bad, (what, len(bad), bad[:5])
    decode_back(amd, pk, d_dst, out, cons)


def test_cchain_device_whole_set(amd, cases):
    """every chain of the set in ONE launch: chains of 1 to 70 blocks side by side on the wavefronts"""
    chains, want = cases
    assert len(chains) >= 300 and stops_early(want) >= 40
    run_device(amd, chains, want, "whole set")


@pytest.mark.parametrize("n_chains", (1, 33))
def test_cchain_device_spread(amd, cases, n_chains):
    """the set again in launches of n_chains chains"""
    chains, want = cases
    for a in range(0, len(chains), n_chains):
        run_device(amd, chains[a:a + n_chains], want[a:a + n_chains], "launches of %d, from %d" % (n_chains, a))


def test_cchain_device_more_chains_than_wavefronts(amd, rc):
    """6000 chains of 2 to 6 blocks of 13 to 300 bytes, of uneven length: more than five wavefronts per CU can hold at once, so every
    wavefront draws several.  150 distinct chains, each at 40 places in the order: a table carried over from the chain before, or
    cleared between two blocks, changes bytes -- equal inputs must give the reference's bytes wherever they are drawn"""
    b = book1()
    rng = random.Random(46)
    distinct = []
    for k in range(150):
        sizes = [rng.randrange(13, 301) for _ in range(rng.randrange(2, 7))]
        o = rng.randrange(1000, 700000)
        P = rng.choice((0, 0, 9, 200))
        distinct.append(chain_of("short %d" % k, b[o:o + sum(sizes)], sizes, history=b[o - P:o]))
    want = expected(rc, distinct)
    idx = [(i * 37 + (i // 150) * 11) % 150 for i in range(6000)]
    assert min(idx.count(k) for k in range(150)) >= 2
    run_device(amd, [distinct[i] for i in idx], [want[i] for i in idx], "6000 chains")


def test_cchain_device_prefix_null_is_zeros(amd, cases):
    """chain_prefix_len == NULL against an array of zeros: the chains without history, both ways"""
    chains, want = cases
    sel = [(c, w) for c, w in zip(chains, want) if not c.history][:200]
    run_device(amd, [c for c, _ in sel], [w for _, w in sel], "zeros", with_prefix=True)
    run_device(amd, [c for c, _ in sel], [w for _, w in sel], "NULL", with_prefix=False)


def test_cchain_device_untrusted_arrays(amd, rc):
    """the kernel's handling of bad arrays: a range past n_blocks is cut, a negative prefix counts as 0, a prefix longer than the
    chain's offset is cut to it; results follow the contract and the guards are intact"""
    b = book1()
    ch = chain_of("bad", b[1000:1000 + 5 * 300], [300] * 5, history=b[900:1000])
    plain = CChain("plain", ch.blocks)
    pk = CPacked([ch])
    pk.prefix = [-5]
    dst, out, cons, d_dst = device_call(amd, pk)
    assert not pk.check(dst, out, cons, [rc.compress(plain)])
    decode_back(amd, pk, d_dst, out, cons, prefix=[0])
    pk = CPacked([ch])
    off = pk.chain_src_off[0]
    pk.prefix = [off + 1000]
    dst, out, cons, d_dst = device_call(amd, pk)
    assert not pk.check(dst, out, cons, [rc.compress(CChain("cut", ch.blocks, history=pk.src[:off]))])
    decode_back(amd, pk, d_dst, out, cons, prefix=[off])
    pk = CPacked([ch])
    pk.chain_first = [0, 9]
    dst, out, cons, d_dst = device_call(amd, pk)
    pk.chain_first = [0, 5]
    assert not pk.check(dst, out, cons, [rc.compress(ch)])
    decode_back(amd, pk, d_dst, out, cons)


def test_cchain_device_offsets_past_2_and_4_gib(amd, rc):
    """chains whose sources and slots lie around and past offsets of 2^31 and 2^32 in src and dst (the buffers are allocated, not
    filled): a 64-bit offset that loses or smears its upper half anywhere in the kernel reads or writes somewhere else.  Guards around
    every source and slot; the produced chains go back through the chain decoder at the same offsets"""
    import torch
    dev = torch.device("cuda", 0)
    b = book1()
    span = (1 << 32) + (1 << 21)
    d_src = torch.empty(span, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(span, dtype=torch.uint8, device=dev)
    places = [(1 << 31) - 700, (1 << 31) + 4096 + 3, (1 << 32) - 900, (1 << 32) + 65536 + 1, 1000]
    chains = [chain_of("far %d" % k, b[20000 * k + P:20000 * k + P + 5 * 400], [400] * 5, history=b[20000 * k:20000 * k + P])
              for k, P in enumerate((0, 100, 9, 0, 300))]
    want = expected(rc, chains)
    cso, pre, sl, first, do, dc = [], [], [], [0], [], []
    cap = bound(400)
    for at, ch in zip(places, chains):
        img = b"\xA5" * GUARD + ch.history + ch.data + b"\xA5" * GUARD
        d_src[at:at + len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8).to(dev)
        cso.append(at + GUARD + len(ch.history)); pre.append(len(ch.history))
        d_dst[at:at + 5 * (cap + GUARD) + GUARD] = 0xA5
        for i in range(5):
            sl.append(400); do.append(at + GUARD + i * (cap + GUARD)); dc.append(cap)
            d_dst[do[-1]:do[-1] + cap] = 0x5A
        first.append(len(sl))
    i64 = lambda v: torch.tensor(np.asarray(v, dtype=np.int64), device=dev)
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32), device=dev)
    out = torch.full((len(sl),), -12345, dtype=torch.int32, device=dev)
    cons = torch.full((len(chains),), -1, dtype=torch.int64, device=dev)
    amd.DeviceBatch.compress_fast_chain(d_src, i64(cso), i32(sl), i32(first), d_dst, i64(do), i32(dc), out, cons, i32(pre))
    torch.cuda.synchronize()
    o, cn = out.cpu().tolist(), cons.cpu().tolist()
    for c, (at, ch, (outs, done, by)) in enumerate(zip(places, chains, want)):
        assert o[5 * c:5 * c + 5] == outs and cn[c] == done == 2000, ch.name
        got = d_dst[at:at + 5 * (cap + GUARD) + GUARD].cpu().numpy().tobytes()
        exp = b"\xA5" * GUARD + b"".join(x + b"\x5A" * (cap - len(x)) + b"\xA5" * GUARD for x in by)
        assert got == exp, ch.name
    # back through the chain decoder: streams at the far offsets of d_dst, regions at the far offsets of a second buffer
    d_back = torch.empty(span, dtype=torch.uint8, device=dev)
    cdo = []
    for at, ch in zip(places, chains):
        P = len(ch.history)
        if P:
            d_back[at:at + P] = torch.frombuffer(bytearray(ch.history), dtype=torch.uint8).to(dev)
        cdo.append(at + P)
    r = torch.full((len(sl),), -12345, dtype=torch.int32, device=dev)
    cout = torch.full((len(chains),), -1, dtype=torch.int64, device=dev)
    amd.DeviceBatch.decompress_safe_chain(d_dst, i64(do), out, i32(sl), i32(first), d_back, i64(cdo), i64([2000] * len(chains)), r, cout, i32(pre))
    torch.cuda.synchronize()
    assert r.cpu().tolist() == sl and cout.cpu().tolist() == [2000] * len(chains)
    for at, ch in zip(cdo, chains):
        assert d_back[at:at + 2000].cpu().numpy().tobytes() == ch.data, ch.name


def host_call(amd, pk, as_numpy=False):
    dst = bytearray(pk.dst)
    if as_numpy:
        out, cons = amd.LZ4HIPBatch.compressFastChain(pk.src, np.array(pk.chain_src_off, dtype=np.uint64), np.array(pk.src_len, dtype=np.int32),
                                                      np.array(pk.chain_first, dtype=np.uint32), dst, np.array(pk.dst_off, dtype=np.uint64),
                                                      np.array(pk.dst_cap, dtype=np.int32), np.array(pk.prefix, dtype=np.int32))
        assert out.dtype == np.int32 and cons.dtype == np.uint64
        return dst, out.tolist(), cons.tolist()
    out, cons = amd.LZ4HIPBatch.compressFastChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, dst, pk.dst_off, pk.dst_cap, pk.prefix)
    return dst, out, cons


def host_set(cases):
    """what the host call and the Python layer accept: every chain without a negative length or capacity"""
    chains, want = cases
    sel = [i for i, c in enumerate(chains) if min(c.lens + [0]) >= 0 and min([cap for _, cap in c.blocks] + [0]) >= 0]
    return [chains[i] for i in sel], [want[i] for i in sel]


def test_cchain_host_call_and_python_layer(amd, cases):
    """the host call through LZ4HIPBatch.compressFastChain, chains with prefixes included: only the last 64 KB of a prefix are uploaded
    (a 70000-byte prefix still gives the reference's bytes), and only the bytes produced come back -- every other byte of the caller's
    buffer is as it was"""
    chains, want = host_set(cases)
    assert any(len(c.history) == 70000 for c in chains) and any(0 in w[0] for w in want)
    pk = CPacked(chains)
    dst, out, cons = host_call(amd, pk)
    bad = pk.check(dst, out, cons, want)
    assert not bad, (len(bad), bad[:5])
    for i in range(pk.n_blocks):   # behind what was produced -- and in the slot of a block that failed -- the caller's bytes
        o, cap, r = pk.dst_off[i], max(pk.dst_cap[i], 0), max(out[i], 0)
        assert dst[o + r:o + cap] == bytes([pk.fill]) * (cap - r), i
    pk = CPacked(chains[:60])
    dst, out, cons = host_call(amd, pk, as_numpy=True)
    assert not pk.check(dst, out, cons, want[:60])
    assert amd.LZ4HIPBatch.compressFastChain(b"", [], [], [0], bytearray(1), [], []) == ([], [])


def test_cchain_host_call_in_small_chunks(amd, cases, rc, monkeypatch):
    """the host call with 1 MiB chunks (LZ4HIP_HOST_CHUNK_MB=1, read per call): the host set, cycled until its 16-byte-rounded sources
    (each with the kept part of its prefix) pass 2 MiB, is staged in three chunks or more through one buffer set -- the 70000-byte
    prefixes, of which 64 KB are kept, cross chunk boundaries -- and a chain of 17 x 65536 bytes in the middle is larger than a chunk
    by itself (a chunk takes one chain at least).  The assertions of test_cchain_host_call_and_python_layer"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    chains, want = host_set(cases)
    assert any(len(c.history) == 70000 for c in chains)
    rounded = lambda ch: (min(len(ch.history), 65536) + len(ch.data) + 15) & ~15
    big = chain_of("book1 17 x 65536", (book1() * 2)[:17 * 65536], [65536] * 17)
    assert rounded(big) > 1 << 20
    sel, total = [], 0
    while total <= 2 << 20 or len(sel) < len(chains):
        sel.append(len(sel) % len(chains))
        total += rounded(chains[sel[-1]])
    assert total > 2 << 20
    use, w = [chains[i] for i in sel], [want[i] for i in sel]
    at = len(use) // 3
    use.insert(at, big)
    w.insert(at, rc.compress(big))
    assert w[at][1] == 17 * 65536
    pk = CPacked(use)
    dst, out, cons = host_call(amd, pk)
    bad = pk.check(dst, out, cons, w)
    assert not bad, (len(bad), bad[:5])
    for i in range(pk.n_blocks):   # behind what was produced -- and in the slot of a block that failed -- the caller's bytes
        o, cap, r = pk.dst_off[i], max(pk.dst_cap[i], 0), max(out[i], 0)
        assert dst[o + r:o + cap] == bytes([pk.fill]) * (cap - r), i


def test_cchain_host_call_negative_values(amd, cases):
    """negative src_len / dst_cap reach the host form of the C ABI as they are (the Python layer refuses them): result 0, chain stopped"""
    import ctypes as C
    chains, want = cases
    sel = [(c, w) for c, w in zip(chains, want) if min(c.lens + [0]) < 0 or min([cap for _, cap in c.blocks] + [0]) < 0]
    assert len(sel) >= 20
    pk = CPacked([c for c, _ in sel])
    dst = bytearray(pk.dst)
    arr = lambda t, v: (t * max(len(v), 1))(*v)
    out, cons = (C.c_int32 * pk.n_blocks)(), (C.c_uint64 * pk.n_chains)()
    dbuf = (C.c_uint8 * len(dst)).from_buffer(dst)
    r = amd.lib().lz4hip_compress_fast_chain_batch(pk.src, arr(C.c_uint64, pk.chain_src_off), arr(C.c_int32, pk.prefix), arr(C.c_int32, pk.src_len),
                                                   arr(C.c_uint32, pk.chain_first), C.addressof(dbuf), arr(C.c_uint64, pk.dst_off), arr(C.c_int32, pk.dst_cap),
                                                   out, cons, pk.n_blocks, pk.n_chains)
    assert r == 0, amd.lib().lz4hip_last_error()
    del dbuf
    assert not pk.check(dst, list(out), list(cons), [w for _, w in sel])


def test_cchain_eight_threads(amd, cases):
    """eight threads calling the host batch concurrently, each with its own slice of the set"""
    chains, want = host_set(cases)
    small = [(c, w) for c, w in zip(chains, want) if len(c.data) + len(c.history) <= 30000]
    errs = []

    def work(t):
        try:
            part = small[t::8]
            pk = CPacked([c for c, _ in part])
            for _ in range(2):
                dst, out, cons = host_call(amd, pk)
                bad = pk.check(dst, out, cons, [w for _, w in part])
                assert not bad, (t, bad[:3])
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs[:3]


def program_cases(cases):
    """a few chains of every kind for the C++ and JNI programs: book1 chains, with a prefix, hand-built, stopped early by tight capacities,
    empty and short blocks (the programs' layers refuse negative lengths and capacities, as the Python layer does)"""
    chains, want = host_set(cases)
    picks, seen = [], set()
    for i, c in enumerate(chains):
        kind = c.name.split(" ")[0] + ("/h" if c.history else "") + ("/stopped" if 0 in want[i][0] else "")
        if kind not in seen and len(c.data) + len(c.history) < 200000 and c.blocks:
            seen.add(kind)
            picks.append(i)
    picks += [i for i, c in enumerate(chains) if c.name in ("book1 mixed", "book1 17 x 4096")]
    assert len(picks) >= 8 and any(0 in want[i][0] for i in picks) and any(chains[i].history for i in picks)
    return [(chains[i], want[i]) for i in picks]


def test_cchain_cpp_mirror(cases, tmp_path):
    """tests/cpp/cchain_mirror_test.cpp: LZ4HIPBatch::compressFastChain of host/lz4hip.hpp, two chains per call"""
    exe = build_mirror("cchain_mirror_test", tmp_path)
    for ch, (outs, done, by) in program_cases(cases):
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert p.stdout.decode().split() == [str(o) for o in outs] + ["|", str(done)], ch.name
        assert (tmp_path / "o.bin").read_bytes() == b"".join(by), ch.name


def test_cchain_jni_program(cases, tmp_path):
    """tests/jni_stub/fake_jni_cchain.c: the JNI shim's LZ4HIP_batchFastChain over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_cchain", tmp_path)
    for ch, (outs, done, by) in program_cases(cases):
        (tmp_path / "c.bin").write_bytes(cchain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and b"checks ok" in p.stdout, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert (tmp_path / "cchain.txt").read_text().split() == [str(o) for o in outs] + ["|", str(done)], ch.name
        assert (tmp_path / "cchain.out").read_bytes() == b"".join(by), ch.name


def test_cchain_frame_writer_with_the_engine(amd, rc, ref, port, tmp_path):
    """LZ4FrameOutputStream(linkedBlocks=True) with HIPEngine, in Python and through host/lz4hip_streams.hpp: the frames equal the frames
    assembled from the reference (the CPU test's expected frames), the reference library decodes them block by block
    (LZ4_decompress_safe_continue), and this project's reader reads them back"""
    import importlib
    import io
    import struct
    from chain_common import RefChain, linked_frame
    S = importlib.import_module("lz4-java_amd.streams")
    b = book1()
    data = b[:300000] + random.Random(9).randbytes(150000) + b[250000:420000]
    B = S.FLG.Bits
    exe = build_mirror("cchain_mirror_test", tmp_path)
    (tmp_path / "d.bin").write_bytes(data)

    def ref_decode(frame, block_id):
        """the frame's blocks through the reference's stream decoder, stored blocks copied"""
        bs, p, streams = 1 << (2 * block_id + 8), 7, []
        out = bytearray()
        Lr = rc.L
        buf = C.create_string_buffer(len(data) + 64)
        base = C.addressof(buf)
        sd = Lr.LZ4_createStreamDecode()
        Lr.LZ4_setStreamDecode(sd, base, 0)
        pos = 0
        while True:
            w = struct.unpack_from("<I", frame, p)[0]; p += 4
            if w == 0:
                break
            n = w & 0x7FFFFFFF
            payload = frame[p:p + n]; p += n + 4            # (+ the block checksum)
            if w & 0x80000000:
                C.memmove(base + pos, payload, n)
                Lr.LZ4_setStreamDecode(sd, base, pos + n)
                r = n
            else:
                sb = C.create_string_buffer(payload + b"\0" * 8, n + 8)
                r = Lr.LZ4_decompress_safe_continue(sd, sb, base + pos, n, bs)
                assert r > 0
            pos += r
        Lr.LZ4_freeStreamDecode(sd)
        return bytes(buf.raw[:pos])

    for block_id, batch in ((4, 64), (4, 3), (5, 2)):
        want = batched_linked_frame(rc, port.xxh32, data, block_id, batch, block_checksum=True, content_checksum=True)
        if batch == 64:
            assert want == linked_frame(RefChain(ref), port.xxh32, data, block_id, block_checksum=True, content_checksum=True)[0]
        sink = io.BytesIO()
        w = S.LZ4FrameOutputStream(sink, block_id, -1, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, batchBlocks=batch, linkedBlocks=True)
        piece = batch << (2 * block_id + 8)
        for a in range(0, len(data), piece):
            w.write(data[a:a + piece])
        w.close()
        got = sink.getvalue()
        assert got == want, (block_id, batch)
        assert ref_decode(got, block_id) == data
        assert S.LZ4FrameInputStream(io.BytesIO(got), linkedBlocks=True).read() == data
        p = subprocess.run([exe, "--frame", str(tmp_path / "d.bin"), str(tmp_path / "f.lz4"), str(block_id), str(batch)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (block_id, batch, p.stderr.decode()[-2000:])
        assert (tmp_path / "f.lz4").read_bytes() == want, (block_id, batch)


def test_cchain_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 2): the host call takes the multi-device branch (whole chains per listed device)"""
    assert "cchain multidev ok D=2" in run_child("cchain_multidev_child.py", "2", "repeat", timeout=600)


def test_cchain_multidev_host_path_two_gpus():
    """two different devices: chains are split at chain boundaries only, each device compressing whole chains"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "cchain multidev ok D=2" in run_child("cchain_multidev_child.py", "2", "distinct", timeout=600)
