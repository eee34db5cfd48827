"""Parity of the HIP engine against the oracle, through the C ABI (-m gpu).

Structure follows the reference's LZ4Test.java: golden/known-answer vectors, the compressor x
decompressor cross-product (here: HIP x reference-liblz4), dest-too-small and malformed-input
behaviour, fixtures (Calgary slices, all-equal, max-distance, random), plus batch / device entry
points the reference does not have.  Bit-exact everywhere: compressed bytes, decoded bytes, return
codes."""
import random

import pytest

from conftest import rnd_inputs, sha
from fast_contract_common import DECODE_VARIANTS
from support import build_mirror

pytestmark = pytest.mark.gpu


def pack(blocks, caps):
    src = b"".join(blocks)
    so, sl, do, p, q = [], [], [], 0, 0
    for b, c in zip(blocks, caps):
        so.append(p); sl.append(len(b)); do.append(q)
        p += len(b); q += c
    return src, so, sl, bytearray(max(q, 1)), do


def gpu_compress_many(amd, blocks, caps):
    src, so, sl, dst, do = pack(blocks, caps)
    out = amd.LZ4HIPBatch.compress(src, so, sl, dst, do, list(caps))
    return [(r, bytes(dst[o:o + max(r, 0)])) for r, o in zip(out, do)]


GUARD = 41   # bytes of 0xA5 in front of, between and behind the destination slots of gpu_decode_safe_many


def gpu_decode_safe_many(amd, streams, caps):
    """safe-decodes a batch whose destination slots are separated by GUARD bytes of 0xA5 and asserts that NOTHING outside the slots
    was written -- valid or malformed stream, whatever the interior loop (the deep and staged loops store whole steps / whole lines
    unconditionally: a malformed stream must not carry one across its slot's end)"""
    src = b"".join(streams)
    so, sl, do, p, q = [], [], [], 0, GUARD
    for b, c in zip(streams, caps):
        so.append(p); sl.append(len(b)); do.append(q)
        p += len(b); q += c + GUARD
    dst = bytearray(b"\xA5" * q)
    out = amd.LZ4HIPBatch.decompressSafe(src, so, sl, dst, do, list(caps))
    guard = b"\xA5" * GUARD
    assert bytes(dst[:GUARD]) == guard, "bytes in front of the first slot were written"
    for k, (o, c) in enumerate(zip(do, caps)):
        assert bytes(dst[o + c:o + c + GUARD]) == guard, ("bytes behind slot %d (capacity %d, stream of %d bytes, result %d) were written"
                                                          % (k, c, sl[k], out[k]))
    return [(r, bytes(dst[o:o + c])) for r, o, c in zip(out, do, caps)]


def test_factory_selftest_and_known_answers(amd):
    f = amd.LZ4Factory.hipInstance()                       # runs LZ4Factory.java:204-220's round trip
    c = f.fastCompressor().compress(b"abcd      abcdefghij")
    assert c.hex() == "5161626364200100a06162636465666768696a"
    assert f.fastCompressor().compress(b"12345345234572").hex() == "e03132333435333435323334353732"
    assert f.safeDecompressor().decompress(c, 20) == b"abcd      abcdefghij"
    assert f.fastDecompressor().decompress(c, 20) == b"abcd      abcdefghij"
    assert f.fastCompressor().compress(b"") == b"\x00"     # LZ4Test.java:111-114 testEmpty
    assert f.safeDecompressor().decompress(b"\x00", 0) == b""
    assert f.fastDecompressor().decompress(b"\x00", 0) == b""


def test_golden_table_gpu(amd, golden, corpus, ref):
    names = list(corpus)
    blocks = [corpus[n] for n in names]
    res = gpu_compress_many(amd, blocks, [ref.compress_bound(len(b)) for b in blocks])
    for n, b, (r, c) in zip(names, blocks, res):
        g = golden["inputs"][n]
        assert (r, sha(c)) == (g["fast_size"], g["fast_sha256"]), n
    # 4x4 cross product (LZ4Test.java:312-324): HIP->reference, reference->HIP, HIP->HIP
    streams = [c for _, c in res]
    for b, c in zip(blocks, streams):
        assert ref.decompress_safe(c, len(b)) == b
    dec = gpu_decode_safe_many(amd, [ref.compress_fast(b) for b in blocks], [len(b) for b in blocks])
    for b, (r, d) in zip(blocks, dec):
        assert r == len(b) and d == b
    src, so, sl, dst, do = pack(streams, [len(b) for b in blocks])
    out = amd.LZ4HIPBatch.decompressFast(src, so, sl, dst, do, [len(b) for b in blocks])
    for b, c, r, o in zip(blocks, streams, out, do):
        assert r == len(c) and bytes(dst[o:o + len(b)]) == b


def test_compress_fuzz_bit_exact(amd, ref, O, corpus):
    rng = random.Random(101)
    blocks, caps = [], []
    for v in rnd_inputs(O, corpus, 41, 1500):
        full = ref.compress_bound(len(v))
        er, _ = ref.compress_fast_raw(v, full)
        for cap in (full, max(0, er + rng.choice([-1, 0, 1, 2, -5, 5, -20, 20])), rng.randrange(0, full + 1)):
            blocks.append(v); caps.append(cap)
    res = gpu_compress_many(amd, blocks, caps)
    for v, cap, (r, c) in zip(blocks, caps, res):
        er, eb = ref.compress_fast_raw(v, cap)
        assert r == er and (er <= 0 or c == eb), (len(v), cap, r, er)


def test_fixtures_like_lz4test(amd, ref):
    """LZ4Test.java:456-485: testAllEqual, testMaxDistance, testRandomData shapes"""
    rng = random.Random(5)
    blocks = [bytes([rng.randrange(256)]) * n for n in (0, 1, 4, 13, 100, 4096, 65535, 65536, 100000)]
    for ln in (1 << 17, (1 << 17) + 12345):                   # repeat at distance 65535
        buf = bytearray(rng.randbytes(ln))
        for i in range(65535, ln):
            if rng.random() < 0.5:
                buf[i] = buf[i - 65535]
        blocks.append(bytes(buf))
    for n in (100, 5000, 70000, 300000):                       # alphabet 1..15
        k = rng.randrange(1, 16)
        blocks.append(bytes(rng.randrange(k) for _ in range(n)))
    res = gpu_compress_many(amd, blocks, [ref.compress_bound(len(b)) for b in blocks])
    for b, (r, c) in zip(blocks, res):
        assert c == ref.compress_fast(b), len(b)
    dec = gpu_decode_safe_many(amd, [c for _, c in res], [len(b) for b in blocks])
    for b, (r, d) in zip(blocks, dec):
        assert r == len(b) and d == b


def test_decode_fuzz_bit_exact(amd, ref, O, corpus):
    """return codes and bytes of LZ4_decompress_safe on valid / truncated / extended / corrupted / random
    streams and wrong capacities (LZ4Test.java:188-255, :350-419)"""
    rng = random.Random(77)
    streams, caps = [], []
    for v in rnd_inputs(O, corpus, 43, 4000, max_n=30000):
        c = bytearray(ref.compress_fast(v))
        mode, cap = rng.randrange(6), len(v)
        if mode == 1:
            cap = max(0, len(v) + rng.choice([-1, 1, -5, 5, -12, 12, -33, 33, 64, 100]))
        elif mode == 2 and c:
            for _ in range(rng.randrange(1, 4)):
                c[rng.randrange(len(c))] = rng.randrange(256)
        elif mode == 3 and len(c) > 1:
            c = c[:rng.randrange(1, len(c))]
        elif mode == 4:
            c = c + rng.randbytes(rng.randrange(1, 20))
        elif mode == 5:
            c, cap = bytearray(rng.randbytes(rng.randrange(1, 40))), rng.randrange(0, 200)
        streams.append(bytes(c)); caps.append(cap)
    # pipe: the pipelined interior loop; stage: output staging in LDS (plain loop only)
    for lanes, pipe, stage, ring in DECODE_VARIANTS:   # every decoder kernel (fast_contract_common.py says which is which)
        amd.set_option("decode_lanes", lanes)
        amd.set_option("decode_pipe", pipe)
        amd.set_option("decode_stage", stage)
        amd.set_option("decode_ring", ring)
        res = gpu_decode_safe_many(amd, streams, caps)
        for c, cap, (r, d) in zip(streams, caps, res):
            er, ed = ref.decompress_safe_raw(c, cap)
            assert r == er, (lanes, pipe, stage, ring, len(c), cap, r, er, c[:24].hex())
            if er >= 0:
                assert d[:er] == ed[:er]
    amd.set_option("decode_lanes", 0)
    amd.set_option("decode_pipe", -1)
    amd.set_option("decode_stage", -1)
    amd.set_option("decode_ring", 0)
    # fast decoder: bounded-input semantics defined by the oracle port; equal to liblz4 on valid streams
    src, so, sl, dst, do = pack(streams, caps)
    out = amd.LZ4HIPBatch.decompressFast(src, so, sl, dst, do, caps)
    for c, cap, r, o in zip(streams, caps, out, do):
        er, ed = O.decompress_fast_bounded(c, len(c), cap)
        assert r == er, (len(c), cap, r, er)
        if er >= 0:
            assert bytes(dst[o:o + cap]) == ed[:cap]


def test_malformed_vectors_gpu(amd, golden):
    """LZ4Test.java:350-419 -- exact oracle return codes, not just 'throws'"""
    vecs = golden["malformed"]
    res = gpu_decode_safe_many(amd, [bytes.fromhex(v["hex"]) for v in vecs], [v["safe_cap"] for v in vecs])
    for v, (r, d) in zip(vecs, res):
        assert r == v["safe_ret"]
        if r >= 0:
            assert d[:r].hex() == v["safe_out_hex"]
    dec = amd.LZ4SafeDecompressor()
    with pytest.raises(amd.LZ4Exception):
        dec.decompress(bytes([96, 42, 43, 44, 45, 46, 47, 5, 0]), 0, 9, bytearray(20), 0, 20)
    assert dec.decompress(bytes([16, 42, 0, 0, 128] + [42] * 8), 0, 13, bytearray(20), 0, 20) == 13  # must not throw or hang


def test_dest_too_small(amd, ref, corpus):
    """LZ4Test.java:188-226"""
    data = corpus["book1[:65536]"]
    f = amd.LZ4Factory.hipInstance()
    c = f.fastCompressor().compress(data)
    with pytest.raises(amd.LZ4Exception):
        f.fastCompressor().compress(data, 0, len(data), bytearray(len(c) - 1), 0, len(c) - 1)
    for bad in (len(data) - 1, len(data) + 1):
        with pytest.raises(amd.LZ4Exception):
            f.fastDecompressor().decompress(c, 0, bytearray(bad), 0, bad)
    with pytest.raises(amd.LZ4Exception):
        f.safeDecompressor().decompress(c, 0, len(c), bytearray(len(data) - 1), 0, len(data) - 1)
    out = bytearray(len(data) + 100)
    assert f.safeDecompressor().decompress(c, 0, len(c), out, 0, len(out)) == len(data)
    try:
        f.safeDecompressor().decompress(c + b"\0", 0, len(c) + 1, bytearray(len(data)), 0, len(data))
        assert False
    except amd.LZ4Exception as e:
        assert str(e) == "Error decoding offset %d of input buffer" % (-ref.decompress_safe_raw(c + b"\0", len(data))[0])


def test_offsets_inside_bigger_buffers(amd, ref, corpus):
    """srcOff/destOff handling (AbstractLZ4Test.java:66-116 slices)"""
    data = corpus["book1[:65536]"][:5000]
    f = amd.LZ4Factory.hipInstance()
    src = b"x" * 17 + data + b"y" * 9
    dest = bytearray(b"\x11" * (33 + amd.maxCompressedLength(len(data)) + 5))
    n = f.fastCompressor().compress(src, 17, len(data), dest, 33, len(dest) - 33 - 5)
    assert bytes(dest[33:33 + n]) == ref.compress_fast(data) and dest[:33] == b"\x11" * 33 and dest[33 + n:] == b"\x11" * (len(dest) - 33 - n)
    out = bytearray(b"\x22" * (len(data) + 20))
    assert f.safeDecompressor().decompress(dest, 33, n, out, 7, len(data)) == len(data)
    assert bytes(out[7:7 + len(data)]) == data and out[:7] == b"\x22" * 7 and out[7 + len(data):] == b"\x22" * 13


def test_small_batches_finder_writer_edges(amd, ref, O, corpus):
    """Many small fast-compress launches (1..48 blocks of random sizes and capacities) against the reference library: the finder /
    writer hand-over of the default kernel at its edges -- fewer blocks than wavefronts (most writers get nothing but EXIT), blocks of
    a few bytes, single-batch blocks, ring wrap inside a launch, byU32 blocks next to tiny ones.  (tools/gpu_small_batches.py is the
    long version; the protocol itself also runs with host threads in tests/test_hostsim.py::test_mail_ring_*.)"""
    rng = random.Random(12)
    book = corpus["book1[:200000]"]
    for it in range(120):
        nb = rng.choice([1, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 16, 33, 48])
        blocks = []
        for _ in range(nb):
            n = rng.choice([0, 1, 12, 13, 14, 20, 64, 200, 1000, 5000, 20000, 65536, 65546, 65547, 70000]) if rng.random() < 0.6 else rng.randrange(0, 3000)
            t = rng.randrange(4)
            if t == 0: v = rng.randbytes(n)
            elif t == 1: o = rng.randrange(len(book) - n); v = book[o:o + n]
            elif t == 2: v = O.gen_block(n, rng.randrange(1 << 20), litmax=rng.choice([2, 38, 200]), win=rng.choice([8, 300, 65535]))
            else: v = bytes(rng.randrange(3) for _ in range(min(n, 8000)))
            blocks.append(v)
        caps = [ref.compress_bound(len(v)) if rng.random() < 0.7 else rng.randrange(0, ref.compress_bound(len(v)) + 1) for v in blocks]
        res = gpu_compress_many(amd, blocks, caps)
        for v, cap, (r, c) in zip(blocks, caps, res):
            er, eb = ref.compress_fast_raw(v, cap)
            assert r == er and (er <= 0 or c == eb[:er]), (it, len(v), cap, r, er)


def test_regression_inputs(amd, ref):
    """tests/golden/regress/*.bin: inputs that once made a kernel under development differ from the reference (round 3: a false
    tentative hit AT the first probe position of a window, left to the C++ step with a row that did not cover ip - 2), through
    every compress core, alone and in one batch"""
    import glob, os
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regress", "*.bin")))
    assert files
    blocks = [open(f, "rb").read() for f in files]
    for core in (1, 3, 5):
        amd.set_option("compress_core", core)
        try:
            res = gpu_compress_many(amd, blocks, [ref.compress_bound(len(b)) for b in blocks])
            for b in blocks:
                res += gpu_compress_many(amd, [b], [ref.compress_bound(len(b))])
        finally:
            amd.set_option("compress_core", 5)
        for b, (r, c) in zip(blocks + blocks, res):
            assert c == ref.compress_fast(b), (core, len(b))


def test_issue12_regression_blob_gpu(amd, ref):
    """LZ4Test.testRoundtripIssue12 (LZ4Test.java:487-541), bytes [9:]: every HIP compressor's output equals the reference
    library's and decodes back through both HIP decompressors"""
    import os
    data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "issue12.bin"), "rb").read()[9:]
    f = amd.LZ4Factory.hipInstance()
    for core in (1, 3, 5):
        amd.set_option("compress_core", core)
        c = f.fastCompressor().compress(data)
        assert c == ref.compress_fast(data), core
        assert f.safeDecompressor().decompress(c, len(data)) == data and f.fastDecompressor().decompress(c, len(data)) == data
    amd.set_option("compress_core", 5)
    for level in (1, 9, 12, 17):
        h = f.highCompressor(level).compress(data)
        assert h == ref.compress_hc(data, min(level, 12)) and f.safeDecompressor().decompress(h, len(data)) == data


def test_decode_variants_at_odd_offsets(amd, ref, corpus):
    """every decoder variant (plain / pipelined / staged interior loop x lane counts) with source and destination slots at odd
    byte offsets (the staged loop flushes whole 128-byte lines by ADDRESS): decoded bytes exact, nothing outside the slot touched"""
    rng = random.Random(5)
    blocks = [corpus["book1[:200000]"][a:a + n] for a, n in ((0, 70000), (1234, 3000), (50000, 65536), (7, 1500), (99999, 40000))]
    blocks += [rng.randbytes(700) * 40, bytes(30000), corpus["geo[:65536]"], corpus["pic[:65536]"][:33333]]
    comp = [ref.compress_fast(b) for b in blocks]
    src, so = bytearray(), []
    for c in comp:
        src += b"\x5A" * rng.choice([1, 3, 5, 7, 11])
        so.append(len(src)); src += c
    dst_off, pos = [], 0
    for b in blocks:
        pos += rng.choice([1, 3, 9, 13, 127, 129])
        dst_off.append(pos); pos += len(b)
    total = pos + 77
    for lanes, pipe, stage, ring in ((4, 0, 1, 0), (8, 0, 1, 0), (16, 0, 1, 0), (64, 0, 1, 0), (4, 0, 0, 0), (8, 1, 0, 0), (16, 1, 0, 0), (4, 2, 0, 0), (8, 2, 0, 0), (16, 2, 0, 0),
                                     (1, 3, 0, 0), (4, 3, 0, 0), (4, 3, 0, 2048), (8, 3, 0, 0), (16, 3, 0, 0),   # (3: the ring loop flushes address-aligned steps)
                                     (64, 4, 0, 0), (64, 4, 0, 8192), (64, 4, 0, 16384), (64, 4, 0, 65536),   # (4: the wave loop flushes 256-byte steps, its first and last byte-exactly)
                                     (64, 5, 0, 0), (64, 5, 0, 8192), (64, 5, 0, 16384), (64, 5, 0, 65536),
                                     (64, 7, 0, 0), (64, 7, 0, 16384), (64, 7, 0, 65536),                       # (7: the pair loop, the same flusher in its copier wavefront)
                                     (64, 8, 0, 0), (64, 8, 0, 32768)):                                         # (8: the trio loop, the same copier)
        amd.set_option("decode_lanes", lanes); amd.set_option("decode_pipe", pipe); amd.set_option("decode_stage", stage); amd.set_option("decode_ring", ring)
        dst = bytearray(b"\xC3" * total)
        out = amd.LZ4HIPBatch.decompressSafe(bytes(src), so, [len(c) for c in comp], dst, dst_off, [len(b) for b in blocks])
        assert list(out) == [len(b) for b in blocks], (lanes, pipe, stage)
        expect = bytearray(b"\xC3" * total)
        for o, b in zip(dst_off, blocks):
            expect[o:o + len(b)] = b
        assert dst == expect, (lanes, pipe, stage, ring)
    amd.set_option("decode_lanes", 0); amd.set_option("decode_pipe", -1); amd.set_option("decode_stage", -1); amd.set_option("decode_ring", 0)


def test_deep_decoder_loop_long_streams(amd, ref, O, corpus):
    """the decoder's deep interior loop (csrc/lz4_decode_deep.h; decode_pipe 2) on streams long enough for it to run -- compressed real
    and synthetic blocks, hand-assembled mixes of every kind of sequence, and the same streams corrupted / truncated / with wrong
    capacities: return codes and bytes of the safe decoder against the reference library, groups of 4 / 8 / 16 lanes (the CPU suite
    runs the same cases in the lane simulator: tests/test_hostsim.py::test_deep_decoder_loop)"""
    from conftest import deep_decoder_cases, lz4_seq
    rng = random.Random(4242)
    valid, cases = deep_decoder_cases(ref, O, corpus, rng, lz4_seq)
    streams = [c for c, _ in cases]
    caps = [cap for _, cap in cases]
    want = [ref.decompress_safe_raw(c, cap) for c, cap in cases]
    try:
        for lanes, pipe, ring in ((4, 2, 0), (8, 2, 0), (16, 2, 0), (1, 3, 256), (1, 3, 512), (4, 3, 512), (4, 3, 1024), (4, 3, 2048), (8, 3, 512), (8, 3, 2048), (8, 3, 4096), (16, 3, 2048), (16, 3, 4096),
                                  (64, 4, 0), (64, 4, 8192), (64, 4, 16384), (64, 4, 32768), (64, 4, 65536),
                                  (64, 5, 0), (64, 5, 8192), (64, 5, 16384), (64, 5, 32768), (64, 5, 65536),
                                  (64, 7, 0), (64, 7, 16384), (64, 7, 32768), (64, 7, 65536),
                                  (64, 8, 0), (64, 8, 8192), (64, 8, 16384), (64, 8, 32768), (64, 8, 65536)):
            amd.set_option("decode_lanes", lanes); amd.set_option("decode_pipe", pipe); amd.set_option("decode_stage", 0); amd.set_option("decode_ring", ring)
            res = gpu_decode_safe_many(amd, streams, caps)
            for k, ((r, d), (er, ed)) in enumerate(zip(res, want)):
                assert r == er and (er < 0 or d[:er] == ed[:er]), (lanes, pipe, ring, k, len(streams[k]), caps[k], r, er)
    finally:
        amd.set_option("decode_lanes", 0); amd.set_option("decode_pipe", -1); amd.set_option("decode_stage", -1); amd.set_option("decode_ring", 0)


def test_wave_par_trip_behind_a_one_sequence_step(amd, ref):
    """conftest.wild_piece_stream on the device (the CPU suite runs it in the lane simulator, where the hazard was found): a trip of the
    parallel wave loop right behind a sequence its one-sequence step took, match sources at the edge of what the output ring still
    holds -- the step's wave-wide pieces have overwritten ring bytes the trip's own rule would still trust.  Every ring size."""
    from conftest import wild_piece_stream
    rng = random.Random(606)
    cases = []
    for log in (13, 14, 15, 16):
        for _ in range(4):
            cases.append(wild_piece_stream(1 << log, rng))
    streams = [c for c, _ in cases]
    caps = [n for _, n in cases]
    want = [ref.decompress_safe_raw(c, n) for c, n in cases]
    assert all(r == n for (r, _), n in zip(want, caps))
    try:
        for pipe, ring in ((5, 0), (5, 8192), (5, 16384), (5, 32768), (5, 65536), (4, 8192), (4, 65536), (7, 0), (7, 16384), (7, 32768), (7, 65536), (8, 0), (8, 8192), (8, 16384), (8, 32768), (8, 65536)):
            amd.set_option("decode_lanes", 64); amd.set_option("decode_pipe", pipe); amd.set_option("decode_stage", 0); amd.set_option("decode_ring", ring)
            res = gpu_decode_safe_many(amd, streams, caps)
            for k, ((r, d), (er, ed)) in enumerate(zip(res, want)):
                assert r == er and d[:er] == ed[:er], (pipe, ring, k, r, er, next((i for i in range(min(r, er)) if d[i] != ed[i]), None))
    finally:
        amd.set_option("decode_lanes", 0); amd.set_option("decode_pipe", -1); amd.set_option("decode_stage", -1); amd.set_option("decode_ring", 0)


def test_wave_loops_ring_edge_streams(amd, ref):
    """conftest.ring_edge_stream on the device: 24 hand-assembled blocks whose match distances cluster around every ring size, with
    one-sequence steps, slow copies and early trip ends in between -- both wave loops, every ring (the CPU suite runs the same
    generator in the lane simulator)"""
    from conftest import ring_edge_stream
    rng = random.Random(8118)
    cases = [ring_edge_stream(rng, rng.choice([20000, 90000, 150000])) for _ in range(24)]
    streams = [c for c, _ in cases]
    caps = [n for _, n in cases]
    want = [ref.decompress_safe_raw(c, n) for c, n in cases]
    assert all(r == n for (r, _), n in zip(want, caps))
    try:
        for pipe, ring in ((5, 0), (5, 8192), (5, 16384), (5, 32768), (5, 65536), (4, 0), (4, 8192), (4, 32768), (7, 0), (7, 16384), (7, 32768), (7, 65536), (8, 0), (8, 8192), (8, 16384), (8, 32768), (8, 65536)):
            amd.set_option("decode_lanes", 64); amd.set_option("decode_pipe", pipe); amd.set_option("decode_stage", 0); amd.set_option("decode_ring", ring)
            res = gpu_decode_safe_many(amd, streams, caps)
            for k, ((r, d), (er, ed)) in enumerate(zip(res, want)):
                assert r == er and d[:er] == ed[:er], (pipe, ring, k, r, er, next((i for i in range(min(max(r, 0), er)) if d[i] != ed[i]), None))
    finally:
        amd.set_option("decode_lanes", 0); amd.set_option("decode_pipe", -1); amd.set_option("decode_stage", -1); amd.set_option("decode_ring", 0)


def test_decode_knobs_that_no_kernel_exists_for_are_named(amd, ref):
    """round-5 advisor: the decode knobs are set one at a time, and a combination without a kernel (a ring-loop ring with a wave loop,
    a wave ring with the pair loop) surfaced as a bare 'kernel launch: invalid value'.  Now an argument error that names the knobs."""
    c = ref.compress_fast(bytes(5000))
    try:
        for lanes, pipe, ring, word in ((64, 5, 2048, "decode_pipe 4 / 5"), (64, 7, 8192, "decode_pipe 7"), (16, 3, 512, "decode_pipe 3"), (1, 2, 0, "decode_lanes 1")):
            amd.set_option("decode_lanes", lanes); amd.set_option("decode_pipe", pipe); amd.set_option("decode_ring", ring)
            with pytest.raises(amd.LZ4HIPError) as ei:
                amd.LZ4HIPBatch.decompressSafe(c, [0], [len(c)], bytearray(5000), [0], [5000])
            assert word in str(ei.value) and "status -3" in str(ei.value), str(ei.value)
    finally:
        amd.set_option("decode_lanes", 0); amd.set_option("decode_pipe", -1); amd.set_option("decode_stage", -1); amd.set_option("decode_ring", 0)
    r = amd.LZ4HIPBatch.decompressSafe(c, [0], [len(c)], bytearray(5000), [0], [5000])
    assert list(r) == [5000]


def test_concurrent_callers(amd, ref, corpus):
    """instances are shared singletons and must be thread-safe (LZ4Compressor.java:25): 32 threads hammer the single-block and
    batch entry points (ctypes releases the GIL across the calls) and every result must equal the reference's"""
    import threading
    f = amd.LZ4Factory.hipInstance()
    xf = amd.XXHashFactory.hipInstance()
    book = corpus["book1[:200000]"]
    errors = []

    def worker(t):
        try:
            rng = random.Random(100 + t)
            for it in range(12):
                a, n = rng.randrange(0, 100000), rng.choice([0, 1, 13, 500, 5000, 70000])
                v = book[a:a + n]
                c = f.fastCompressor().compress(v)
                assert c == ref.compress_fast(v)
                assert f.safeDecompressor().decompress(c, len(v)) == v
                assert f.fastDecompressor().decompress(c, len(v)) == v
                assert xf.hash32().hash(v, 0, len(v), t) == ref.xxh32(v, t)
                if it % 4 == 0:
                    blocks = [book[rng.randrange(0, 150000):][:rng.choice([100, 4000, 30000])] for _ in range(5)]
                    caps = [ref.compress_bound(len(b)) for b in blocks]
                    src = b"".join(blocks); so = [sum(map(len, blocks[:i])) for i in range(5)]
                    do = [sum(caps[:i]) for i in range(5)]
                    dst = bytearray(sum(caps))
                    out = amd.LZ4HIPBatch.compress(src, so, [len(b) for b in blocks], dst, do, caps)
                    for b, o, r in zip(blocks, do, out):
                        assert bytes(dst[o:o + r]) == ref.compress_fast(b)
                    h = f.highCompressor(9).compress(blocks[0])
                    assert h == ref.compress_hc(blocks[0], 9)
        except Exception as e:  # noqa: BLE001 -- reported on the main thread
            errors.append((t, repr(e)))

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(32)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors


def test_single_block_calls_of_many_threads_coalesce(amd, ref, O):
    """re-entrant, no global lock in the steady state.  The reference's API shape is one block per call from many
    threads; liblz4hip combines concurrent single-block calls into shared launches (api.cpp `single`), so 32 caller threads must
    get through well over 4x the calls per second of one thread -- and every result is still the reference's."""
    import ctypes as C
    import threading
    import time
    l = amd.lib()
    blocks = [O.gen_block(65536, 7000 + i) for i in range(32)]
    want = [ref.compress_fast(b) for b in blocks]
    cap = ref.compress_bound(65536)

    def run(nthreads, calls):
        errs, done = [], [0] * nthreads

        def worker(t):
            src = blocks[t]
            dst = (C.c_uint8 * cap)()
            for _ in range(calls):
                r = l.lz4hip_compress_fast(src, len(src), dst, cap)
                if r != len(want[t]) or bytes(dst[:r]) != want[t]:
                    errs.append((t, r))
                    return
                done[t] += 1
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        dt = time.perf_counter() - t0
        assert not errs, errs[:3]
        return sum(done) / dt
    run(4, 5)                      # warm-up: staging buffers, streams
    one = run(1, 60)
    many = run(32, 60)
    assert many >= 4.0 * one, (one, many)


def test_device_batch_and_generator(amd, O, ref):
    """device-pointer entry points (what bench.py times) + the on-device workload generator"""
    import torch
    n, blk = 256, 65536
    cap = amd.maxCompressedLength(blk)
    dev = torch.device("cuda:0")
    src = torch.empty(n * blk, dtype=torch.uint8, device=dev)
    amd.DeviceBatch.gen_blocks(src, blk, blk, n, first_idx=5)
    host = src.cpu().numpy().tobytes()
    for i in (0, 1, 100, 255):
        assert host[i * blk:(i + 1) * blk] == O.gen_block(blk, 5 + i)
    i64, i32 = torch.int64, torch.int32
    so = torch.arange(n, dtype=i64, device=dev) * blk
    sl = torch.full((n,), blk, dtype=i32, device=dev)
    comp = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    co = torch.arange(n, dtype=i64, device=dev) * cap
    cc = torch.full((n,), cap, dtype=i32, device=dev)
    clen = torch.zeros(n, dtype=i32, device=dev)
    amd.DeviceBatch.compress_fast(src, so, sl, comp, co, cc, clen)
    back = torch.zeros(n * blk, dtype=torch.uint8, device=dev)
    dlen = torch.zeros(n, dtype=i32, device=dev)
    amd.DeviceBatch.decompress_safe(comp, co, clen, back, so, sl, dlen)
    back2 = torch.zeros(n * blk, dtype=torch.uint8, device=dev)
    used = torch.zeros(n, dtype=i32, device=dev)
    amd.DeviceBatch.decompress_fast(comp, co, cc, back2, so, sl, used)
    torch.cuda.synchronize()
    assert torch.equal(back, src) and torch.equal(back2, src)
    assert torch.equal(dlen, sl) and torch.equal(used, clen)
    ch = comp.cpu().numpy().tobytes()
    cl = clen.cpu().tolist()
    for i in (0, 7, 255):
        assert ch[i * cap:i * cap + cl[i]] == ref.compress_fast(host[i * blk:(i + 1) * blk])


def test_large_blocks_byu32(amd, O, ref):
    """blocks >= 65547 B use the 5-byte-hash / 4096-entry table; 4 MiB = LZ4Frame default.  One batch mixes the
    three table kinds of the fast compressor -- byU16 blocks, byU32 blocks of at most 4 MiB (packed entries on the ten-chain kernel)
    and bigger ones (64-bit entries) -- and runs with "compress_pack" 1 (default) and 0 (everything on the five-chain kernel)."""
    blocks = [O.gen_block(4 << 20, 0, win=4096), O.gen_block(1 << 20, 1, win=65535), O.gen_block(300000, 2, litmax=4, win=8),
              O.gen_block(65536, 3), O.gen_block((4 << 20) + 1, 4, win=4096), O.gen_block(65547, 5), O.gen_block(4000, 6), O.gen_block(5000000, 7, litmax=200)]
    want = [ref.compress_fast(b) for b in blocks]
    for pack in (0, 1):
        amd.set_option("compress_pack", pack)
        try:
            res = gpu_compress_many(amd, blocks, [ref.compress_bound(len(b)) for b in blocks])
        finally:
            amd.set_option("compress_pack", 1)
        for k, (b, (r, c)) in enumerate(zip(blocks, res)):
            assert c == want[k], (pack, k, len(b))
    dec = gpu_decode_safe_many(amd, [c for _, c in res], [len(b) for b in blocks])
    for b, (r, d) in zip(blocks, dec):
        assert r == len(b) and d == b


def test_full_size_roundtrip_properties(amd):
    """BASELINE.json configs[1] shape (64 KiB blocks, ratio ~2) at 16384 blocks = 1 GiB: size-independent
    properties -- decode(encode(x)) == x for BOTH decoders, every size in (0, bound], hash-of-hashes stable"""
    import torch
    n, blk = 16384, 65536
    cap = amd.maxCompressedLength(blk)
    dev = torch.device("cuda:0")
    src = torch.empty(n * blk, dtype=torch.uint8, device=dev)
    amd.DeviceBatch.gen_blocks(src, blk, blk, n)
    so = torch.arange(n, dtype=torch.int64, device=dev) * blk
    sl = torch.full((n,), blk, dtype=torch.int32, device=dev)
    comp = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    co = torch.arange(n, dtype=torch.int64, device=dev) * cap
    cc = torch.full((n,), cap, dtype=torch.int32, device=dev)
    clen = torch.zeros(n, dtype=torch.int32, device=dev)
    amd.DeviceBatch.compress_fast(src, so, sl, comp, co, cc, clen)
    back = torch.zeros(n * blk, dtype=torch.uint8, device=dev)
    dlen = torch.zeros(n, dtype=torch.int32, device=dev)
    amd.DeviceBatch.decompress_safe(comp, co, clen, back, so, sl, dlen)
    torch.cuda.synchronize()
    assert int(clen.min()) > 0 and int(clen.max()) <= cap
    ratio = n * blk / float(clen.sum())
    assert 1.9 < ratio < 2.1, ratio                              # 2.0035
    assert torch.equal(dlen, sl) and torch.equal(back, src)
    h1 = torch.zeros(n, dtype=torch.int32, device=dev)
    h2 = torch.zeros(n, dtype=torch.int32, device=dev)
    amd.DeviceBatch.xxh32(src, so, sl, 0, h1)
    amd.DeviceBatch.xxh32(back, so, sl, 0, h2)
    torch.cuda.synchronize()
    assert torch.equal(h1, h2)


def test_cpp_host_mirror_runs():
    import os, subprocess
    from conftest import ROOT
    exe = build_mirror("host_mirror_test", os.path.join(ROOT, "tests", "cpp"))
    assert subprocess.call([exe]) == 0


@pytest.mark.parametrize("core,switch", [(1, 20), (3, 20), (5, 0), (5, 20), (5, 1024)])
def test_compress_core_variants_same_bytes(amd, ref, O, corpus, core, switch):
    """compress_core 1 (window-parallel core only), 3 (lean core + writer wavefronts only) and 5 (adaptive two-pass over both) with
    extreme routing thresholds produce the reference's bytes, like the default (5, threshold 20 bytes per sequence)"""
    import random as _r
    rng = _r.Random(304)
    blocks, caps = [], []
    for v in list(corpus.values()) + rnd_inputs(O, corpus, 92, 400):
        full = ref.compress_bound(len(v))
        er, _ = ref.compress_fast_raw(v, full)
        for cap in (full, max(0, er + rng.choice([-1, 0, 1, -7, 9]))):
            blocks.append(v); caps.append(cap)
    amd.set_option("compress_core", core)
    amd.set_option("compress_switch", switch)
    try:
        res = gpu_compress_many(amd, blocks, caps)
    finally:
        amd.set_option("compress_core", 5)
        amd.set_option("compress_switch", 16)
    for v, cap, (r, c) in zip(blocks, caps, res):
        er, eb = ref.compress_fast_raw(v, cap)
        assert r == er and (er <= 0 or c == eb), (len(v), cap, r, er)
