"""The stream/container twins on the product path (-m gpu): same cases as tests/test_streams_host.py, with every
compress / decompress / xxh32 served by liblz4hip batches; the oracle is only the checker inside the cases."""
import importlib
import io

import pytest

import streams_common as sc
from support import build_mirror

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def engine(S):
    return S.HIPEngine()


@pytest.fixture(scope="module")
def data(corpus, O):
    return sc.payload(corpus, O)


def test_frame_layout_and_roundtrip(S, engine, port, data):
    sc.case_frame_layout_and_roundtrip(S, engine, port, data)


def test_frame_size_sweep(S, engine, data):
    sc.case_frame_size_sweep(S, engine, data)


def test_frame_known_header_bytes(S, engine):
    sc.case_frame_known_header_bytes(S, engine)


def test_frame_flush_and_bytewise(S, engine, port, data):
    sc.case_frame_flush_and_bytewise(S, engine, port, data)


def test_frame_concat_skippable_single(S, engine, data):
    sc.case_frame_concat_skippable_single(S, engine, data)


def test_frame_errors(S, engine, data):
    sc.case_frame_errors(S, engine, data)


@pytest.mark.skipif(sc.LZ4_CLI is None, reason="lz4 CLI not installed")
def test_frame_cli_interop(S, engine, data):
    sc.case_frame_cli_interop(S, engine, data)


def test_frame_hc(S, port, data):
    """HC level 9 behind the frame container: blocks are bit-exact LZ4_compress_HC output"""
    sink = io.BytesIO()
    f = S.LZ4FrameOutputStream(sink, S.BLOCKSIZE.SIZE_256KB, -1, engine=S.HIPEngine(hcLevel=9))
    f.write(data)
    f.close()
    _, _, _, _, blocks, _, _ = sc.parse_frame(sink.getvalue())
    for i, (stored_raw, body, _) in enumerate(blocks):
        raw = data[i << 18:(i + 1) << 18]
        comp = port.compress_hc(raw, 9)
        assert (stored_raw and body == raw) if len(comp) >= len(raw) else (not stored_raw and body == comp)
    assert S.LZ4FrameInputStream(io.BytesIO(sink.getvalue())).read() == data


def test_block_stream(S, engine, port, data):
    sc.case_block_stream(S, engine, port, data)


def test_with_length(S, engine, port, data):
    sc.case_with_length(S, engine, port, data, hc_engine=S.HIPEngine(hcLevel=9))


def test_cpp_stream_mirror_runs_and_interoperates(S, engine):
    """the C++ twins (lz4-java_amd/host/lz4hip_streams.hpp): their own checks pass, and the containers they write are the
    Python twin's byte for byte, decode with the lz4 CLI, and a CLI frame decodes with them"""
    import os
    import subprocess
    import tempfile
    from conftest import ROOT
    exe = build_mirror("stream_mirror_test", os.path.join(ROOT, "tests", "cpp"))
    with tempfile.TemporaryDirectory() as d:
        cli_payload = bytes(range(256)) * 3000 + b"tail"
        if sc.LZ4_CLI:
            open(os.path.join(d, "cli_payload.bin"), "wb").write(cli_payload)
            open(os.path.join(d, "cli.lz4"), "wb").write(sc.cli(["-1", "-B5", "-BX"], cli_payload))
        assert subprocess.call([exe, d]) == 0
        data = open(os.path.join(d, "cpp_payload.bin"), "rb").read()
        B = S.FLG.Bits
        for name, bs, bits, known in (("cpp_frame_default.lz4", S.BLOCKSIZE.SIZE_4MB, (B.BLOCK_INDEPENDENCE,), -1),
                                      ("cpp_frame_all.lz4", S.BLOCKSIZE.SIZE_64KB,
                                       (B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE), len(data)),
                                      ("cpp_frame_256k_cc.lz4", S.BLOCKSIZE.SIZE_256KB, (B.BLOCK_INDEPENDENCE, B.CONTENT_CHECKSUM), -1)):
            fr = open(os.path.join(d, name), "rb").read()
            assert fr == sc.frame_bytes(S, data, engine, bs, bits, known), name
            assert S.LZ4FrameInputStream(io.BytesIO(fr), engine=engine).read() == data
            if sc.LZ4_CLI:
                assert sc.cli(["-d"], fr) == data
        blk = open(os.path.join(d, "cpp_stream.blk"), "rb").read()
        assert blk == sc.block_stream_bytes(S, data, engine, 1 << 16)
        assert S.LZ4BlockInputStream(io.BytesIO(blk), engine=engine).read() == data


class _HostAssembly:
    """the HIP engine WITHOUT the device-side container assembly: the writers then assemble on the host (the round-1/2 path)"""

    def __init__(self, eng):
        self._e = eng
        self.hcLevel = eng.hcLevel
        self.compress, self.decompressSafe, self.decompressFast, self.xxh32 = eng.compress, eng.decompressSafe, eng.decompressFast, eng.xxh32
        self.newStreamingHash32 = eng.newStreamingHash32


def test_device_assembled_containers_equal_host_assembled(S, amd, O, corpus, ref):
    """frames and LZ4Block streams whose blocks are laid out ON THE DEVICE (raw fallback, size scan, headers,
    payload compaction, block / original-data checksums: lz4hip_container_blocks) are byte-identical to the ones assembled on the host
    around the batch launches -- which the other cases of this file pin to the `lz4` CLI and to the reference's layout -- for every
    block size class, with and without block checksums, fast and HC, incl. empty input, a short tail block, incompressible blocks
    (stored raw) next to compressible ones, and the raw C entry point itself"""
    import os, random
    rng = random.Random(77)
    book = corpus["book1[:200000]"]
    inputs = [b"", b"x", b"abcd" * 40, rng.randbytes(70000), book[:150000], O.gen_block(300000, 11, win=4096),
              rng.randbytes(65536) + book[:65536] + bytes(65536) + rng.randbytes(100), O.gen_block(1 << 20, 12) + book[:12345]]
    for hc in (None, 9):
        dev, host = S.HIPEngine(hc), _HostAssembly(S.HIPEngine(hc))
        for v in inputs if hc is None else inputs[:6]:
            for bs in (S.BLOCKSIZE.SIZE_64KB, S.BLOCKSIZE.SIZE_256KB, S.BLOCKSIZE.SIZE_4MB):
                for bits in ((S.FLG.Bits.BLOCK_INDEPENDENCE,), (S.FLG.Bits.BLOCK_INDEPENDENCE, S.FLG.Bits.BLOCK_CHECKSUM, S.FLG.Bits.CONTENT_CHECKSUM)):
                    got = []
                    for eng in (dev, host):
                        o = io.BytesIO()
                        w = S.LZ4FrameOutputStream(o, bs, -1, *bits, engine=eng, batchBlocks=5)
                        w.write(v); w.close()
                        got.append(o.getvalue())
                    assert got[0] == got[1], ("frame", hc, len(v), bs, bits)
                    assert S.LZ4FrameInputStream(io.BytesIO(got[0]), engine=dev).read() == v
            for block in (64, 1000, 65536, 1 << 20):
                got = []
                for eng in (dev, host):
                    o = io.BytesIO()
                    w = S.LZ4BlockOutputStream(o, block, engine=eng, batchBlocks=7)
                    w.write(v); w.close()
                    got.append(o.getvalue())
                assert got[0] == got[1], ("lz4block", hc, len(v), block)
                assert S.LZ4BlockInputStream(io.BytesIO(got[0]), engine=dev).read() == v
    # the C entry points: a destination that is too small is an error, never a truncated container; the device-pointer form
    import torch
    v = inputs[4]
    want = amd.LZ4HIPBatch.containerBlocks(0, v, 65536, True)
    import ctypes as C
    dst = bytearray(len(want) - 1)
    out = C.c_uint64(0)
    rc = amd.lib().lz4hip_container_blocks(0, 1, 0, v, len(v), 65536, (C.c_uint8 * len(dst)).from_buffer(dst), len(dst), C.byref(out))
    assert rc != 0 and out.value == 0
    dev0 = torch.device("cuda:0")
    src = torch.frombuffer(bytearray(v), dtype=torch.uint8).to(dev0)
    d = torch.zeros(len(v) + 64, dtype=torch.uint8, device=dev0)
    total = torch.zeros(1, dtype=torch.int64, device=dev0)
    amd.DeviceBatch.container_blocks(0, src, 65536, d, total, block_checksum=True)
    torch.cuda.synchronize()
    assert int(total.item()) == len(want) and d[:len(want)].cpu().numpy().tobytes() == want


def test_device_container_exact_capacity_and_too_small(amd, O, corpus):
    """lz4hip_container_blocks_dev with a destination of EXACTLY the container's size (round-3 advisor finding: without block
    checksums the copy kernel's capacity guard counted 4 bytes the scan had not, and silently dropped the last block of an exactly
    sized buffer), and with one that is too small: *total says so, nothing beyond dst_cap is written, and the checksum pass that
    follows never reads payloads of skipped blocks beyond the capacity."""
    import random
    import torch
    rng = random.Random(9)
    dev0 = torch.device("cuda:0")
    incompressible = rng.randbytes(3 * 65536 + 1000)          # stored raw: n_bytes + 4 n
    mixed = corpus["book1[:200000]"][:150000] + rng.randbytes(70000)
    for v in (incompressible, mixed):
        for kind in (0, 1):
            for chk in ((False, True) if kind == 0 else (False,)):
                want = amd.LZ4HIPBatch.containerBlocks(kind, v, 65536, chk)
                src = torch.frombuffer(bytearray(v), dtype=torch.uint8).to(dev0)
                total = torch.zeros(1, dtype=torch.int64, device=dev0)
                # exact capacity (a guard region behind it lives in the same tensor so that an overrun is seen, not faulted)
                buf = torch.full((len(want) + 256,), 0xA5, dtype=torch.uint8, device=dev0)
                amd.DeviceBatch.container_blocks(kind, src, 65536, buf[:len(want)], total, block_checksum=chk)
                torch.cuda.synchronize()
                assert int(total.item()) == len(want), (kind, chk)
                assert buf[:len(want)].cpu().numpy().tobytes() == want, (kind, chk, "exactly sized destination")
                assert bool((buf[len(want):] == 0xA5).all()), (kind, chk, "bytes beyond dst_cap written")
                # too small by 1 .. a block: total reports the need, the guard stays intact
                for short in (1, 3, 4, 700, 70000):
                    cap = max(0, len(want) - short)
                    buf.fill_(0xA5)
                    amd.DeviceBatch.container_blocks(kind, src, 65536, buf[:cap], total, block_checksum=chk)
                    torch.cuda.synchronize()
                    assert int(total.item()) == len(want) > cap
                    assert bool((buf[cap:] == 0xA5).all()), (kind, chk, short, "bytes beyond dst_cap written")


def test_lz4block_parallel_walk_equals_serial_rules(S, amd, O, port, corpus):
    """LZ4Block streams of more than 64 KB are walked IN PARALLEL on the device (container.hip container_find_kernel +
    container_walk_par_kernel: a candidate header per region, a lane per region, a stitch in stream order; the serial walk behind it
    for whatever the stitch cannot vouch for).  lz4hip_container_decode against the host restatement of the walk's rules
    (streams_common.OracleDeviceEngine.containerDecode: LZ4BlockInputStream.java:191-264 in order): blocks delivered, their sizes and
    bytes, container bytes consumed and the stop reason -- on bodies of thousands of blocks (1024 lanes), with raw blocks whose PAYLOAD
    holds magics and whole valid-looking headers (in front of and behind a region's true header), slot limits inside / exactly at
    the end of a lane's run, a missing / damaged empty block, cut tails, and damage anywhere."""
    import random
    import struct
    import streams_common as sc
    rng = random.Random(2048)
    eng = S.HIPEngine()
    host = sc.OracleDeviceEngine(port, O)
    B = amd.LZ4HIPBatch
    book = corpus["book1[:200000]"]

    def stream(n_blocks, block, decoys=0.0):
        """an LZ4Block stream of n_blocks blocks (compressible, incompressible = stored raw, and -- decoys -- raw blocks whose bytes
        contain magics and valid-looking headers)"""
        parts = []
        for i in range(n_blocks):
            k = rng.random()
            if k < decoys:      # incompressible noise with LZ4Block headers inside (a stored container in a container)
                inner = b"LZ4Block" + bytes([0x20 | 6]) + struct.pack("<iiI", rng.randrange(1, 400), rng.randrange(400, 65000), rng.randrange(1 << 28))
                b = bytearray(rng.randbytes(block))
                for _ in range(rng.randrange(1, 6)):
                    at = rng.randrange(0, block - 40)
                    b[at:at + len(inner)] = inner if rng.random() < 0.7 else b"LZ4Block" + rng.randbytes(13)
                parts.append(bytes(b))
            elif k < decoys + 0.3:
                parts.append(rng.randbytes(block))
            else:
                at = rng.randrange(0, len(book) - 5000)
                parts.append((book[at:] + book * (block // len(book) + 1))[:block])
        v = b"".join(parts)
        o = io.BytesIO()
        w = S.LZ4BlockOutputStream(o, block, engine=eng, batchBlocks=256)
        w.write(v); w.close()
        return o.getvalue(), v

    def same(body, max_block, n_max):
        want = host.containerDecode(B.LZ4BLOCK_BLOCKS, body, max_block, n_max)
        got = B.containerDecode(B.LZ4BLOCK_BLOCKS, body, max_block, n_max)
        assert got[1:4] == want[1:4], (len(body), n_max, got[1:4][1:], want[1:4][1:], len(got[1]), len(want[1]))
        assert got[0] == want[0]
        return want

    n_stop = {}
    for n_blocks, block, decoys in ((3000, 4096, 0.0), (2500, 4096, 0.15), (700, 65536, 0.1), (40, 1 << 20, 0.2)):
        body, v = stream(n_blocks, block, decoys)
        assert len(body) > 65536
        mb = 1 << max(10, (block - 1).bit_length())
        r = same(body, mb, n_blocks + 10)                     # the whole stream: every block, the empty block reached
        assert r[3] == B.CR_END and len(r[1]) == n_blocks and r[0] == v
        for n_max in (1, 7, n_blocks // 3, n_blocks - 1, n_blocks, n_blocks + 1):
            r = same(body, mb, n_max)
            n_stop[r[3]] = n_stop.get(r[3], 0) + 1
        end = len(body) - 21                                   # (the empty block)
        for cut in (end, end + 5, end - 1, end - 3000, len(body) // 2, 70000):
            r = same(body[:cut], mb, n_blocks + 10)
            n_stop[r[3]] = n_stop.get(r[3], 0) + 1
        heads = [m for m in range(0, len(body) - 8) if body[m:m + 8] == b"LZ4Block"][:0]   # (positions come from a walk, below)
        pos, p = [], 0
        while p + 21 <= len(body):
            pos.append(p)
            p += 21 + struct.unpack_from("<i", body, p + 9)[0]
        for _ in range(14):                                    # damage: header fields, payload bytes, a magic
            d = bytearray(body)
            h = pos[rng.randrange(len(pos))]
            kind = rng.randrange(5)
            if kind == 0:
                d[h + rng.randrange(8)] ^= 0x20
            elif kind == 1:
                d[h + 8] ^= rng.choice([0x10, 0x30, 0x80])
            elif kind == 2:
                d[h + 9 + rng.randrange(8)] ^= 1 << rng.randrange(8)
            elif kind == 3:
                d[h + 17 + rng.randrange(4)] ^= 1 << rng.randrange(8)
            else:
                d[rng.randrange(len(d))] ^= 1 << rng.randrange(8)
            r = same(bytes(d), mb, n_blocks + 10)
            n_stop[r[3]] = n_stop.get(r[3], 0) + 1
    assert n_stop.get(B.CR_CORRUPT, 0) > 10 and n_stop.get(B.CR_SLOTS, 0) > 5 and n_stop.get(B.CR_TRUNCATED, 0) > 3 and n_stop.get(B.CR_MORE, 0) >= 1, n_stop


def test_frame_parallel_walk_equals_serial_rules(S, amd, O, port, corpus):
    """LZ4 Frame bodies have no marker in front of a block; the device walks them in parallel all the same: a region's candidate is a
    position whose chain of size words holds for three (five: blocks over 256 KB) blocks, and the stitch accepts it only if the true
    chain from offset 0 lands on it (else the serial walk does the body).  lz4hip_container_decode against the host restatement of
    LZ4FrameInputStream.java:258-322: blocks delivered, sizes, bytes, consumed, stop reason and liblz4's code -- bodies of thousands of
    blocks, with and without block checksums, raw blocks, an end mark / none, slot limits, cut tails, damaged size words, payloads and
    checksums, and payloads made of small little-endian integers (every position a plausible size word: the serial walk's case)."""
    import random
    import struct
    import streams_common as sc
    rng = random.Random(4096)
    host = sc.OracleDeviceEngine(port, O)
    B = amd.LZ4HIPBatch
    book = corpus["book1[:200000]"]
    n_stop = {}

    def same(body, max_block, n_max, cks):
        want = host.containerDecode(B.FRAME_BLOCKS, body, max_block, n_max, cks)
        got = B.containerDecode(B.FRAME_BLOCKS, body, max_block, n_max, cks)
        assert got[1:] == want[1:], (len(body), n_max, cks, got[2:], want[2:], len(got[1]), len(want[1]))
        assert got[0] == want[0]
        n_stop[want[3]] = n_stop.get(want[3], 0) + 1
        return want

    for n_blocks, block, cks, kind in ((3000, 4096, False, "mixed"), (2000, 4096, True, "mixed"), (600, 65536, True, "mixed"), (300, 65536, False, "ints"),
                                       (24, 1 << 20, False, "mixed")):
        parts = []
        for i in range(n_blocks):
            k = rng.random()
            if kind == "ints":          # raw blocks full of small integers: every aligned position looks like a size word
                parts.append(b"".join(struct.pack("<I", rng.randrange(1, 3000)) for _ in range(block // 4)))
            elif k < 0.3:
                parts.append(rng.randbytes(block))
            else:
                at = rng.randrange(0, len(book) - 5000)
                parts.append((book[at:] + book * (block // len(book) + 1))[:block])
        v = b"".join(parts)
        body = B.containerBlocks(B.FRAME_BLOCKS, v, block, cks)
        assert len(body) > 65536
        r = same(body + b"\0\0\0\0", block, n_blocks + 10, cks)     # with the end mark
        assert r[3] == B.CR_END and len(r[1]) == n_blocks and r[0] == v
        r = same(body, block, n_blocks + 10, cks)                       # the body ends at a block boundary
        assert r[3] == B.CR_MORE and len(r[1]) == n_blocks
        for n_max in (1, 5, n_blocks // 2, n_blocks - 1, n_blocks):
            same(body, block, n_max, cks)
        for cut in (len(body) - 1, len(body) - 3, len(body) - block // 3, len(body) // 2, 70001):
            same(body[:cut], block, n_blocks + 10, cks)
        pos, p = [], 0
        while p + 4 <= len(body):
            pos.append(p)
            p += 4 + (struct.unpack_from("<I", body, p)[0] & 0x7FFFFFFF) + (4 if cks else 0)
        for _ in range(12):                                             # damage: a size word, a payload byte, a checksum
            d = bytearray(body)
            h = pos[rng.randrange(len(pos))]
            k = rng.randrange(4)
            if k == 0:
                d[h + rng.randrange(4)] ^= 1 << rng.randrange(8)
            elif k == 1:
                d[h:h + 4] = struct.pack("<I", rng.choice([0, block + 1, 0x7FFFFFFF, 1]))
            elif k == 2 and cks:
                e = h + 4 + (struct.unpack_from("<I", body, h)[0] & 0x7FFFFFFF)
                d[e + rng.randrange(4)] ^= 1 << rng.randrange(8)
            else:
                d[rng.randrange(len(d))] ^= 1 << rng.randrange(8)
            same(bytes(d), block, n_blocks + 10, cks)
    assert n_stop.get(B.CR_SLOTS, 0) > 5 and n_stop.get(B.CR_TRUNCATED, 0) > 5 and n_stop.get(B.CR_END, 0) >= 5 and \
        n_stop.get(B.CR_BLOCK_TOO_BIG, 0) + n_stop.get(B.CR_DECODE, 0) + n_stop.get(B.CR_BLOCK_CHECKSUM, 0) > 5, n_stop


def test_device_read_path_equals_host_walk(S, amd, O, corpus, ref):
    """SURVEY.md 8(f) f1 / f2, READ side: frames and LZ4Block streams whose headers are walked, checksums verified and blocks decoded ON
    THE DEVICE (lz4hip_container_decode{,_dev}) deliver the same bytes and raise the same exception, at the same point of the stream,
    as the readers that walk the headers on the host around the batch launches (hostWalk=True; the other cases of this file pin
    those to the reference's readers) -- intact streams of every shape and the same streams damaged at every kind of place:
    size words, payload bytes, block / content checksums, headers' magic / token / lengths / check, truncation anywhere."""
    import random
    rng = random.Random(404)
    book = corpus["book1[:200000]"]
    inputs = [b"", b"x", rng.randbytes(70000), book[:150000], O.gen_block(300000, 21, win=4096),
              rng.randbytes(65536) + book[:65536] + bytes(65536) + rng.randbytes(100)]
    eng = S.HIPEngine()

    def drain(stream):
        got = bytearray()
        try:
            while True:
                b = stream.read(50000)
                if not b:
                    return bytes(got), None
                got += b
        except Exception as e:  # noqa: BLE001 -- the exception's type and text are what is compared
            return bytes(got), (type(e).__name__, str(e))

    def both(make):
        a, b = drain(make(False)), drain(make(True))
        assert a == b, (a[1], b[1], len(a[0]), len(b[0]))
        return a

    streams = []
    for v in inputs:
        for bs, bits in ((S.BLOCKSIZE.SIZE_64KB, (S.FLG.Bits.BLOCK_INDEPENDENCE,)),
                         (S.BLOCKSIZE.SIZE_64KB, (S.FLG.Bits.BLOCK_INDEPENDENCE, S.FLG.Bits.BLOCK_CHECKSUM, S.FLG.Bits.CONTENT_CHECKSUM)),
                         (S.BLOCKSIZE.SIZE_256KB, (S.FLG.Bits.BLOCK_INDEPENDENCE, S.FLG.Bits.CONTENT_SIZE))):
            o = io.BytesIO()
            w = S.LZ4FrameOutputStream(o, bs, len(v) if S.FLG.Bits.CONTENT_SIZE in bits else -1, *bits, engine=eng, batchBlocks=5)
            w.write(v); w.close()
            streams.append(("frame", o.getvalue(), v))
        for block in (64, 1000, 65536):
            o = io.BytesIO()
            w = S.LZ4BlockOutputStream(o, block, engine=eng, batchBlocks=7)
            w.write(v); w.close()
            streams.append(("block", o.getvalue(), v))
    n_err = 0
    for kind, data, v in streams:
        def make(hw, d=data, k=kind, bb=3):
            return (S.LZ4FrameInputStream(io.BytesIO(d), engine=eng, batchBlocks=bb, hostWalk=hw) if k == "frame"
                    else S.LZ4BlockInputStream(io.BytesIO(d), engine=eng, batchBlocks=bb, hostWalk=hw))
        got, exc = both(make)
        assert exc is None and got == v
        for _ in range(6 if len(data) > 40 else 2):   # damage: a flipped byte anywhere, or a cut
            d = bytearray(data)
            if rng.random() < 0.3 and len(d) > 1:
                d = d[:rng.randrange(1, len(d))]
            else:
                d[rng.randrange(len(d))] ^= 1 << rng.randrange(8)
            r = both(lambda hw, d=bytes(d), k=kind: make(hw, d, k, rng.choice([1, 2, 64])) if False else make(hw, d, k))
            n_err += r[1] is not None
    assert n_err > 50
    # stopOnEmptyBlock = False: the reader goes on behind an empty block
    o = io.BytesIO()
    for part in (book[:3000], b"", book[3000:9000]):
        w = S.LZ4BlockOutputStream(o, 1000, engine=eng); w.write(part); w.finish()
    cat = o.getvalue()
    a = both(lambda hw: S.LZ4BlockInputStream(io.BytesIO(cat), stopOnEmptyBlock=False, engine=eng, batchBlocks=4, hostWalk=hw))
    assert a == (book[:9000], None)
    # the device-pointer entry itself: a frame body in device memory
    import ctypes as C
    import torch
    o = io.BytesIO()
    w = S.LZ4FrameOutputStream(o, S.BLOCKSIZE.SIZE_64KB, -1, S.FLG.Bits.BLOCK_INDEPENDENCE, S.FLG.Bits.BLOCK_CHECKSUM, engine=eng)
    w.write(book[:150000] + rng.randbytes(66000)); w.close()
    body = o.getvalue()[7:]   # magic, FLG, BD, HC: 7 bytes
    dev0 = torch.device("cuda:0")
    t = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev0)
    n_max = 8
    dst = torch.zeros(n_max * 65536, dtype=torch.uint8, device=dev0)
    sizes = torch.zeros(n_max, dtype=torch.int32, device=dev0)
    info = torch.zeros(5, dtype=torch.int64, device=dev0)
    wsb = amd.lib().lz4hip_container_decode_workspace_bytes(n_max)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev0)
    rc = amd.lib().lz4hip_container_decode_dev(0, 1, t.data_ptr(), len(body), 65536, dst.data_ptr(), 65536, n_max, sizes.data_ptr(), info.data_ptr(),
                                               ws.data_ptr(), wsb, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    n_ok, consumed, why, total = (int(x) for x in info[:4].cpu())
    assert (n_ok, why, total, consumed) == (4, 0, 216000, len(body))
    out = b"".join(dst[k * 65536:k * 65536 + int(sizes[k])].cpu().numpy().tobytes() for k in range(n_ok))
    assert out[:150000] == book[:150000] and len(out) == 216000
