"""The case list of the many-container read call (lz4hip_container_decode_many) and what its tests share.  The bodies are built from the
reference library alone (`ref`: oracle.ref(), liblz4 1.9.3 and its XXH32): LZ4 Frame bodies (kind 0, from the first block's size word
on) and lz4-java "LZ4Block" streams (kind 1).  A case is (name, kind, body, max_block, block_checksum)."""
import ctypes as C
import random
import struct

import numpy as np

FRAME, LZ4BLOCK = 0, 1
CHECK_SEED = 0x9747b28c


def frame_body(ref, blocks, cks, end=True):
    """what LZ4FrameOutputStream.writeBlock emits per block (raw where compression does not gain), + the end mark"""
    out = bytearray()
    for b in blocks:
        c = ref.compress_fast(b)
        raw = len(c) >= len(b)
        pay = b if raw else c
        out += struct.pack("<I", len(pay) | (0x80000000 if raw else 0)) + pay
        if cks:
            out += struct.pack("<I", ref.xxh32(pay, 0))
    return bytes(out) + (b"\0\0\0\0" if end else b"")


def level_nibble(block_size):
    return max(0, (block_size - 1).bit_length() - 10)


def block_header(method, nibble, clen, olen, check, magic=b"LZ4Block"):
    return magic + bytes([method | nibble]) + struct.pack("<iiI", clen, olen, check)


def block_stream(ref, blocks, block_size, end=True):
    """what LZ4BlockOutputStream.flushBufferedData emits per block, + the empty block"""
    nib = level_nibble(block_size)
    out = bytearray()
    for b in blocks:
        c = ref.compress_fast(b)
        raw = len(c) >= len(b)
        pay = b if raw else c
        out += block_header(0x10 if raw else 0x20, nib, len(pay), len(b), ref.xxh32(b, CHECK_SEED) & 0x0FFFFFFF) + pay
    return bytes(out) + (block_header(0x10, nib, 0, 0, 0) if end else b"")


def cut(data, sizes):
    out, p = [], 0
    for s in sizes:
        out.append(data[p:p + s]); p += s
    return out


def hostile_headers():
    """5 KB of LZ4Block headers {level nibble 15, original length 32 MiB, compressed length 1}: they must size nothing"""
    return b"".join(block_header(0x20, 15, 1, 32 << 20, 0) + b"\0" for _ in range(256))


_CASES = {}


def cases(ref, corpus):
    """the case list (built once, shared and left unchanged)"""
    if "all" in _CASES:
        return _CASES["all"]
    rng = random.Random(4242)
    text, noise = corpus["book1[:200000]"], rng.randbytes(200000)
    out = []
    add = lambda name, kind, body, mb, cks=False: out.append((name, kind, bytes(body), mb, bool(cks)))
    # items of 0, 1, 2 and 3 blocks with a short last block; compressible, incompressible (raw), empty; with and without the end mark /
    # empty block; with and without block checksums
    for nb in range(4):
        for what, data in (("text", text), ("raw", noise)):
            for end in (True, False):
                for bs in (65536,):
                    sizes = ([bs] * (nb - 1) + [1000 + 37 * nb]) if nb else []
                    for cks in (False, True):
                        add("frame-%d-%s-end%d-cks%d" % (nb, what, end, cks), FRAME, frame_body(ref, cut(data, sizes), cks, end), 65536, cks)
                for bs in (1024, 65536):
                    sizes = ([bs] * (nb - 1) + [bs // 3 + nb]) if nb else []
                    add("lz4block-%d-%s-end%d-bs%d" % (nb, what, end, bs), LZ4BLOCK, block_stream(ref, cut(data, sizes), bs, end), bs)
    add("frame-empty-body", FRAME, b"", 65536)
    add("lz4block-empty-body", LZ4BLOCK, b"", 65536)
    mixed = [text[1000:1100] * 3, noise[:64], text[5000:5075] * 2]     # compressed, raw, compressed: blocks of 64 .. 300 bytes
    assert [len(ref.compress_fast(b)) < len(b) for b in mixed] == [True, False, True]
    # EVERY cut of one three-block body of each kind
    fb, lb = frame_body(ref, mixed, True), block_stream(ref, mixed, 1024)
    for i in range(len(fb) + 1):
        add("frame-cut-%d" % i, FRAME, fb[:i], 65536, True)
    for i in range(len(lb) + 1):
        add("lz4block-cut-%d" % i, LZ4BLOCK, lb[:i], 1024)
    # damage in the second block: a flipped checksum, a flipped payload byte, a size word above max_block
    f_nocks = frame_body(ref, mixed, False)
    len0 = struct.unpack_from("<I", fb, 0)[0] & 0x7FFFFFFF
    b1 = 4 + len0 + 4                                     # block 1's size word in fb (block checksums)
    bad = bytearray(fb); bad[b1 + 4 + 64] ^= 1; add("frame-flipped-checksum", FRAME, bad, 65536, True)
    bad = bytearray(fb); bad[b1 + 4 + 10] ^= 0x55; add("frame-flipped-payload-cks", FRAME, bad, 65536, True)
    bad = bytearray(f_nocks); bad[4 + 1] ^= 0x55; add("frame-flipped-payload-nocks", FRAME, bad, 65536, False)
    bad = bytearray(fb); bad[b1:b1 + 4] = struct.pack("<I", 65537); add("frame-size-above-max", FRAME, bad, 65536, True)
    bad = bytearray(fb); bad[b1:b1 + 4] = struct.pack("<I", 0x7FFFFFFF); add("frame-size-huge", FRAME, bad, 65536, True)
    junk = rng.randbytes(200)                             # a block marked compressed that is no LZ4 stream: liblz4's negative code
    add("frame-undecodable", FRAME, fb[:b1] + struct.pack("<I", 200) + junk + struct.pack("<I", ref.xxh32(junk, 0)) + fb[b1:], 65536, True)
    add("frame-small-max-block", FRAME, fb, 128, True)    # block 0 (300 bytes of text, compressed) may exceed this frame's maximum
    add("frame-first-block-above-max", FRAME, fb, 16, True)
    add("lz4block-first-block-above-max", LZ4BLOCK, lb, 128)
    # each header rule of LZ4BlockInputStream, in the second block
    clen0 = struct.unpack_from("<i", lb, 9)[0]
    h1 = 21 + clen0                                       # block 1's header in lb (raw, 64 bytes)
    def lz4block_bad(name, **kw):
        magic = kw.pop("magic", b"LZ4Block")
        f = dict(method=0x10, nibble=0, clen=64, olen=64, check=struct.unpack_from("<I", lb, h1 + 17)[0])
        f.update(kw)
        add("lz4block-" + name, LZ4BLOCK, lb[:h1] + block_header(f["method"], f["nibble"], f["clen"], f["olen"], f["check"], magic) + lb[h1 + 21:], 1024)
    lz4block_bad("bad-magic", magic=b"LZ4Blocl")
    lz4block_bad("bad-method", method=0x30)
    lz4block_bad("olen-above-level", clen=2000, olen=2000)
    lz4block_bad("olen-negative", olen=-5)
    lz4block_bad("clen-negative", clen=-5)
    lz4block_bad("olen0-clen-not0", olen=0)
    lz4block_bad("clen0-olen-not0", clen=0)
    lz4block_bad("raw-olen-not-clen", olen=63)
    lz4block_bad("empty-block-with-check", clen=0, olen=0)
    lz4block_bad("flipped-check", check=struct.unpack_from("<I", lb, h1 + 17)[0] ^ 1)
    lz4block_bad("method-lz4-on-raw-bytes", method=0x20)                 # the decoder fails or consumes another length
    lz4block_bad("olen-above-max-block", nibble=5, clen=64, olen=2048, method=0x20)
    lz4block_bad("over-announcing", method=0x20, nibble=15, clen=64, olen=32 << 20)
    bad = bytearray(lb); bad[21 + 5] ^= 0x55; add("lz4block-flipped-payload", LZ4BLOCK, bad, 1024)
    add("lz4block-hostile-5k", LZ4BLOCK, hostile_headers(), 1 << 25)
    add("lz4block-hostile-behind-good", LZ4BLOCK, lb[:h1] + hostile_headers(), 1 << 25)
    _CASES["all"] = out
    return out


def frame_header(ref, cks=False, content_checksum=False, content_size=None, independent=True):
    """magic, FLG, BD (64 KiB blocks), [content size], header checksum"""
    flg = 0x40 | (0x20 if independent else 0) | (0x10 if cks else 0) | (0x08 if content_size is not None else 0) | (0x04 if content_checksum else 0)
    desc = bytes([flg, 0x40]) + (struct.pack("<Q", content_size) if content_size is not None else b"")
    return struct.pack("<I", 0x184D2204) + desc + bytes([(ref.xxh32(desc, 0) >> 8) & 0xFF])


def stream_items(ref, corpus, case_list):
    """-> (frames, block streams): whole streams for streams.readFrames / readBlockStreams -- the case list wrapped in frame headers,
    concatenated and skippable frames, a wrong content checksum, a wrong content size, a linked-block frame"""
    text = corpus["book1[:200000]"]
    frames = [frame_header(ref, cks) + body for (_, kind, body, mb, cks) in case_list if kind == FRAME and mb == 65536]
    blocks = [text[:65536], text[65536:65536 + 70000 - 65536 + 300]]
    content = b"".join(blocks)
    body = frame_body(ref, blocks, True)
    good = frame_header(ref, True, True, len(content)) + body + struct.pack("<I", ref.xxh32(content, 0))
    small = frame_header(ref) + frame_body(ref, [text[:500]], False)
    skippable = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    frames += [good, good + small + good, skippable + good + skippable + small, small + b"\x01\x02\x03\x04" + small, good[:-1],
               frame_header(ref, True, True, len(content)) + body + struct.pack("<I", ref.xxh32(content, 0) ^ 1),
               frame_header(ref, True, True, len(content) + 1) + body + struct.pack("<I", ref.xxh32(content, 0)),
               small + frame_header(ref, True, True, len(content) + 1) + body + struct.pack("<I", ref.xxh32(content, 0)) + small,
               frame_header(ref, independent=False) + frame_body(ref, [text[:500]], False),
               small[:5], b"", skippable, skippable[:9],
               frame_header(ref) + frame_body(ref, cut(text, [65536] * 3 + [77]), False)]
    # (not the 256 hostile headers: behind a first header that announces smaller blocks the READERS take their host path, which
    # allocates what every header announces -- 8 GiB per batch; the call itself sizes nothing by them, which is what the other tests check)
    streams = [body for (name, kind, body, mb, cks) in case_list if kind == LZ4BLOCK and "hostile" not in name]
    streams += [block_stream(ref, cut(text, [65536] * 3 + [77]), 65536), block_stream(ref, cut(text, [1024] * 9 + [5]), 1024) + b"trailing"]
    return frames, streams


def read_sequentially(make_reader, item):
    """(data, error) of the sequential reader over one item"""
    import io
    r, got = make_reader(io.BytesIO(item)), bytearray()
    try:
        while True:
            c = r.read(1 << 16)
            if not c:
                return bytes(got), None
            got += c
    except Exception as e:   # noqa: BLE001 -- the reader's own exception is the expected result
        return bytes(got), e


def same_reads(got, want, tag):
    assert len(got) == len(want)
    for i, ((gd, ge), (wd, we)) in enumerate(zip(got, want)):
        assert gd == wd, (tag, i, len(gd), len(wd), ge, we)
        assert (type(ge), str(ge)) == (type(we), str(we)), (tag, i, ge, we)


def case_file(items, n_max, slot=2 ** 64 - 1):
    """the file the C++ programs read (tests/cpp/container_rules_test.cpp says the format)"""
    return struct.pack("<I", len(items)) + b"".join(struct.pack("<IIIIQQ", kind, 1 if cks else 0, mb, n_max, slot, len(body)) + body
                                                    for (_, kind, body, mb, cks) in items)


def run_mirror(exe, tmp_path, items, n_max):
    """tests/cpp/container_many_mirror_test.cpp over the items -> per item (bytes, sizes, consumed, why, code)"""
    import subprocess
    f, o = tmp_path / "cases.bin", tmp_path / "out.bin"
    f.write_bytes(case_file(items, n_max))
    p = subprocess.run([exe, str(f), str(o)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return parse_results(p.stdout, o.read_bytes(), len(items))


def parse_results(text, data, n):
    """the "I <blocks> <consumed> <why> <code> <decoded bytes> <sizes...>" lines of the C++ and fake-JNI programs and the decoded bytes"""
    at, out = 0, []
    for line in text.split("\n"):
        t = line.split()
        if t:
            assert t[0] == "I" and int(t[1]) == len(t) - 6
            out.append((data[at:at + int(t[5])], [int(v) for v in t[6:]], int(t[2]), int(t[3]), int(t[4])))
            at += int(t[5])
    assert at == len(data) and len(out) == n
    return out


def run_fake_jni(exe, tmp_path, items, n_max):
    """tests/jni_stub/fake_jni_container_many.c over the items -> per item (bytes, sizes, consumed, why, code)"""
    import subprocess
    f = tmp_path / "jni_cases.bin"
    f.write_bytes(case_file(items, n_max))
    p = subprocess.run([exe, str(f), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "checks ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    return parse_results((tmp_path / "results.txt").read_text(), (tmp_path / "decoded.bin").read_bytes(), len(items))


def run_mirror_streams(exe, tmp_path, kind, items, batch):
    """readFrames / readBlockStreams of the C++ host mirror over whole streams (the program compares every item with the C++ sequential
    reader itself) -> per item (bytes, exception class name or None, message)"""
    import subprocess
    f, o = tmp_path / ("streams_%d.bin" % kind), tmp_path / ("streams_%d.out" % kind)
    f.write_bytes(struct.pack("<I", len(items)) + b"".join(struct.pack("<Q", len(it)) + it for it in items))
    p = subprocess.run([exe, "--streams", str(kind), str(batch), str(f), str(o)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    data, at, out = o.read_bytes(), 0, []
    for line in p.stdout.split("\n"):
        t = line.split(" ", 3)
        if t[0] == "R":
            out.append((data[at:at + int(t[1])], None if t[2] == "-" else t[2], t[3] if len(t) > 3 else ""))
            at += int(t[1])
    assert at == len(data) and len(out) == len(items)
    return out


def of_kind(case_list, kind):
    return [c for c in case_list if c[1] == kind]


# ---- the C ABI, called directly ----
def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Packed:
    """the items of a call as the C ABI takes them (numpy arrays that outlive the call)"""

    def __init__(self, items, pad=0):
        n = len(items)
        self.n = n
        self.len = np.array([len(c[2]) for c in items] + [0], dtype=np.uint64)   # (one entry more everywhere: no empty arrays)
        self.off = np.zeros(n + 1, dtype=np.uint64)
        p = 0
        parts = []
        for i, c in enumerate(items):                      # (`pad` bytes of 0xA5 between the bodies: a walk that leaves its item reads them)
            self.off[i] = p; parts.append(c[2]); parts.append(b"\xa5" * pad); p += len(c[2]) + pad
        self.blob = np.frombuffer(b"".join(parts) + b"\xa5", dtype=np.uint8).copy()
        self.mb = np.array([c[3] for c in items] + [1], dtype=np.uint32)
        self.fl = np.array([1 if c[4] else 0 for c in items] + [0], dtype=np.uint8)

    def head(self, kind, n_max):
        return (kind, _p(self.blob, C.c_uint8), _p(self.off, C.c_uint64), _p(self.len, C.c_uint64), _p(self.mb, C.c_uint32), _p(self.fl, C.c_uint8),
                self.n, n_max)


def bound_many(L, kind, pk, n_max):
    nb, need = np.zeros(pk.n + 1, dtype=np.uint32), np.zeros(pk.n + 1, dtype=np.uint64)
    rc = L.lz4hip_container_decode_many_bound(*pk.head(kind, n_max), _p(nb, C.c_uint32), _p(need, C.c_uint64))
    assert rc == 0, (rc, L.lz4hip_last_error())
    return nb[:pk.n], need[:pk.n]


GUARD = 256


def decode_many(L, kind, items, n_max, pad=0):
    """one lz4hip_container_decode_many over `items` -> per item (bytes, sizes, consumed, why, code), after checking the arrays' shape,
    the 0xEE guard bytes at and behind item_dst_off[n] and the untouched sizes entries at and behind item_first[n]"""
    pk = Packed(items, pad)
    n = pk.n
    nb, need = bound_many(L, kind, pk, n_max)
    cap, scap = int(need.sum()), int(nb.sum())
    dst = np.full(cap + GUARD, 0xEE, dtype=np.uint8)
    sizes = np.full(scap + GUARD, -77, dtype=np.int32)
    info = np.zeros(5 * n + 1, dtype=np.uint64)
    doff, first = np.full(n + 2, 99, dtype=np.uint64), np.full(n + 2, 99, dtype=np.uint32)
    rc = L.lz4hip_container_decode_many(*pk.head(kind, n_max), _p(dst, C.c_uint8), cap, _p(doff, C.c_uint64), _p(first, C.c_uint32), _p(sizes, C.c_int32),
                                        scap, _p(info, C.c_uint64))
    assert rc == 0, (rc, L.lz4hip_last_error())
    assert doff[0] == 0 and first[0] == 0 and doff[n + 1] == 99 and first[n + 1] == 99
    total, nblk = int(doff[n]), int(first[n])
    assert total <= cap and nblk <= scap
    assert (dst[total:] == 0xEE).all(), "bytes at or behind item_dst_off[n] were written"
    assert (sizes[nblk:] == -77).all(), "sizes entries at or behind item_first[n] were written"
    out = []
    for c in range(n):
        n_ok, consumed, why, tot, code = (int(v) for v in info[5 * c:5 * c + 5])
        if code >= 1 << 63:
            code -= 1 << 64
        assert int(first[c + 1]) - int(first[c]) == n_ok and int(doff[c + 1]) - int(doff[c]) == tot, (c, items[c][0])
        assert n_ok <= nb[c] and tot <= need[c], (c, items[c][0])
        out.append((dst[int(doff[c]):int(doff[c + 1])].tobytes(), [int(v) for v in sizes[int(first[c]):int(first[c + 1])]], consumed, why, code))
    return out


def oracle_results(engine, items, n_max):
    """the reference-backed restatement (streams_common.OracleDeviceEngine.containerDecode) per item"""
    return [tuple(engine.containerDecode(kind, body, mb, n_max, cks)) for (_, kind, body, mb, cks) in items]
