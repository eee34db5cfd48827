"""Shared pieces of the decoded-size tests (test_size_hostsim.py, test_size_abi.py, test_gpu_size.py): the reference library's own
LZ4_decompress_safe through ctypes -- called with a real buffer of cap + 64 bytes, so capacities stay at or below 8 MiB --, the
capacity list, the stream set (the one of test_partial_hostsim.py plus damaged, truncated and random streams) and hand-built
streams whose token, length-extension run, offset bytes and end of block fall on the seams of the fast interior's LDS window
(256 bytes) and stream ring (2048 bytes)."""
import ctypes as C
import random

from conftest import calgary, lz4_seq
from partial_common import damaged, long_literal_stream, overlap_stream

_u8p = C.POINTER(C.c_uint8)
CAP_MAX = 8 << 20
SEAM_SIZES = (256, 2048)          # the loop's window of the stream; its stream ring (group_dev.h SizeWaveDev<2048>)


def ref_size(ref):
    """(stream, cap) -> the reference's LZ4_decompress_safe(stream, buffer of cap + 64 bytes, len, cap)"""
    f = C.CDLL(ref.path).LZ4_decompress_safe
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int]
    out = (C.c_uint8 * (CAP_MAX + 64))()
    outp = C.cast(out, _u8p)

    def run(s, cap):
        assert 0 <= cap <= CAP_MAX
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)   # (slack behind the stream, as the oracle gives liblz4)
        return f(buf, outp, len(s), cap)
    return run


def ref_decode(ref):
    """(stream, cap) -> (the reference's return value, the bytes it decoded)"""
    f = C.CDLL(ref.path).LZ4_decompress_safe
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int]
    out = (C.c_uint8 * (CAP_MAX + 64))()

    def run(s, cap):
        assert 0 <= cap <= CAP_MAX
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)
        r = f(buf, C.cast(out, _u8p), len(s), cap)
        return r, C.string_at(out, max(r, 0))
    return run


def caps_for(d, slen):
    """the capacity list for a stream of slen bytes that decodes (or whose undamaged form decodes) to d bytes"""
    cs = {0, max(d - 1, 0), d, d + 1, d + 63, d + 64, d + 65, d + 605, d + 606, d + 607, 63, 64, 65}
    if 255 * slen + 64 <= CAP_MAX:
        cs.add(255 * slen + 64)
    return sorted(c for c in cs if c <= CAP_MAX)


def valid_streams(ref, O):
    from test_partial_hostsim import streams
    return streams(ref, O)


def stream_set(ref, O, rng, n_small=1000, n_large=30):
    """[(name, stream, d)]: d = the decoded size of the stream's undamaged form (what the capacity list is built around)"""
    book1 = calgary("book1")
    out = list(valid_streams(ref, O))
    for off in range(1, 16):
        for _ in range(2):
            s, d = overlap_stream(rng, off)
            out.append(("overlap off=%d" % off, s, d))
    small = [(ref.compress_fast(book1[:4000]), 4000), (ref.compress_hc(book1[9000:13000], 12), 4000), (ref.compress_fast(O.gen_block(4000, 2)), 4000)]
    large = [(ref.compress_fast(book1[:65536]), 65536), (ref.compress_fast(O.gen_block(65536, 3)), 65536)]
    for bases, count in ((small, n_small), (large, n_large)):
        for s, d in bases:
            for _ in range(count):
                out.append(("damaged", damaged(s, rng, flips=rng.randrange(1, 4)), d))
    short = ref.compress_fast(book1[:300])
    for cut in range(len(short) + 1):
        out.append(("cut %d/%d" % (cut, len(short)), short[:cut], 300))
    for _ in range(400):
        s = rng.randbytes(rng.randrange(0, 300))
        out.append(("random", s, rng.randrange(0, 400)))
    return out


def _filler_to(c, n, target, rng):
    """plain short sequences (3 + literals bytes each) until the stream is exactly `target` bytes long"""
    assert target - len(c) >= 6 or target == len(c)
    while len(c) < target:
        r = target - len(c)
        size = 6 if r >= 12 else r              # (r in 6 .. 11: one last sequence of that size)
        lit = size - 3
        ml = rng.randrange(4, 19)
        c.extend(lz4_seq(lit, ml, rng.randrange(1, min(n + lit, 60000) + 1), rng))
        n += lit + ml
    return n


def seam_stream(kind, pos, rng, tail=900):
    """a valid block in which one feature lies at stream position `pos` exactly: kind "token" -- a sequence starts there; "litrun" /
    "matchrun" -- a literal / match length-extension run of 1 .. 3 bytes starts there; "offset" -- the two offset bytes; "end" -- the
    block ends there (its last byte is pos - 1).  Behind the feature `tail` bytes of plain sequences keep it inside the fast
    interior.  Returns (stream, decoded size)"""
    c, n = bytearray(), 0
    c.extend(lz4_seq(20, 8, 7, rng)); n += 28   # some history
    if kind == "end":
        n = _filler_to(c, n, pos - 8, rng)
        c.extend(bytes([0x70]) + rng.randbytes(7))
        assert len(c) == pos
        return bytes(c), n + 7
    ext = rng.choice([0, 1, 2])                 # 255-bytes in front of the run's last byte
    if kind == "token":
        n = _filler_to(c, n, pos, rng)
        lit, ml = rng.randrange(0, 15), rng.randrange(4, 19)
    elif kind == "litrun":
        n = _filler_to(c, n, pos - 1, rng)       # the token, then the run
        lit, ml = 15 + 255 * ext + rng.randrange(0, 255), rng.randrange(4, 40)
    elif kind == "matchrun":
        lit = rng.randrange(0, 15)
        n = _filler_to(c, n, pos - 3 - lit, rng)  # token, literals, offset, then the run
        ml = 19 + 255 * ext + rng.randrange(0, 255)
    else:
        assert kind == "offset"
        lit = rng.randrange(0, 15)
        n = _filler_to(c, n, pos - 1 - lit, rng)
        ml = rng.randrange(4, 30)
    c.extend(lz4_seq(lit, ml, rng.randrange(1, n + lit + 1), rng))
    n += lit + ml
    n = _filler_to(c, n, len(c) + tail, rng)
    c.extend(bytes([0x80]) + rng.randbytes(8))
    return bytes(c), n + 8


def seam_streams(rng):
    out = []
    for S in SEAM_SIZES:
        for base in (S, 2 * S):
            for delta in range(-2, 3):
                for kind in ("token", "litrun", "matchrun", "offset", "end"):
                    for _ in range(2):
                        s, d = seam_stream(kind, base + delta, rng)
                        out.append(("seam %s at %d%+d" % (kind, base, delta), s, d))
    return out


def edge_streams(rng):
    """(name, stream, capacity): an offset equal to op, an offset of op + 1 (liblz4's error code), an offset of 0, in the exact code
    (first sequence) and in the fast interior (behind ~1000 bytes of plain sequences, ~1000 in front of the end)"""
    out = []
    for where in ("first", "interior"):
        for name, delta in (("offset == op", 0), ("offset == op + 1", 1), ("offset 0", None)):
            c, n = bytearray(), 0
            if where == "interior":
                c.extend(lz4_seq(20, 8, 7, rng)); n += 28
                n = _filler_to(c, n, 1000, rng)
            lit = 9
            off = 0 if delta is None else n + lit + delta
            c.extend(lz4_seq(lit, 6, off, rng)); n += lit + 6
            n = _filler_to(c, n, len(c) + 1000, rng)
            c.extend(bytes([0x80]) + rng.randbytes(8))
            out.append(("%s, %s" % (name, where), bytes(c), n + 8))
    return out


def rng_for(seed):
    return random.Random(seed)


__all__ = ["ref_size", "ref_decode", "caps_for", "stream_set", "seam_streams", "edge_streams", "valid_streams", "long_literal_stream", "rng_for", "SEAM_SIZES",
           "CAP_MAX"]
