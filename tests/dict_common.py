"""Shared pieces of the dictionary-decoder tests (test_dict_hostsim.py, test_dict_abi.py, test_gpu_dict.py): the reference library's own
LZ4_decompress_safe_usingDict through ctypes -- the dictionary in a buffer of its own whose end is NOT the destination's address (liblz4
would switch to prefix mode), 64 bytes of slack behind the stream, cap + 64 bytes of destination --, its dictionary compressors
(LZ4_loadDict + LZ4_compress_fast_continue, LZ4_loadDictHC + LZ4_compress_HC_continue), and the case set: every case is
(name, stream, d, L) -- a stream, the decoded size of its undamaged form (what the capacity list is built around) and the length L of
its dictionary book1[:L]."""
import ctypes as C
import random

from conftest import calgary, lz4_seq
from partial_common import damaged
from size_common import caps_for

_u8p = C.POINTER(C.c_uint8)
DICT_LENS = (1, 3, 4, 100, 4096, 65535, 65536, 65537, 100000)
RECORD_SIZES = (64, 300, 1000, 4096)
BIG_RECORDS = (70000, 200000)          # past the dictionary's reach (op >= 65536) and into the unchanged loops
RECORD_BASE = 200000                   # records are slices of book1[200000:]


def book1():
    return calgary("book1")


class RefDict:
    """the reference library's dictionary entry points"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStream.restype = C.c_void_p
        L.LZ4_freeStream.argtypes = [C.c_void_p]
        L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.LZ4_createStreamHC.restype = C.c_void_p
        L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
        L.LZ4_setCompressionLevel.argtypes = [C.c_void_p, C.c_int]
        L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.LZ4_decompress_safe_usingDict.restype = C.c_int
        L.LZ4_decompress_safe_usingDict.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.LZ4_decompress_safe.restype = C.c_int
        L.LZ4_decompress_safe.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int]
        self._dicts = {}

    def _dict_buf(self, d):
        """the dictionary in a buffer of its own, kept for the object's life (so its address is stable and is never a destination's)"""
        b = self._dicts.get(d)
        if b is None:
            b = self._dicts[d] = C.create_string_buffer(bytes(d), max(len(d), 1))
        return b

    def compress(self, d, s, hc=0):
        """s compressed alone against the dictionary d: LZ4_compress_fast_continue (hc == 0) or LZ4_compress_HC_continue at level hc"""
        L = self.L
        db, sb = self._dict_buf(d), C.create_string_buffer(bytes(s), max(len(s), 1))
        out = C.create_string_buffer(len(s) + len(s) // 255 + 64)
        if hc:
            st = L.LZ4_createStreamHC()
            L.LZ4_setCompressionLevel(st, hc)
            L.LZ4_loadDictHC(st, db, len(d))
            n = L.LZ4_compress_HC_continue(st, sb, out, len(s), len(out))
            L.LZ4_freeStreamHC(st)
        else:
            st = L.LZ4_createStream()
            L.LZ4_loadDict(st, db, len(d))
            n = L.LZ4_compress_fast_continue(st, sb, out, len(s), len(out), 1)
            L.LZ4_freeStream(st)
        assert n > 0
        return out.raw[:n]

    def decode(self, s, cap, d):
        """-> (the reference's LZ4_decompress_safe_usingDict(s, dst, len(s), cap, d, len(d)), the bytes it decoded)"""
        assert cap >= 0
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)   # (slack behind the stream, as the oracle gives liblz4)
        out = (C.c_uint8 * (cap + 64))()
        db = self._dict_buf(d)
        assert C.addressof(db) + len(d) != C.addressof(out), "the dictionary must not end where the destination starts (prefix mode)"
        r = self.L.LZ4_decompress_safe_usingDict(buf, C.cast(out, _u8p), len(s), cap, db, len(d))
        return r, C.string_at(out, max(r, 0))

    def plain(self, s, cap):
        """the reference's LZ4_decompress_safe: its return value"""
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)
        out = (C.c_uint8 * (cap + 64))()
        return self.L.LZ4_decompress_safe(buf, C.cast(out, _u8p), len(s), cap)


def valid_streams(rd, rng, per_size=3):
    """[(name, stream, d, L)]: per dictionary length `per_size` records of each small size and one of each big size, compressed by both
    dictionary compressors"""
    b = book1()
    out = []
    for L in DICT_LENS:
        d = b[:L]
        recs = []
        for size in RECORD_SIZES:
            for _ in range(per_size):
                o = rng.randrange(RECORD_BASE, len(b) - size)
                recs.append(b[o:o + size])
        for size in BIG_RECORDS:
            o = rng.randrange(RECORD_BASE, len(b) - size)
            recs.append(b[o:o + size])
        for r in recs:
            out.append(("fast %d/%d" % (len(r), L), rd.compress(d, r), len(r), L))
            out.append(("hc9 %d/%d" % (len(r), L), rd.compress(d, r, 9), len(r), L))
    return out


def _last(n, rng):
    """the last sequence of a block: n literals (n < 15)"""
    return bytes([n << 4]) + rng.randbytes(n)


def hand_streams(rng):
    """[(name, stream, d, L)] hand-assembled around the rules of liblz4's external-dictionary mode; the flags of the straddling matches
    (rest overlaps what it writes / does not) are checked by test_dict_hostsim.py"""
    out = []

    def one(name, L, seqs, last=5):
        c, n = bytearray(), 0
        for lit, ml, off in seqs:
            c += lz4_seq(lit, ml, off, rng); n += lit + ml
        last = max(last, 12 - seqs[-1][1])   # (a block's last match starts at least 12 bytes in front of its end)
        c += _last(last, rng); n += last
        out.append((name, bytes(c), n, L))

    for L in (100, 4096, 65536, 100000):
        one("wholly in the dictionary", L, [(5, 8, 5 + 20)])
        one("wholly, extended length", L, [(5, 40, 5 + 60)])
        one("ending exactly at the dictionary's end", L, [(5, 8, 5 + 8)])
        one("ending at the end, extended", L, [(3, 30, 3 + 30)])
        one("the whole reach", L, [(2, 6, 2 + min(L, 65533))])
    for L in (3, 4, 100, 65537):
        for k in (1, 2, 3):                       # dictionary bytes of the match
            for op in (0, 1, 2, 3):               # literals in front of it
                for ml in (4, 5, 8, 20, 300):     # rest = ml - k bytes from the block's start: overlaps what it writes once rest > op + k
                    one("straddle k=%d op=%d ml=%d%s" % (k, op, ml, " overlap" if ml - k > op + k else ""), L, [(op, ml, op + k)])
    one("the issue's example", 100, [(1, 4, 2)])
    for L in (1, 3, 100, 4096, 65535):
        for lit in (1, 7):
            for ml in (6, 30, 600):               # short and extended match lengths
                one("offset == op + L, ml=%d" % ml, L, [(lit, ml, lit + L)] if lit + L <= 65535 else [(lit, ml, 65535)])
                if lit + L + 1 <= 65535:
                    one("offset == op + L + 1, ml=%d" % ml, L, [(lit, ml, lit + L + 1)])
    for L in (65536, 65537):
        one("offset 65535, no check", L, [(1, 6, 65535)])
        one("offset 65535, extended", L, [(1, 40, 65535)])
    for L in (100, 4096):
        # a dictionary match followed by exactly five literals: it ends at cap - 5 with cap = d and at cap - 4 with cap = d - 1
        one("dictionary match, then five literals", L, [(2, 10, 2 + 50)], last=5)
        one("straddling match, then five literals", L, [(2, 10, 2 + 3)], last=5)
        one("extended dictionary match, then five literals", L, [(2, 70, 2 + 90)], last=5)
    return out


def mixed_stream(rng, L, n_seq, p_dict=0.6):
    """a valid block of n_seq short sequences: matches wholly in the dictionary (many of them ending within 16 bytes of its end: the
    interior loops' byte-exact copies), straddles, in-block matches near and far, a few long literal runs and long matches.  The
    matches lie in the last 64 bytes of the capacity d as well as far before them.  Returns (stream, d)"""
    c, n = bytearray(), 0
    reach = min(L, 65535)
    for _ in range(n_seq):
        k = rng.random()
        lit = rng.randrange(0, 20) if k < 0.9 else rng.randrange(20, 400)
        ml = rng.randrange(4, 40) if rng.random() < 0.9 else rng.randrange(40, 700)
        p = n + lit
        r = rng.random()
        if r < p_dict and p + ml <= 65535 and reach >= ml:
            back = min(reach, ml + rng.choice([0, 1, 3, 7, 8, 15, 16, rng.randrange(0, reach)]))   # wholly in the dictionary
            off = p + back
        elif r < p_dict + 0.1 and p < 65000 and reach >= 1:
            off = p + rng.randrange(1, min(reach, ml - 1, 65535 - p) + 1)                            # straddles the block's start
        elif p > 0:
            off = rng.choice([rng.randrange(1, min(p, 64) + 1), rng.randrange(1, min(p, 65535) + 1)])
        else:
            lit, off = lit + 1, 1
        off = min(off, 65535)
        c += lz4_seq(lit, ml, off, rng); n += lit + ml
    last = rng.randrange(5, 15)
    c += _last(last, rng)
    return bytes(c), n + last


def mixed_streams(rng):
    out = []
    for L in (100, 4096, 65536, 100000):
        for n_seq in (6, 40, 150, 1500):   # 1500 sequences: more than 2 KB of stream, the deep loop
            s, d = mixed_stream(rng, L, n_seq)
            out.append(("mixed %d sequences" % n_seq, s, d, L))
    s, d = mixed_stream(rng, 65536, 6000, p_dict=0.9)   # runs out of the dictionary's reach
    out.append(("mixed past 64 KB", s, d, 65536))
    return out


def case_set(rd, rng, n_damaged=8, n_random=200):
    """the shared set: (valid, all) -- valid streams as valid_streams gives them; all = those, their forms damaged by 1 to 3 flips,
    every truncation of one short stream, random bytes, the hand-built and the mixed streams"""
    valid = valid_streams(rd, rng)
    cases = list(valid) + hand_streams(rng) + mixed_streams(rng)
    for name, s, d, L in list(cases):
        if len(s) <= 4200:
            k = n_damaged if name.startswith(("fast", "hc9", "mixed")) else 1
            for _ in range(k):
                cases.append(("damaged " + name, damaged(s, rng, flips=rng.randrange(1, 4)), d, L))
        elif rng.random() < 0.5:
            cases.append(("damaged " + name, damaged(s, rng, flips=rng.randrange(1, 4)), d, L))
    short = next(c for c in valid if c[2] == 300 and c[3] == 4096)
    for cut in range(len(short[1]) + 1):
        cases.append(("cut %d/%d" % (cut, len(short[1])), short[1][:cut], short[2], short[3]))
    for _ in range(n_random):
        cases.append(("random", rng.randbytes(rng.randrange(0, 300)), rng.randrange(0, 400), rng.choice(DICT_LENS)))
    return valid, cases


def rng_for(seed):
    return random.Random(seed)


__all__ = ["DICT_LENS", "RefDict", "book1", "caps_for", "case_set", "hand_streams", "mixed_stream", "mixed_streams", "rng_for",
           "valid_streams"]
