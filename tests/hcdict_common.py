"""Shared pieces of the dictionary HC compressor's tests (test_hcdict_hostsim.py, test_hcdict_abi.py, test_gpu_hcdict.py).  The
reference is the reference library's own LZ4_resetStreamHC_fast + LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream, with an
explicit capacity (which can return 0), the dictionary in a buffer of its own whose end is not the source's address (liblz4 would link
the two as a prefix).  Every reference result is computed once and shared (REF below).  The set: dictionaries book1[:L], records cut
from book1[200000:], mixed inputs, records cut out of the dictionary itself, 200 repeated-pattern cases (level 9's pattern analysis on
both sides of the dictionary's end) and hand-built cases on a random dictionary, each of which names the sequence it is about."""
import ctypes as C
import random

from dict_common import RefDict, book1
from dictc_common import bound, caps_for, dict_cuts, other_records, parse

DICT_LENS = (0, 3, 4, 5, 100, 4096, 65535, 65536, 65537, 100000)
SMALL_SIZES = (0, 1, 12, 13, 64, 300, 1000, 4096)
BIG_SIZES = (70000, 200000)
RECORD_BASE = 200000
LEVELS = (1, 3, 4, 8, 9, 10, 12)       # on records up to 4096 bytes
BIG_LEVELS = (9, 10)                   # on the big ones: level 9 and one optimal level
CLAMPS = ((0, 9), (13, 12))            # (level asked for, level it means)


def keep_of(L):
    """what LZ4_loadDictHC keeps: the last 64 KB, with no minimum"""
    return min(L, 65536)


def clamp(level):
    return 9 if level < 1 else min(level, 12)


class Ref:
    """LZ4_resetStreamHC_fast(level) + LZ4_loadDictHC(d) + LZ4_compress_HC_continue(s, cap) on a fresh stream; results are kept"""

    def __init__(self, ref):
        self.rd = RefDict(ref)
        L = self.L = self.rd.L
        L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
        L.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        self.memo = {}

    def compress(self, d, s, level, cap=None):
        """-> (r, bytes); cap None = the bound; r == 0: does not fit"""
        cap = bound(len(s)) if cap is None else cap
        key = (len(d), hash(d), len(s), hash(s), level, cap)
        got = self.memo.get(key)
        if got is None:
            L = self.L
            db, sb = self.rd._dict_buf(bytes(d)), C.create_string_buffer(bytes(s), max(len(s), 1))
            assert C.addressof(db) + len(d) != C.addressof(sb), "the dictionary must not end where the source starts (prefix mode)"
            out = C.create_string_buffer(max(cap, 1))
            st = L.LZ4_createStreamHC()
            L.LZ4_resetStreamHC_fast(st, level)
            L.LZ4_loadDictHC(st, db, len(d))
            r = L.LZ4_compress_HC_continue(st, sb, out, len(s), cap)
            L.LZ4_freeStreamHC(st)
            assert r >= 0
            got = self.memo[key] = (r, out.raw[:r])
        return got

    def plain(self, s, level):
        """LZ4_compress_HC at the bound"""
        out = C.create_string_buffer(bound(len(s)))
        r = self.L.LZ4_compress_HC(bytes(s), out, len(s), len(out), level)
        return r, out.raw[:r]


def book_records(sizes=SMALL_SIZES + BIG_SIZES):
    b = book1()
    return [("book1 %d" % n, b[RECORD_BASE:RECORD_BASE + n]) for n in sizes]


def pattern_cases():
    """200 x (name, dictionary, record): runs of a short unit on both sides of the dictionary's end"""
    rng = random.Random(4242)
    out = []
    for i in range(200):
        unit = rng.choice([b"a", b"ab", b"abcd", b"\0"])

        def run(units):
            r = rng.randrange(len(unit))
            return (unit * (units + 1))[r:r + units * len(unit)]

        d = rng.randbytes(rng.choice([0, 50, 3000, 65000])) + unit * rng.randrange(2, 400)
        if i % 10 < 3:
            d += rng.randbytes(rng.randrange(1, 4))
        rec = run(rng.randrange(0, 200)) + rng.randbytes(rng.randrange(1, 9)) + run(rng.randrange(2, 400)) + rng.randbytes(13)
        out.append(("pattern %d" % i, d, rec))
    return out


def has_dict_match(seqs):
    return any(off > pos for pos, off, ml in seqs)


def has_straddle(seqs):
    """a match that starts in the dictionary and runs over its end into the record"""
    return any(off > pos and off - pos < ml for pos, off, ml in seqs)


def hand_cases():
    """[(name, dictionary, record, check)]: check(sequences of the REFERENCE's level 9 output) asserts the intended sequence"""
    rng = random.Random(777)
    d = bytearray(rng.randbytes(4096))
    d[2002:2008] = d[1000:1006]          # (the lazy-evaluation case below)
    d = bytes(d)
    K = len(d)
    out = []

    def has(*want):
        def chk(seqs):
            for q in want:
                assert q in seqs, "%r not in %r" % (q, seqs[:8])
        return chk

    def no_dict_match(seqs):
        assert not has_dict_match(seqs), seqs[:8]

    out.append(("over the end", d, d[-40:] * 2 + rng.randbytes(30), has((0, 40, 80))))
    out.append(("over the end, to matchlimit", d, d[-40:] * 3, has((0, 40, 115))))
    # the dictionary's last k bytes in the record: positions K-3 .. K-1 are never inserted, K-4 is
    out.append(("last 3 bytes", d, rng.randbytes(20) + d[-3:] + rng.randbytes(20), no_dict_match))
    out.append(("last 4 bytes", d, rng.randbytes(20) + d[-4:] + rng.randbytes(20), has((20, 24, 4))))
    out.append(("last 5 bytes", d, rng.randbytes(20) + d[-5:] + rng.randbytes(20), has((20, 25, 5))))
    # the dictionary's last three bytes followed by the record's own start would match 13 bytes at dictionary position K-3, which is
    # no candidate; the ten bytes match the record's start instead
    r0 = rng.randbytes(20)
    out.append(("last three positions are no candidates", d, r0 + d[-3:] + r0[:10] + rng.randbytes(20), no_dict_match))
    # the same content in the dictionary and earlier in the record: the most recent position wins
    w = d[300:354]
    out.append(("dictionary versus record", d, w + w + rng.randbytes(20), has((0, K - 300, 54), (54, 54, 54))))
    # a dictionary copy behind compressible filler: in reach at distance 64000 + 3096, out of reach behind 66000 bytes
    filler = bytes(rng.choice(b"ab") for _ in range(66000))
    out.append(("in reach", d, filler[:60000] + d[1000:1040] + rng.randbytes(20), has((60000, 60000 + K - 1000, 40))))

    def far(seqs):
        assert seqs and not any(66000 <= pos < 66040 and ml >= 8 for pos, off, ml in seqs), [q for q in seqs if q[0] >= 65990][:8]
    out.append(("out of reach", d, filler + d[1000:1040] + rng.randbytes(20), far))
    d4 = rng.randbytes(4)
    out.append(("K = 4", d4, rng.randbytes(20) + d4 + rng.randbytes(20), has((20, 24, 4))))
    # lazy evaluation: the first match (8 bytes of the dictionary at 2000) is found at 20; the wider search from 26 finds the
    # dictionary at 1004 and extends it backwards over 25 .. 22, which leaves the first match two bytes: it is dropped, 20 and 21
    # become literals in front of the dictionary match at 22
    out.append(("wider search extends backwards", d, rng.randbytes(20) + d[2000:2002] + d[1000:1050] + rng.randbytes(20),
                has((22, 22 + K - 1000, 50))))
    return out


def check_hand_cases(R):
    for name, d, rec, chk in hand_cases():
        r, by = R.compress(d, rec, 9)
        assert r > 0, name
        try:
            chk(parse(by))
        except AssertionError as e:
            raise AssertionError("hand-built case %r: %s" % (name, e))


__all__ = ["BIG_LEVELS", "BIG_SIZES", "CLAMPS", "DICT_LENS", "LEVELS", "Ref", "SMALL_SIZES", "book1", "book_records", "bound", "caps_for",
           "check_hand_cases", "clamp", "dict_cuts", "hand_cases", "has_dict_match", "has_straddle", "keep_of", "other_records", "parse",
           "pattern_cases"]
