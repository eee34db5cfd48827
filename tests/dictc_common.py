"""Shared pieces of the dictionary-compressor tests (test_dictc_hostsim.py, test_dictc_abi.py, test_gpu_dictc.py).  The reference is
always dict_common.RefDict -- the reference library's own LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream, the dictionary in
a buffer of its own whose end is not the source's address (liblz4 would switch to prefix mode) --, here also with an explicit capacity,
which can return 0.  The set: dictionaries book1[:L], records cut from book1[200000:], mixed inputs, records cut out of the dictionary
itself, and hand-built cases around the rules of liblz4's external-dictionary mode, each of which names the sequence it is about so
that a mis-built case fails against the reference's own output."""
import ctypes as C
import random

from conftest import rnd_inputs
from dict_common import RefDict, book1

DICT_LENS = (0, 1, 7, 8, 9, 100, 4096, 65535, 65536, 65537, 100000)
RECORD_SIZES = (0, 1, 12, 13, 14, 64, 300, 1000, 4096, 65546, 65547, 70000, 200000)
RECORD_BASE = 200000
BIG = (1 << 20) + 3


def bound(n):
    return n + n // 255 + 16


def keep_of(L):
    """what LZ4_loadDict keeps: nothing of a dictionary under 8 bytes, else the last 64 KB"""
    return 0 if L < 8 else min(L, 65536)


def ref_compress(rd, d, s, cap=None):
    """-> (r, bytes): LZ4_loadDict(d) + LZ4_compress_fast_continue(s, cap, 1) on a fresh stream; cap None = the bound; r == 0: too small"""
    L = rd.L
    cap = bound(len(s)) if cap is None else cap
    db, sb = rd._dict_buf(d), C.create_string_buffer(bytes(s), max(len(s), 1))
    assert C.addressof(db) + len(d) != C.addressof(sb), "the dictionary must not end where the source starts (prefix mode)"
    out = C.create_string_buffer(max(cap, 1))
    st = L.LZ4_createStream()
    L.LZ4_loadDict(st, db, len(d))
    r = L.LZ4_compress_fast_continue(st, sb, out, len(s), cap, 1)
    L.LZ4_freeStream(st)
    assert r >= 0
    return r, out.raw[:r]


def parse(stream):
    """-> [(position of the match in the block, offset, match length)] of a valid LZ4 block"""
    s, i, pos, out = stream, 0, 0, []
    while True:
        tok = s[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = s[i]; i += 1; lit += b
                if b != 255:
                    break
        i += lit; pos += lit
        if i >= len(s):
            assert i == len(s)
            return out
        off = s[i] | (s[i + 1] << 8); i += 2
        ml = (tok & 15) + 4
        if ml == 19:
            while True:
                b = s[i]; i += 1; ml += b
                if b != 255:
                    break
        out.append((pos, off, ml))
        pos += ml


def caps_for(n, size, small):
    """the bound, the exact reference size, one byte less, 1 and 0 (`small`: all five; else the bound and the two around the size)"""
    c = [bound(n), size, size - 1]
    return c + [1, 0] if small else c


def book_records():
    b = book1()
    return [("book1 %d" % n, b[RECORD_BASE:RECORD_BASE + n]) for n in RECORD_SIZES]


def other_records(O, corpus, n_rnd=40):
    geo = corpus["geo[:65536]"]
    out = [("rnd %d" % i, v) for i, v in enumerate(rnd_inputs(O, corpus, 77, n_rnd))]
    out += [("equal 70", b"\x55" * 70), ("equal 5000", bytes(5000)), ("equal 70000", b"\xaa" * 70000), ("geo 8000", geo[1000:9000])]
    return out


def big_record(O):
    return ("1 MiB + 3", O.gen_block(BIG, 3, win=4096))


def dict_cuts(L, rng, count=12):
    """records cut out of the dictionary book1[:L] itself: anywhere, at its start, at its end, across its end (what follows the
    dictionary in book1 is NOT part of it), each with a random tail so that the block does not end in the match"""
    b = book1()
    if L < 16:
        return []
    out = []
    for _ in range(count):
        o = rng.randrange(0, L - 13)
        n = rng.randrange(13, min(L - o, 3000) + 1)
        out.append(("cut %d+%d" % (o, n), b[o:o + n] + rng.randbytes(rng.randrange(0, 30))))
    out.append(("cut start", b[:min(L, 500)] + rng.randbytes(20)))
    for k in (7, 8, 9, 10, 11, 12, 13, 40, min(L, 300)):
        if k <= L:
            out.append(("cut end %d" % k, rng.randbytes(5) + b[L - k:L] + rng.randbytes(20)))
    out.append(("cut across the end", b[max(L - 40, 0):L + 40] + rng.randbytes(20)))
    out.append(("cut end twice", b[max(L - 40, 0):L] * 2 + rng.randbytes(20)))
    return out


# ---- hand-built cases: a random (incompressible) dictionary, so that only the intended match exists ---------------------------------
def hand_cases():
    """[(name, dictionary, record, check)]: check(sequences of the REFERENCE's output) asserts that the intended sequence is there.
    Optional fifth element: the byte the arena holds in front of the dictionary's kept tail (test_dictc_hostsim.py)"""
    rng = random.Random(4242)
    d = rng.randbytes(4096)          # 4096 = 1 mod 3: the stride positions 0, 3, .. end at L - 10
    L = len(d)
    out = []

    def has(seq):
        return lambda seqs: seq in seqs or pytest_fail("%r not in %r" % (seq, seqs[:8]))

    def no_dict_match(seqs):
        assert all(off <= pos for pos, off, ml in seqs), seqs[:8]

    def some_dict_match(seqs):
        assert any(off > pos for pos, off, ml in seqs), seqs[:8]

    # a match that runs over the dictionary's end into the record's own start
    out.append(("over the end", d, d[-40:] * 2 + rng.randbytes(30), has((0, 40, 80))))
    out.append(("over the end, to matchlimit", d, d[-40:] * 3, has((0, 40, 115))))
    # the dictionary's last k bytes: positions L-7 .. L-1 are never inserted, and with L = 1 mod 3 neither are L-8 and L-9
    for k in range(7, 13):
        out.append(("last %d bytes" % k, d, rng.randbytes(20) + d[-k:] + rng.randbytes(20), no_dict_match if k < 10 else some_dict_match))
    # dictionary positions off the stride of 3: a later stride position hits, the match is extended backwards
    for k in (0, 1, 2):
        out.append(("stride +%d" % k, d, rng.randbytes(16) + d[999 + k:999 + k + 20] + rng.randbytes(20), has((16, 3113 - k, 20))))
    # the dictionary's first byte behind one literal: the catch-up stops at the start of the kept tail (whose arena neighbour is that
    # literal); with 65537 bytes the tail starts at d[1], index 0, which the distance rule keeps out of reach -- and a 64 KB dictionary
    # has overwritten the buckets of its early positions many times over --: no match at all
    x = bytes([d[0] ^ 0xFF])
    out.append(("tail start, L=4096", d, x + d[:30] + rng.randbytes(20), has((1, 4097, 30)), x))
    d2 = rng.randbytes(65537)
    out.append(("tail start, L=65537", d2, d2[:1] + d2[1:31] + rng.randbytes(20), no_dict_match))
    # the same content in the dictionary and earlier in the block: the latest insert wins
    w = d[300:354]
    out.append(("dictionary versus block", d, w + w + rng.randbytes(20), lambda seqs: (has((0, L - 300, 54))(seqs), has((54, 54, 54))(seqs))))
    # a dictionary copy behind more than 65535 bytes of compressible filler is out of reach
    filler = bytes(rng.choice(b"ab") for _ in range(66000))
    def far(seqs):
        assert seqs and all(off <= pos for pos, off, ml in seqs if pos >= 65536), [q for q in seqs if q[0] >= 65536][:8]
    out.append(("out of reach", d, filler + d[1000:1040] + rng.randbytes(20), far))
    # the whole dictionary inside the record, at the smallest lengths that load
    for n in (8, 9, 16):
        dn = rng.randbytes(n)
        out.append(("whole dictionary, L=%d" % n, dn, rng.randbytes(20) + dn + rng.randbytes(20), has((20, 20 + n, n))))
    return out


def pytest_fail(msg):
    raise AssertionError(msg)


def check_hand_cases(rd):
    """every hand-built case against the reference's own output: the intended sequence is there"""
    for c in hand_cases():
        r, by = ref_compress(rd, c[1], c[2])
        assert r > 0, c[0]
        try:
            c[3](parse(by))
        except AssertionError as e:
            raise AssertionError("hand-built case %r: %s" % (c[0], e))


def rng_for(seed):
    return random.Random(seed)


__all__ = ["BIG", "DICT_LENS", "RECORD_SIZES", "RefDict", "big_record", "book1", "book_records", "bound", "caps_for", "check_hand_cases",
           "dict_cuts", "hand_cases", "keep_of", "other_records", "parse", "ref_compress", "rng_for"]
