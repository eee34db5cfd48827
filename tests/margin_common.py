"""Boundary streams for the decoders' end-of-block margins (test_margin_hostsim.py, test_gpu_margins.py).

Every interior decode loop runs a sequence without liblz4's per-sequence checks while ip <= iend - LZ4HIP_DECODE_IN_MARGIN (306) and
op <= oend - LZ4HIP_DECODE_OUT_MARGIN (606) (lz4-java_amd/csrc/lz4_decode_core.h).  liblz4's own output never puts a long sequence
near a block's end, so the streams here are hand-assembled: a PROLOGUE (more than 2 KB of stream, more than 4 KB of output, so that
every loop is running and an offset of 4096 has a source; one variant with more than 65535 bytes of history), one PROBE sequence
whose literal run, match length and offset come from a grid around the values at which a length takes one more extension byte, placed
so that it STARTS d bytes from the position at which a loop decides to stay or leave, and an EPILOGUE of short sequences and last
literals that keeps liblz4's end rules.  build_stream asserts nothing itself; CaseSet asserts with the reference library that every
stream decodes to exactly its size, and the count of every part.

Which end "binds" is the mode's:
  a  exact capacity: both ends of the block at once (where no valid stream has both placements, one stream for each)
  b  capacity short by SHORT_BY: the output end arrives mid-stream, the reference's negative code is the expected value.  FAR_SHORT is
     this file's addition: with 3000 bytes cut, 2 KB and more of stream lie ahead of the probe, which the deep, ring, wave, pair and
     trio loops need to be running at all -- the only placement at which THEIR output test decides
  c  capacity long by LONG_BY: the input end binds
  d  the fast decoder, src_cap = stream length + FAST_EXTRA: expected values from the oracle's bounded fast decoder
  e  partial decode, the target at the probe's start + d
  f  the same block behind a dictionary, the probe's offset reaching into it (wholly, or straddling the block's start)
  g  the same block as the second block of a chain, the probe's offset reaching into the first
  h, i  (this file's addition) the stream cut CUT_LEFT bytes behind the probe's start, safe and fast decoder: the one way the input
     test of a loop can be wrong about a sequence it runs, since a valid stream ends 6 bytes or more behind its last sequence

What a valid stream cannot hold is placed as near as it can: a probe that consumes 277 bytes cannot start 241 bytes in front of its
stream's end (d = 65 of the input placement) -- it starts where the shortest epilogue (a token and five literals; behind a literal
run that needs liblz4's twelve bytes, more) lets it.  No grid point is dropped: such a point keeps its place in every list and the
CaseSet counts them (`clamped`).

Expected values come from the reference library and the oracle's port of the fast decoder alone."""
import random
from typing import NamedTuple

LITS = (0, 14, 15, 268, 269, 270)
MLS = (4, 18, 19, 272, 273, 274)
PAST = "past"                      # an offset of literals + 1: the source starts one byte in front of the probe's own literals
OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, PAST, 4096, 65535)
DS = (-65, -64, -17, -16, -1, 0, 1, 16, 63, 64, 65)
NEAR_DS = (-1, 0, 1)
# The pairs that get every offset at every d: the four corners of the grid -- (0, 274), (270, 4) and (270, 274) hold a length of two
# extension bytes, which every loop must hand to the exact code wherever it stands -- and the corners of what an interior loop RUNS (one
# extension byte per length): (269, 273) is the longest sequence a loop takes, the one a weakened margin lets past a block's end.
CORNERS = ((0, 4), (0, 274), (270, 4), (270, 274), (0, 273), (269, 4), (269, 273))
IN_MARGIN, OUT_MARGIN = 306, 606   # the values of lz4_decode_core.h, restated: the placements are the issue's, not the header's
SHORT_BY = (1, 5, 64, 541, 542, 543, 606, 607)
FAR_SHORT = 3000
LONG_BY = (1, 64, 700)
FAST_EXTRA = (0, 3, 16)
SEED = 20261020


def _ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)
    return bytes(out)


def ext_bytes(length, base):
    """how many extension bytes a length takes (base: 0 for literals, 4 for a match)"""
    return 0 if length - base < 15 else 1 + (length - base - 15) // 255


def seq(lit, ml, off, rng):
    """one sequence: `lit` literals from rng, a match of ml >= 4 bytes at distance off"""
    tok = (min(lit, 15) << 4) | min(ml - 4, 15)
    return bytes([tok]) + (_ext(lit - 15) if lit >= 15 else b"") + rng.randbytes(lit) + bytes([off & 255, off >> 8]) + \
        (_ext(ml - 19) if ml >= 19 else b"")


def seq_in(lit, ml):
    return 1 + ext_bytes(lit, 0) + lit + 2 + ext_bytes(ml, 4)


def last_literals(n, rng):
    return bytes([min(n, 15) << 4]) + (_ext(n - 15) if n >= 15 else b"") + rng.randbytes(n)


def last_in(n):
    return 1 + ext_bytes(n, 0) + n


# ---- epilogue: sequences (lit, ml) and last literals that produce exactly out_e bytes from exactly in_e bytes -----------------------
def _sequences(i, o):
    """[(lit, ml)] that consume i and produce o bytes, or None.  Short sequences (literals <= 14, match <= 18) where the numbers allow,
    literal runs of up to 200 bytes where the input is long, one long match where the output is"""
    S = o - i           # a sequence produces at least as much as it consumes
    if i < 0 or S < 0:
        return None
    if i == 0:
        return [] if o == 0 else None
    seqs = []
    if S > 0:
        a = -(-S // 15)
        if 3 * a <= i:
            parts = [S // a + (1 if k < S % a else 0) for k in range(a)]
            seqs = [[0, 3 + p] for p in parts]
        else:                                   # one long match: ml - 3 - its extension bytes = S
            for e in range(1, 8):
                ml = S + 3 + e
                if ext_bytes(ml, 4) == e and 3 + e <= i:
                    seqs = [[0, ml]]
                    break
            else:
                return None
    rem = i - sum(seq_in(l, m) for l, m in seqs)
    room = 14 * sum(1 for l, m in seqs if m <= 18)
    runs = []
    while rem > room:                           # literal runs of 15 .. 200 bytes with a minimal match: in = out = run + 4
        if rem < 19:
            return None
        take = min(rem, 204)
        if 0 < rem - take <= room:
            pass
        elif 0 < rem - take < 19:
            take = rem - 19
        if take < 19:
            return None
        runs.append([take - 4, 4])
        rem -= take
    for s in seqs:
        if s[1] <= 18 and rem:
            add = min(14, rem)
            s[0] += add; rem -= add
    if rem:
        return None
    return [tuple(s) for s in runs + seqs]


def epilogue(out_e, in_e, ml=12):
    """-> ([(lit, ml)], last literals) with exactly these sizes behind a match of ml bytes, or None"""
    if out_e is None or in_e is None:
        return None
    for ll in (5, 6, 7):                                       # last literals alone (liblz4: the literals in front of the last match end >= 12 bytes from the end)
        if (out_e, in_e) == (ll, ll + 1) and ml + ll >= 12:
            return [], ll
    for ll in list(range(8, 15)) + list(range(15, 60)):       # (>= 8: a literal run in front of the last match ends >= 12 bytes from the end)
        if (out_e, in_e) == (ll, last_in(ll)):
            return [], ll
        s = _sequences(in_e - last_in(ll), out_e - ll)
        if s:
            return s, ll
    return None


class Stream(NamedTuple):
    data: bytes        # the stream
    n: int             # its decoded size
    p_ip: int          # where the probe starts in the stream
    p_op: int          # and in the output
    lit: int
    ml: int
    off: int
    out_tail: int      # n - p_op
    in_tail: int       # len(data) - p_ip


class Builder:
    """streams by (lit, ml, off, out_tail, in_tail); the two prologues are built once"""

    def __init__(self):
        self._pro = {}
        self._cache = {}

    def prologue(self, long_history):
        if long_history not in self._pro:
            rng = random.Random(SEED + (1 if long_history else 0))
            c, n = bytearray(), 0
            if long_history:                 # 100 literals repeated over 66000 bytes: a few hundred bytes of stream, > 65535 bytes of history
                c += seq(100, 66000, 100, rng); n += 66100
            c += seq(70, 8, 3, rng); n += 78
            for k in range(340):
                lit, ml = 1 + k % 13, 4 + (k * 7) % 15
                c += seq(lit, ml, 1 + (k * 37) % min(n + lit, 1500), rng); n += lit + ml
            self._pro[long_history] = (bytes(c), n)
        return self._pro[long_history]

    def build(self, lit, ml, off, out_tail, in_tail, reach=None):
        """the stream in which the probe (lit, ml, off) starts out_tail bytes in front of the decoded end and in_tail bytes in front of
        the stream's end, or None.  reach: the probe's offset is p_op + lit + reach instead (it reaches that far in front of the block)"""
        key = (lit, ml, off, out_tail, in_tail, reach)
        if key not in self._cache:
            self._cache[key] = self._build(*key)
        return self._cache[key]

    def _build(self, lit, ml, off, out_tail, in_tail, reach):
        ep = epilogue(out_tail - lit - ml, in_tail - seq_in(lit, ml), ml)
        if ep is None:
            return None
        pro, n = self.prologue(off == 65535)
        rng = random.Random("%d %r" % (SEED, (lit, ml, off, out_tail, in_tail, reach)))
        o = lit + 1 if off == PAST else off
        if reach is not None:
            o = n + lit + reach
        assert 1 <= o <= 65535 and (reach is not None or o <= n + lit)
        c = bytearray(pro)
        p_ip, p_op = len(c), n
        c += seq(lit, ml, o, rng); n += lit + ml
        for l, m in ep[0]:
            c += seq(l, m, 9, rng); n += l + m
        c += last_literals(ep[1], rng); n += ep[1]
        assert n - p_op == out_tail and len(c) - p_ip == in_tail
        return Stream(bytes(c), n, p_ip, p_op, lit, ml, o, out_tail, in_tail)

    # -- placements ---------------------------------------------------------------------------------------------------------------
    def min_tails(self, lit, ml):
        """the nearest a valid stream lets the probe start to its two ends: (out_tail, in_tail)"""
        return lit + max(ml + 5, 12), seq_in(lit, ml) + max(6, 13 - ml)

    def place(self, lit, ml, off, out_tail=None, in_tail=None, reach=None):
        """-> (streams, clamped): the probe placed out_tail / in_tail bytes from the ends (None: wherever a natural epilogue puts it), each
        moved to the nearest value a valid stream has.  Both given and no stream has both: one stream per placement."""
        mo, mi = self.min_tails(lit, ml)
        clamped = False
        if out_tail is not None and out_tail < mo:
            out_tail, clamped = mo, True
        if in_tail is not None and in_tail < mi:
            in_tail, clamped = mi, True
        if out_tail is not None and in_tail is not None:
            s = self.build(lit, ml, off, out_tail, in_tail, reach)
            if s:
                return [s], clamped
            a, _ = self.place(lit, ml, off, out_tail, None, reach)
            b, _ = self.place(lit, ml, off, None, in_tail, reach)
            return a + b, clamped
        pin = seq_in(lit, ml)
        if out_tail is not None:
            oe = out_tail - lit - ml
            tries = [oe * 3 // 4, oe // 2, oe * 9 // 10, oe // 3, oe + 1, oe + 2] + [oe - k for k in range(0, 40)]
            for ie in tries:
                s = self.build(lit, ml, off, out_tail, pin + ie, reach) if ie >= 6 else None
                if s:
                    return [s], clamped
        else:
            ie = in_tail - pin
            tries = [ie * 3 // 2, ie * 2, ie + 20, ie * 3] + [ie + k for k in range(-2, 60)]
            for oe in tries:
                s = self.build(lit, ml, off, lit + ml + oe, in_tail, reach) if oe >= 5 else None
                if s:
                    return [s], clamped
        raise AssertionError(("no stream for", lit, ml, off, out_tail, in_tail))


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
def grid():
    """[(lit, ml, off, d_out, d_in)]: every literal x match pair at d_out, d_in in {-1, 0, 1} (offsets in rotation), then the CORNERS
    pairs with every offset at every d -- once on the output side (d, 0), once on the input side (0, d)"""
    pts, k = [], 0
    for lit in LITS:
        for ml in MLS:
            for do in NEAR_DS:
                for di in NEAR_DS:
                    pts.append((lit, ml, OFFSETS[k % len(OFFSETS)], do, di)); k += 1
    for lit, ml in CORNERS:
        for off in OFFSETS:
            for d in DS:
                pts.append((lit, ml, off, d, 0))
                if d:
                    pts.append((lit, ml, off, 0, d))
    return pts


GRID_POINTS = 36 * 9 + len(CORNERS) * 15 * (2 * 11 - 1)


class Case(NamedTuple):
    mode: str          # "a" .. "g"
    s: Stream
    cap: int           # a, b, c, f, g: the capacity; d: the decoded size; e: the capacity (the decoded size)
    aux: object        # d: src_cap; e: the target; f: the dictionary; g: the first block's size; h, i: the bytes of stream given; else None
    tag: tuple


MODES = "abcdefghi"
# modes h and i (this file's addition; the issue's modes are all valid streams, and in a valid stream a sequence that consumes 274 bytes
# starts 280 or more in front of the end -- the input margin would have no case that tells 273 from 306): the probes and how many bytes of
# stream are left from the probe's start on
CUT_PROBES = ((269, 273), (269, 4), (257, 18), (0, 273), (15, 19))
CUT_LEFT = tuple(range(273, 308))
# mode b, this file's addition: the longest simple sequence, and the one whose match ends one byte into a 64-byte step, at EVERY d of
# 1 .. 65 on the output side -- a loop whose stores run k bytes past a match's end needs 542 + k, and only the placement 606 - (542 + k)
# shows whether it has them (profiles/decode_margin_audit.txt)
SWEEP_PROBES = ((269, 273), (269, 257))
SWEEP_OFFSETS = (1, 4096)
SWEEP_CUTS = (64, FAR_SHORT)


def source(case):
    """modes a .. d, h, i: (the bytes of the source slot, safe decoder?)"""
    if case.mode == "d":
        return fast_slot(case), False
    if case.mode in "hi":
        return case.s.data[:case.aux], case.mode == "h"
    return case.s.data, True


def fast_slot(case):
    """mode d: the source slot of exactly src_cap bytes (the stream and 0xFF behind it)"""
    return case.s.data + b"\xFF" * (case.aux - len(case.s.data))


class CaseSet:
    """every case with its expected value, computed once: want[i] = (return code, bytes) -- g: (out_len list, chain length, bytes)"""

    def __init__(self, ref, O):
        from chain_common import Chain, RefChain, lit_block
        from dict_common import RefDict
        from partial_common import ref_partial
        B = self.B = Builder()
        pts = grid()
        assert len(pts) == GRID_POINTS, (len(pts), GRID_POINTS)
        cases, self.clamped = [], 0
        for k, (lit, ml, off, do, di) in enumerate(pts):
            # a: both ends
            ss, cl = B.place(lit, ml, off, OUT_MARGIN - do, IN_MARGIN - di)
            self.clamped += cl
            cases += [Case("a", s, s.n, None, (k, do, di)) for s in ss]
            # b: the output end mid-stream (points of the output side and the near grid)
            if di in NEAR_DS:
                cut = (SHORT_BY + (FAR_SHORT,))[k % 9]
                if OUT_MARGIN - do + cut < lit + ml + 12:     # (no stream is that short behind its probe: the next cut that has one)
                    cut = 64
                if cut == FAR_SHORT:
                    ss, cl = B.place(lit, ml, off, OUT_MARGIN - do + cut, OUT_MARGIN - do + cut - 320)
                else:
                    ss, cl = B.place(lit, ml, off, OUT_MARGIN - do + cut, None)
                assert not cl and len(ss) == 1
                cases.append(Case("b", ss[0], ss[0].n - cut, None, (k, do, cut)))
            if do in NEAR_DS:
                # c: the input end (points of the input side and the near grid)
                ss, cl = B.place(lit, ml, off, None, IN_MARGIN - di)
                cases.append(Case("c", ss[0], ss[0].n + LONG_BY[k % 3], None, (k, di, LONG_BY[k % 3])))
                # d: the fast decoder on the same stream
                cases.append(Case("d", ss[0], ss[0].n, len(ss[0].data) + FAST_EXTRA[(k // 3) % 3], (k, di)))
        for lit, ml in SWEEP_PROBES:
            for off in SWEEP_OFFSETS:
                for d in range(1, 66):
                    for cut in SWEEP_CUTS:
                        tail = OUT_MARGIN - d + cut
                        ss, cl = B.place(lit, ml, off, tail, tail - 320 if cut == FAR_SHORT else None)
                        assert not cl and len(ss) == 1
                        cases.append(Case("b", ss[0], ss[0].n - cut, None, ("sweep", d, cut, lit, ml, off)))
        # e: partial decode around the probe's start: every pair at d in {-1, 0, 1}, the corners with every offset at every d
        k = 0
        for lit in LITS:
            for ml in MLS:
                for d in NEAR_DS:
                    s = B.place(lit, ml, OFFSETS[k % len(OFFSETS)], OUT_MARGIN, IN_MARGIN)[0][0]; k += 1
                    cases.append(Case("e", s, s.n, s.p_op + d, (lit, ml, d)))
        for lit, ml in CORNERS:
            for off in OFFSETS:
                s = B.place(lit, ml, off, OUT_MARGIN, IN_MARGIN)[0][0]
                cases += [Case("e", s, s.n, s.p_op + d, (lit, ml, off, d)) for d in DS]
        # f, g: the probe's offset reaches `reach` bytes in front of the block: a match wholly in front of it, and one that straddles its start
        rng = random.Random(SEED + 7)
        self.dicts = {n: rng.randbytes(n) for n in (400, 70000)}
        reaches = []
        for lit in LITS:
            for ml in MLS:
                for d in NEAR_DS:
                    reaches.append((lit, ml, (ml + 40, 8)[(lit + ml + d) % 2], d, d))
        for lit, ml in CORNERS:
            for d in DS:
                for reach in (ml + 40, 8):
                    reaches.append((lit, ml, reach, d, 0))
                    reaches.append((lit, ml, reach, 0, d))
        for k, (lit, ml, reach, do, di) in enumerate(reaches):
            for s in B.place(lit, ml, 0, OUT_MARGIN - do, IN_MARGIN - di, reach=reach)[0]:
                cases.append(Case("f", s, s.n, (400, 70000)[k % 5 == 0], (lit, ml, reach, do, di)))
                cases.append(Case("g", s, s.n, 400, (lit, ml, reach, do, di)))
        # h, i: the stream CUT `left` bytes behind the probe's start (safe decoder: src_len, fast decoder: src_cap): the input end where no
        # valid stream has it
        for lit, ml in CUT_PROBES:
            for off in (1, 4096):
                s = B.place(lit, ml, off, 2000, None)[0][0]
                for left in CUT_LEFT:
                    cases.append(Case("h", s, s.n, s.p_ip + left, (lit, ml, off, left)))
                    cases.append(Case("i", s, s.n, s.p_ip + left, (lit, ml, off, left)))
        self.cases = cases
        self.by_mode = {m: [c for c in cases if c.mode == m] for m in MODES}
        # ---- the reference's word on every case
        rp, rd, self.rc = ref_partial(ref), RefDict(ref), RefChain(ref)
        self.first_block = lit_block(400, random.Random(SEED + 8))
        self.chain = lambda c: Chain("margin", [(self.first_block, False, 400), (c.s.data, False, c.cap)])
        valid = set()
        self.want = []
        for c in cases:
            if c.mode in "abc":
                if id(c.s) not in valid:
                    r, d = ref.decompress_safe_raw(c.s.data, c.s.n)
                    assert r == c.s.n, ("not a valid stream", c.mode, c.tag, c.s[1:], r)
                    valid.add(id(c.s))
                r, d = ref.decompress_safe_raw(c.s.data, c.cap)
                assert (r == c.s.n) if c.mode in "ac" else r < 0, (c.mode, c.tag, r)
                self.want.append((r, d[:max(r, 0)]))
            elif c.mode == "h":
                r, d = ref.decompress_safe_raw(c.s.data[:c.aux], c.cap)
                assert r < 0, (c.tag, r)
                self.want.append((r, b""))
            elif c.mode == "i":
                r, d = O.decompress_fast_bounded(c.s.data[:c.aux], c.aux, c.cap)
                assert r < 0, (c.tag, r)
                self.want.append((r, d))
            elif c.mode == "d":
                r, d = O.decompress_fast_bounded(fast_slot(c), c.aux, c.cap)
                assert r == len(c.s.data) and (r, d) == ref.decompress_fast_raw(c.s.data, c.cap), (c.tag, r)
                self.want.append((r, d))
            elif c.mode == "e":
                assert ref.decompress_safe_raw(c.s.data, c.s.n)[0] == c.s.n
                self.want.append(rp(c.s.data, c.aux, c.cap))
                assert self.want[-1][0] == c.aux, (c.tag, self.want[-1][0])
            elif c.mode == "f":
                r, d = rd.decode(c.s.data, c.cap, self.dicts[c.aux])
                assert r == c.s.n, ("not a valid stream behind its dictionary", c.tag, r)
                self.want.append((r, d))
            else:
                outs, done, data = self.rc.decode(self.chain(c))
                assert outs == [400, c.s.n] and done == 400 + c.s.n, (c.tag, outs)
                self.want.append((outs, done, data))
        self.counts = {m: len(v) for m, v in self.by_mode.items()}


# ---- the two host images of a device batch -----------------------------------------------------------------------------------------
FILL = 0xA5
MIN_GUARD = 128


def image(sizes, start_mod=(0, 1, 127, 77)):
    """offsets of slots of these sizes in one image: slot k starts at an address = start_mod[k % 4] (mod 128) -- 0, 1, 127 and another odd
    one --, at least MIN_GUARD bytes of fill in front of, between and behind the slots.  -> (offsets, image size)"""
    off, p = [], MIN_GUARD
    for k, n in enumerate(sizes):
        p += (start_mod[k % len(start_mod)] - p) % 128
        off.append(p)
        p += n + MIN_GUARD
    return off, p


def check_guards(img, off, sizes, written, what):
    """every byte of the image outside [off[k], off[k] + written[k]) is still FILL"""
    import numpy as np
    a = np.frombuffer(img, dtype=np.uint8)
    keep = np.ones(len(a), dtype=bool)
    for o, w in zip(off, written):
        keep[o:o + w] = False
    bad = np.flatnonzero(keep & (a != FILL))
    if len(bad):
        p = int(bad[0])
        k = max((i for i, o in enumerate(off) if o <= p), default=-1)
        raise AssertionError((what, "a byte outside every result was written", "at", p, "slot", k, "slot offset", off[k] if k >= 0 else None,
                              "slot size", sizes[k] if k >= 0 else None, "written", written[k] if k >= 0 else None, len(bad)))
