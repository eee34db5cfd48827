"""Shared pieces of the HC linked-block compressor's tests (test_hcchain_hostsim.py, test_hcchain_abi.py, test_gpu_hcchain.py): the
reference library's own stream calls through ctypes (LZ4_createStreamHC / LZ4_resetStreamHC_fast / LZ4_loadDictHC /
LZ4_compress_HC_continue over one contiguous buffer: prefix mode), the case set and the layout of one call.  The chains are
cchain_common's CChain records.  The expected value of every case is what the reference library returns and writes -- never this
project's output.  A block whose result is 0 does not end its chain here: the loop goes on, and a block with a negative src_len
counts as 0 bytes, so its bytes are not part of the chain's source."""
import ctypes as C
import random

from cchain_common import GUARD, PREFIXES, CChain, CPacked, book1, book_chains, bound, chain_of, hand_chains, prefix_chains
from dictc_common import parse

LEVELS = (1, 3, 4, 8, 9, 10, 12)       # on chains of up to SMALL bytes
BIG_LEVELS = (9, 10)                   # on the larger ones
CLAMPS = ((0, 9), (13, 12))            # (level asked for, level it means)
SMALL = 20000


def clamp(level):
    return 9 if level < 1 else min(level, 12)


def source_of(ch):
    """the chain's contiguous source: the bytes of its blocks whose src_len is not negative"""
    return b"".join(s for (s, _), sl in zip(ch.blocks, ch.lens) if sl >= 0)


class RefHCChain:
    """the reference library's HC stream entry points; results are kept (one computation per chain and level)"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStreamHC.restype = C.c_void_p
        L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
        L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
        L.LZ4_loadDictHC.restype = C.c_int
        L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_compress_HC_continue.restype = C.c_int
        L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        self.memo = {}

    def _stream(self, level, base, P):
        st = self.L.LZ4_createStreamHC()
        self.L.LZ4_resetStreamHC_fast(st, level)
        if P > 0:
            self.L.LZ4_loadDictHC(st, base, P)
        return st

    def compress(self, ch, level, fresh=False):
        """-> (out_len per block, [bytes per block]): LZ4_createStreamHC, LZ4_resetStreamHC_fast(level), LZ4_loadDictHC of the history
        if there is any, then LZ4_compress_HC_continue block by block over the contiguous source.  A block that returns 0 does not
        stop the loop; a negative src_len or dst_cap gives 0 without a call (the block's source, if its length is not negative, is
        taken into the stream with a call at capacity 0, which is what liblz4 does with a block that fails).  fresh = True (fact 1,
        not the contract): every block on a stream of its own that has loaded everything in front of it"""
        key = (id(ch), level, fresh)
        got = self.memo.get(key)
        if got is not None and got[0] is ch:
            return got[1]
        L = self.L
        P = len(ch.history)
        data = source_of(ch)
        buf = C.create_string_buffer(GUARD + P + len(data) + GUARD)
        base = C.addressof(buf) + GUARD
        C.memmove(base, ch.history + data, P + len(data))
        st = self._stream(level, base, P)
        outs, by, pos = [], [], 0
        for (s, cap), sl in zip(ch.blocks, ch.lens):
            if sl < 0:
                outs.append(0); by.append(b"")
                continue
            if fresh:
                L.LZ4_freeStreamHC(st)
                st = self._stream(level, base, P + pos)
            dst = C.create_string_buffer(max(cap, 1) + 8)
            r = L.LZ4_compress_HC_continue(st, base + P + pos, dst, sl, max(cap, 0))
            assert 0 <= r <= max(cap, 0)
            outs.append(r)
            by.append(dst.raw[:r])
            pos += sl
        L.LZ4_freeStreamHC(st)
        self.memo[key] = (ch, (outs, by))
        return outs, by


# ---- the case set ----
def hc_hand_chains(rng):
    """hand-built data for HC in prefix mode -> [(chain, check or None)]; check(sequences of the REFERENCE's level 9 output of the
    chain's last block) asserts the sequence the case is about"""
    out = []

    def has(*want):
        def chk(seqs):
            for q in want:
                assert q in seqs, "%r not in %r" % (q, seqs[:8])
        return chk

    def both(name, hist, blocks, chk):
        data = b"".join(blocks)
        out.append((chain_of(name + " (history = prefix)", data, [len(x) for x in blocks], history=hist), chk))
        out.append((chain_of(name + " (history = block)", hist + data, [len(hist)] + [len(x) for x in blocks]), chk))

    # a match that starts in the history and runs into the block: the history's last 40 bytes, twice
    h = rng.randbytes(300)
    both("from the history into the block", h, [h[-40:] * 2 + rng.randbytes(30)], has((0, 40, 80)))
    both("from the history into the block, to matchlimit", h, [h[-40:] * 3], has((0, 40, 115)))
    # a copy of the previous block's last k bytes: its last three positions are inserted late, with bytes of THIS block in their
    # hashes, and are candidates here (they are none behind a dictionary)
    for k in (3, 4, 5):
        h = rng.randbytes(500)
        lead = rng.randbytes(20)
        both("the last %d bytes of the history" % k, h, [lead + h[-k:] + rng.randbytes(20)], has((20, 20 + k, k)) if k >= 4 else None)
    # the history's last three bytes, then this block's own first ten: 13 bytes that match at history position -3, a late-inserted one
    h = rng.randbytes(500)
    r0 = rng.randbytes(20)
    both("a late-inserted position is a candidate", h, [r0 + h[-3:] + r0[:10] + rng.randbytes(20)], has((20, 23, 13)))
    # lazy evaluation: the first match (8 history bytes from 2000) is found at 20; the wider search from 26 finds the history at 1004
    # and extends it backwards over 25 .. 22, which leaves the first match two bytes: it is dropped
    d = bytearray(rng.randbytes(4096))
    d[2002:2008] = d[1000:1006]
    d = bytes(d)
    both("a lazy match widened backwards into the history", d, [rng.randbytes(20) + d[2000:2002] + d[1000:1050] + rng.randbytes(20)],
         has((22, 22 + len(d) - 1000, 50)))
    # a match whose backward extension stops at the block's first byte although the history goes on matching
    h = rng.randbytes(200)
    both("backward extension stops at the anchor", h, [h[100:160] + rng.randbytes(20)], has((0, 100, 60)))
    return out


def pattern_chains():
    """200 chains of runs of a short unit (after hcdict_common.pattern_cases): the runs lie across block boundaries, and every fifth
    chain has a history longer than 64 KB"""
    rng = random.Random(4343)
    out = []
    for i in range(200):
        unit = rng.choice([b"a", b"ab", b"abcd", b"\0"])

        def run(units):
            r = rng.randrange(len(unit))
            return (unit * (units + 1))[r:r + units * len(unit)]

        hist = rng.randbytes(rng.choice([0, 50, 3000])) + unit * rng.randrange(2, 400)
        if i % 5 == 0:
            hist = rng.randbytes(100) + run(rng.randrange(2, 300)) + rng.randbytes(67000 - (i % 3) * 400) + hist
        if i % 10 < 3:
            hist += rng.randbytes(rng.randrange(1, 4))
        data = run(rng.randrange(0, 200)) + rng.randbytes(rng.randrange(1, 9)) + run(rng.randrange(2, 400)) + rng.randbytes(rng.randrange(1, 9)) + \
            run(rng.randrange(2, 300)) + rng.randbytes(13)
        cuts = sorted(rng.randrange(0, len(data) + 1) for _ in range(rng.randrange(1, 4)))   # anywhere: inside the runs, mostly
        sizes = [b - a for a, b in zip([0] + cuts, cuts + [len(data)])]
        out.append(chain_of("pattern %d" % i, data, sizes, history=hist))
    return out


def zero_chain():
    return chain_of("zeros 300000 in 4096", bytes(300000), [4096] * 73 + [300000 - 73 * 4096])


def capacity_chains(rc, chains, level=9):
    """capacities: the exact output size, one less on one middle block and on all, 0 and a negative capacity in the middle, a negative
    src_len in the middle.  The chain goes on behind a block that fails"""
    out = []
    for ch in chains:
        sizes = rc.compress(ch, level)[0]
        assert all(r > 0 for r in sizes), ch.name
        m = len(ch.blocks) // 2
        out.append(ch.with_caps(lambda i, c: sizes[i], "exact caps"))
        out.append(ch.with_caps(lambda i, c: sizes[i] - 1 if i == m else c, "cap - 1 at %d" % m))
        out.append(ch.with_caps(lambda i, c: sizes[i] - 1, "cap - 1"))
        out.append(ch.with_caps(lambda i, c: 0 if i == m else c, "cap 0 at %d" % m))
        out.append(ch.with_caps(lambda i, c: -1 if i == m else c, "cap -1 at %d" % m))
        out.append(CChain(ch.name + " src_len -1 at %d" % m, ch.blocks, ch.history, [(-1 if i == m else n) for i, n in enumerate(ch.lens)]))
    return out


def is_small(ch):
    return len(ch.history) + len(ch.data) <= SMALL


def levels_of(ch):
    return LEVELS + tuple(a for a, _ in CLAMPS) if is_small(ch) else BIG_LEVELS


_SET = {}


def case_set(rc):
    """every chain of the CPU and GPU tests (built once per process: the reference's results are kept by chain object)"""
    if "chains" not in _SET:
        rng = random.Random(51)
        books = book_chains()
        pre = prefix_chains()
        hand = hand_chains(rng) + [c for c, _ in hc_hand_chains(rng)]
        base = books + [c for P in PREFIXES for c in pre[P]] + hand
        small = [c for c in books + pre[0] + pre[100] + hand if is_small(c) and len(c.blocks) >= 2 and len(c.data) >= 64]
        _SET["chains"] = base + pattern_chains() + [zero_chain()] + capacity_chains(rc, small[::3])
    return _SET["chains"]


def expected(rc, chains, level):
    """[(out_len, [bytes per block])] per chain at `level`, from the reference"""
    return [rc.compress(c, clamp(level)) for c in chains]


class HCPacked(CPacked):
    """cchain_common.CPacked's layout of one call -- every chain's history and source in src with GUARD bytes of 0xA5 between the chains
    and at both ends, every block's slot of max(dst_cap, 0) bytes in dst with GUARD bytes of 0xA5 around it -- with the HC chain's
    source (a block with a negative src_len has no bytes in it) and a checker of its own: no consumed array, no stopped blocks"""

    def __init__(self, chains, fill=0x5A):
        self.chains, self.fill = chains, fill
        src = bytearray(b"\xA5" * GUARD)
        dst = bytearray(b"\xA5" * GUARD)
        self.chain_src_off, self.prefix, self.src_len, self.chain_first, self.dst_off, self.dst_cap = [], [], [], [0], [], []
        for ch in chains:
            src += ch.history
            self.chain_src_off.append(len(src)); self.prefix.append(len(ch.history))
            src += source_of(ch) + b"\xA5" * GUARD
            for (s, cap), sl in zip(ch.blocks, ch.lens):
                self.src_len.append(sl); self.dst_off.append(len(dst)); self.dst_cap.append(cap)
                dst += bytes([fill]) * max(cap, 0) + b"\xA5" * GUARD
            self.chain_first.append(len(self.src_len))
        self.src, self.dst = bytes(src), dst
        self.n_blocks, self.n_chains = len(self.src_len), len(chains)
        self.span = len(self.src) - GUARD

    def check(self, dst, out_len, want):
        """dst / out_len as the call left them against the reference's results `want` (expected()): the values, the bytes produced, and
        every byte the call must not have written -- the guards and, in each slot, what lies past the result (a block that does not
        fit has written the sequences that did, as liblz4 has: inside its slot)"""
        bad = []
        dst = bytes(dst)
        assert len(dst) == len(self.dst)
        if dst[:GUARD] != b"\xA5" * GUARD:
            bad.append(("front guard written",))
        for c, (ch, (outs, by)) in enumerate(zip(self.chains, want)):
            b0, b1 = self.chain_first[c], self.chain_first[c + 1]
            if [int(v) for v in out_len[b0:b1]] != outs:
                got = [int(v) for v in out_len[b0:b1]]
                k = next(i for i in range(b1 - b0) if got[i] != outs[i])
                bad.append((ch.name, "values", k, got[k], outs[k]))
                continue
            for i in range(b0, b1):
                o, cap, r = self.dst_off[i], max(self.dst_cap[i], 0), outs[i - b0]
                if dst[o:o + r] != by[i - b0]:
                    bad.append((ch.name, "bytes of block", i - b0))
                    break
                if r > 0 and dst[o + r:o + cap] != bytes([self.fill]) * (cap - r):
                    bad.append((ch.name, "written past the result", i - b0))
                    break
                if dst[o + cap:o + cap + GUARD] != b"\xA5" * GUARD:
                    bad.append((ch.name, "guard written", i - b0))
                    break
        return bad


def oracle_hcchain_engine(base, rc, **kw):
    """`base` (an oracle engine class of the stream tests) plus compressHCChain served by the reference library: the engine the writer
    logic of LZ4FrameOutputStream(linkedBlocks=True, level=N) is tested with on the CPU"""

    class HCChainOracleEngine(base):
        hcchain_calls = 0

        def compressHCChain(self, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None, level=9):
            type(self).hcchain_calls += 1
            outs = []
            for c in range(len(chainSrcOff)):
                b0, b1, off = chainFirst[c], chainFirst[c + 1], chainSrcOff[c]
                P = chainPrefixLen[c] if chainPrefixLen is not None else 0
                blocks, o = [], off
                for i in range(b0, b1):
                    blocks.append((bytes(src[o:o + srcLen[i]]), dstCap[i]))
                    o += srcLen[i]
                r, by = rc.compress(CChain("frame", blocks, history=bytes(src[off - P:off])), clamp(level))
                for i, x in zip(range(b0, b1), by):
                    dst[dstOff[i]:dstOff[i] + len(x)] = x
                outs += r
            return outs

    return HCChainOracleEngine(**kw)


def hc_linked_frame(rc, xxh32, data, block_id, level, block_checksum=False, content_checksum=False):
    """the frame LZ4FrameOutputStream(linkedBlocks=True, level=level) must write, whatever its batchBlocks, assembled from the reference:
    ONE stream over the whole data (LZ4_compress_HC_continue block by block); a block that does not shrink is stored raw and is
    history all the same"""
    import struct
    bs = 1 << (2 * block_id + 8)
    flg = (1 << 6) | (16 if block_checksum else 0) | (4 if content_checksum else 0)
    desc = bytes([flg, block_id << 4])
    out = bytearray(struct.pack("<I", 0x184D2204) + desc + bytes([(xxh32(desc, 0) >> 8) & 0xFF]))
    sizes = [min(bs, len(data) - o) for o in range(0, len(data), bs)]
    outs, by = rc.compress(chain_of("frame", data, sizes), clamp(level))
    o = 0
    for n, s in zip(sizes, by):
        raw = len(s) >= n
        payload = data[o:o + n] if raw else s
        out += struct.pack("<I", len(payload) | (0x80000000 if raw else 0)) + payload
        if block_checksum:
            out += struct.pack("<I", xxh32(payload, 0))
        o += n
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", xxh32(data, 0))
    return bytes(out)


__all__ = ["BIG_LEVELS", "CLAMPS", "HCPacked", "LEVELS", "RefHCChain", "SMALL", "capacity_chains", "case_set", "clamp", "expected",
           "hc_hand_chains", "hc_linked_frame", "is_small", "oracle_hcchain_engine", "levels_of", "parse", "pattern_chains", "source_of", "zero_chain"]
