"""Shared pieces of the linked-block decoder tests (test_chain_hostsim.py, test_chain_abi.py, test_chain_streams_host.py,
test_gpu_chain.py): the reference library's own stream calls through ctypes (LZ4_createStream / LZ4_compress_fast_continue for the
writers, LZ4_createStreamDecode / LZ4_setStreamDecode / LZ4_decompress_safe_continue for the expected values), the Chain record and
the case set.  The expected value of every case is what the reference library returns and writes -- never this project's output."""
import ctypes as C
import random

from conftest import calgary, lz4_seq
from partial_common import damaged

CHAIN_STOPPED = -(2 ** 31) + 6          # include/lz4hip.h LZ4HIP_CHAIN_STOPPED
OFFSET_RULE_P = (1, 100, 65533, 65534, 65535, 65536, 70000)
STRADDLE_DISTANCES = (1, 2, 3, 7, 8, 15)
GUARD = 64


def book1():
    return calgary("book1")


def rng_for(seed):
    return random.Random(seed)


class Chain:
    """one chain: blocks = [(stream, stored, dst_cap)], `history` = the bytes in front of the chain's destination (its length is
    prefix_len), ccap = chain_dst_cap"""

    def __init__(self, name, blocks, history=b"", ccap=None):
        self.name, self.blocks, self.history = name, [(bytes(s), bool(st), int(cap)) for s, st, cap in blocks], bytes(history)
        self.ccap = sum(max(c, 0) for _, _, c in self.blocks) if ccap is None else ccap

    def with_caps(self, f, name):
        return Chain(self.name + " " + name, [(s, st, f(i, cap)) for i, (s, st, cap) in enumerate(self.blocks)], self.history, None)


class RefChain:
    """the reference library's stream entry points"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStream.restype = C.c_void_p
        L.LZ4_freeStream.argtypes = [C.c_void_p]
        L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.LZ4_createStreamDecode.restype = C.c_void_p
        L.LZ4_freeStreamDecode.argtypes = [C.c_void_p]
        L.LZ4_setStreamDecode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_decompress_safe_continue.restype = C.c_int
        L.LZ4_decompress_safe_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.LZ4_decompress_safe.restype = C.c_int
        L.LZ4_decompress_safe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def compress_chain(self, data, block_size):
        """data cut into block_size pieces, each compressed by LZ4_compress_fast_continue on ONE stream over the contiguous source
        (liblz4's prefix mode): -> [(stream, decoded size)]"""
        L = self.L
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        st = L.LZ4_createStream()
        out = []
        for o in range(0, len(data), block_size):
            n = min(block_size, len(data) - o)
            dst = C.create_string_buffer(n + n // 255 + 32)
            r = L.LZ4_compress_fast_continue(st, C.addressof(src) + o, dst, n, len(dst), 1)
            assert r > 0
            out.append((dst.raw[:r], n))
        L.LZ4_freeStream(st)
        return out

    def compress_alone(self, data):
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        dst = C.create_string_buffer(len(data) + len(data) // 255 + 32)
        r = self.L.LZ4_compress_default(src, dst, len(data), len(dst))
        assert r > 0
        return dst.raw[:r]

    def plain(self, s, cap):
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)
        out = C.create_string_buffer(cap + 64)
        return self.L.LZ4_decompress_safe(buf, out, len(s), cap)

    def decode(self, ch):
        """-> (out_len per block, chain_out_len, the bytes decoded): LZ4_setStreamDecode(sd, chain_dst - prefix_len, prefix_len), then
        LZ4_decompress_safe_continue block by block, every destination where the previous one ended, with the capacity
        min(dst_cap, what is left of ccap).  A stored block is copied and the stream is told about the longer history; a negative
        result ends the chain"""
        L = self.L
        P = len(ch.history)
        buf = C.create_string_buffer(GUARD + P + ch.ccap + 64)
        base = C.addressof(buf) + GUARD
        C.memmove(base, ch.history, P)
        sd = L.LZ4_createStreamDecode()
        L.LZ4_setStreamDecode(sd, base, P)
        outs, done, alive = [], 0, True
        for s, stored, cap in ch.blocks:
            if not alive:
                outs.append(CHAIN_STOPPED)
                continue
            cap = min(cap, ch.ccap - done)
            if cap < 0:
                r = -1
            elif stored:
                r = len(s) if len(s) <= cap else -1
                if r >= 0:
                    C.memmove(base + P + done, s, len(s))
                    L.LZ4_setStreamDecode(sd, base, P + done + r)
            else:
                sb = C.create_string_buffer(s + b"\0" * 64, len(s) + 64)
                r = L.LZ4_decompress_safe_continue(sd, sb, base + P + done, len(s), cap)
            outs.append(r)
            if r < 0:
                alive = False
            else:
                done += r
        L.LZ4_freeStreamDecode(sd)
        return outs, done, C.string_at(base + P, done)


def lit_block(n, rng):
    """a block of n literals and nothing else"""
    b = bytearray()
    if n < 15:
        b.append(n << 4)
    else:
        b.append(0xF0)
        r = n - 15
        while r >= 255:
            b.append(255); r -= 255
        b.append(r)
    return bytes(b) + rng.randbytes(n)


def seq_block(seqs, last, rng):
    """a block of the sequences (lit, ml, off) and `last` (< 15) final literals -> (stream, decoded size)"""
    c, n = bytearray(), 0
    for lit, ml, off in seqs:
        c += lz4_seq(lit, ml, off, rng); n += lit + ml
    c += bytes([last << 4]) + rng.randbytes(last)
    return bytes(c), n + last


def both_ways(name, P, block, size, cap, rng):
    """the same block behind P bytes of history, supplied (a) as an earlier block of P literals and (b) as prefix_len: the results of the
    block must be equal"""
    h = rng.randbytes(P)
    first = lit_block(P, random.Random(0))
    first = first[:len(first) - P] + h
    return (Chain(name + " (history = block)", [(first, False, P), (block, False, cap)]),
            Chain(name + " (history = prefix)", [(block, False, cap)], history=h))


def offset_rule_chains(rng):
    """the issue's offset rule: first block of P literals, second block (1 literal, match 6, offset) + 6 literals = 13 bytes"""
    out = []
    for P in OFFSET_RULE_P:
        for off in (1 + P - 1, 1 + P, 1 + P + 1, 65535):
            if 1 <= off <= 65535:
                blk, n = seq_block([(1, 6, off)], 6, rng)
                assert n == 13
                out += both_ways("offset rule P=%d off=%d" % (P, off), P, blk, n, n, rng)
    return out


def end_rule_chains(rng):
    """a match that starts in the history obeys the ordinary end-of-block rules"""
    out = []
    for ml, caps in ((6, (12, 13)), (8, (14, 15))):
        blk, n = seq_block([(1, ml, 50)], 5, rng)
        for cap in caps:
            out += both_ways("end rule ml=%d cap=%d" % (ml, cap), 100, blk, n, cap, rng)
    return out


def straddle_chains(rng):
    """a match that starts d bytes in front of the block and runs into it: one overlapping copy"""
    out = []
    for d in STRADDLE_DISTANCES:
        for lit in (0, 1, 5):
            for ml in (4, 9, 40, 300, 700):
                for P in (d, 100, 70000):
                    blk, n = seq_block([(lit, ml, lit + d)], 12, rng)
                    out += both_ways("straddle d=%d lit=%d ml=%d P=%d" % (d, lit, ml, P), P, blk, n, n + (64 if ml == 40 else 0), rng)
    return out


def book_chains(rc):
    """chains the reference wrote from book1 with LZ4_compress_fast_continue: 1 .. 70 blocks of 1000 / 4096 / 65536 bytes (70 x 1000 and
    17+ x 4096 cross P = 65535 mid-chain), whole and with their first blocks supplied as history"""
    b = book1()
    out = []
    for bs, counts in ((1000, (1, 2, 3, 16, 67, 70)), (4096, (1, 2, 5, 17, 70)), (65536, (1, 2, 3, 11))):
        for k in counts:
            o = (bs * 7 + k * 1013) % 100000
            data = b[o:o + bs * k]
            blocks = rc.compress_chain(data, bs)
            out.append(Chain("book1 %d x %d" % (k, bs), [(s, False, n) for s, n in blocks]))
            if k >= 3:
                m = k // 2
                out.append(Chain("book1 %d x %d, %d as history" % (k, bs, m), [(s, False, n) for s, n in blocks[m:]], history=data[:m * bs]))
    return out


def stored_and_empty_chains(rc):
    b = book1()
    data = b[300000:300000 + 8 * 4096]
    blocks = rc.compress_chain(data, 4096)
    raw = lambda i: (data[i * 4096:(i + 1) * 4096], True, 4096)
    out = [Chain("stored blocks 2 and 5", [raw(i) if i in (2, 5) else (s, False, n) for i, (s, n) in enumerate(blocks)]),
           Chain("stored first block", [raw(i) if i == 0 else (s, False, n) for i, (s, n) in enumerate(blocks)]),
           Chain("stored block too big", [raw(i)[:2] + (4095,) if i == 2 else (s, False, n) for i, (s, n) in enumerate(blocks)])]
    cooked = [(s, False, n) for s, n in blocks]
    for empty in ((b"\x00", False, 0), (b"\x00", False, 16), (b"", True, 0), (b"", True, 9)):
        out.append(Chain("empty block %r" % (empty,), cooked[:3] + [empty] + cooked[3:]))
        out.append(Chain("empty first block %r" % (empty,), [empty] + cooked))
    return out


def damaged_chains(rc, rng, n_flipped=40):
    """streams damaged by 1 to 3 flipped bytes in one block of a chain, and every truncation of one short block in the middle"""
    b = book1()
    out = []
    for bs, k in ((1000, 6), (4096, 5), (1000, 70)):
        data = b[123456:123456 + bs * k]
        blocks = [(s, False, n) for s, n in rc.compress_chain(data, bs)]
        for t in range(n_flipped if k < 70 else 6):
            i = rng.randrange(k)
            bl = list(blocks)
            bl[i] = (damaged(bl[i][0], rng, flips=rng.randrange(1, 4)), False, bl[i][2])
            out.append(Chain("damaged block %d of %d x %d (%d)" % (i, k, bs, t), bl))
    data = b[50000:50000 + 300 * 5]
    blocks = [(s, False, n) for s, n in rc.compress_chain(data, 300)]
    s = blocks[2][0]
    for cut in range(len(s)):
        bl = list(blocks)
        bl[2] = (s[:cut], False, 300)
        out.append(Chain("cut %d/%d" % (cut, len(s)), bl))
    return out


def capacity_chains(chains):
    """block capacities of exact size (the chains as they are), one less and size + 64 -- on one block in the middle and on all of them --
    and a chain_dst_cap that runs out mid-chain"""
    out = []
    for ch in chains:
        k = len(ch.blocks)
        m = k // 2
        out.append(ch.with_caps(lambda i, c: c - 1 if i == m else c, "cap - 1 at %d" % m))
        out.append(ch.with_caps(lambda i, c: c + 64, "cap + 64"))
        out.append(ch.with_caps(lambda i, c: c + 64 if i == m else c, "cap + 64 at %d" % m))
        out.append(ch.with_caps(lambda i, c: max(c - 1, 0), "cap - 1"))
        total = ch.ccap
        for short in (1, 500, total // 2):
            if 0 < short < total:
                out.append(Chain(ch.name + " chain cap - %d" % short, [(s, st, c + 64) for s, st, c in ch.blocks], ch.history, total - short))
    return out


def hand_chains(rng):
    return offset_rule_chains(rng) + end_rule_chains(rng) + straddle_chains(rng)


def case_set(rc, rng):
    """every chain of the CPU and GPU tests"""
    books = book_chains(rc)
    small = [c for c in books if sum(len(s) for s, _, _ in c.blocks) < 120000]
    stored = stored_and_empty_chains(rc)
    return books + hand_chains(rng) + stored + damaged_chains(rc, rng) + capacity_chains(small + stored[:1])


def expected(rc, chains):
    """[(out_len, chain_out_len, bytes)] per chain, from the reference"""
    return [rc.decode(c) for c in chains]


class Packed:
    """chains laid out for one call of the C ABI: streams back to back in src, every chain's history and region in one dst buffer with
    GUARD bytes of 0xA5 between the chains and at both ends"""

    def __init__(self, chains, fill=0x5A, order=None):
        self.chains = chains
        src, self.src_off, self.src_len, self.stored, self.dst_cap, self.chain_first = bytearray(), [], [], [], [], [0]
        dst = bytearray(b"\xA5" * GUARD)
        self.chain_dst_off, self.chain_dst_cap, self.prefix = [], [], []
        for ch in chains:
            for s, st, cap in ch.blocks:
                self.src_off.append(len(src)); self.src_len.append(len(s)); self.stored.append(1 if st else 0); self.dst_cap.append(cap)
                src += s
            self.chain_first.append(len(self.src_off))
            dst += ch.history
            self.chain_dst_off.append(len(dst)); self.chain_dst_cap.append(ch.ccap); self.prefix.append(len(ch.history))
            dst += bytes([fill]) * ch.ccap + b"\xA5" * GUARD
        self.src, self.dst, self.fill = bytes(src) if src else b"\0", dst, fill
        self.n_blocks, self.n_chains = len(self.src_off), len(chains)

    def check(self, dst, out_len, chain_out, want):
        """dst / out_len / chain_out as the call left them against the reference's results `want` (expected()): the values, the bytes
        decoded, and every byte the call must not have written -- the guards, the histories and, in each region, what lies past
        the capacity of the last block that ran"""
        bad = []
        dst = bytes(dst)
        assert len(dst) == len(self.dst)
        for c, (ch, (outs, done, data)) in enumerate(zip(self.chains, want)):
            b0, b1, off = self.chain_first[c], self.chain_first[c + 1], self.chain_dst_off[c]
            if list(out_len[b0:b1]) != outs or chain_out[c] != done:
                bad.append((ch.name, "values", list(out_len[b0:b1])[:8], outs[:8], chain_out[c], done))
            elif dst[off:off + done] != data:
                bad.append((ch.name, "bytes"))
            P = len(ch.history)
            if dst[off - P:off] != ch.history or dst[off - P - GUARD:off - P] != b"\xA5" * GUARD or dst[off + ch.ccap:off + ch.ccap + GUARD] != b"\xA5" * GUARD:
                bad.append((ch.name, "history or guard written"))
            # past the reach of the last block that ran (its start + its capacity), the region is untouched
            reach, pos = 0, 0
            for (s, st, cap), r in zip(ch.blocks, outs):
                if r == CHAIN_STOPPED:
                    break
                reach = max(reach, pos + max(min(cap, ch.ccap - pos), 0))
                pos += max(r, 0)
            if dst[off + reach:off + ch.ccap] != bytes([self.fill]) * (ch.ccap - reach):
                bad.append((ch.name, "written past a block's capacity"))
        return bad


def chain_file(ch):
    """one chain as the file tests/cpp/chain_mirror_test.cpp and tests/jni_stub/fake_jni_chain.c read: u32 n_blocks, u32 prefix_len, u64
    chain capacity, per block {u32 stream length, u32 stored, i32 capacity}, the history, the streams back to back"""
    import struct
    return (struct.pack("<IIQ", len(ch.blocks), len(ch.history), ch.ccap) + b"".join(struct.pack("<IIi", len(s), 1 if st else 0, c) for s, st, c in ch.blocks) +
            ch.history + b"".join(s for s, _, _ in ch.blocks))


def oracle_chain_engine(base, rc, **kw):
    """streams_common.OracleEngine (or a subclass, `base`) plus decompressSafeChain served by the reference library: the engine the
    reader logic of LZ4FrameInputStream(linkedBlocks=True) is tested with on the CPU"""

    class ChainOracleEngine(base):
        chain_calls = 0

        def decompressSafeChain(self, src, srcOff, srcLen, dstCap, chainFirst, dst, chainDstOff, chainDstCap, chainPrefixLen=None, stored=None):
            type(self).chain_calls += 1
            outs, dones = [], []
            for c in range(len(chainDstOff)):
                b0, b1, off = chainFirst[c], chainFirst[c + 1], chainDstOff[c]
                P = chainPrefixLen[c] if chainPrefixLen is not None else 0
                ch = Chain("frame", [(bytes(src[srcOff[i]:srcOff[i] + srcLen[i]]), bool(stored[i]) if stored is not None else False, dstCap[i])
                                     for i in range(b0, b1)], history=bytes(dst[off - P:off]), ccap=chainDstCap[c])
                o, done, data = rc.decode(ch)
                dst[off:off + done] = data
                outs += o
                dones.append(done)
            return outs, dones

    return ChainOracleEngine(**kw)


def linked_frame(rc, xxh32, data, block_id, block_checksum=False, content_checksum=False, content_size=False):
    """an LZ4 frame WITHOUT block independence, assembled from a chain the reference compressed (LZ4_compress_fast_continue over the
    contiguous data, as lz4frame does for linked blocks); a block that does not shrink is stored raw.  block_id: 4 .. 7"""
    import struct
    bs = 1 << (2 * block_id + 8)
    flg = (1 << 6) | (16 if block_checksum else 0) | (8 if content_size else 0) | (4 if content_checksum else 0)
    desc = bytes([flg, block_id << 4]) + (struct.pack("<Q", len(data)) if content_size else b"")
    out = bytearray(struct.pack("<I", 0x184D2204) + desc + bytes([(xxh32(desc, 0) >> 8) & 0xFF]))
    spans = []   # (offset of the payload in the frame, its length, stored?) per block
    for (s, n), o in zip(rc.compress_chain(data, bs), range(0, len(data), bs)):
        raw = len(s) >= n
        payload = data[o:o + n] if raw else s
        out += struct.pack("<I", len(payload) | (0x80000000 if raw else 0))
        spans.append((len(out), len(payload), raw))
        out += payload
        if block_checksum:
            out += struct.pack("<I", xxh32(payload, 0))
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", xxh32(data, 0))
    return bytes(out), spans


__all__ = ["CHAIN_STOPPED", "Chain", "GUARD", "OFFSET_RULE_P", "Packed", "RefChain", "STRADDLE_DISTANCES", "book1", "both_ways", "book_chains",
           "capacity_chains", "case_set", "chain_file", "damaged_chains", "end_rule_chains", "expected", "hand_chains", "lit_block", "linked_frame", "offset_rule_chains", "oracle_chain_engine",
           "rng_for", "seq_block", "stored_and_empty_chains", "straddle_chains"]
