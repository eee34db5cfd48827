"""Shared pieces of the linked-block compressor tests (test_cchain_hostsim.py, test_cchain_abi.py, test_cchain_streams_host.py,
test_gpu_cchain.py): the reference library's own stream calls through ctypes (LZ4_createStream / LZ4_loadDict /
LZ4_compress_fast_continue), the CChain record, the case set and the layout of one call.  The expected value of every case is what the
reference library returns and writes -- never this project's output."""
import ctypes as C
import os
import random

from conftest import GOLD, calgary

CHAIN_STOPPED = -(2 ** 31) + 6          # include/lz4hip.h LZ4HIP_CHAIN_STOPPED
GUARD = 64
PREFIXES = (0, 1, 7, 8, 9, 100, 65535, 65536, 70000)


def bound(n):
    return n + n // 255 + 16


def book1():
    return calgary("book1")


class CChain:
    """one chain: `history` = the bytes directly in front of the chain's source (its length is chain_prefix_len), blocks =
    [(source bytes, dst_cap)]; src_len[i] is len(source) unless lens[i] says otherwise (a negative length)"""

    def __init__(self, name, blocks, history=b"", lens=None):
        self.name, self.history = name, bytes(history)
        self.blocks = [(bytes(s), int(cap)) for s, cap in blocks]
        self.lens = list(lens) if lens is not None else [len(s) for s, _ in self.blocks]

    def with_caps(self, f, name):
        return CChain(self.name + " " + name, [(s, f(i, cap)) for i, (s, cap) in enumerate(self.blocks)], self.history, self.lens)

    @property
    def data(self):
        return b"".join(s for s, _ in self.blocks)


def chain_of(name, data, sizes, history=b""):
    """data cut into blocks of the given sizes, every capacity the bound"""
    blocks, o = [], 0
    for n in sizes:
        blocks.append((data[o:o + n], bound(n)))
        o += n
    assert o == len(data), (name, o, len(data))
    return CChain(name, blocks, history)


class RefCChain:
    """the reference library's stream entry points"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStream.restype = C.c_void_p
        L.LZ4_freeStream.argtypes = [C.c_void_p]
        L.LZ4_loadDict.restype = C.c_int
        L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_compress_fast_continue.restype = C.c_int
        L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.LZ4_decompress_safe_continue.restype = C.c_int
        L.LZ4_decompress_safe_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.LZ4_createStreamDecode.restype = C.c_void_p
        L.LZ4_freeStreamDecode.argtypes = [C.c_void_p]
        L.LZ4_setStreamDecode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

    def compress(self, ch, reload_every=0):
        """-> (out_len per block, chain_consumed, [bytes per block]): LZ4_createStream, LZ4_loadDict of the history if there is any, then
        LZ4_compress_fast_continue block by block over the contiguous source.  A block whose result is 0 ends the chain: the blocks
        behind it get CHAIN_STOPPED.  (reload_every = k: a probe, not the contract -- a fresh stream with LZ4_loadDict of everything
        in front every k blocks)"""
        L = self.L
        P = len(ch.history)
        data = ch.data
        buf = C.create_string_buffer(GUARD + P + len(data) + GUARD)
        base = C.addressof(buf) + GUARD
        C.memmove(base, ch.history + data, P + len(data))
        st = L.LZ4_createStream()
        if P > 0:
            L.LZ4_loadDict(st, base, P)
        outs, by, pos, alive = [], [], 0, True
        for k, ((s, cap), sl) in enumerate(zip(ch.blocks, ch.lens)):
            if not alive:
                outs.append(CHAIN_STOPPED); by.append(b"")
                continue
            if reload_every and k and k % reload_every == 0:
                L.LZ4_freeStream(st)
                st = L.LZ4_createStream()
                L.LZ4_loadDict(st, base, P + pos)
            if sl < 0 or cap < 0:
                r = 0
            else:
                dst = C.create_string_buffer(max(cap, 1) + 8)
                r = L.LZ4_compress_fast_continue(st, base + P + pos, dst, sl, cap, 1)
                assert 0 <= r <= cap
            outs.append(r)
            if r == 0:
                alive = False
                by.append(b"")
            else:
                by.append(dst.raw[:r])
                pos += sl
        L.LZ4_freeStream(st)
        return outs, pos, by

    def decode(self, history, streams, sizes):
        """LZ4_decompress_safe_continue block by block behind `history` -> the decoded bytes"""
        L = self.L
        P, total = len(history), sum(sizes)
        buf = C.create_string_buffer(P + total + 64)
        base = C.addressof(buf)
        C.memmove(base, history, P)
        sd = L.LZ4_createStreamDecode()
        L.LZ4_setStreamDecode(sd, base, P)
        pos = 0
        for s, n in zip(streams, sizes):
            sb = C.create_string_buffer(bytes(s) + b"\0" * 8, len(s) + 8)
            r = L.LZ4_decompress_safe_continue(sd, sb, base + P + pos, len(s), n)
            assert r == n, (r, n)
            pos += n
        L.LZ4_freeStreamDecode(sd)
        return C.string_at(base + P, total)


# ---- the case set ----
def book_chains():
    """book1 cut into blocks of every listed size, 1 .. 70 blocks per chain; 70 x 1000, 17 x 4096 and 3 x 65536 carry the chain past
    64 KB mid-chain; one chain of mixed sizes with empty blocks and blocks under 13 bytes in the middle"""
    b = book1()
    out = []
    for bs, counts in ((1, (1, 2, 30)), (5, (1, 3, 16)), (12, (1, 2, 40)), (13, (1, 2, 3, 70)), (14, (1, 2, 33)), (100, (1, 2, 3, 16, 70)),
                       (256, (1, 2, 16, 64)), (1000, (1, 2, 3, 16, 67, 70)), (4096, (1, 2, 5, 17)), (65536, (1, 2, 3))):
        for k in counts:
            o = (bs * 7 + k * 1013) % 100000
            out.append(chain_of("book1 %d x %d" % (k, bs), b[o:o + bs * k], [bs] * k))
    sizes = [300, 0, 5, 1000, 12, 0, 0, 13, 4096, 1, 14, 700, 0, 12, 2000]
    out.append(chain_of("book1 mixed", b[5000:5000 + sum(sizes)], sizes))
    sizes = [0, 5, 12, 0, 100, 7, 300]
    out.append(chain_of("book1 small blocks first", b[9000:9000 + sum(sizes)], sizes))
    out.append(chain_of("empty only", b"", [0, 0, 0]))
    return out


def prefix_chains():
    """the same data with its first P bytes supplied as prefix: -> {P: [chains]}"""
    b = book1()
    out = {}
    for P in PREFIXES:
        out[P] = []
        for o, sizes in ((70000, [1000] * 6), (90000, [4096] * 3), (120000, [100] * 20), (150000, [5, 0, 13, 300, 12, 2000]), (80000, [65536, 4096])):
            out[P].append(chain_of("prefix P=%d %r at %d" % (P, sizes[:3], o), b[o:o + sum(sizes)], sizes, history=b[o - P:o]))
    return out


def hand_chains(rng):
    """hand-built data; each with the history as a prefix and as an earlier block of the chain"""
    out = []

    def both(name, hist, blocks):
        data = b"".join(blocks)
        out.append(chain_of(name + " (history = prefix)", data, [len(x) for x in blocks], history=hist))
        out.append(chain_of(name + " (history = block)", hist + data, [len(hist)] + [len(x) for x in blocks]))

    # a repeat of the history's last bytes at the block's first positions: a match that starts in front of the block and runs into it
    for rep in (1, 2, 3, 5, 20):
        h = rng.randbytes(100 - rep) + bytes([7 + rep] * rep) if rep < 20 else rng.randbytes(100)
        first = (h[-rep:] * 40)[:40] if rep < 20 else h[-20:] * 2
        both("repeat of the last %d history bytes" % rep, h, [first + rng.randbytes(30)])
    # a copy of history bytes off the stride-3 grid: found through backward extension
    for shift in (1, 2):
        h = rng.randbytes(300)
        both("copy off the grid by %d" % shift, h, [rng.randbytes(20) + h[99 + shift:99 + shift + 40] + rng.randbytes(20)])
    # identical data at distance 65535 / 65536 / 65537 across a block boundary (the boundary in front of and inside the copy)
    for D in (65535, 65536, 65537):
        for cut in (0, 10):
            A = rng.randbytes(40)
            data = A + rng.randbytes(D - 40) + A + rng.randbytes(20)
            out.append(chain_of("distance %d, boundary %d into the copy" % (D, cut), data, [D + cut, len(data) - D - cut]))
            out.append(chain_of("distance %d, boundary %d into the copy, prefix" % (D, cut), data[100:], [D + cut - 100, len(data) - D - cut],
                                history=data[:100]))
    # incompressible blocks: 4114 bytes out for 4096 in
    out.append(chain_of("incompressible 3 x 4096", rng.randbytes(3 * 4096), [4096] * 3))
    out.append(chain_of("incompressible 2 x 4096, prefix", rng.randbytes(2 * 4096), [4096] * 2, history=rng.randbytes(500)))
    # all-equal bytes (every step collides in the table) around text
    b = book1()
    out.append(chain_of("zeros and text", bytes(300) + b[200000:200300] + bytes(300), [250, 400, 250]))
    for name in ("geo_65536.bin", "pic_65536.bin"):
        d = open(os.path.join(GOLD, name), "rb").read()
        out.append(chain_of(name + " 4 x 4096", d[8192:8192 + 4 * 4096], [4096] * 4))
        out.append(chain_of(name + " 16 x 256, prefix", d[30000:30000 + 16 * 256], [256] * 16, history=d[30000 - 3000:30000]))
    return out


def capacity_chains(rc, chains):
    """capacities: the exact output size, one less on one middle block and on all (stopped chains), 0, and a negative src_len and a
    negative dst_cap in the middle"""
    out = []
    for ch in chains:
        sizes = rc.compress(ch)[0]
        assert all(r > 0 for r in sizes), ch.name
        k = len(ch.blocks)
        m = k // 2
        out.append(ch.with_caps(lambda i, c: sizes[i], "exact caps"))
        out.append(ch.with_caps(lambda i, c: sizes[i] - 1 if i == m else c, "cap - 1 at %d" % m))
        out.append(ch.with_caps(lambda i, c: sizes[i] - 1, "cap - 1"))
        out.append(ch.with_caps(lambda i, c: 0 if i == m else c, "cap 0 at %d" % m))
        out.append(ch.with_caps(lambda i, c: -1 if i == m else c, "cap -1 at %d" % m))
        neg = CChain(ch.name + " src_len -1 at %d" % m, ch.blocks, ch.history, [(-1 if i == m else n) for i, n in enumerate(ch.lens)])
        out.append(neg)
    return out


def case_set(rc, rng):
    """every chain of the CPU and GPU tests"""
    books = book_chains()
    pre = prefix_chains()
    hand = hand_chains(rng)
    small = [c for c in books + pre[0] + pre[100] + pre[70000] + hand if len(c.data) <= 20000]
    chains = books + [c for P in PREFIXES for c in pre[P]] + hand + capacity_chains(rc, small)
    return chains


def expected(rc, chains):
    """[(out_len, chain_consumed, [bytes per block])] per chain, from the reference"""
    return [rc.compress(c) for c in chains]


def stops_early(want):
    return sum(1 for outs, _, _ in want if 0 in outs)


class CPacked:
    """chains laid out for one call of the C ABI: every chain's history and source in src with GUARD bytes of 0xA5 between the chains and
    at both ends, every block's slot of max(dst_cap, 0) bytes in dst with GUARD bytes of 0xA5 around it.  (A block with a negative
    src_len still has its bytes in src, so that the blocks behind it keep their places.)"""

    def __init__(self, chains, fill=0x5A):
        self.chains, self.fill = chains, fill
        src = bytearray(b"\xA5" * GUARD)
        dst = bytearray(b"\xA5" * GUARD)
        self.chain_src_off, self.prefix, self.src_len, self.chain_first, self.dst_off, self.dst_cap = [], [], [], [0], [], []
        for ch in chains:
            src += ch.history
            self.chain_src_off.append(len(src)); self.prefix.append(len(ch.history))
            src += ch.data + b"\xA5" * GUARD
            for (s, cap), sl in zip(ch.blocks, ch.lens):
                self.src_len.append(sl); self.dst_off.append(len(dst)); self.dst_cap.append(cap)
                dst += bytes([fill]) * max(cap, 0) + b"\xA5" * GUARD
            self.chain_first.append(len(self.src_len))
        self.src, self.dst = bytes(src), dst
        self.n_blocks, self.n_chains = len(self.src_len), len(chains)

    def check(self, dst, out_len, consumed, want):
        """dst / out_len / consumed as the call left them against the reference's results `want` (expected()): the values, the bytes
        produced, and every byte the call must not have written -- the guards and, in each slot, what lies past the result"""
        bad = []
        dst = bytes(dst)
        assert len(dst) == len(self.dst)
        if dst[:GUARD] != b"\xA5" * GUARD:
            bad.append(("front guard written",))
        for c, (ch, (outs, done, by)) in enumerate(zip(self.chains, want)):
            b0, b1 = self.chain_first[c], self.chain_first[c + 1]
            if [int(v) for v in out_len[b0:b1]] != outs or int(consumed[c]) != done:
                bad.append((ch.name, "values", [int(v) for v in out_len[b0:b1]][:8], outs[:8], int(consumed[c]), done))
                continue
            for i in range(b0, b1):
                o, cap, r = self.dst_off[i], max(self.dst_cap[i], 0), max(outs[i - b0], 0)
                if dst[o:o + r] != by[i - b0]:
                    bad.append((ch.name, "bytes of block", i - b0))
                    break
                if outs[i - b0] > 0 and dst[o + r:o + cap] != bytes([self.fill]) * (cap - r):
                    bad.append((ch.name, "written past the result", i - b0))
                    break
                if outs[i - b0] == CHAIN_STOPPED and dst[o:o + cap] != bytes([self.fill]) * cap:
                    bad.append((ch.name, "a stopped block's slot written", i - b0))
                    break
                if dst[o + cap:o + cap + GUARD] != b"\xA5" * GUARD:
                    bad.append((ch.name, "guard written", i - b0))
                    break
        return bad


def cchain_file(ch):
    """one chain as the file tests/cpp/cchain_mirror_test.cpp and tests/jni_stub/fake_jni_cchain.c read: u32 n_blocks, u32 prefix_len, per
    block {i32 src_len, i32 dst_cap}, the history, the source"""
    import struct
    return struct.pack("<II", len(ch.blocks), len(ch.history)) + b"".join(struct.pack("<ii", sl, c) for (s, c), sl in zip(ch.blocks, ch.lens)) + ch.history + ch.data


def oracle_cchain_engine(base, rc, **kw):
    """`base` (streams_common.OracleEngine or a subclass of it) plus compressFastChain served by the reference library: the engine the
    writer logic of LZ4FrameOutputStream(linkedBlocks=True) is tested with on the CPU"""

    class CChainOracleEngine(base):
        cchain_calls = 0

        def compressFastChain(self, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None):
            type(self).cchain_calls += 1
            outs, cons = [], []
            for c in range(len(chainSrcOff)):
                b0, b1, off = chainFirst[c], chainFirst[c + 1], chainSrcOff[c]
                P = chainPrefixLen[c] if chainPrefixLen is not None else 0
                blocks, o = [], off
                for i in range(b0, b1):
                    blocks.append((bytes(src[o:o + srcLen[i]]), dstCap[i]))
                    o += srcLen[i]
                r, done, by = rc.compress(CChain("frame", blocks, history=bytes(src[off - P:off])))
                for i, x in zip(range(b0, b1), by):
                    dst[dstOff[i]:dstOff[i] + len(x)] = x
                outs += r
                cons.append(done)
            return outs, cons

    return CChainOracleEngine(**kw)


def batched_linked_frame(rc, xxh32, data, block_id, batch_blocks, block_checksum=False, content_checksum=False):
    """the frame LZ4FrameOutputStream(linkedBlocks=True) must write when it compresses batch_blocks blocks at a time, assembled from the
    reference: every batch is a fresh stream that loads the last 64 KB written before it (LZ4_loadDict) and compresses its blocks
    with LZ4_compress_fast_continue; a block that does not shrink is stored raw"""
    import struct
    bs = 1 << (2 * block_id + 8)
    flg = (1 << 6) | (16 if block_checksum else 0) | (4 if content_checksum else 0)
    desc = bytes([flg, block_id << 4])
    out = bytearray(struct.pack("<I", 0x184D2204) + desc + bytes([(xxh32(desc, 0) >> 8) & 0xFF]))
    for a in range(0, len(data), bs * batch_blocks):
        part = data[a:a + bs * batch_blocks]
        sizes = [min(bs, len(part) - o) for o in range(0, len(part), bs)]
        outs, done, by = rc.compress(chain_of("batch", part, sizes, history=data[max(a - 65536, 0):a]))
        assert done == len(part)
        o = 0
        for n, s in zip(sizes, by):
            raw = len(s) >= n
            payload = part[o:o + n] if raw else s
            out += struct.pack("<I", len(payload) | (0x80000000 if raw else 0)) + payload
            if block_checksum:
                out += struct.pack("<I", xxh32(payload, 0))
            o += n
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", xxh32(data, 0))
    return bytes(out)


__all__ = ["batched_linked_frame", "oracle_cchain_engine", "CChain", "CHAIN_STOPPED", "CPacked", "GUARD", "PREFIXES", "RefCChain", "book1", "book_chains", "bound", "capacity_chains", "case_set", "cchain_file",
           "chain_of", "expected", "hand_chains", "prefix_chains", "stops_early"]
