"""Shared pieces of the tests of the HC stream compressor for sources that land anywhere (test_hcstream_hostsim.py, test_hcstream_abi.py,
test_gpu_hcstream.py): the reference library's own LZ4_streamHC_t driven through ctypes on REAL arenas -- a ring that wraps, two
buffers, a save area, a dictionary elsewhere -- with its bookkeeping read back after every step at the offsets liblz4 1.9.3 has on
x86-64, the offsets model of that bookkeeping, the layouts and the case list, and the runner that cuts a stream into calls.  The
expected value of every case is what the reference library returns and writes -- never this project's output."""
import ctypes as C
import random

from cchain_common import GUARD, book1, bound
from dictc_common import parse

LEVELS = (1, 3, 4, 8, 9, 10, 12)
CLAMPS = ((0, 9), (13, 12))
MAXB = 4096                             # the largest block of the layouts
# LZ4_streamHC_t of liblz4 1.9.3, x86-64: hashTable[32768] u32, chainTable[65536] u16, then the fields
F_END, F_BASE, F_DICTBASE, F_DICTLIMIT, F_LOWLIMIT = 262144, 262152, 262160, 262168, 262172


def clamp(level):
    return 9 if level < 1 else min(level, 12)


class Op:
    """one step of a stream's life: kind 'B' a block (data is written to arena[off:] by the producer right before it is compressed, n =
    src_len, cap = dst_cap), 'L' LZ4_loadDictHC(arena + off - n, n) (the dictionary's bytes lie there from the start), 'S'
    LZ4_saveDictHC(arena + off, k)"""

    def __init__(self, kind, off, n=0, cap=0, data=b"", k=0):
        self.kind, self.off, self.n, self.cap, self.data, self.k = kind, int(off), int(n), int(cap), bytes(data), int(k)


def block(off, data, cap=None, n=None):
    return Op("B", off, len(data) if n is None else n, bound(len(data)) if cap is None else cap, data)


class Script:
    """a stream: the arena's size, what lies in it from the start ([(offset, bytes)]: dictionaries), and its ops"""

    def __init__(self, name, arena, ops, init=()):
        self.name, self.arena, self.ops, self.init = name, int(arena), list(ops), list(init)

    def blocks(self):
        return [o for o in self.ops if o.kind == "B"]

    def with_caps(self, f, name):
        k, ops = 0, []
        for o in self.ops:
            if o.kind == "B":
                ops.append(Op("B", o.off, o.n, f(k, o.cap), o.data)); k += 1
            else:
                ops.append(o)
        return Script(self.name + " " + name, self.arena, ops, self.init)


# ---- the offsets model: the stream's bookkeeping is a function of addresses and lengths alone ----
def runs(n):
    return 0 <= n <= 0x7E000000


def model_enter(st, s, n):
    """steps 1 and 2 in front of the block [s, s + n) -> the state the block is parsed in"""
    pe, pl, ee, el, ix = st
    if s != pe:
        ee, el, pl, pe = pe, pl, 0, s
    if runs(n) and el > 0 and s + n > ee - el and s < ee:
        el = ee - min(s + n, ee)
        if el < 4:
            el = 0
    return (pe, pl, ee, el, ix)


def model_block(st, s, n):
    pe, pl, ee, el, ix = model_enter(st, s, n)
    if not runs(n):
        return (pe, pl, ee, el, ix)
    return (s + n, pl + n, ee, el, ix + n)


def model_load(end, n):
    k = min(n, 65536)
    return (end, k, 0, 0, k)


def model_save(st, buf, k):
    pe, pl, ee, el, ix = st
    kept = min(max(k, 0), 65536)
    if kept < 4:
        kept = 0
    kept = min(kept, pl)
    return (buf + kept, kept, ee, 0, ix), kept


def same_state(a, b):
    """two states name the same stream: a history of no bytes has no end worth comparing"""
    return a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and (a[3] == 0 or a[2] == b[2])


# ---- the reference ----
class RefHCStream:
    """ONE LZ4_streamHC_t of the reference library per script and level, on a real arena; results are kept"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStreamHC.restype = C.c_void_p
        L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
        L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
        L.LZ4_loadDictHC.restype = C.c_int
        L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_saveDictHC.restype = C.c_int
        L.LZ4_saveDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_compress_HC_continue.restype = C.c_int
        L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        self.memo = {}

    @staticmethod
    def fields(st, base):
        """the stream's bookkeeping as offsets into the arena -> (prefix_end, prefix_len, ext_end, ext_len, index)"""
        u64 = lambda o: C.c_uint64.from_address(st + o).value
        u32 = lambda o: C.c_uint32.from_address(st + o).value
        end, b, db, dl, ll = u64(F_END), u64(F_BASE), u64(F_DICTBASE), u32(F_DICTLIMIT), u32(F_LOWLIMIT)
        if end == 0:
            return (0, 0, 0, 0, 0)
        total = (end - b) & 0xFFFFFFFFFFFFFFFF
        return (end - base, total - dl, ((db + dl) & 0xFFFFFFFFFFFFFFFF) - base, dl - ll, total - 65536)

    def run(self, sc, level):
        """-> per op: ('B', r, bytes, state) / ('L', state) / ('S', kept, state); state = fields() behind the step"""
        key = (id(sc), level)
        got = self.memo.get(key)
        if got is not None and got[0] is sc:
            return got[1]
        L = self.L
        mem = C.create_string_buffer(b"\xA5" * (sc.arena + 2 * GUARD), sc.arena + 2 * GUARD)
        base = C.addressof(mem) + GUARD
        for off, by in sc.init:
            C.memmove(base + off, by, len(by))
        st = L.LZ4_createStreamHC()
        L.LZ4_resetStreamHC_fast(st, level)
        res = []
        for o in sc.ops:
            if o.kind == "L":
                L.LZ4_loadDictHC(st, base + o.off - o.n, o.n)
                res.append(("L", self.fields(st, base)))
            elif o.kind == "S":
                kept = L.LZ4_saveDictHC(st, base + o.off, o.k)
                res.append(("S", kept, self.fields(st, base)))
            else:
                C.memmove(base + o.off, o.data, len(o.data))
                if not runs(o.n) or o.cap < 0:
                    # (the engine's rule, not liblz4's: a length that cannot run jumps and consumes nothing -- a 0-byte call at the same
                    # address does exactly that to the reference's stream; a negative capacity is a call at capacity 0)
                    dst = C.create_string_buffer(8)
                    L.LZ4_compress_HC_continue(st, base + o.off, dst, o.n if runs(o.n) else 0, 0)
                    res.append(("B", 0, b"", self.fields(st, base)))
                    continue
                dst = C.create_string_buffer(max(o.cap, 1) + 8)
                r = L.LZ4_compress_HC_continue(st, base + o.off, dst, o.n, o.cap)
                assert 0 <= r <= o.cap
                res.append(("B", r, dst.raw[:r], self.fields(st, base)))
        L.LZ4_freeStreamHC(st)
        assert mem.raw[:GUARD] == b"\xA5" * GUARD and mem.raw[GUARD + sc.arena:] == b"\xA5" * GUARD
        self.memo[key] = (sc, res)
        return res


# ---- cutting a stream into calls ----
def mandatory_cuts(sc):
    """the op indexes in front of which a call MUST end (a call is a snapshot of the arena): every state edit, and every block whose
    bytes land on anything an earlier block of the same call reads -- its source, or the pieces of the two histories it can reach"""
    cuts, st, read = set(), (0, 0, 0, 0, 0), []
    for i, o in enumerate(sc.ops):
        if o.kind == "L":
            st = model_load(o.off, o.n); cuts.add(i); cuts.add(i + 1); read = []
        elif o.kind == "S":
            st, _ = model_save(st, o.off, o.k); cuts.add(i); cuts.add(i + 1); read = []
        else:
            w = (o.off, o.off + len(o.data))
            if any(w[0] < b and a < w[1] for a, b in read):
                cuts.add(i); read = []
            e = model_enter(st, o.off, o.n)
            read += [(o.off, o.off + max(o.n, 0)), (e[2] - min(e[3], 65536), e[2]), (e[0] - min(e[1], 65536), e[0])]
            st = model_block(st, o.off, o.n)
    return cuts


def cut_into_calls(sc, how, rng=None):
    """-> [[op index, ...]] the blocks of each call.  how: 'each' (a call per block), 'one' (as few calls as the snapshot rule allows),
    'random', 'few' (2 .. 6 calls where the layout leaves the choice)"""
    must = mandatory_cuts(sc)
    few = set()
    if how == "few":   # 2 .. 6 calls where the snapshot rule and the state edits leave the choice
        free = [i for i, o in enumerate(sc.ops) if o.kind == "B" and i not in must and i and sc.ops[i - 1].kind == "B"]
        few = set(rng.sample(free, min(len(free), rng.randrange(1, 6))))
    calls, cur = [], []
    for i, o in enumerate(sc.ops):
        if o.kind != "B":
            if cur:
                calls.append(cur); cur = []
            calls.append(i)
            continue
        if cur and (i in must or how == "each" or (how == "random" and rng.random() < 0.4) or (how == "few" and i in few)):
            calls.append(cur); cur = []
        cur.append(i)
    if cur:
        calls.append(cur)
    return calls


def run_cut(sc, calls, call_fn, load_fn, save_fn):
    """the stream through an engine: call_fn(state, arena bytes, [(off, n, cap)]) -> ([r], [bytes], new state); load_fn(end, n) -> state;
    save_fn(state, buf, k) -> (state, kept).  The arena is brought, in front of every call, to what the producer has written up to
    the call's last block.  -> per op what RefHCStream.run gives; the state only behind a call's LAST block (None elsewhere)"""
    arena = bytearray(b"\xA5" * sc.arena)
    for off, by in sc.init:
        arena[off:off + len(by)] = by
    st, res = (0, 0, 0, 0, 0), [None] * len(sc.ops)
    for call in calls:
        if isinstance(call, int):
            o = sc.ops[call]
            if o.kind == "L":
                st = load_fn(o.off, o.n)
                res[call] = ("L", st)
            else:
                end = st[0]
                st, kept = save_fn(st, o.off, o.k)
                arena[o.off:o.off + kept] = bytes(arena[end - kept:end])   # (the caller's part of LZ4_saveDictHC: the copy)
                res[call] = ("S", kept, st)
            continue
        for i in call:
            o = sc.ops[i]
            arena[o.off:o.off + len(o.data)] = o.data
        rs, bys, st = call_fn(st, bytes(arena), [(sc.ops[i].off, sc.ops[i].n, sc.ops[i].cap) for i in call])
        for k, i in enumerate(call):
            res[i] = ("B", rs[k], bys[k], st if k == len(call) - 1 else None)
    return res


def compare(sc, want, got, level, bad, tag=(), left_out=None):
    """results of run_cut against the reference's -> appends to bad, every difference (a block's bytes depend on data, level and
    capacity alone: one difference does not spoil the blocks behind it).  left_out: levels 10..12 only, the list that takes -- instead
    of bad -- a block that differs where the header's stated exception applies (is_old_at_jump)"""
    old = is_old_at_jump(sc) if left_out is not None and clamp(level) >= 10 else None
    for i, (w, g) in enumerate(zip(want, got)):
        if w[0] == "B":
            if (w[1], w[2]) != (g[1], g[2]):
                (left_out if old and old[i] else bad).append((sc.name, level) + tuple(tag) + ("block at op", i, "got", g[1], "want", w[1]))
            if g[3] is not None and not same_state(w[3], g[3]):
                bad.append((sc.name, level) + tuple(tag) + ("state behind op", i, g[3], w[3]))
        elif w[0] == "S":
            if w[1] != g[1] or not same_state(w[2], g[2]):
                bad.append((sc.name, level) + tuple(tag) + ("saveDict at op", i, g[1:], w[1:]))
        elif not same_state(w[1], g[1]):
            bad.append((sc.name, level) + tuple(tag) + ("loadDict at op", i, g[1], w[1]))


# ---- the layouts ----
def sizes_of(rng, total, maxb=MAXB, tiny=True):
    out = []
    while total > 0:
        n = rng.choice([maxb, maxb, rng.randrange(14, maxb + 1), rng.randrange(0, 14) if tiny else maxb])
        n = min(n, total)
        out.append(n); total -= n
    return out


def pieces(data, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(data[o:o + n]); o += n
    return out


def lay_contiguous(name, data, sizes):
    ops, o = [], 0
    for p in pieces(data, sizes):
        ops.append(block(o, p)); o += len(p)
    return Script(name + " contiguous", o + 1, ops)


def lay_two_buffers(name, data, sizes, gap, maxb=MAXB):
    """two alternating block buffers, `gap` bytes apart (0: adjacent -- a block that fills buffer 0 is followed contiguously)"""
    at = (0, maxb + gap)
    ops = [block(at[i & 1], p) for i, p in enumerate(pieces(data, sizes))]
    return Script(name + (" two buffers, gap %d" % gap), 2 * maxb + gap, ops)


def lay_ring(name, data, sizes, ring):
    """a ring: a block that does not fit behind the last one starts at the ring's first byte.  (A ring longer than 64 KB loses nothing
    of its history at a wrap but the three positions liblz4 never inserts: so that its bytes differ from a contiguous stream's, the
    block behind a wrap repeats, 20 bytes in, the last three bytes in front of the wrap and its own first thirty)"""
    ops, o, prev = [], 0, b""
    for p in pieces(data, sizes):
        if o + len(p) > ring:
            o = 0
            if len(p) >= 60 and len(prev) >= 3:
                p = p[:20] + prev[-3:] + p[:30] + p[53:]
        ops.append(block(o, p)); o += len(p); prev = p
    return Script(name + " ring %d" % ring, ring, ops)


def lay_save_area(name, data, sizes, k, maxb=MAXB):
    """LZ4_saveDictHC(k) into a save area behind every block, the next block right behind the kept bytes (liblz4's blockStreaming
    example with a save area: the block area follows the save area, prefix mode throughout)"""
    ops, blk_at = [], 65536 + 8
    o = blk_at
    st = (0, 0, 0, 0, 0)
    for p in pieces(data, sizes):
        ops.append(block(o, p))
        st = model_block(st, o, len(p))
        ops.append(Op("S", 0, k=k))
        st, kept = model_save(st, 0, k)
        o = kept
    return Script(name + " save area k=%d" % k, blk_at + 65536 + maxb + 8, ops)


def lay_dict_elsewhere(name, dic, data, sizes, follow=False):
    """LZ4_loadDictHC of a dictionary that lies elsewhere (follow: directly in front of the first block), then contiguous blocks"""
    d_at = 16
    o = d_at + len(dic) + (0 if follow else 1000)
    ops = [Op("L", d_at + len(dic), n=len(dic))]
    for p in pieces(data, sizes):
        ops.append(block(o, p)); o += len(p)
    return Script(name + (" dictionary %d %s" % (len(dic), "in front" if follow else "elsewhere")), o + 16, ops, [(d_at, dic)])


def is_jump_layout(sc):
    return " two buffers, gap " in sc.name or " ring " in sc.name


def layouts(name, data, rng, n_blocks=16, tiny=True, maxb=MAXB, big_ring=True):
    """every layout of the issue over `data` (at least n_blocks x maxb bytes, and 65535 + 8 x maxb for the large ring) with blocks of at
    most maxb bytes"""
    d = data[:n_blocks * maxb]
    s = sizes_of(rng, len(d), maxb, tiny)
    out = [lay_contiguous(name, d, s), lay_two_buffers(name, d, s, 100, maxb), lay_two_buffers(name, d, s, 0, maxb), lay_ring(name, d, s, 5 * maxb + 100)]
    if big_ring:
        big = data[:65535 + 8 * maxb]
        out.append(lay_ring(name, big, sizes_of(rng, len(big), maxb, tiny), 65535 + 2 * maxb))
    for k in (0, 3, 4, 100, maxb, 65536, 70000):
        out.append(lay_save_area(name, d[:8 * maxb], sizes_of(rng, min(len(d), 8 * maxb), maxb, tiny), k, maxb))
    out.append(lay_dict_elsewhere(name, data[-3000:], d[:6 * maxb], sizes_of(rng, min(len(d), 6 * maxb), maxb, tiny)))
    out.append(lay_dict_elsewhere(name, data[-3000:], d[:6 * maxb], sizes_of(rng, min(len(d), 6 * maxb), maxb, tiny), follow=True))
    return out


def hand_scripts(rng):
    """the smallest shapes that can go wrong"""
    b = book1()
    out = []
    # blocks of 0 .. 13 bytes at jumps, runs of 1 .. 7 bytes (fewer than 4: nothing is inserted), between ordinary blocks
    for n in list(range(0, 14)):
        ops = [block(0, b[:3000]), block(5000, b[3000:3000 + n]), block(9000, b[2990:2990 + 40] + b[3000:3000 + n] + b[100:1100]), block(0, b[3000:3000 + n] + b[200:900])]
        out.append(Script("a %d-byte block at a jump" % n, 12000, ops))
    for n in range(1, 8):
        ops = [block(0, b[:2000]), block(4000, b[2000:2000 + n]), block(4000 + n, b[2000 + n:2000 + n + 3]), block(8000, b[1990:2020] + b[:500]),
               block(0, b[1999:2000 + n + 3] * 3 + b[300:700])]
        out.append(Script("a run of %d bytes, then 3 more" % n, 10000, ops))
    # ext_len trimmed to 3, 4 and 5 by the overlap rule: the next block ends that many bytes in front of the dictionary's end
    # (the dictionary's last bytes are the only ones left, and a match that starts in them goes on at the block's own first bytes)
    for left in (3, 4, 5, 9, 0):
        first = b[:3000]
        lead = b[5000:5040]
        body = lead + first[-8:] + lead[:30] + b[5100:5100 + 6000]
        ops = [block(3000, first), block(0, body[:6000 - left]), block(7000, first[-20:] + body[100:600])]
        out.append(Script("ext_len trimmed to %d" % left, 8000, ops))
    # prefix lengths 65534, 65535 and 65536 with an external piece present: the last byte(s) of the piece are in reach or not
    for plen in (65534, 65535, 65536):
        ext = b[:5000]
        pre = b[100000:100000 + plen - 1000]
        ops = [block(0, ext), block(8000, pre, n=len(pre)), block(8000 + len(pre), ext[-60:] + b[7000:7000 + 940]), block(8000 + plen, ext[-50:] + b[9000:9500] + ext[-45:])]
        out.append(Script("prefix %d with an external piece" % plen, 8000 + plen + 1000, ops))
    # a match that ends exactly at, and one that crosses, the external piece's end
    ext = rng.randbytes(2000)
    pre = rng.randbytes(30)
    out.append(Script("a match ends exactly at the external end", 9000, [block(0, ext), block(4000, pre + rng.randbytes(20) + ext[-40:] + rng.randbytes(30))]))
    out.append(Script("a match crosses the external end", 9000, [block(0, ext), block(4000, pre + rng.randbytes(20) + ext[-40:] + pre[:25] + rng.randbytes(30))]))
    out.append(Script("a match crosses the external end, lazily", 9000,
                      [block(0, ext), block(4000, pre + rng.randbytes(5) + ext[-9:-2] + rng.randbytes(3) + ext[-40:] + pre[:25] + rng.randbytes(30))]))
    # the last k bytes of a run that a jump ended: its last three positions are no candidates
    for k in (3, 4, 5, 6, 7):
        ext = rng.randbytes(500)
        out.append(Script("the last %d bytes in front of a jump" % k, 4000, [block(0, ext), block(1000, rng.randbytes(20) + ext[-k:] + rng.randbytes(20) + ext[-k:] + rng.randbytes(13))]))
    # one-, two- and four-byte-period runs that span a jump
    for unit in (b"a", b"ab", b"abcd", b"\0"):
        for tail in (0, 1, 3):
            run = unit * 300
            ops = [block(0, rng.randbytes(50) + run[:len(run) - tail]), block(3000, run[len(run) - tail:] + run + rng.randbytes(9) + run[:200] + rng.randbytes(13)),
                   block(6000, run[1:700] + rng.randbytes(5))]
            out.append(Script("period %d across a jump, tail %d" % (len(unit), tail), 9000, ops))
    return out


def capacity_scripts(rr, scripts, level=9):
    """dst_cap at the bound, bound - 1, the result and the result - 1, 0 and negative values in mid-stream, a negative and an
    oversized src_len in mid-stream: a block that returns 0 does not end its stream"""
    out = []
    for sc in scripts:
        sizes = [r[1] for r in rr.run(sc, level) if r[0] == "B"]
        nb = len(sizes)
        m = nb // 2
        out.append(sc.with_caps(lambda i, c: sizes[i], "exact caps"))
        out.append(sc.with_caps(lambda i, c: sizes[i] - 1 if i == m else c, "result - 1 at %d" % m))
        out.append(sc.with_caps(lambda i, c: sizes[i] - 1, "result - 1"))
        out.append(sc.with_caps(lambda i, c: c - 1, "bound - 1"))
        out.append(sc.with_caps(lambda i, c: 0 if i == m else c, "cap 0 at %d" % m))
        out.append(sc.with_caps(lambda i, c: -1 if i == m else c, "cap -1 at %d" % m))
        for bad_n in (-1, 0x7E000001):
            k, ops = 0, []
            for o in sc.ops:
                if o.kind == "B":
                    ops.append(Op("B", o.off, bad_n, o.cap, o.data) if k == m else o); k += 1
                else:
                    ops.append(o)
            out.append(Script(sc.name + " src_len %d at %d" % (bad_n, m), sc.arena, ops, sc.init))
    return out


_SET = {}


def case_set(rr):
    """every script of the CPU tests (built once per process)"""
    if "s" not in _SET:
        rng = random.Random(77)
        b = book1()
        lay = layouts("book1", b[10000:], rng) + layouts("book1 1K", b[300000:], rng, maxb=1024)
        small = [s for s in lay if s.arena < 60000]
        hand = hand_scripts(rng)
        _SET["s"] = lay + hand + capacity_scripts(rr, small[1:5] + hand[::9])
    return _SET["s"]


def levels_of(sc):
    big = any(o.kind == "B" and len(o.data) > 20000 for o in sc.ops) or len(sc.blocks()) > 20
    return (9, 10) if big else LEVELS + tuple(a for a, _ in CLAMPS)


def is_old_at_jump(sc):
    """-> per op: the block is parsed behind a jump on a stream that had consumed more than 64 KB by then (levels 10..12: liblz4's
    stale chain entries of never-inserted positions can be non-zero there, the stated exception)"""
    st, out = (0, 0, 0, 0, 0), []
    for o in sc.ops:
        if o.kind == "L":
            st = model_load(o.off, o.n)
        elif o.kind == "S":
            st, _ = model_save(st, o.off, o.k)
        else:
            e = model_enter(st, o.off, o.n)
            out.append(e[3] > 0 and st[4] - e[1] > 65536)   # (the never-inserted positions lie more than 64 KB into the stream)
            st = model_block(st, o.off, o.n)
            continue
        out.append(False)
    return out


def walk_offsets(sc, res):
    """-> True when a block's reference bytes hold a match whose offset exceeds its position in its run (it reaches across a jump)"""
    st = (0, 0, 0, 0, 0)
    for o, r in zip(sc.ops, res):
        if o.kind == "L":
            st = model_load(o.off, o.n)
        elif o.kind == "S":
            st, _ = model_save(st, o.off, o.k)
        else:
            e = model_enter(st, o.off, o.n)
            if r[1] > 0 and any(off > e[1] + pos for pos, off, ml in parse(r[2])):
                return True
            st = model_block(st, o.off, o.n)
    return False


def script_file(sc, level):
    """the file tests/cpp/hcstream_mirror_test.cpp reads: the script as int64 words, then the bytes of its blocks and dictionaries"""
    import struct
    q = lambda *v: struct.pack("<%dq" % len(v), *v)
    dic = {off: by for off, by in sc.init}
    out, body = q(level, sc.arena, len(sc.ops)), b""
    for o in sc.ops:
        if o.kind == "L":
            out += q(1, o.off, o.n, 0, 0); body += dic[o.off - o.n]
        elif o.kind == "S":
            out += q(2, o.off, 0, 0, o.k)
        else:
            assert not runs(o.n) or o.n == len(o.data)
            out += q(0, o.off, o.n, o.cap, 0); body += o.data if runs(o.n) else b""
    return out + body


def read_results(sc, blob):
    """what the program wrote -> per op what run_cut gives (a call per block)"""
    import struct
    n = len(sc.ops)
    w = struct.unpack("<%dq" % (6 * n), blob[:48 * n])
    body, res = blob[48 * n:], []
    for i, o in enumerate(sc.ops):
        r, st = w[6 * i], tuple(w[6 * i + 1:6 * i + 6])
        if o.kind == "L":
            res.append(("L", st))
        elif o.kind == "S":
            res.append(("S", r, st))
        else:
            res.append(("B", r, body[:max(r, 0)], st)); body = body[max(r, 0):]
    assert not body
    return res


# ---- many streams side by side through the Python class (the GPU tests and their child scripts) ----
class Fleet:
    """many scripts side by side in ONE source buffer (GUARD bytes of 0xA5 between their arenas), driven through a CompressStreamsHC set:
    round after round, every stream that has a call left takes part in one lz4hip_compress_hc_stream_batch"""

    def __init__(self, amd, scripts, level):
        self.amd, self.scripts = amd, scripts
        self.base, o = [], GUARD
        for sc in scripts:
            self.base.append(o); o += sc.arena + GUARD
        self.src = bytearray(b"\xA5" * o)
        for sc, b in zip(scripts, self.base):
            for off, by in sc.init:
                self.src[b + off:b + off + len(by)] = by
        self.set = amd.CompressStreamsHC(len(scripts), level)
        self.rounds = 0

    def state(self, s):
        pe, pl, ee, el, ix = self.set.state([s])[0]
        b = self.base[s]
        return (pe - b, pl, ee - b if el else 0, el, ix) if (pe or pl or el or ix) else (0, 0, 0, 0, 0)

    def run(self, calls):
        """calls[s] = cut_into_calls of script s -> per script what run_cut gives"""
        res = [[None] * len(sc.ops) for sc in self.scripts]
        at = [0] * len(self.scripts)
        while True:
            ids, offs, lens, caps, first, who = [], [], [], [], [0], []
            for s, sc in enumerate(self.scripts):
                b = self.base[s]
                while at[s] < len(calls[s]) and isinstance(calls[s][at[s]], int):   # the state edits in front of the stream's next call
                    i = calls[s][at[s]]; o = sc.ops[i]; at[s] += 1
                    if o.kind == "L":
                        self.set.loadDict(s, b + o.off, o.n)
                        res[s][i] = ("L", self.state(s))
                    else:
                        end = self.set.state([s])[0][0]
                        kept = self.set.saveDict(s, b + o.off, o.k)
                        self.src[b + o.off:b + o.off + kept] = bytes(self.src[end - kept:end])
                        res[s][i] = ("S", kept, self.state(s))
                if at[s] == len(calls[s]):
                    continue
                call = calls[s][at[s]]; at[s] += 1
                for i in call:
                    o = sc.ops[i]
                    self.src[b + o.off:b + o.off + len(o.data)] = o.data
                    offs.append(b + o.off); lens.append(o.n); caps.append(o.cap)
                ids.append(s); first.append(len(offs)); who.append((s, call))
            if not ids:
                return res
            self.rounds += 1
            doff, total = [], GUARD
            for c in caps:
                doff.append(total); total += max(c, 0) + GUARD
            dst = bytearray(b"\xEE" * total)
            out = self.set.compress(ids, bytes(self.src), offs, lens, first, dst, doff, caps)
            k = 0
            for s, call in who:
                for j, i in enumerate(call):
                    r, cap = max(out[k], 0), max(caps[k], 0)
                    assert dst[doff[k] - GUARD:doff[k]] == b"\xEE" * GUARD and dst[doff[k] + cap:doff[k] + cap + GUARD] == b"\xEE" * GUARD, "written outside the slot"
                    assert r == 0 or dst[doff[k] + r:doff[k] + cap] == b"\xEE" * (cap - r), "written past the result"
                    res[s][i] = ("B", out[k], bytes(dst[doff[k]:doff[k] + r]), self.state(s) if j == len(call) - 1 else None)
                    k += 1


def drive(amd, rr, scripts, level, rng, how="random", left_out=None):
    fleet = Fleet(amd, scripts, level)
    got = fleet.run([cut_into_calls(sc, how, rng) for sc in scripts])
    bad = []
    for sc, g in zip(scripts, got):
        compare(sc, rr.run(sc, clamp(level)), g, level, bad, (how,), left_out)
    return bad, fleet


def make(layout, data, rng, tag, maxb=1024, n_blocks=16):
    d = data[:n_blocks * maxb]
    s = sizes_of(rng, len(d), maxb)
    if layout == "contiguous":
        return lay_contiguous(tag, d, s)
    if layout == "two":
        return lay_two_buffers(tag, d, s, 100, maxb)
    if layout == "adjacent":
        return lay_two_buffers(tag, d, s, 0, maxb)
    if layout == "ring":
        return lay_ring(tag, d, s, 5 * maxb + 100)
    if layout == "save":
        return lay_save_area(tag, d[:6 * maxb], sizes_of(rng, 6 * maxb, maxb), rng.choice([0, 3, 4, 100, maxb, 65536, 70000]), maxb)
    return lay_dict_elsewhere(tag, data[-2000:], d, s, follow=rng.random() < 0.3)
