"""Shared pieces of the stream decoder's tests (test_dstream_hostsim.py, test_dstream_abi.py, test_gpu_dstream.py, dstream_multidev_child.py):
streams whose blocks land anywhere -- the layouts liblz4's users decode into -- with every expected value taken from the reference
library alone.  Each stream gets ONE LZ4_streamDecode_t; LZ4_decompress_safe_continue is called at the same destinations, and its four
fields (1.9.3: externalDict, extDictSize, prefixEnd, prefixSize) are read back through ctypes as offsets.  The inputs are written by the
reference's LZ4_compress_fast_continue on an encoder buffer of the same layout.

The layouts (a window is the stream's own piece of the destination; offsets below are relative to it):
  a  contiguous                                         exact
  b  two alternating buffers of one block               exact
  c  a 64 KB save area + a block area, the history moved there as LZ4_saveDict's users move it          exact
  d  a ring of 65535 + 2 x maxBlock that wraps to 0 when the next block no longer fits                   exact
  e  a ring of 200000 bytes, blocks up to 60000 (reaches the 64k-prefix branch)                          exact
  f  contiguous, starting from ONE shared dictionary outside every window (7, 4096, 70000 bytes); `lead`: the dictionary
     directly in front of the window                                                                     exact
  g  a ring of 8192 with 1500-byte blocks: slots overlap the history they can reach, so results and states are compared and
     nothing else
"exact" = every block's slot is disjoint from the history the block can reach: there the bytes are compared too.
A 0-byte block (the one-byte stream 00) falls at a jump in every layout: liblz4 then replaces the external dictionary by the prefix
and leaves the prefix standing."""
import ctypes as C
import random

from conftest import calgary, lz4_seq

CHAIN_STOPPED = -(2 ** 31) + 6          # include/lz4hip.h LZ4HIP_CHAIN_STOPPED
GUARD = 128
FILL = 0xEE
BRANCHES = ("plain", "prefix64k", "smallprefix", "doubledict", "extdict")
DICT = "D"                               # a state's end offset that is the end of the stream's outside dictionary


def book1():
    return calgary("book1")


def rng_for(seed):
    return random.Random(seed)


class Block:
    """one block of a stream: `comp` decoded to the window offset `off` with the capacity `cap`; `size` = what the writer put in (None:
    not a writer's block).  src_len / dst_cap: what the call is given where that is not len(comp) / cap (the negative-length cases)"""

    def __init__(self, comp, off, cap, size=None, src_len=None):
        self.comp, self.off, self.cap, self.size = bytes(comp), int(off), int(cap), size
        self.src_len = len(self.comp) if src_len is None else src_len


class Stream:
    """one stream: its window's length, its blocks, the state it starts from (window-relative ends; DICT: the dictionary's end), the
    outside dictionary (None: none; lead: it lies directly in front of the window) and `before[k]`: what the caller does to window and
    state in front of block k, as [(dst offset, src offset, length)] moves + a (prefix_end, prefix_len) to set (layout c)"""

    def __init__(self, name, layout, win_len, blocks, exact, dictionary=None, lead=False, state=(0, 0, 0, 0)):
        self.name, self.layout, self.win_len, self.blocks, self.exact = name, layout, int(win_len), blocks, exact
        self.dictionary, self.lead, self.state = dictionary, lead, state
        self.before = {}


def model_branch(state, off):
    """the branch LZ4_decompress_safe_continue takes for a block at `off` from `state` (the issue's state machine)"""
    pe, pl, ee, el = state
    if pl == 0:
        return "plain"
    if pe == off:
        return "prefix64k" if pl >= 65535 else ("smallprefix" if el == 0 else "doubledict")
    return "extdict"


class Want:
    """what the reference says about one stream cut into calls: per block the result (CHAIN_STOPPED behind a call's first negative
    one), the bytes it decoded and the branch taken; per call the state behind it"""

    def __init__(self):
        self.out, self.data, self.branch, self.states = [], [], [], []


class RefStream:
    """the reference library's stream entry points"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_createStream.restype = C.c_void_p
        L.LZ4_freeStream.argtypes = [C.c_void_p]
        L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_saveDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.LZ4_createStreamDecode.restype = C.c_void_p
        L.LZ4_freeStreamDecode.argtypes = [C.c_void_p]
        L.LZ4_setStreamDecode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_decompress_safe_continue.restype = C.c_int
        L.LZ4_decompress_safe_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    # ---- the writer ----
    def write(self, name, layout, win_len, pieces, place, exact, dictionary=None, lead=False, save_area=0, zero_at_jump=True, rng=None):
        """pieces (the blocks' contents) compressed by ONE LZ4_stream_t on an encoder buffer of the decoder's layout: place(k, n, pos) ->
        the window offset of block k of n bytes when the block before it ended at pos.  save_area: layout c.  A 0-byte block is put in
        front of the first block that jumps (zero_at_jump), at that block's place -- or, where no block jumps, at the window's start"""
        L = self.L
        D = len(dictionary) if dictionary else 0
        gap = 0 if lead else GUARD
        buf = C.create_string_buffer(D + gap + win_len + 64)
        win = C.addressof(buf) + D + gap
        st = L.LZ4_createStream()
        if D:
            C.memmove(buf, dictionary, D)
            L.LZ4_loadDict(st, C.addressof(buf), D)
        s = Stream(name, layout, win_len, [], exact, dictionary, lead, (DICT, D, 0, 0) if D else (0, 0, 0, 0))
        pos, total, zeroed, prev_end = 0, 0, not zero_at_jump, (None if not D else (0 if lead else DICT))
        for k, p in enumerate(pieces):
            n = len(p)
            if save_area and k:   # LZ4_saveDict: the last <= 64 KB of history into the save area, so that they END where the block area
                keep = min(save_area, total)   # begins and the history goes on growing; the decoder's caller moves its bytes the same way
                assert L.LZ4_saveDict(st, win + save_area - keep, keep) == keep
                s.before[len(s.blocks)] = ([(save_area - keep, pos - keep, keep)], (save_area, keep))
                prev_end = save_area if keep else prev_end
            off = place(k, n, pos)
            assert 0 <= off and off + n <= win_len, (name, k, off, n)
            jump = prev_end is not None and prev_end != off
            if not zeroed and (jump or (k == len(pieces) - 1 and k)):
                # (a stream without a jump: the 0-byte block goes to the window's start, a new place for every stream that has come this far)
                zoff = off if jump else 0
                if zoff != prev_end:
                    s.blocks.append(Block(b"\0", zoff, rng.choice((0, 0, 16)) if rng else 0, 0))
                    zeroed = True
            C.memmove(win + off, p, n)
            dst = C.create_string_buffer(n + n // 255 + 32)
            r = L.LZ4_compress_fast_continue(st, win + off, dst, n, len(dst), 1)
            assert r > 0
            s.blocks.append(Block(dst.raw[:r], off, n, n))
            pos, total = off + n, total + n
            if n:
                prev_end = pos
        L.LZ4_freeStream(st)
        return s

    # ---- the expected values ----
    def decode(self, s, cuts):
        """stream s decoded by ONE LZ4_streamDecode_t, its blocks cut into calls at `cuts` (ascending block indices, the last one
        len(s.blocks)).  Within a call a negative result ends the stream's part: the blocks behind it get CHAIN_STOPPED (the
        engine's rule; liblz4 has left its state as it was in front of that block -- but for a jump's ext = prefix).  A block with a
        negative length is not shown to the reference: it counts as answered with -1, a jump's ext = prefix included"""
        L = self.L
        D = len(s.dictionary) if s.dictionary else 0
        gap = 0 if s.lead else GUARD
        buf = C.create_string_buffer(D + gap + GUARD + s.win_len + GUARD)
        C.memset(buf, FILL, len(buf))
        base = C.addressof(buf)
        win = base + D + gap + (0 if s.lead else GUARD)
        if D:
            C.memmove(base, s.dictionary, D)
        sd = L.LZ4_createStreamDecode()
        fields = (C.c_uint64 * 4).from_address(sd)

        def rel(p, n):
            if n == 0:
                return 0
            if D and p == base + D and not s.lead:
                return DICT
            return p - win

        def state():
            return (rel(fields[2], fields[3]), fields[3], rel(fields[0] + fields[1], fields[1]), fields[1])   # (externalDict is the START)

        pe, pl = s.state[0], s.state[1]
        L.LZ4_setStreamDecode(sd, (base if pe == DICT else win + pe - pl) if pl else None, pl)
        w = Want()
        k = 0
        for cut in cuts:
            alive = True
            while k < cut:
                b = s.blocks[k]
                if k in s.before:
                    moves, (se, sn) = s.before[k]
                    for d_, s_, n_ in moves:
                        C.memmove(win + d_, win + s_, n_)
                    L.LZ4_setStreamDecode(sd, win + se - sn, sn)
                if not alive:
                    w.out.append(CHAIN_STOPPED); w.data.append(b""); w.branch.append(None)
                    k += 1
                    continue
                now = state()
                w.branch.append(model_branch(now, b.off))
                if b.src_len < 0 or b.cap < 0:
                    r = -1
                    if w.branch[-1] == "extdict":
                        fields[0], fields[1] = fields[2] - fields[3], fields[3]
                else:
                    sb = C.create_string_buffer(b.comp + b"\0" * 64, len(b.comp) + 64)
                    r = L.LZ4_decompress_safe_continue(sd, sb, win + b.off, b.src_len, b.cap)
                w.out.append(r)
                w.data.append(C.string_at(win + b.off, r) if r > 0 else b"")
                if r < 0:
                    alive = False
                k += 1
            w.states.append(state())
        # (the reference wrote nothing outside the window)
        assert C.string_at(win + s.win_len, GUARD) == bytes([FILL]) * GUARD
        assert s.lead or C.string_at(win - GUARD, GUARD) == bytes([FILL]) * GUARD
        L.LZ4_freeStreamDecode(sd)
        return w


def same_state(got, want):
    """lengths always; an end only where its length is not 0 (liblz4's pointers of empty histories are whatever they were)"""
    return got[1] == want[1] and got[3] == want[3] and (want[1] == 0 or got[0] == want[0]) and (want[3] == 0 or got[2] == want[2])


# ---- the layouts ----
def cut_pieces(data, rng, n_blocks, lo, hi):
    """n_blocks pieces of lo .. hi bytes from consecutive places of `data` (real text: later blocks match into earlier ones)"""
    out, o = [], rng.randrange(0, max(1, len(data) - n_blocks * hi - 1))
    for _ in range(n_blocks):
        n = rng.randrange(lo, hi + 1)
        if rng.random() < 0.15:
            back = rng.randrange(0, min(o, 30000) + 1)      # a block seen a while ago: far matches
            out.append(data[o - back:o - back + n])
        else:
            out.append(data[o:o + n]); o += n
    return out


def ring_place(ring):
    return lambda k, n, pos: pos if pos + n <= ring else 0


def make_stream(rs, layout, rng, data, n_blocks=None, tag="", zero_at_jump=True, dictionary=None, lead=False, max_block=4096):
    name = "%s%s %s" % (layout, "-lead" if lead else "", tag)
    if layout == "a":
        n = n_blocks or rng.randrange(4, 30)
        p = cut_pieces(data, rng, n, 0, max_block)
        return rs.write(name, "a", sum(map(len, p)) + 16, p, lambda k, n_, pos: pos, True, zero_at_jump=zero_at_jump, rng=rng)
    if layout == "b":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(4, 30), 0, max_block)
        return rs.write(name, "b", 2 * max_block, p, lambda k, n_, pos: (k & 1) * max_block, True, rng=rng)
    if layout == "c":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(4, 40), 1, max_block)
        return rs.write(name, "c", 65536 + max_block, p, lambda k, n_, pos: 65536, True, save_area=65536, rng=rng)
    if layout == "d":
        ring = 65535 + 2 * max_block
        p = cut_pieces(data, rng, n_blocks or rng.randrange(20, 60), 0, max_block)
        return rs.write(name, "d", ring, p, ring_place(ring), True, rng=rng)
    if layout == "e":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(6, 14), 0, 60000)
        return rs.write(name, "e", 200000, p, ring_place(200000), True, rng=rng)
    if layout == "f":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(6, 30), 0, max_block)
        return rs.write(name, "f", sum(map(len, p)) + 16, p, lambda k, n_, pos: pos, True, dictionary=dictionary, lead=lead, rng=rng)
    if layout == "g":
        p = cut_pieces(data, rng, n_blocks or rng.randrange(10, 40), 1500, 1500)
        return rs.write(name, "g", 8192, p, ring_place(8192), False, rng=rng)
    raise ValueError(layout)


def shared_dicts(data):
    return {7: data[1000:1007], 4096: data[20000:24096], 70000: data[100000:170000]}


def layout_set(rs, rng, per_layout, dicts=None):
    """per_layout streams of every layout a .. g (f: spread over the three dictionaries, a sixth of them `lead`) -> [Stream]"""
    data = book1()
    dicts = dicts or shared_dicts(data)
    out = []
    for layout in "abcdefg":
        for t in range(per_layout):
            if layout == "f":
                size = (7, 4096, 70000)[t % 3]
                out.append(make_stream(rs, "f", rng, data, tag="dict%d #%d" % (size, t), dictionary=dicts[size], lead=(t % 6 == 5)))
            else:
                out.append(make_stream(rs, layout, rng, data, tag="#%d" % t))
    return out


def random_cuts(n, calls, rng):
    """n blocks in `calls` calls (fewer when n is small): ascending cut points, the last one n"""
    calls = max(1, min(calls, n))
    return sorted(rng.sample(range(1, n), calls - 1)) + [n] if n > 1 else [n]


# ---- the hostile cases ----
def lit_block(n, rng):
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


def offset_rule_streams(rng):
    """offsets at and one past the reachable history, with ext_len below and at least 65536.  Block 0 is E literals far up in the
    window, block 1 is P literals at the window's start (a jump: ext = block 0), block 2 follows block 1 (doubleDict) or lands
    elsewhere (forceExtDict of block 1) and holds one match of the given offset behind one literal"""
    out = []
    P = 10
    for E in (100, 65523, 65524, 65535, 65536, 70000):   # (65523: the farthest offset there is, 65535, is one past the history)
        for off in sorted({1 + P + E, 1 + P + E + 1, 65535}):
            if not 1 <= off <= 65535:
                continue
            comp = lz4_seq(1, 6, off, rng) + bytes([6 << 4]) + rng.randbytes(6)
            blocks = [Block(lit_block(E, rng), 1000, E, E), Block(lit_block(P, rng), 0, P, P), Block(comp, P, 13)]
            out.append(Stream("double E=%d off=%d" % (E, off), "h", 1000 + E + 16, blocks, True))
    for off in (1 + P, 1 + P + 1):
        comp = lz4_seq(1, 6, off, rng) + bytes([6 << 4]) + rng.randbytes(6)
        out.append(Stream("ext P=%d off=%d" % (P, off), "h", 600, [Block(lit_block(P, rng), 0, P, P), Block(comp, 500, 13)], True))
    return out


def hostile_set(rs, rng, per_kind=8):
    """per exact layout: a flipped byte per stream, a capacity one short, a negative length -- and the offset-rule streams"""
    data = book1()
    dicts = shared_dicts(data)
    out = []
    for layout in "abcdef":
        for t in range(per_kind):
            kw = dict(dictionary=dicts[(7, 4096, 70000)[t % 3]]) if layout == "f" else {}
            s = make_stream(rs, layout, rng, data, tag="hostile #%d" % t, **kw)
            real = [i for i, b in enumerate(s.blocks) if b.size]
            i = rng.choice(real)
            b = s.blocks[i]
            kind = t % 4
            if kind == 0:
                c = bytearray(b.comp); j = rng.randrange(len(c)); c[j] ^= 1 << rng.randrange(8)
                s.blocks[i] = Block(c, b.off, b.cap, None); s.name += " flipped"
            elif kind == 1:
                s.blocks[i] = Block(b.comp, b.off, b.cap - 1, None); s.name += " cap-1"
            elif kind == 2:
                s.blocks[i] = Block(b.comp, b.off, b.cap, None, src_len=-1); s.name += " src_len<0"
            else:
                s.blocks[i] = Block(b.comp, b.off, -5, None); s.name += " dst_cap<0"
            if layout == "c":      # (its caller goes on moving "the last 64 KB" into the save area: a failed block's slot, whose bytes are
                s.exact = False    # nobody's, becomes history -- results and states still are liblz4's, the bytes behind it need not be)
            out.append(s)
    return out + offset_rule_streams(rng)


# ---- many streams in one destination, as the C call takes them ----
class Placed:
    """streams side by side in one destination: the shared dictionaries first, then every window behind GUARD bytes of FILL (a `lead`
    stream: its own copy of the dictionary directly in front of its window).  call(k) -> the arrays of call k (every stream's blocks
    [cuts[k - 1], cuts[k])); apply(...) compares what came back"""

    def __init__(self, streams, cuts):
        self.streams, self.cuts = streams, cuts
        self.dst = bytearray()
        self.dict_end = {}
        for s in streams:
            if s.dictionary and not s.lead and s.dictionary not in self.dict_end:
                self.dst += s.dictionary
                self.dict_end[s.dictionary] = len(self.dst)
                self.dst += bytes([FILL]) * GUARD
        self.win = []
        for s in streams:
            self.dst += bytes([FILL]) * GUARD
            if s.lead:
                self.dst += s.dictionary
            self.win.append(len(self.dst))
            self.dst += bytes([FILL]) * s.win_len
        self.dst += bytes([FILL]) * GUARD
        self.state = [self.absolute(i, s.state) for i, s in enumerate(streams)]
        self.model = bytearray(self.dst)     # what the destination must look like (exact streams' windows; everything outside windows)

    def dend(self, i):
        s = self.streams[i]
        return self.win[i] if s.lead else self.dict_end[s.dictionary]

    def absolute(self, i, st):
        f = lambda e, n: 0 if n == 0 else (self.dend(i) if e == DICT else self.win[i] + e)
        return (f(st[0], st[1]), st[1], f(st[2], st[3]), st[3])

    def relative(self, i, st):
        s = self.streams[i]
        f = lambda e, n: 0 if n == 0 else (DICT if s.dictionary and not s.lead and e == self.dend(i) else e - self.win[i])
        return (f(st[0], st[1]), st[1], f(st[2], st[3]), st[3])

    def call(self, k):
        """-> (src, src_off, src_len, chain_first, dst_off, dst_cap, win_off, win_len, [(stream, block)])"""
        src, so, sl, first, do, dc, idx = bytearray(), [], [], [0], [], [], []
        for i, s in enumerate(self.streams):
            lo, hi = (self.cuts[i][k - 1] if k else 0), self.cuts[i][k]
            for j in range(lo, hi):
                b = s.blocks[j]
                if j in s.before:          # the caller's own moves and LZ4_setStreamDecode in front of this block (layout c: one block per call)
                    assert j == lo
                    moves, (se, sn) = s.before[j]
                    for d_, s_, n_ in moves:
                        for buf in (self.dst, self.model):
                            buf[self.win[i] + d_:self.win[i] + d_ + n_] = bytes(buf[self.win[i] + s_:self.win[i] + s_ + n_])
                    self.state[i] = (self.win[i] + se, sn, 0, 0)
                so.append(len(src)); sl.append(b.src_len); src += b.comp + bytes(3)
                do.append(self.win[i] + b.off); dc.append(b.cap); idx.append((i, j))
            first.append(len(so))
        # (a `lead` stream: the first call's window begins behind the dictionary -- the prefix ends exactly where the window begins --,
        # the later ones' at the dictionary's start: the prefix has grown into the window and must not straddle its edge)
        lead = [len(s.dictionary) if s.lead and k else 0 for s in self.streams]
        return (bytes(src) + bytes(64), so, sl, first, do, dc, [w - d for w, d in zip(self.win, lead)],
                [s.win_len + d for s, d in zip(self.streams, lead)], idx)

    def check(self, k, idx, out, wants, tag=()):
        """after call k: results, states, bytes (exact streams: the whole window against the replayed model; a failed block's slot is
        the one place left open) and every byte outside the windows"""
        bad = []
        for t, (i, j) in enumerate(idx):
            s, w = self.streams[i], wants[i]
            if int(out[t]) != w.out[j]:
                bad.append(("result", s.name, j, int(out[t]), w.out[j]))
            b = s.blocks[j]
            o = self.win[i] + b.off
            if w.out[j] > 0:
                self.model[o:o + w.out[j]] = w.data[j]
            elif w.out[j] < 0 and w.out[j] != CHAIN_STOPPED and b.cap > 0:
                self.model[o:o + b.cap] = self.dst[o:o + b.cap]
        for i, s in enumerate(self.streams):
            if not same_state(self.relative(i, self.state[i]), wants[i].states[k]):
                bad.append(("state", s.name, k, self.relative(i, self.state[i]), wants[i].states[k]))
            if not s.exact:
                self.model[self.win[i]:self.win[i] + s.win_len] = self.dst[self.win[i]:self.win[i] + s.win_len]
        if self.dst != self.model:
            d = next(x for x in range(len(self.dst)) if self.dst[x] != self.model[x])
            i = max((x for x in range(len(self.win)) if self.win[x] <= d), default=-1)
            bad.append(("bytes", self.streams[i].name if i >= 0 else None, k, d - (self.win[i] if i >= 0 else 0)))
        return [tuple(tag) + b for b in bad]


def padded_cuts(streams, calls, rng):
    """every stream cut into calls at random block boundaries, `calls` at the most -- a layout-c stream at every boundary, as its caller
    moves the history between two calls -- and padded to one number of calls: a stream that has run out sits in the later calls with
    an empty block range"""
    cuts = [list(range(1, len(s.blocks) + 1)) if s.before else random_cuts(len(s.blocks), calls, rng) for s in streams]
    most = max(map(len, cuts))
    return [c + [c[-1]] * (most - len(c)) for c in cuts]


def run_placed(streams, cuts, wants, decode, tag=()):
    """the streams side by side through `decode(state, src, src_off, src_len, first, dst, dst_off, dst_cap, win_off, win_len) ->
    (status, out, new state)`, call after call (cuts: padded_cuts'; wants[i] = RefStream.decode(streams[i], cuts[i])) -> mismatches"""
    p = Placed(streams, cuts)
    bad = []
    for k in range(len(cuts[0])):
        src, so, sl, first, do, dc, wo, wl, idx = p.call(k)
        rc, out, new = decode(p.state, src, so, sl, first, p.dst, do, dc, wo, wl)
        if rc != 0:
            return [tuple(tag) + ("status", k, rc)]
        p.state = [tuple(int(v) for v in st) for st in new]
        bad += p.check(k, idx, out, wants, tag)
        if len(bad) > 20:
            break
    return bad


def lib_decoder(L):
    """run_placed's `decode` over the C call itself (L: the package's ctypes library) -- no layer in between checks the arrays, so
    the negative lengths of the hostile cases reach the library"""
    def arr(t, v):
        return (t * max(len(v), 1))(*v)

    def decode(state, src, so, sl, first, dst, do, dc, wo, wl):
        n, nc = len(so), len(state)
        st = (C.c_uint64 * max(4 * nc, 1))(*[int(v) for s in state for v in s])
        out = (C.c_int32 * max(n, 1))(*([12345] * max(n, 1)))
        dbuf = (C.c_uint8 * len(dst)).from_buffer(dst)
        rc = L.lz4hip_decompress_safe_stream_batch(st, src, arr(C.c_uint64, so), arr(C.c_int32, sl), arr(C.c_uint32, first), dbuf, arr(C.c_uint64, do),
                                                   arr(C.c_int32, dc), arr(C.c_uint64, wo), arr(C.c_uint64, wl), out, n, nc)
        del dbuf
        return rc, list(out[:n]), [tuple(st[4 * c:4 * c + 4]) for c in range(nc)]
    return decode


def check_set(rs, streams, calls, rng, decode, tag=()):
    """the streams cut into `calls` calls at the most, the reference cut the same way, through `decode` -> (mismatches, calls made)"""
    cuts = padded_cuts(streams, calls, rng)
    wants = [rs.decode(s, c) for s, c in zip(streams, cuts)]
    return run_placed(streams, cuts, wants, decode, tag), len(cuts[0])


def stream_file(s, cuts):
    """stream s and its cut points for the C++ and JNI programs (tests/cpp/dstream_mirror_test.cpp says the format)"""
    import struct
    d = s.dictionary or b""
    q = lambda *v: struct.pack("<%dq" % len(v), *v)
    st = [(-1 if v == DICT else v) for v in s.state]
    out = q(s.win_len, len(d), 1 if s.lead else 0, len(s.blocks), len(cuts)) + q(*st) + q(*cuts)
    for b in s.blocks:
        assert b.src_len == len(b.comp)
        out += q(b.off, b.cap, b.src_len)
    return out + d + b"".join(b.comp for b in s.blocks)
