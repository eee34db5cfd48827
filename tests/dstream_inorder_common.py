"""Shared pieces of the in-order stream decoder's tests (test_dstream_inorder_plain.py, test_dstream_inorder_hostsim.py,
test_dstream_inorder_abi.py, test_gpu_dstream_inorder.py, dstream_inorder_multidev_child.py): the layouts in which a block's slot
overlaps the history the block can reach, on top of dstream_common's streams and reference calls.

  m-fit / m-max   liblz4's minimal ring, LZ4_decoderRingBufferSize(max_block) = 65536 + 14 + max_block bytes.  The blocks are layout a's:
                  40 .. 90 pieces of 1 .. max_block bytes at max_block 4096 compressed by a contiguous writer -- and 4096 / max_block
                  times as many at 1024 and 64: a slot can overlap reachable history only once some 64 KB have been decoded, which
                  40 .. 90 small pieces never reach --; only their `off` is re-placed: the ring wraps to 0 when the block's true size
                  no longer fits (fit) or when max_block no longer fit (max).  dst_cap = size, or (full=True) min(max_block, ring - off).
                  A stream starts up to half its length in front of the ring's end.
  s               rings in step with the writer's (liblz4's ring-buffer streaming example): the writer itself wraps to 0 when the next
                  piece no longer fits -- 8192/1500 fixed (dstream_common's layout g, its maker), 8192/1..1500, 4096/1..1000,
                  1024/1..300, 70000/1..4096.  Most slots overlap.
  grid            hand-built two-block streams: block 0 is 600 literals at window offset 1000; block 1 jumps to a slot that reaches into
                  block 0 and is `lit` literals, ONE match whose source lies `ahead` bytes in front of its own destination inside block 0,
                  and a literal tail -- of 300 bytes (liblz4's fast loop runs), of 6 bytes (its safe loop alone), or ("cross") of 6 bytes
                  behind a match that starts near the dictionary's end, runs past it and continues in the block's own first bytes.
                  dst_cap = size + 64.  Expected bytes: the plain definition's (plain_block), nothing else.
  behind          the same two blocks with the match's source `k` bytes BEHIND its destination inside the overlapped dictionary, the
                  match longer than k: byte-forward, the match reads what it has just written (a pattern of period k).  k below the
                  lane group's chunk (1 .. 7) is the core's pattern copy, k from the chunk up to the match length the copy in pieces
                  behind waits.  Not an encoder's output; the contract promises the plain definition there too.

All of these streams are `exact` in dstream_common's sense: the window is compared, byte for byte, with the replay of the reference's
decoded bytes block by block in order (NOT with the reference's window: liblz4 over-stores inside a slot whose capacity exceeds the
block) -- and on the grid with the plain definition's."""
from dstream_common import (CHAIN_STOPPED, FILL, Block, Stream, book1, cut_pieces, lit_block, make_stream, ring_place, rng_for)  # noqa: F401
from conftest import lz4_seq

RING_BLOCKS = (4096, 1024, 64)
S_RINGS = ((8192, 1, 1500), (4096, 1, 1000), (1024, 1, 300), (70000, 1, 4096))
GRID_AHEAD = (1, 2, 7, 8, 9, 15, 16, 17, 30, 31, 32, 33, 47, 48, 63, 64, 65, 100, 200)
GRID_LIT = (0, 1, 7, 14, 15, 16, 31, 32, 33, 40, 100)
GRID_ML = (4, 5, 8, 15, 16, 17, 19, 20, 32, 33, 64, 65, 200)
GRID_TAILS = ("long", "short", "cross")
GRID_WIN = 1900


def ring_size(max_block):
    """LZ4_DECODER_RING_BUFFER_SIZE(max_block)"""
    return 65536 + 14 + max_block


# ---- the plain definition ----
def plain_block(win, state, off, comp):
    """One VALID block decoded into the bytearray `win` at `off` by the plain definition: sequence by sequence, literals first, then
    the match byte by byte forward, each byte read at the moment it is due.  Sources follow the stream state as lz4_decode_stream.h
    states it: the prefix directly in front of the block, else offset - position bytes back from ext_end, and a match that runs past
    the dictionary's end continues at the prefix's start (the block's own start without a prefix) -> (decoded size, state behind it)"""
    pe, pl, ee, el = state
    grows = pl != 0 and pe == off
    if pl != 0 and not grows:
        ee, el = pe, pl
    start = off - (min(pl, 65535) if grows else 0)      # where output position 0 lies
    ip, op, n = 0, off, len(comp)
    while True:
        tok = comp[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = comp[ip]; ip += 1; lit += b
                if b != 255:
                    break
        win[op:op + lit] = comp[ip:ip + lit]
        ip += lit; op += lit
        if ip >= n:
            break
        o = comp[ip] | (comp[ip + 1] << 8); ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = comp[ip]; ip += 1; ml += b
                if b != 255:
                    break
        ml += 4
        in_dict = o > op - start
        s = ee - (o - (op - start)) if in_dict else op - o
        for _ in range(ml):
            if in_dict and s == ee:
                s, in_dict = start, False
            win[op] = win[s]
            op += 1; s += 1
    r = op - off
    if r > 0:
        pe, pl = (pe + r, pl + r) if grows else (off + r, r)
    return r, (pe, pl, ee, el)


def plain_stream(s, wants_out):
    """stream s (no outside dictionary) through plain_block from a FILL-initialised window, up to its first block the reference did not
    decode -> [bytes of block k as they stood directly behind block k]"""
    win, st, out = bytearray([FILL]) * s.win_len, tuple(s.state), []
    for b, r in zip(s.blocks, wants_out):
        if r < 0:
            break
        got, st = plain_block(win, st, b.off, b.comp)
        assert got == r, (s.name, got, r)
        out.append(bytes(win[b.off:b.off + got]))
    return out


def slot_overlaps(state, off, cap):
    """the walk's per-block test, restated: does [off, off + cap) intersect the piece of the external dictionary the block can reach?"""
    pe, pl, ee, el = state
    grows = pl != 0 and pe == off
    if pl != 0 and not grows:
        ee, el = pe, pl
    if cap <= 0 or pl == 0 or el == 0:
        return False
    reach = min(el, 65535 - (min(pl, 65535) if grows else 0))
    return reach != 0 and off < ee and off + cap > ee - reach


def count_overlaps(s, w):
    """how many blocks of stream s (one call; w: the reference's Want) have a slot that overlaps reachable history"""
    st, n = tuple(s.state), 0
    for b, r in zip(s.blocks, w.out):
        if r == CHAIN_STOPPED:
            break
        n += 1 if slot_overlaps(st, b.off, b.cap) else 0
        pe, pl, ee, el = st
        grows = pl != 0 and pe == b.off
        if pl != 0 and not grows:
            ee, el = pe, pl
        if r > 0:
            pe, pl = (pe + r, pl + r) if grows else (b.off + r, r)
        st = (pe, pl, ee, el)
        if r < 0:
            break
    return n


# ---- the layouts ----
def minimal_ring_stream(rs, rng, data, max_block, rule, full, tag=""):
    """layout a's contiguous writer, the blocks re-placed in the minimal ring of max_block by `rule` ("fit" / "max")"""
    ring = ring_size(max_block)
    pieces = cut_pieces(data, rng, rng.randrange(40, 91) * (4096 // max_block), 1, max_block)
    s = rs.write("m-%s%s mb=%d %s" % (rule, "-full" if full else "", max_block, tag), "m", sum(map(len, pieces)) + 16, pieces,
                 lambda k, n, pos: pos, True, zero_at_jump=False)
    total = sum(b.size for b in s.blocks)
    pos = ring - rng.randrange(0, max(1, min(ring, total) // 2))     # (the first block wraps at once where it does not fit)
    for b in s.blocks:
        if pos + (b.size if rule == "fit" else max_block) > ring:
            pos = 0
        b.off = pos
        b.cap = min(max_block, ring - pos) if full else b.size
        pos += b.size
    s.win_len = ring
    return s


def step_ring_stream(rs, rng, data, ring, lo, hi, tag="", n_blocks=None):
    """a ring in step with the writer's: the writer's own buffer is the ring"""
    pieces = cut_pieces(data, rng, n_blocks or rng.randrange(20, 61), lo, hi)
    return rs.write("s %d/%d..%d %s" % (ring, lo, hi, tag), "s", ring, pieces, ring_place(ring), True, zero_at_jump=False)


def overlap_set(rs, rng, per_kind, blocks=RING_BLOCKS):
    """per_kind streams of every m-* kind (rule x capacity x max_block) and of every s ring -> [Stream], all `exact`"""
    data = book1()
    out = []
    for mb in blocks:
        for rule in ("fit", "max"):
            for full in (False, True):
                out += [minimal_ring_stream(rs, rng, data, mb, rule, full, "#%d" % t) for t in range(per_kind)]
    for t in range(per_kind):
        g = make_stream(rs, "g", rng, data, tag="(s 8192/1500) #%d" % t)
        g.exact = True
        out.append(g)
    for ring, lo, hi in S_RINGS:
        out += [step_ring_stream(rs, rng, data, ring, lo, hi, "#%d" % t) for t in range(per_kind)]
    return out


def hostile_overlap_set(rs, rng, per_kind=2):
    """dstream_common.hostile_set's four faults (a flipped byte, a capacity one short, a negative source length, a negative capacity) on
    streams of the overlap layouts"""
    out = []
    for t, s in enumerate(overlap_set(rs, rng, per_kind, blocks=(4096, 64))):
        real = [i for i, b in enumerate(s.blocks) if b.size]
        i = rng.choice(real[len(real) // 2:])          # (in the stream's second half: behind the wrap)
        b = s.blocks[i]
        kind = t % 4
        if kind == 0:
            c = bytearray(b.comp); j = rng.randrange(len(c)); c[j] ^= 1 << rng.randrange(8)
            s.blocks[i] = Block(c, b.off, b.cap, None); s.name += " flipped"
        elif kind == 1:
            s.blocks[i] = Block(b.comp, b.off, b.size - 1, None); s.name += " cap-1"
        elif kind == 2:
            s.blocks[i] = Block(b.comp, b.off, b.cap, None, src_len=-1); s.name += " src_len<0"
        else:
            s.blocks[i] = Block(b.comp, b.off, -5, None); s.name += " dst_cap<0"
        out.append(s)
    return out


# ---- the grid ----
class GridCase:
    def __init__(self, stream, ahead, lit, ml, tail):
        self.stream, self.ahead, self.lit, self.ml, self.tail = stream, ahead, lit, ml, tail


def grid_case(rng, ahead, lit, ml, tail):
    """block 0: 600 literals at 1000.  long / short: the match's source is byte `delta` of block 0, `ahead` bytes in front of the
    match's destination, so the slot begins below 1000.  cross: the source begins ml // 2 bytes in front of block 0's end, the match
    runs past it into the block's own first bytes"""
    b0 = Block(lit_block(600, rng), 1000, 600, 600)
    if tail == "cross":
        c = ml // 2
        d = 1600 - c - ahead - lit
        off = lit + c
    else:
        delta = min((7 * lit + ml) % 40, lit + ahead - 1)
        d = 1000 + delta - ahead - lit
        off = 1600 - (d + lit + ahead) + lit
    tl = 300 if tail == "long" else 6
    comp = lz4_seq(lit, ml, off, rng) + lit_block(tl, rng)
    size = lit + ml + tl
    assert 0 <= d and d + size + 64 <= GRID_WIN and 1 <= off <= 65535
    s = Stream("grid %s ahead=%d lit=%d ml=%d" % (tail, ahead, lit, ml), "grid", GRID_WIN, [b0, Block(comp, d, size + 64, size)], True)
    return GridCase(s, ahead, lit, ml, tail)


def grid(rng, tails=GRID_TAILS):
    return [grid_case(rng, a, l, m, t) for t in tails for a in GRID_AHEAD for l in GRID_LIT for m in GRID_ML]


BEHIND_K = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 64, 100)
BEHIND_ML = (4, 8, 9, 20, 65, 200)
BEHIND_LIT = (0, 7, 40)


def behind_case(rng, k, lit, ml):
    """block 1 at 1100 inside block 0; the match of ml > k bytes has its source k bytes behind its own destination, wholly in block 0"""
    b0 = Block(lit_block(600, rng), 1000, 600, 600)
    d = 1100
    off = lit + (1600 - (d + lit - k))
    comp = lz4_seq(lit, ml, off, rng) + lit_block(6, rng)
    size = lit + ml + 6
    assert d + lit - k >= 1000 and d + lit - k + ml <= 1600 and d + size + 64 <= GRID_WIN
    s = Stream("behind k=%d lit=%d ml=%d" % (k, lit, ml), "grid", GRID_WIN, [b0, Block(comp, d, size + 64, size)], True)
    return GridCase(s, -k, lit, ml, "behind")


def behind_grid(rng):
    return [behind_case(rng, k, l, m) for k in BEHIND_K for l in BEHIND_LIT for m in BEHIND_ML if m > k]


def grid_expected(case):
    """the plain definition's window behind both blocks, from a FILL-initialised one -> (bytes of the window, [r0, r1])"""
    win, st, rs_ = bytearray([FILL]) * GRID_WIN, (0, 0, 0, 0), []
    for b in case.stream.blocks:
        r, st = plain_block(win, st, b.off, b.comp)
        rs_.append(r)
    return bytes(win), rs_


# ---- the C call ----
def inorder_decoder(L, name="lz4hip_decompress_safe_stream_inorder_batch"):
    """dstream_common.run_placed's `decode` over lz4hip_decompress_safe_stream_inorder_batch itself (L: the package's ctypes library)"""
    import ctypes as C

    def arr(t, v):
        return (t * max(len(v), 1))(*v)

    def decode(state, src, so, sl, first, dst, do, dc, wo, wl):
        n, nc = len(so), len(state)
        st = (C.c_uint64 * max(4 * nc, 1))(*[int(v) for s in state for v in s])
        out = (C.c_int32 * max(n, 1))(*([12345] * max(n, 1)))
        dbuf = (C.c_uint8 * len(dst)).from_buffer(dst)
        rc = getattr(L, name)(st, src, arr(C.c_uint64, so), arr(C.c_int32, sl), arr(C.c_uint32, first), dbuf, arr(C.c_uint64, do), arr(C.c_int32, dc),
                              arr(C.c_uint64, wo), arr(C.c_uint64, wl), out, n, nc)
        del dbuf
        return rc, list(out[:n]), [tuple(st[4 * c:4 * c + 4]) for c in range(nc)]
    return decode


def layout_streams(rs, rng, kind, count):
    """`count` streams of one new layout: ("m", rule, max_block, full) or ("s", ring, lo, hi) or ("g",)"""
    data = book1()
    if kind[0] == "m":
        return [minimal_ring_stream(rs, rng, data, kind[2], kind[1], kind[3], "#%d" % t) for t in range(count)]
    if kind[0] == "g":
        out = [make_stream(rs, "g", rng, data, tag="(s 8192/1500) #%d" % t) for t in range(count)]
        for s in out:
            s.exact = True
        return out
    return [step_ring_stream(rs, rng, data, kind[1], kind[2], kind[3], "#%d" % t) for t in range(count)]
