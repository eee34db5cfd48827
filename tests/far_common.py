"""Shared pieces of the far-offset tests (test_far_table.py on the CPU, test_gpu_far_offsets.py on the GPU): every device entry point
of include/lz4hip.h that takes 64-bit offsets, strides or lengths, run at offsets around and past 2^31 and 2^32.

The addresses of a launch are formed in the kernel wrappers of csrc/*.hip (a.src + a.src_off[b], ws + a.src_off[b], dst + k * slot),
not in the algorithm cores the lane simulator runs: an offset that is narrowed, sign-extended or multiplied in 32 bits there is
invisible to the CPU suite, and to a GPU test that packs its blocks from offset 0.

A FAR BUFFER is one allocation of RED + SPAN bytes; the library is handed the VIEW that starts RED bytes in.  An offset that loses its
upper half lands inside the view, one that is treated as a signed 32-bit value lands in the red zone in front of it: both belong to the
test, both show as a wrong byte, neither leaves the allocation.  The destination is filled with one byte before every call and, once
the expected regions are compared and refilled, must hold nothing else anywhere; the source holds a non-constant decoy pattern
around the placed inputs.

Expected values come from the reference library (`ref`, and the RefDict / hcdict Ref / ref_partial / ref_size helpers of the other
*_common modules) and, for the fast decoder and the block generator, from the oracle port -- never from this project's output.

TABLE names every entry point with its case builder and the GPU test that runs it; test_far_table.py fails when include/lz4hip.h
declares a *_dev function that is neither in TABLE nor in EXEMPT."""
import ctypes as C
import os
import random
import re
from typing import NamedTuple, Optional

from conftest import ROOT

_u8p = C.POINTER(C.c_uint8)

RED = (1 << 31) + 4096
SPAN = (1 << 32) + (1 << 22)
B31, B32 = 1 << 31, 1 << 32
CHUNK = 256 << 20                        # the whole-allocation scan goes in pieces of this size
TILE = 1 << 20                           # the decoy pattern: one random tile of this size, repeated
TAIL = 1 << 16                           # nothing is placed within this distance of the view's end (decoders read ahead of a stream)
PLACES = ("straddle31", "behind31", "straddle32", "past32", "control")
_ZONE = {"control": 1000, "behind31": B31 + (1 << 20) + 4097, "past32": B32 + (1 << 20) + 77}   # where each zone's first slot starts
_FALLBACK = {"straddle31": "behind31", "straddle32": "past32"}


def place_class(at, n):
    """the place class of the region [at, at + n) of the view (None: a neighbour of a straddling slot, no class of its own)"""
    if at < B31 < at + n:
        return "straddle31"
    if at < B32 < at + n:
        return "straddle32"
    if at < (1 << 30):
        return "control"
    if B31 <= at < B31 + (1 << 22):
        return "behind31"
    if at >= B32:
        return "past32"
    return None


class Placer:
    """hands out regions of the view, one zone per place class.  A boundary can be straddled by one region only: layout() chooses it
    (straddle); every other request for that class goes to the zone behind the boundary"""

    def __init__(self, gap):
        self.gap = gap
        self.cur = dict(_ZONE)

    def straddle(self, cls, n):
        assert n >= 2
        return (B31 if cls == "straddle31" else B32) - ((n // 2) | 1 if n > 2 else 1)

    def take(self, cls, n):
        cls = _FALLBACK.get(cls, cls)
        at = self.cur[cls]
        self.cur[cls] = (at + n + self.gap) | 1      # odd: never on a 128-byte line
        return at


STRADDLER_MIN = 64      # a slot that lies across a boundary carries at least this many compared bytes


class Slot(NamedTuple):
    """one block of a launch: `data` at src_at of the source view; it owns dst[dst_at, dst_at + own) of the destination view"""
    name: str
    data: bytes
    src_at: int
    dst_at: int
    own: int
    p1: int                  # the per-block int32 array next to the source length: capacity / target / decoded size
    ret: int                 # the reference's return value
    out: Optional[bytes]     # the reference's bytes at dst_at; None where the contract leaves them open (a failed block)
    p2: int = 0              # a second per-block parameter (partial decoder: the capacity) or result (destSize: the input consumed)


def _carries(item, has_out):
    """the item is worth a place across a boundary: its result is compared byte for byte (where the list has bytes at all) and is
    not trivial"""
    name, data, own, p1, ret, by, p2 = item
    if has_out:
        return by is not None and len(by) >= STRADDLER_MIN and len(data) >= STRADDLER_MIN
    return len(data) >= STRADDLER_MIN and ret >= 0


def layout(items, src_gap=67, dst_gap=41):
    """items = [(name, data, own, p1, ret, out, p2)] -> [Slot]: source and destination places are drawn independently -- block k's
    source takes class k, its slot class 2k + 3 + k // 5 of PLACES --, so a near source meets a far slot and the reverse.  The four
    regions that lie ACROSS 2^31 and 2^32 (one source and one slot each) go to four different items whose bytes are compared"""
    ps, pd = Placer(src_gap), Placer(dst_gap)
    has_out = any(it[5] for it in items)
    good = [k for k, it in enumerate(items) if _carries(it, has_out)]
    assert len(good) >= 4, "too few items with compared bytes to lie across the boundaries"
    pick = [good[(j * len(good)) // 4] for j in range(4)]
    src_st = {pick[0]: "straddle31", pick[2]: "straddle32"}
    dst_st = {pick[1]: "straddle31", pick[3]: "straddle32"}
    out = []
    for k, (name, data, own, p1, ret, by, p2) in enumerate(items):
        s_at = ps.straddle(src_st[k], len(data)) if k in src_st else ps.take(PLACES[k % 5], len(data))
        d_at = pd.straddle(dst_st[k], own) if k in dst_st and own >= 2 else pd.take(PLACES[(2 * k + 3 + k // 5) % 5], own)
        out.append(Slot(name, data, s_at, d_at, own, p1, ret, by, p2))
    return out


def check_layout(slots, need_dst=True):
    """what test_far_table.py asks of every case list: each place class on both sides, no overlap, everything inside the view and
    clear of its end, and a red zone that covers the sign-extension of every address used"""
    for side, regions in (("src", [(s.src_at, len(s.data)) for s in slots]), ("dst", [(s.dst_at, s.own) for s in slots])):
        if side == "dst" and not need_dst:
            continue
        seen = {place_class(at, n) for at, n in regions}
        assert set(PLACES) <= seen, (side, "no slot at", sorted(set(PLACES) - seen))
        has_out = any(s.out for s in slots)
        for s, (at, n) in zip(slots, regions):          # what lies across a boundary is compared, and is not trivial
            if place_class(at, n) in _FALLBACK:
                assert _carries((s.name, s.data, s.own, s.p1, s.ret, s.out, s.p2), has_out), (side, "nothing is compared across the boundary", s.name)
        assert any(place_class(at, n) == "behind31" and at & 1 for at, n in regions), (side, "no odd address behind 2^31")
        assert any(place_class(at, n) == "past32" and at & 1 and at & 127 for at, n in regions), (side, "no odd, unaligned address past 2^32")
        last = -1
        for at, n in sorted(regions):
            assert at > last, (side, "overlap at", at)
            last = at + n - 1 if n else last
            assert 0 <= at and at + n <= SPAN - TAIL, (side, "outside the view", at, n)
            for a in (at, at + max(n, 1) - 1):
                low = a & 0xFFFFFFFF
                assert low < B31 or low - B32 >= -RED, (side, "sign-extended, it leaves the allocation", a)


# ---- the reference library's calls that no other *_common module wraps ---------------------------------------------------------------
def bound(n):
    return n + n // 255 + 16


class RefMore:
    """LZ4_compress_fast(acceleration), LZ4_compress_destSize and LZ4_compress_HC_destSize of the reference library"""

    def __init__(self, ref):
        L = self.L = C.CDLL(ref.path)
        L.LZ4_compress_fast.restype = C.c_int
        L.LZ4_compress_fast.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_int]
        L.LZ4_compress_destSize.restype = C.c_int
        L.LZ4_compress_destSize.argtypes = [C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int]
        L.LZ4_compress_HC_destSize.restype = C.c_int
        L.LZ4_compress_HC_destSize.argtypes = [C.c_void_p, C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int, C.c_int]
        L.LZ4_sizeofStateHC.restype = C.c_int
        self._state = C.create_string_buffer(L.LZ4_sizeofStateHC() + 64)

    def accel(self, v, cap, a):
        out = (C.c_uint8 * max(cap, 1))()
        r = self.L.LZ4_compress_fast(bytes(v), out, len(v), cap, a)
        return r, bytes(out[:max(r, 0)])

    def dest_size(self, v, t):
        """-> (ret, consumed, bytes)"""
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int(len(v))
        r = self.L.LZ4_compress_destSize(bytes(v), out, C.byref(sz), t)
        return r, sz.value, bytes(out[:max(r, 0)])

    def hc_dest_size(self, v, t, level):
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int(len(v))
        r = self.L.LZ4_compress_HC_destSize((C.addressof(self._state) + 15) & ~15, bytes(v), out, C.byref(sz), t, level)
        return r, sz.value, bytes(out[:max(r, 0)])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
FAST_SIZES = (0, 13, 1000, 65536, 65546, 65547, 200000)
HC_SIZES = (0, 13, 1000, 4096, 70000)
DICT_LENS = (4096, 65536)
RECORD_SIZES = (0, 12, 13, 1000, 70000)


def _book(corpus):
    return corpus["book1[:200000]"]


def compress_blocks(corpus, sizes):
    """text of every size, and one block that does not compress at all (random bytes: the bound is the only capacity that fits)"""
    b = _book(corpus)
    return [("book1 %d" % n, b[:n]) for n in sizes] + [("random 3000", random.Random(5).randbytes(3000))]


def compress_items(blocks, fn):
    """every block at the bound (fits), at the reference's size (fits exactly) and one byte below it (does not: 0); fn(v, cap) -> (r, bytes)"""
    items = []
    for name, v in blocks:
        r0, by0 = fn(v, bound(len(v)))
        assert r0 > 0
        for cap in (bound(len(v)), r0, r0 - 1):
            r, by = fn(v, cap)
            assert (r == r0 and by == by0) if cap >= r0 else r == 0, (name, cap, r)
            items.append(("%s cap %d" % (name, cap), v, cap, cap, r, by if r > 0 else None, 0))
    return items


def compress_fast_cases(ref, corpus):
    return layout(compress_items(compress_blocks(corpus, FAST_SIZES), ref.compress_fast_raw))


def compress_accel_cases(ref, corpus, a):
    rm = RefMore(ref)
    return layout(compress_items(compress_blocks(corpus, FAST_SIZES), lambda v, cap: rm.accel(v, cap, a)))


def compress_hc_cases(ref, corpus, level):
    return layout(compress_items(compress_blocks(corpus, HC_SIZES), lambda v, cap: ref.compress_hc_raw(v, level, cap)))


def dest_items(blocks, full, fn):
    """targets below, at and above the full compressed size, and the zero result (target 0); fn(v, t) -> (ret, consumed, bytes)"""
    items = []
    for name, v in blocks:
        f = full(v)
        for t in sorted({0, 1, max(f // 3, 1), f - 1, f, f + 1, bound(len(v))}):
            r, cons, by = fn(v, t)
            assert len(by) == r <= max(t, 0)
            items.append(("%s target %d" % (name, t), v, t, t, r, by, cons))
    return items


def dest_size_cases(ref, corpus):
    rm = RefMore(ref)
    return layout(dest_items(compress_blocks(corpus, (0, 13, 1000, 65546, 65547)), lambda v: len(ref.compress_fast(v)), rm.dest_size))


def hc_dest_size_cases(ref, corpus, level):
    rm = RefMore(ref)
    return layout(dest_items(compress_blocks(corpus, (0, 13, 1000, 70000)), lambda v: ref.compress_hc_raw(v, level, bound(len(v)))[0],
                              lambda v, t: rm.hc_dest_size(v, t, level)))


def dict_of(L):
    from dict_common import book1
    return book1()[:L]


def dict_records():
    from dict_common import RECORD_BASE, book1
    b = book1()
    return [("record %d" % n, b[RECORD_BASE:RECORD_BASE + n]) for n in RECORD_SIZES] + [("random 3000", random.Random(6).randbytes(3000))]


def compress_dict_cases(ref, L):
    from dict_common import RefDict
    from dictc_common import ref_compress
    rd, d = RefDict(ref), dict_of(L)
    return layout(compress_items(dict_records(), lambda v, cap: ref_compress(rd, d, v, cap)))


_HC_REF = {}


def compress_hc_dict_cases(ref, L, level=9):
    from hcdict_common import Ref
    R = _HC_REF.setdefault(id(ref), Ref(ref))
    d = dict_of(L)
    return layout(compress_items(dict_records(), lambda v, cap: R.compress(d, v, level, cap)))


def damage(valid, seed):
    """[(name, stream, n)] -> [(name, stream, capacity)]: every stream as it is, with one flipped byte, truncated, and with capacity - 1"""
    rng = random.Random(seed)
    out = []
    for name, s, n in valid:
        out.append((name, s, n))
        if len(s) > 1:
            b = bytearray(s)
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            out.append((name + " flipped", bytes(b), n))
            out.append((name + " truncated", s[:rng.randrange(len(s) // 2, len(s))], n))
        if n > 0:
            out.append((name + " capacity - 1", s, n - 1))
    return out


def decode_streams(ref, O, corpus):
    """valid streams of the reference compressor: text, App. F, a long-match block, a mostly-literal block (up to 200000 decoded bytes)
    and three small ones -> [(name, stream, decoded size)]"""
    b = _book(corpus)
    rng = random.Random(7)
    unit = rng.randbytes(37)
    vs = [("text 200000", b), ("App. F 65536", O.gen_block(65536, 1)), ("long matches", unit * 1400 + rng.randbytes(3000) + unit * 1000),
          ("mostly literals", corpus["geo[:65536]"]), ("text 1000", b[5000:6000]), ("text 13", b[:13]), ("empty", b"")]
    return [(name, ref.compress_fast(v), len(v)) for name, v in vs]


# the decoders' items, before layout() places them: cases = [(name, stream, capacity)] (tests/userstream_common.py builds its own lists)
def decode_safe_items(ref, cases):
    items = []
    for name, s, cap in cases:
        r, by = ref.decompress_safe_raw(s, cap)
        items.append((name, s, cap, cap, r, by[:r] if r >= 0 else None, 0))
    return items


def decode_safe_cases(ref, O, corpus):
    return layout(decode_safe_items(ref, damage(decode_streams(ref, O, corpus), 8)))


def decode_fast_cases(ref, O, corpus):
    """the fast decoder: the slot is the stream (src_cap = its length), p1 = the decoded size asked for; O.decompress_fast_bounded"""
    return layout(decode_fast_items(O, damage(decode_streams(ref, O, corpus), 9)))


def decode_fast_items(O, cases):
    items = []
    for name, s, n in cases:
        r, by = O.decompress_fast_bounded(s, len(s), n)
        items.append((name, s, n, n, r, by if r >= 0 else None, 0))
    return items


def decode_partial_cases(ref, O, corpus):
    """targets of 1, 4096 and the whole block; p1 = target, p2 = capacity; the slot owns min(target, capacity) bytes"""
    return layout(decode_partial_items(ref, damage(decode_streams(ref, O, corpus), 10)))


def decode_partial_items(ref, cases, targets=lambda k, cap: (1, 4096, cap)):
    """targets(k, cap): the targets of case k"""
    from partial_common import ref_partial
    run = ref_partial(ref)
    items = []
    for k, (name, s, cap) in enumerate(cases):
        for t in targets(k, cap):
            r, by = run(s, t, cap)
            items.append(("%s target %d" % (name, t), s, min(t, cap), t, r, by if r >= 0 else None, cap))
    return items


def decode_size_cases(ref, O, corpus):
    """the size query has no destination: only the sources are placed"""
    return layout(decode_size_items(ref, damage(decode_streams(ref, O, corpus), 11)))


def decode_size_items(ref, cases):
    from size_common import ref_size
    run = ref_size(ref)
    return [(name, s, 0, cap, run(s, cap), None, 0) for name, s, cap in cases]


def decode_dict_cases(ref, L):
    """records compressed against the dictionary by both of the reference's dictionary compressors, valid and damaged, through
    LZ4_decompress_safe_usingDict"""
    from dict_common import RefDict
    rd, d = RefDict(ref), dict_of(L)
    valid = []
    for name, v in dict_records():
        if v:
            valid.append((name + " fast", rd.compress(d, v), len(v)))
            valid.append((name + " hc9", rd.compress(d, v, 9), len(v)))
    return layout(decode_dict_items(rd, d, damage(valid, 12 + L)))


def decode_dict_items(rd, d, cases):
    items = []
    for name, s, cap in cases:
        r, by = rd.decode(s, cap, d)
        items.append((name, s, cap, cap, r, by if r >= 0 else None, 0))
    return items


ROUTED_SIZES = (1024, 16384)     # 1 KiB: the route kernel reads the sizes only; 16 KiB: streams of 4 KiB and more, whose middle it samples


def routed_streams(ref, O, corpus, kind, n, size=1024):
    """n streams of `size`-byte blocks (text slices / App. F blocks) -> (streams, blocks)"""
    from dict_common import book1
    b = book1()
    blocks = [b[(173 * i) % (len(b) - size):][:size] for i in range(n)] if kind == "text" else [O.gen_block(size, i) for i in range(n)]
    return [ref.compress_fast(v) for v in blocks], blocks


def routed_place(boundary, n):
    """where a contiguous run of n bytes goes: centred on the boundary at an odd address, or as far behind it as the view allows"""
    return min(boundary - (n // 2 | 1), (SPAN - TAIL - n) | 1)


XXH_LONG = (0, 15, 8191, 8193, 100000)
XXH_SEEDS = (0, 0x9747b28c)


def xxh_long_cases(rng_seed=13):
    """a few long buffers for the wave-per-buffer kernels (at most 512 buffers per launch) -> [Slot] without destinations"""
    rng = random.Random(rng_seed)
    sizes = [XXH_LONG[(j + k) % 5] for k in range(1, 4) for j in range(5)]     # every length at three places
    return layout([("%d bytes #%d" % (n, k), rng.randbytes(n), 0, 0, 0, None, 0) for k, n in enumerate(sizes)])


def xxh_short_layout(n=600, seed=14):
    """more than 512 short buffers (the lane-group kernels), back to back with odd gaps, the run straddling 2^32
    -> (image, its place in the view, offsets relative to the view, lengths)"""
    rng = random.Random(seed)
    lens = [rng.choice((0, 1, 15, 16, 31, 32, 33, 100, 255, 256, 257, 1000, 4096)) for _ in range(n)]
    img, off = bytearray(), []
    for ln in lens:
        off.append(len(img))
        img += rng.randbytes(ln + rng.choice((0, 1, 3)))
    at = B32 - (len(img) // 2 | 1)
    return bytes(img), at, [at + o for o in off], lens


GEN_STRIDE, GEN_LEN, GEN_BLOCKS = 1 << 26, 1000, 70
CONTAINER_BLOCK, CONTAINER_BLOCKS = 4 << 20, 1030
# what the 1030 blocks hold, as (count, gen_blocks parameters) runs.  "appf": the default App. F data, ratio 2 -- the container stays
# under 2^32 bytes.  "dense": 1000 blocks of literal runs of up to 64 KiB, which the reference compressor expands (stored raw: 4000 MiB),
# then 30 of runs of up to 600 bytes, ratio 1.02 -- the container is about 4117 MiB and passes 2^32 inside those compressed blocks
CONTAINER_INPUTS = {"appf": ((1030, {}),), "dense": ((1000, {"litmax": 65536}), (30, {"litmax": 600}))}


class Entry(NamedTuple):
    call: str        # the DeviceBatch method or lib() function that reaches the entry point
    cases: str       # the case builder(s) of this module
    expected: str    # where the expected values come from
    test: str        # the test of test_gpu_far_offsets.py that runs it


TABLE = {
    "lz4hip_compress_fast_batch_dev": Entry("DeviceBatch.compress_fast", "compress_fast_cases", "ref.compress_fast_raw", "test_far_compress_fast"),
    "lz4hip_compress_fast_accel_batch_dev": Entry("DeviceBatch.compress_fast(acceleration)", "compress_accel_cases", "RefMore.accel", "test_far_compress_accel"),
    "lz4hip_compress_dest_size_batch_dev": Entry("DeviceBatch.compress_dest_size", "dest_size_cases", "RefMore.dest_size", "test_far_compress_dest_size"),
    "lz4hip_compress_hc_batch_dev_ws": Entry("DeviceBatch.compress_hc", "compress_hc_cases", "ref.compress_hc_raw", "test_far_compress_hc"),
    "lz4hip_compress_hc_batch_dev": Entry("DeviceBatch.compress_hc_sync", "compress_hc_cases", "ref.compress_hc_raw", "test_far_compress_hc"),
    "lz4hip_compress_hc_dest_size_batch_dev_ws": Entry("DeviceBatch.compress_hc_dest_size", "hc_dest_size_cases", "RefMore.hc_dest_size",
                                                       "test_far_compress_hc_dest_size"),
    "lz4hip_compress_hc_dest_size_batch_dev": Entry("DeviceBatch.compress_hc_dest_size_sync", "hc_dest_size_cases", "RefMore.hc_dest_size",
                                                    "test_far_compress_hc_dest_size"),
    "lz4hip_compress_fast_dict_batch_dev": Entry("DeviceBatch.compress_dict", "compress_dict_cases", "dictc_common.ref_compress", "test_far_dictionary"),
    "lz4hip_compress_hc_dict_batch_dev_ws": Entry("DeviceBatch.compress_hc_dict", "compress_hc_dict_cases", "hcdict_common.Ref", "test_far_dictionary"),
    "lz4hip_compress_hc_dict_batch_dev": Entry("DeviceBatch.compress_hc_dict_sync", "compress_hc_dict_cases", "hcdict_common.Ref", "test_far_dictionary"),
    "lz4hip_decompress_safe_dict_batch_dev": Entry("DeviceBatch.decompress_safe_dict", "decode_dict_cases", "dict_common.RefDict.decode", "test_far_dictionary"),
    "lz4hip_decompress_safe_batch_dev": Entry("DeviceBatch.decompress_safe", "decode_safe_cases, routed_streams", "ref.decompress_safe_raw",
                                              "test_far_decode_variants, test_far_decode_routed"),
    "lz4hip_decompress_fast_batch_dev": Entry("DeviceBatch.decompress_fast", "decode_fast_cases", "O.decompress_fast_bounded", "test_far_decode_fast_partial_size"),
    "lz4hip_decompress_safe_partial_batch_dev": Entry("DeviceBatch.decompress_safe_partial", "decode_partial_cases", "partial_common.ref_partial",
                                                      "test_far_decode_fast_partial_size"),
    "lz4hip_decompressed_size_batch_dev": Entry("DeviceBatch.decoded_size", "decode_size_cases", "size_common.ref_size", "test_far_decode_fast_partial_size"),
    "lz4hip_xxh32_batch_dev": Entry("DeviceBatch.xxh32", "xxh_long_cases, xxh_short_layout", "ref.xxh32", "test_far_xxh"),
    "lz4hip_xxh64_batch_dev": Entry("DeviceBatch.xxh64", "xxh_long_cases, xxh_short_layout", "ref.xxh64", "test_far_xxh"),
    "lz4hip_gen_blocks_dev": Entry("DeviceBatch.gen_blocks", "GEN_STRIDE, GEN_LEN, GEN_BLOCKS", "O.gen_block", "test_far_gen_blocks"),
    "lz4hip_container_blocks_dev": Entry("DeviceBatch.container_blocks", "CONTAINER_BLOCK, CONTAINER_BLOCKS, CONTAINER_INPUTS", "ref.compress_fast, ref.xxh32", "test_far_containers"),
    "lz4hip_container_decode_dev": Entry("lib().lz4hip_container_decode_dev", "CONTAINER_BLOCK, CONTAINER_BLOCKS, CONTAINER_INPUTS", "the generated input", "test_far_containers"),
    # the two chain kernels: tests/test_gpu_cchain.py, which this table grew out of, places chains around 2^31 and 2^32
    "lz4hip_decompress_safe_chain_batch_dev": Entry("DeviceBatch.decompress_safe_chain", "test_gpu_cchain.py", "cchain_common.RefCChain",
                                                    "test_gpu_cchain.py::test_cchain_device_offsets_past_2_and_4_gib"),
    "lz4hip_compress_fast_chain_batch_dev": Entry("DeviceBatch.compress_fast_chain", "test_gpu_cchain.py", "cchain_common.RefCChain",
                                                  "test_gpu_cchain.py::test_cchain_device_offsets_past_2_and_4_gib"),
}
EXEMPT = {
    "lz4hip_xxh_stream_update_dev": "a pointer and a 32-bit length: it takes no offset",
    "lz4hip_dbg_compress_fast_profile_dev": "developer diagnostic, not in the release library",
}


def declared_dev_entry_points(header=None):
    """every lz4hip_*_dev* function include/lz4hip.h declares"""
    text = open(header or os.path.join(ROOT, "include", "lz4hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lz4hip_\w*_dev\w*)\s*\(", text)))


# ---- the device side (torch is imported by the caller) ------------------------------------------------------------------------------
class FarBuffers:
    """one source and one destination far buffer on the device, with the views the library is handed"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.src_all = torch.empty(RED + SPAN, dtype=torch.uint8, device=dev)
        self.dst_all = torch.empty(RED + SPAN, dtype=torch.uint8, device=dev)
        self.src, self.dst = self.src_all[RED:], self.dst_all[RED:]
        self.tile = torch.frombuffer(bytearray(random.Random(99).randbytes(TILE)), dtype=torch.uint8).to(dev)
        self.decoy(self.src_all)

    def decoy(self, buf):
        """the non-constant pattern: a read from the wrong place yields wrong bytes, not zeros that could happen to compress alike"""
        k = buf.numel() // TILE
        buf[:k * TILE].view(k, TILE).copy_(self.tile.expand(k, TILE))
        buf[k * TILE:] = self.tile[:buf.numel() - k * TILE]

    def free(self):
        self.src = self.dst = self.src_all = self.dst_all = self.tile = None
        self.torch.cuda.empty_cache()

    def up(self, data):
        return self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8).to(self.dev)

    def i32(self, v):
        import numpy as np
        return self.torch.from_numpy(np.asarray(v, dtype=np.int32)).to(self.dev)

    def i64(self, v):
        import numpy as np
        return self.torch.from_numpy(np.asarray(v, dtype=np.int64)).to(self.dev)

    def put(self, slots):
        for s in slots:
            if s.data:
                self.src[s.src_at:s.src_at + len(s.data)] = self.up(s.data)

    def fill(self, byte):
        self.dst_all.fill_(byte)

    def get(self, at, n, view=None):
        view = self.dst if view is None else view
        return view[at:at + n].cpu().numpy().tobytes() if n else b""

    def untouched(self, buf, byte):
        """how many bytes of the whole allocation differ from `byte`, taken in pieces so that no multi-GiB temporary appears"""
        bad = 0
        for a in range(0, buf.numel(), CHUNK):
            bad += int(self.torch.count_nonzero(buf[a:a + CHUNK] != byte))
        return bad

    def settle(self, slots, rets, byte, what, ret2=None, same=None):
        """after a call (and a synchronize): return values and bytes against the reference, then every owned region refilled and
        nothing but `byte` left anywhere in the destination allocation, red zone included"""
        bad = []
        for k, s in enumerate(slots):
            if rets[k] != s.ret or (ret2 is not None and ret2[k] != s.p2):
                bad.append((s.name, "returned", rets[k], None if ret2 is None else ret2[k], "reference", s.ret, s.p2))
            elif s.out is not None:
                got = self.get(s.dst_at, len(s.out))
                if got != s.out and not (same and same(s, got)):
                    bad.append((s.name, "bytes differ", s.src_at, s.dst_at))
            if s.own:
                self.dst[s.dst_at:s.dst_at + s.own] = byte
        assert not bad, (what, len(bad), bad[:4])
        n = self.untouched(self.dst_all, byte)
        assert n == 0, (what, "bytes written outside the blocks' slots", n)
