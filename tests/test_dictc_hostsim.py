"""The dictionary compressor (LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream) on the CPU: tests/hostsim/hostsim_dictc.cpp
compiles FastCore<..., DICT = true> and dict_image_build of lz4-java_amd/csrc/lz4_fast_core.h -- what compress_fast_dict_cu_kernel and
dict_image_kernel run -- against the lock-step lane simulator, and this file checks value and bytes against the reference library on the
shared set (tests/dictc_common.py).  Every case runs in two arena layouts; a read in front of the dictionary's kept tail, behind the
dictionary's end or outside the source is flagged by the simulator, and the dictionary's arena neighbours hold bytes that would extend a
match if they were read."""
import ctypes as C
import random

import pytest

from dictc_common import (DICT_LENS, RefDict, big_record, book1, book_records, bound, caps_for, check_hand_cases, dict_cuts, hand_cases,
                          keep_of, other_records, parse, ref_compress)
from support import build_sim

IMAGE = 32768


def load_sim():
    l = build_sim("hostsim_dictc")
    l.sim_dict_keep.restype = C.c_uint32
    l.sim_dict_keep.argtypes = [C.c_int]
    l.sim_dict_image.restype = C.c_int
    l.sim_dict_image.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    l.sim_compress_fast_dict.restype = C.c_int
    l.sim_compress_fast_dict.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_uint64]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def rd(ref):
    return RefDict(ref)


class Arena:
    """One dictionary and one record in ONE buffer, in two layouts: 0 = [front | dictionary | behind | gap | record], 1 = [record | gap |
    front | dictionary | behind].  `front` ends in the bytes in front of the kept tail -- the dictionary's own earlier bytes where it is
    longer than 64 KB, else `pre` repeated --, `behind` is what follows the dictionary.  Neither belongs to what may be read."""

    def __init__(self, d, rec, layout, pre, post):
        keep = keep_of(len(d))
        front = (pre * 64)[:64]
        body = front + bytes(d) + (post + bytes(64))[:64]
        gap = b"\xEE" * 64
        if layout == 0:
            buf, d0, r0 = body + gap + bytes(rec), 64, len(body) + 64
        else:
            buf, d0, r0 = bytes(rec) + gap + body, len(rec) + 64 + 64, 0
        self.buf = C.create_string_buffer(buf, len(buf) + 1)
        base = C.addressof(self.buf)
        self.keep = keep
        self.tail = base + d0 + len(d) - keep
        self.src = base + r0
        assert self.tail + keep != self.src


def image_of(sim, arena, seed=0):
    img = C.create_string_buffer(IMAGE)
    if arena.keep:
        assert sim.sim_dict_image(arena.tail, arena.keep, img, seed) == 0
    return img


def run(sim, arena, img, n, cap, seed):
    out = C.create_string_buffer(max(cap, 1) + 16)
    r = sim.sim_compress_fast_dict(arena.tail, arena.keep, img, arena.src, n, out, cap, None, seed)
    return r, out.raw[:max(r, 0)], out.raw[max(cap, 1):]


def check(sim, rd, d, rec, rng, small_caps, pre=None, post=None, name=""):
    """one record against one dictionary: both layouts, the capacity list; value and bytes are the reference's"""
    want_r, want = ref_compress(rd, d, rec)
    assert want_r > 0
    pre = pre if pre is not None else (bytes(d[:len(d) - 65536][-64:]) if len(d) > 65536 else bytes(rec[:1]) or b"\0")
    post = post if post is not None else bytes(rec[:64])
    for layout in (0, 1):
        a = Arena(d, rec, layout, pre, post)
        img = image_of(sim, a, rng.getrandbits(63) | 1)
        for cap in (caps_for(len(rec), want_r, small_caps) if small_caps or layout == 0 else [bound(len(rec))]):
            er, eb = (want_r, want) if cap >= want_r else ref_compress(rd, d, rec, cap)
            r, by, behind = run(sim, a, img, len(rec), cap, rng.getrandbits(63) | 1)
            assert r != -1000, ("out-of-bounds access", name, len(d), len(rec), layout, cap)
            assert r == er and (r == 0 or by == eb), (name, len(d), len(rec), layout, cap, r, er)
            assert behind == bytes(16), ("wrote behind the capacity", name, cap)


def test_keep_rule(sim):
    """what the library keeps of a dictionary is what LZ4_loadDict keeps: nothing under 8 bytes, the last 64 KB"""
    for L in list(range(0, 20)) + [65535, 65536, 65537, 100000, 2 ** 31 - 1]:
        assert sim.sim_dict_keep(L) == keep_of(L), L
    assert sim.sim_dict_keep(-1) == 0


def loaddict_replay(tail):
    """LZ4_loadDict's loop on the kept tail: positions 0, 3, 6, .. while p <= keep - 8, hash of the 5 bytes at p, the last insert wins;
    the entries in the core's layout: index (65536 - keep + p) in the high word, the 16 high bits of the 4-byte product below"""
    keep = len(tail)
    t = [0] * 4096
    for p in range(0, keep - 8 + 1, 3):
        x = int.from_bytes(tail[p:p + 8], "little")
        h = (((x << 24) & (2 ** 64 - 1)) * 889523592379 & (2 ** 64 - 1)) >> 52
        fp = (((x & 0xFFFFFFFF) * 2654435761) & 0xFFFFFFFF) >> 16
        t[h] = ((65536 - keep + p) << 32) | fp
    return t


def test_image_is_loaddicts_table(sim):
    """the image, entry by entry, against a replay of LZ4_loadDict's loop; several lane orders of the LDS atomic"""
    b = book1()
    rng = random.Random(11)
    for L in (8, 9, 10, 11, 16, 100, 191, 192, 193, 200, 4096, 65535, 65536, 65537, 100000):
        d = b[:L]
        for layout in (0, 1):
            a = Arena(d, b"x" * 20, layout, b"\0", b[L:L + 64])
            img = image_of(sim, a, rng.getrandbits(63) | 1)
            got = list((C.c_uint64 * 4096).from_buffer_copy(img.raw))
            want = loaddict_replay(d[L - a.keep:])
            assert got == want, (L, layout, [i for i in range(4096) if got[i] != want[i]][:5])
    n_entries = sum(1 for e in want if e)
    assert n_entries > 3000   # (a 64 KB dictionary fills most of the table)


def test_hand_built_cases_are_what_they_say(rd):
    """the reference's own output holds the sequence each hand-built case is about (a mis-built case fails here)"""
    check_hand_cases(rd)


def test_hand_built_cases(sim, rd):
    rng = random.Random(12)
    for c in hand_cases():
        check(sim, rd, c[1], c[2], rng, True, pre=c[4] if len(c) > 4 else None, name=c[0])


def test_reference_conditions(rd):
    """what the set relies on, by the reference: every record of at least 300 bytes against a dictionary of at least 4096 bytes has a
    sequence whose offset exceeds its position (a dictionary match) and differs from the empty-dictionary output (the reference gives
    600 of 600 on both; the test asks for 90 %)"""
    b = book1()
    rng = random.Random(13)
    total = uses = differs = 0
    for L in (4096, 65535, 65536, 65537, 100000):
        for size in (300, 1000, 4096):
            for _ in range(40):
                o = rng.randrange(200000, len(b) - size)
                rec = b[o:o + size]
                _, by = ref_compress(rd, b[:L], rec)
                _, plain = ref_compress(rd, b"", rec)
                total += 1
                uses += any(off > pos for pos, off, ml in parse(by))
                differs += by != plain
    assert total == 600 and uses >= 540 and differs >= 540, (total, uses, differs)


def test_empty_dictionary_is_not_the_plain_compressor_below_65547(rd, ref):
    """byU32 at every size: an empty dictionary does not give LZ4_compress_default's bytes for small records, and does from 65547 on"""
    b = book1()
    rng = random.Random(14)
    diff = 0
    for _ in range(100):
        n = rng.randrange(64, 4097)
        o = rng.randrange(200000, len(b) - n)
        diff += ref_compress(rd, b"", b[o:o + n])[1] != ref.compress_fast(b[o:o + n])
    assert diff >= 50
    for n in (65547, 70000):
        assert ref_compress(rd, b"", b[200000:200000 + n])[1] == ref.compress_fast(b[200000:200000 + n])
    for L in (1, 7):
        assert ref_compress(rd, b[:L], b[200000:201000]) == ref_compress(rd, b"", b[200000:201000])
    assert ref_compress(rd, b[:100000], b[200000:204096]) == ref_compress(rd, b[100000 - 65536:100000], b[200000:204096])


@pytest.mark.parametrize("L", DICT_LENS)
def test_dict_core_set(sim, rd, O, corpus, L):
    """the shared set against the dictionary book1[:L]: slices of book1[200000:] of every listed size, mixed inputs, all-equal bytes,
    geo, and records cut out of the dictionary itself (what follows the dictionary in book1 sits right behind it in the arena)"""
    b = book1()
    d = b[:L]
    rng = random.Random(100 + L)
    recs = book_records() + other_records(O, corpus, n_rnd=24) + dict_cuts(L, rng)
    for name, rec in recs:
        check(sim, rd, d, rec, rng, len(rec) <= 4096, post=b[L:L + 64] if name.startswith("cut") else None, name=name)


def test_dict_core_big_block(sim, rd, O):
    """one 1 MiB + 3 block: positions far beyond the dictionary's reach, extended lengths"""
    name, rec = big_record(O)
    rng = random.Random(15)
    for L in (0, 65536):
        d = book1()[:L]
        want_r, want = ref_compress(rd, d, rec)
        a = Arena(d, rec, L and 1, b"\0", rec[:64])
        r, by, _ = run(sim, a, image_of(sim, a), len(rec), bound(len(rec)), rng.getrandbits(63) | 1)
        assert (r, by) == (want_r, want)


def test_collision_path_is_exercised(sim, rd):
    """the exact resolution of intra-step bucket collisions runs in the dictionary core too (all-equal bytes collide in every step)"""
    d = book1()[:4096]
    rec = bytes(300) + book1()[200000:200300] + bytes(300)
    a = Arena(d, rec, 0, b"\0", b"")
    st = (C.c_uint64 * 4)()
    out = C.create_string_buffer(2000)
    r = sim.sim_compress_fast_dict(a.tail, a.keep, image_of(sim, a), a.src, len(rec), out, 2000, st, 5)
    assert (r, out.raw[:r]) == ref_compress(rd, d, rec) and st[1] > 0
