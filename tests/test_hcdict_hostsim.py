"""The dictionary HC compressor (LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream) on the CPU: tests/hostsim/hostsim_hcdict.cpp
compiles hc_dict_image_build, HcBuild<..., DICT = true> and HcParse<..., false, DICT = true> of lz4-java_amd/csrc/lz4_hc_core.h -- what
hc_dict_image_kernel, hc_build_dict_kernel and hc_parse_dict_kernel run -- against the lock-step lane simulator, and this file checks
value and bytes against the reference library on the shared set (tests/hcdict_common.py).  Every case runs in two memory layouts: the
dictionary far from the source, and right in front of it (where the engine, unlike liblz4, still treats the two as separate), with
different fill round each; the simulator flags a wave access outside the kept tail, the source and the slot."""
import ctypes as C
import random

import pytest

from hcdict_common import (BIG_LEVELS, BIG_SIZES, CLAMPS, DICT_LENS, LEVELS, SMALL_SIZES, Ref, book1, book_records, bound, caps_for,
                           check_hand_cases, clamp, dict_cuts, hand_cases, has_dict_match, has_straddle, keep_of, other_records, parse,
                           pattern_cases)
from support import build_sim

HEAD = 32768


def load_sim():
    l = build_sim("hostsim_hcdict")
    l.sim_hc_dict_image.restype = C.c_int
    l.sim_hc_dict_image.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    l.sim_compress_hc_dict.restype = C.c_int
    l.sim_compress_hc_dict.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def R(ref):
    return Ref(ref)


class Arena:
    """One dictionary and one record in ONE buffer.  Layout 0 = [front | dictionary | behind | gap | record]: far apart; `front` is the
    dictionary's own earlier bytes where it is longer than 64 KB, else `pre`; `behind` is `post`.  Layout 1 = [front' | dictionary |
    record]: the dictionary ends where the record starts, with another fill in front.  Nothing but the kept tail and the record may
    be read."""

    def __init__(self, d, rec, layout, pre, post):
        keep = keep_of(len(d))
        if layout == 0:
            front = (pre * 64)[:64]
            body = front + bytes(d) + (post + bytes(64))[:64]
            buf, d0, r0 = body + b"\xEE" * 64 + bytes(rec), 64, len(body) + 64
        else:
            front = bytes(x ^ 0x5A for x in (pre * 64)[:64])
            buf, d0, r0 = front + bytes(d) + bytes(rec), 64, 64 + len(d)
        self.buf = C.create_string_buffer(buf, len(buf) + 1)
        base = C.addressof(self.buf)
        self.keep = keep
        self.tail = base + d0 + len(d) - keep
        self.src = base + r0


class Image:
    def __init__(self, sim, arena, seed=0):
        self.head = (C.c_uint32 * HEAD)()
        self.delta = (C.c_uint16 * max(arena.keep, 1))()
        assert sim.sim_hc_dict_image(arena.tail, arena.keep, self.head, self.delta, seed) == 0


def run(sim, arena, img, n, cap, level, seed):
    out = C.create_string_buffer(max(cap, 1) + 16)
    r = sim.sim_compress_hc_dict(arena.tail, arena.keep, img.head, img.delta, arena.src, n, out, cap, level, seed)
    return r, out.raw[:max(r, 0)], out.raw[max(cap, 1):]


def check(sim, R, d, rec, rng, levels, all_caps, pre=None, post=None, name=""):
    """one record against one dictionary: both layouts, the levels, the capacity list (layout 1: the bound); value and bytes are the
    reference's"""
    pre = pre if pre is not None else (bytes(d[:len(d) - 65536][-64:]) if len(d) > 65536 else bytes(rec[:1]) or b"\0")
    post = post if post is not None else bytes(rec[:64])
    for layout in (0, 1):
        a = Arena(d, rec, layout, pre, post)
        img = Image(sim, a, rng.getrandbits(63) | 1)
        for level in levels:
            want_r, want = R.compress(d, rec, clamp(level))
            assert want_r > 0
            for cap in (caps_for(len(rec), want_r, all_caps) if layout == 0 else [bound(len(rec))]):
                er, eb = (want_r, want) if cap >= want_r else R.compress(d, rec, clamp(level), cap)
                r, by, behind = run(sim, a, img, len(rec), cap, level, rng.getrandbits(63) | 1)
                assert r != -1000, ("out-of-bounds access", name, len(d), len(rec), layout, level, cap)
                assert r == er and (r == 0 or by == eb), (name, len(d), len(rec), layout, level, cap, r, er)
                assert behind == bytes(16), ("wrote behind the capacity", name, cap)


def loaddicthc_replay(tail):
    """LZ4_loadDictHC's inserts on the kept tail -- positions 0 .. K - 4, index 65536 + q, hash of the 4 bytes at q -- in the image's
    layout: the head table, and delta[q] = distance to the previous position of the same hash (0: none within 65535; 0 for the last
    three positions, which are never inserted)"""
    K = len(tail)
    head, delta = [0] * HEAD, [0] * K
    for q in range(0, K - 3):
        h = ((int.from_bytes(tail[q:q + 4], "little") * 2654435761) & 0xFFFFFFFF) >> 17
        dist = 65536 + q - head[h]
        delta[q] = dist if dist <= 65535 else 0
        head[h] = 65536 + q
    return head, delta


def test_image_is_loaddicthcs_tables(sim):
    """the image, entry by entry, against a replay of LZ4_loadDictHC's inserts, for every dictionary length of the set; several lane
    orders of the LDS atomic"""
    b = book1()
    rng = random.Random(11)
    for L in DICT_LENS + (1, 2, 6, 7, 8, 63, 64, 65, 67):
        d = b[:L]
        for layout in (0, 1):
            a = Arena(d, b"x" * 20, layout, b"\0", b[L:L + 64])
            img = Image(sim, a, rng.getrandbits(63) | 1)
            head, delta = loaddicthc_replay(d[L - a.keep:])
            assert list(img.head) == head, (L, layout, [i for i in range(HEAD) if img.head[i] != head[i]][:5])
            assert list(img.delta)[:a.keep] == delta, (L, layout, [i for i in range(a.keep) if img.delta[i] != delta[i]][:5])
    head, _ = loaddicthc_replay(b[:65536])
    assert sum(1 for e in head if e) > 10000   # (a 64 KB dictionary fills a good part of the table)


def test_hand_built_cases_are_what_they_say(R):
    """the reference's own level 9 output holds the sequence each hand-built case is about (a mis-built case fails here)"""
    check_hand_cases(R)


def test_pattern_census(R):
    """what the repeated-pattern set relies on, computed from the reference alone: conditions on the set, so that a mis-built
    generator fails rather than tests nothing (the reference gives 97, 48, 187, 88 and 187)"""
    l89 = l912 = dm = st = plain = 0
    cases = pattern_cases()
    assert len(cases) == 200
    for name, d, rec in cases:
        o = {lv: R.compress(d, rec, lv)[1] for lv in (8, 9, 12)}
        seqs = parse(o[9])
        l89 += o[8] != o[9]
        l912 += o[9] != o[12]
        dm += has_dict_match(seqs)
        st += has_straddle(seqs)
        plain += o[9] != R.plain(rec, 9)[1]
    print("census: 8/9 differ %d, 9/12 differ %d, dictionary match %d, straddling %d, differs from plain HC %d" % (l89, l912, dm, st, plain))
    assert l89 >= 40 and l912 >= 15 and dm >= 100 and st >= 40, (l89, l912, dm, st)


def test_hand_built_cases(sim, R):
    rng = random.Random(12)
    for name, d, rec, _ in hand_cases():
        check(sim, R, d, rec, rng, LEVELS if len(rec) <= 4096 else BIG_LEVELS, True, name=name)


def test_pattern_cases(sim, R):
    """200 repeated-pattern cases at every level: pattern analysis across the dictionary's end, both ways"""
    rng = random.Random(13)
    for name, d, rec in pattern_cases():
        check(sim, R, d, rec, rng, LEVELS, False, name=name)


@pytest.mark.parametrize("L", DICT_LENS)
def test_hcdict_core_set(sim, R, O, corpus, L):
    """the shared set against the dictionary book1[:L]: slices of book1[200000:], mixed inputs, records cut out of the dictionary
    itself (what follows the dictionary in book1 sits right behind it in the arena); every level and the two clamps on records up
    to 4096 bytes, level 9 and one optimal level on the bigger ones"""
    b = book1()
    d = b[:L]
    rng = random.Random(100 + L)
    recs = book_records() + other_records(O, corpus, n_rnd=24) + dict_cuts(L, rng)
    for name, rec in recs:
        small = len(rec) <= 4096
        levels = LEVELS + tuple(a for a, _ in CLAMPS) if small else BIG_LEVELS
        check(sim, R, d, rec, rng, levels, small, post=b[L:L + 64] if name.startswith("cut") else None, name=name)


def test_fewer_than_four_kept_bytes_is_plain_hc(sim, R, O, corpus):
    """a dictionary of 0 .. 3 bytes has no candidate position: the bytes are LZ4_compress_HC's (and lz4hip_compress_hc's, which are
    those)"""
    b = book1()
    rng = random.Random(14)
    recs = book_records(SMALL_SIZES + BIG_SIZES[:1]) + other_records(O, corpus, n_rnd=12)
    for L in (0, 1, 2, 3):
        for name, rec in recs:
            a = Arena(b[:L], rec, 0, b"\0", b"")
            img = Image(sim, a, 3)
            for level in (LEVELS if len(rec) <= 4096 else BIG_LEVELS):
                r, by, _ = run(sim, a, img, len(rec), bound(len(rec)), level, rng.getrandbits(63) | 1)
                assert (r, by) == R.plain(rec, level), (L, name, level)
