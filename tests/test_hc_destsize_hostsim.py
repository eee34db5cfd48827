"""The fill-mode HC compressor (LZ4_compress_HC_destSize) on the CPU: tests/hostsim/hostsim_hc_destsize.cpp compiles HcBuild and
HcParse<..., FILL = true> of lz4-java_amd/csrc/lz4_hc_core.h -- what hc_build_kernel + hc_parse_dest_kernel run -- against the
lock-step lane simulator, with the simulator's bounds set to [src, src+n) and [dst, dst+target), and this file checks return value,
consumed size and every output byte against the reference library's own LZ4_compress_HC_destSize (ctypes on oracle.ref().path).

Every case also checks: the destination is pre-filled and nothing at or past `target` changes (simulator and reference alike), and
the reference's output, decoded with LZ4_decompress_safe, is src[:consumed] (no exception was found: KNOWN_ROUNDTRIP_BREAKS is
empty).  No case is skipped or filtered; the number of compared cases is asserted per test.

Bound chosen for the optimal parser (levels 10..12, and 13 for the clamp): inputs of at most 16 KiB, except three 64 KiB inputs at
level 10 and 12 for the table wrap of LZ4_OPT_NUM = 4096 positions -- the whole file runs in about two minutes."""
import ctypes as C
import glob
import os
import random

import pytest

from conftest import ROOT, calgary
from support import build_sim

_u8p = C.POINTER(C.c_uint8)
CHAIN_LEVELS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)    # 0 -> 9 (the clamp)
OPT_LEVELS = (10, 11, 12, 13)                    # 13 -> 12 (the clamp)
OPT_MAX_INPUT = 16384
GUARD = 32
KNOWN_ROUNDTRIP_BREAKS = set()   # (len(src), target, level) where liblz4 1.9.3's own output does not decode to src[:consumed]: none found


def bound(n):
    return n + n // 255 + 16 if 0 <= n <= 0x7E000000 else 0


def load_sim():
    l = build_sim("hostsim_hc_destsize")
    l.sim_compress_hc_dest_size.restype = C.c_int
    l.sim_compress_hc_dest_size.argtypes = [C.c_char_p, C.c_int, _u8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_uint64]
    return l


def _guarded(t):
    """a destination of max(t, 0) bytes with GUARD bytes behind it, all 0xA5"""
    size = max(t, 0) + GUARD
    buf = (C.c_uint8 * size)()
    C.memset(buf, 0xA5, size)
    return buf


def ref_hc_dest_size(ref):
    """(src, target, level) -> (ret, consumed, bytes, tail untouched): the reference library's LZ4_compress_HC_destSize itself"""
    lib = C.CDLL(ref.path)
    f = lib.LZ4_compress_HC_destSize
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int, C.c_int]
    lib.LZ4_sizeofStateHC.restype = C.c_int
    state = C.create_string_buffer(lib.LZ4_sizeofStateHC() + 64)
    base = (C.addressof(state) + 15) & ~15

    def run(v, t, level, state=state):   # (the default keeps the state buffer alive)
        out = _guarded(t)
        sz = C.c_int(len(v))
        r = f(base, bytes(v), out, C.byref(sz), t, level)
        return r, sz.value, bytes(out[:max(r, 0)]), bytes(out[max(t, 0):]) == b"\xa5" * GUARD
    return run


def sim_hc_dest(sim, v, t, level, seed=0):
    out = _guarded(t)
    cons = C.c_int(-7)
    r = sim.sim_compress_hc_dest_size(bytes(v), len(v), out, t, level, C.byref(cons), seed)
    return r, cons.value, bytes(out[:max(r, 0)]), bytes(out[max(t, 0):]) == b"\xa5" * GUARD


class Checker:
    def __init__(self, sim, lz4, ref):
        self.sim, self.lz4, self.ref = sim, lz4, ref
        self.rng = random.Random(29)
        self.n = 0
        self.cut = 0          # cases whose output stops before the end of the input
        self.hc_len = {}

    def check(self, v, t, level, what=""):
        want = self.lz4(v, t, level)
        got = sim_hc_dest(self.sim, v, t, level, seed=self.rng.getrandbits(63) | 1)
        assert want[3], ("the reference wrote at or past its target", what, len(v), t, level)
        assert got[3], ("the simulated wave wrote at or past the target", what, len(v), t, level)
        assert got == want, (what, len(v), t, level, got[:2], want[:2])
        r, consumed, data = want[:3]
        assert r <= max(t, 0) and 0 <= consumed <= len(v)
        if r > 0:
            ok = self.ref.decompress_safe_raw(data, len(v) + 8)
            good = ok[0] == consumed and ok[1][:consumed] == bytes(v[:consumed])
            assert good != ((len(v), t, level) in KNOWN_ROUNDTRIP_BREAKS), ("round trip of the reference's output", what, len(v), t, level)
        else:
            assert consumed == len(v)    # returned 0 up front: the size is untouched
        self.cut += 0 < r and consumed < len(v)
        self.n += 1

    def hc(self, v, level):
        key = (bytes(v), level)
        if key not in self.hc_len:
            self.hc_len[key] = len(self.ref.compress_hc(v, level))
        return self.hc_len[key]

    def targets(self, v, level, n_random=4):
        """the band of +-16 around len(LZ4_compress_HC(src, level)), targets >= compressBound, and random targets"""
        n, dl, b = len(v), self.hc(v, level), bound(len(v))
        ts = set(range(dl - 16, dl + 17)) | {b, b + 1, b + 100}
        ts |= {self.rng.randrange(1, b + 3) for _ in range(n_random)}
        return sorted(t for t in ts if t >= 0)


@pytest.fixture(scope="module")
def chk(ref):
    return Checker(load_sim(), ref_hc_dest_size(ref), ref)


def small_inputs(O, corpus):
    book1 = corpus["book1[:200000]"]
    out = []
    for n in list(range(0, 14)) + [20, 40]:
        out += [book1[7000:7000 + n], O.gen_block(n, n, litmax=4, win=8), bytes(n)]
    return out


def test_small_inputs_every_target(chk, O, corpus):
    """lengths 0 .. 13, 20 and 40 (text, App. F, one byte repeated): every target from 0 to 40, and -1, at every level 0 .. 13"""
    n0 = chk.n
    ins = small_inputs(O, corpus)
    for level in CHAIN_LEVELS + OPT_LEVELS:
        for v in ins:
            for t in range(-1, 41):
                chk.check(v, t, level, "small")
    assert chk.n - n0 == len(ins) * 42 * 14 == 28224


def medium_inputs(O, corpus, rng):
    """up to 16 KiB: slices of the golden files, the regress vectors, App. F blocks, runs of one byte, incompressible bytes"""
    book1, geo, pic = corpus["book1[:200000]"], corpus["geo[:65536]"], corpus["pic[:65536]"]
    ins = [book1[:4096], book1[100000:100000 + 16384], geo[:8192], geo[30000:30000 + 3000], pic[:16384], pic[40000:40000 + 5000],
           O.gen_block(4096, 0), O.gen_block(16384, 5, litmax=4, win=64), O.gen_block(9000, 7, litmax=200, win=4096),
           bytes(5000), b"\x37" * 16384, rng.randbytes(3000), rng.randbytes(16384),
           (b"abcdefghijklmnopqrstuvwxyz" * 3 + rng.randbytes(11)) * 100, bytes(2000) + rng.randbytes(300) + bytes(2000)]
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "regress", "*.bin"))):
        ins.append(open(f, "rb").read())
    return ins


def test_optimal_levels(chk, O, corpus):
    """levels 10 .. 12 and 13 (clamped to 12) on inputs of at most OPT_MAX_INPUT bytes: the band around the level's own compressed
    size, targets >= compressBound, random targets and every fifth target 0 .. 40 (every target 0 .. 40: the small inputs)"""
    n0, cut0 = chk.n, chk.cut
    ins = medium_inputs(O, corpus, random.Random(41))
    assert len(ins) == 18 and all(len(v) <= OPT_MAX_INPUT for v in ins)
    for level in OPT_LEVELS:
        for v in ins:
            for t in sorted(set(chk.targets(v, level)) | set(range(0, 41, 5))):
                chk.check(v, t, level, "optimal")
    assert chk.n - n0 >= 300 and chk.n - n0 >= 18 * 4 * 36, chk.n - n0
    assert chk.cut - cut0 >= 300, "too few of the optimal-parser cases stop short of the input"


def test_optimal_levels_table_wrap(chk, O, corpus):
    """three 64 KiB inputs at levels 10 and 12: more than LZ4_OPT_NUM positions, so the price table is reused many times"""
    n0 = chk.n
    for v in (corpus["book1[:65536]"], O.gen_block(65536, 1), corpus["pic[:65536]"]):
        for level in (10, 12):
            dl = chk.hc(v, level)
            for t in (4096, dl // 2, dl - 1, dl, dl + 12, bound(len(v))):
                chk.check(v, t, level, "optimal 64k")
    assert chk.n - n0 == 36


def test_chain_levels_medium(chk, O, corpus):
    """levels 0 .. 9 on the same inputs as the optimal levels"""
    n0, cut0 = chk.n, chk.cut
    ins = medium_inputs(O, corpus, random.Random(41))
    for level in CHAIN_LEVELS:
        for v in ins:
            for t in chk.targets(v, level):
                chk.check(v, t, level, "chain medium")
    assert chk.n - n0 >= 18 * 10 * 36, chk.n - n0
    assert chk.cut - cut0 >= 1000


def test_chain_levels_big(chk, O, corpus):
    """levels 0 .. 9 on whole golden files and around the 65547 boundary (64 KiB of text, binary and image data, App. F blocks, a
    run of one byte, incompressible bytes; 65546, 65547, 65548 and 200,000 bytes): the band, targets >= compressBound, random
    targets and the fixed-size units of a page and a quarter block"""
    n0, cut0 = chk.n, chk.cut
    rng = random.Random(43)
    book1 = corpus["book1[:200000]"]
    ins = [corpus["book1[:65536]"], corpus["geo[:65536]"], corpus["pic[:65536]"], O.gen_block(65536, 0), O.gen_block(65536, 1),
           bytes(65536), rng.randbytes(65536), book1[:65546], book1[:65547], book1[:65548], O.gen_block(65549, 3, litmax=4, win=64),
           b"\x00" * 70000, book1]
    for level in CHAIN_LEVELS:
        for v in ins:
            for t in sorted(set(chk.targets(v, level, 3)) | {4096, 16384}):
                chk.check(v, t, level, "chain big")
    assert chk.n - n0 >= 13 * 10 * 36, chk.n - n0
    assert chk.n - n0 >= 2000
    assert chk.cut - cut0 >= 1000


def test_calgary_slices(chk):
    """64 KiB slices further into the Calgary files book1, geo and pic, at levels 1, 4 and 9"""
    n0 = chk.n
    for name in ("book1", "geo", "pic"):
        data = calgary(name)
        for o in (65536 * 2, len(data) - 65536):
            v = data[o:o + 65536]
            for level in (1, 4, 9):
                for t in chk.targets(v, level, 2) + [4096, 32768]:
                    chk.check(v, t, level, name)
    assert chk.n - n0 >= 3 * 2 * 3 * 36
