"""The fill compressor (LZ4_compress_destSize) on the CPU: tests/hostsim/hostsim_destsize.cpp compiles FastCore with
DirectOut<..., FILL = true> of lz4-java_amd/csrc/lz4_fast_core.h -- the core compress_fast_dest_cu_kernel runs -- against the
lock-step lane simulator, with the simulator's bounds set to [src, src+n) and [dst, dst+target), and this file checks return value,
consumed size and bytes against the reference library's own LZ4_compress_destSize."""
import ctypes as C
import random

import pytest

from conftest import calgary, rnd_inputs
from support import build_sim

_u8p = C.POINTER(C.c_uint8)


def bound(n):
    return n + n // 255 + 16 if 0 <= n <= 0x7E000000 else 0


def load_sim():
    l = build_sim("hostsim_destsize")
    l.sim_compress_dest_size.restype = C.c_int
    l.sim_compress_dest_size.argtypes = [C.c_char_p, C.c_int, _u8p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_uint64]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


def ref_dest_size(ref):
    """(src, target) -> (ret, consumed, bytes): the reference library's LZ4_compress_destSize itself"""
    f = C.CDLL(ref.path).LZ4_compress_destSize
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.POINTER(C.c_int), C.c_int]

    def run(v, t):
        out = (C.c_uint8 * max(t, 1))()
        sz = C.c_int(len(v))
        r = f(bytes(v), out, C.byref(sz), t)
        return r, sz.value, bytes(out[:max(r, 0)])
    return run


@pytest.fixture(scope="module")
def lz4dest(ref):
    return ref_dest_size(ref)


def sim_dest(sim, v, t, seed=0):
    out = (C.c_uint8 * max(t, 1))()
    cons = C.c_int(-7)
    r = sim.sim_compress_dest_size(bytes(v), len(v), out, t, C.byref(cons), None, seed)
    return r, cons.value, bytes(out[:max(r, 0)])


def sequences(b):
    """an LZ4 block -> ([(literals, offset, matchlen)], last literals)"""
    i, seqs = 0, []
    while True:
        tok = b[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                x = b[i]; i += 1; lit += x
                if x != 255:
                    break
        lits = b[i:i + lit]; i += lit
        if i >= len(b):
            return seqs, lits
        off = b[i] | (b[i + 1] << 8); i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                x = b[i]; i += 1; ml += x
                if x != 255:
                    break
        seqs.append((lits, off, ml + 4))


def shape(out, default):
    """the structural property: 'prefix' (the first k sequences of the default parse, then literals) or 'short' (the same plus
    sequence k with its literals and offset and a shorter match); anything else fails"""
    s, _ = sequences(out)
    d, _ = sequences(default)
    k = len(s)
    if k == 0 or s[-1] == d[k - 1]:
        assert s == d[:k]
        return "prefix"
    assert s[:-1] == d[:k - 1] and s[-1][:2] == d[k - 1][:2] and s[-1][2] < d[k - 1][2]
    return "short"


class Checker:
    def __init__(self, sim, lz4dest, ref):
        self.sim, self.lz4dest, self.ref = sim, lz4dest, ref
        self.rng = random.Random(11)
        self.kinds = {"prefix": 0, "short": 0}
        self.default = {}

    def check(self, v, t, what=""):
        want = self.lz4dest(v, t)
        got = sim_dest(self.sim, v, t, seed=self.rng.getrandbits(63) | 1)
        assert got == want, (what, len(v), t, got[:2], want[:2])
        if 0 < t < bound(len(v)) and want[0] > 0:
            key = bytes(v)
            if key not in self.default:
                self.default[key] = self.ref.compress_fast(v)
            self.kinds[shape(want[2], self.default[key])] += 1

    def targets(self, v, n_random=3):
        n = len(v)
        dl = len(self.ref.compress_fast(v))
        b = bound(n)
        ts = {1, 5, 6, 11, 12, 17, dl - 1, dl, dl + 1, b - 1, b}
        ts |= {self.rng.randrange(1, b + 3) for _ in range(n_random)}
        return sorted(t for t in ts if t >= -1)


@pytest.fixture(scope="module")
def chk(sim, lz4dest, ref):
    return Checker(sim, lz4dest, ref)


def test_small_inputs_every_target(chk, O, corpus):
    """n = 0 .. 40, 100, 1000: every target from -1 to compressBound + 2"""
    book1 = corpus["book1[:200000]"]
    for n in list(range(0, 41)) + [100, 1000]:
        for v in (book1[5000:5000 + n], O.gen_block(n, n, litmax=4, win=8)):
            for t in range(-1, bound(n) + 3):
                chk.check(v, t, "small")


def test_fuzz(chk, O, corpus):
    """about 1,500 mixed inputs at the targets around every edge: 1, 5, 6, 11, 12, 17, len(default) +- 1, bound - 1, bound, random"""
    for v in rnd_inputs(O, corpus, 23, 1500):
        for t in chk.targets(v):
            chk.check(v, t, "fuzz")


def test_calgary_slices(chk):
    """Calgary 64 KiB slices of book1, geo and pic at the edge targets and at the fixed-size units of a page / quarter block"""
    for name in ("book1", "geo", "pic"):
        data = calgary(name)
        for o in range(0, len(data) - 65536 + 1, 65536 * 2):
            v = data[o:o + 65536]
            for t in chk.targets(v, 2) + [4096, 16384, 32768]:
                chk.check(v, t, name)


def test_zero_and_two_symbol(chk):
    """zero-filled inputs (one long match) and two-symbol inputs; by the structural check, at least 50 of these outputs end with a
    shortened match, so the suite demonstrably covers that path"""
    rng = random.Random(3)
    short0 = chk.kinds["short"]
    for n in (13, 100, 1000, 4096, 65535, 65536, 65547):
        z = bytes(n)
        two = bytes(rng.choice((0x41, 0x42)) for _ in range(n))
        for v in (z, two):
            for t in chk.targets(v, 6) + list(range(1, 40)):
                chk.check(v, t, "zero/two")
    assert chk.kinds["short"] - short0 >= 50, chk.kinds


def test_byu32_inputs(chk, O, corpus):
    """byU32 tables: 65547, 70000 and 200,000 bytes"""
    book1 = corpus["book1[:200000]"]
    for v in (book1[:65547], O.gen_block(70000, 4), book1, O.gen_block(200000, 9, win=4096), bytes(70000)):
        for t in chk.targets(v, 4) + [1000, 4096, 65536]:
            chk.check(v, t, "byU32")
