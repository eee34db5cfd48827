"""The accelerated fast compressor (LZ4_compress_fast with acceleration > 1) on the CPU: tests/hostsim/hostsim_accel.cpp compiles
FastCore<..., ACC = true> of lz4-java_amd/csrc/lz4_fast_core.h -- the core compress_fast_accel_cu_kernel runs -- against the lock-step
lane simulator, and this file checks it bit-for-bit against the reference library's own LZ4_compress_fast."""
import ctypes as C
import random

import pytest

from conftest import rnd_inputs
from support import build_sim

_u8p = C.POINTER(C.c_uint8)
ACCELS = (-5, 0, 1, 2, 3, 4, 7, 8, 9, 16, 17, 63, 64, 65, 100, 1000, 65536, 65537, 65538)


def clamp(a):
    """LZ4_compress_fast_extState: < 1 -> 1, > LZ4_ACCELERATION_MAX (65537) -> 65537 (the library does the same before a launch)"""
    return 1 if a < 1 else min(a, 65537)


def load_sim():
    l = build_sim("hostsim_accel")
    l.sim_compress_fast_accel.restype = C.c_int
    l.sim_compress_fast_accel.argtypes = [C.c_char_p, C.c_int, _u8p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint64]
    l.sim_accel_offsets.restype = None
    l.sim_accel_offsets.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def lz4fast(ref):
    """(src, cap, acceleration) -> (ret, bytes): the reference library's LZ4_compress_fast itself"""
    f = C.CDLL(ref.path).LZ4_compress_fast
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_int]

    def run(v, cap, a):
        out = (C.c_uint8 * max(cap, 1))()
        r = f(bytes(v), out, len(v), cap, a)
        return r, bytes(out[:max(r, 0)])
    return run


def sim_compress(sim, v, cap, a, seed=0):
    out = (C.c_uint8 * max(cap, 1))()
    st = (C.c_uint64 * 4)()
    r = sim.sim_compress_fast_accel(bytes(v), len(v), out, cap, clamp(a), st, seed)
    return r, bytes(out[:max(r, 0)]), list(st)


def g_replay(a, kmax):
    """liblz4's miss-run loop (LZ4_compress_generic: forwardIp += step; step = searchMatchNb++ >> LZ4_skipTrigger), replayed:
    the offset of every probe from the run start"""
    pos, step, nb, out = 0, 1, a << 6, []
    for _ in range(kmax):
        out.append(pos)
        pos += step
        step = nb >> 6
        nb += 1
    return out


def test_probe_offsets_match_liblz4_step_loop(sim):
    """g_a(k) = g_1(k) + (a - 1)(k - 1) for k >= 1, checked lane by lane against a replay of liblz4's step loop"""
    buf = (C.c_uint32 * 64)()
    for a in (1, 2, 3, 7, 8, 64, 65, 1000, 65537):
        want = g_replay(a, 5000 + 64)
        for k0 in list(range(0, 5000, 64)) + [1, 2, 63, 65, 127, 129, 4990]:
            sim.sim_accel_offsets(a, k0, buf)
            assert list(buf) == want[k0:k0 + 64], (a, k0)


def caps_for(lz4fast, v, a):
    """full (compressBound), tight (exactly the size) and one byte short"""
    full = len(v) + len(v) // 255 + 16
    er, _ = lz4fast(v, full, a)
    return full, [full, er, max(0, er - 1)]


def test_accel_core_corpus(sim, lz4fast, corpus):
    """every corpus input (the 65546 / 65547 table boundary, 200000 B and 1 MiB byU32 blocks, zeros, lengths 0 / 12 / 13) x every
    acceleration (clamped ones included) x full / tight / one-byte-short capacities, several LDS-atomic lane orders"""
    rng = random.Random(5)
    slow = 0
    for name, v in corpus.items():
        for a in ACCELS:
            full, caps = caps_for(lz4fast, v, a)
            for cap in caps:
                want = lz4fast(v, cap, a)
                r, b, st = sim_compress(sim, v, cap, a, seed=rng.getrandbits(63) | 1)
                assert r == want[0] and (r <= 0 or b == want[1]), (name, a, cap, r, want[0])
                slow += st[1]
    assert slow > 0   # the collision-resolution path was exercised


def test_accel_changes_the_bytes(sim, lz4fast, corpus):
    """the core really runs the accelerated parse: on text, acceleration 8 finds fewer sequences and a different stream"""
    v = corpus["book1[:65536]"]
    r1, b1, st1 = sim_compress(sim, v, 70000, 1)
    r8, b8, st8 = sim_compress(sim, v, 70000, 8)
    assert b1 == lz4fast(v, 70000, 1)[1] and b8 == lz4fast(v, 70000, 8)[1]
    assert b1 != b8 and st8[3] < st1[3] and st8[0] < st1[0]


def test_accel_core_fuzz(sim, lz4fast, O, corpus):
    """a few hundred mixed inputs x random accelerations x {full, tight, one byte short, random} capacities x random lane orders"""
    rng = random.Random(7)
    for v in rnd_inputs(O, corpus, 31, 300):
        for a in rng.sample(ACCELS, 3):
            full, caps = caps_for(lz4fast, v, a)
            for cap in caps + [rng.randrange(0, full + 1)]:
                want = lz4fast(v, cap, a)
                r, b, _ = sim_compress(sim, v, cap, a, seed=rng.getrandbits(63) | 1)
                assert r == want[0] and (r <= 0 or b == want[1]), (len(v), a, cap, r, want[0])
