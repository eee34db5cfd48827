"""The decoded-size query on the CPU: tests/hostsim/hostsim_size.cpp compiles lz4-java_amd/csrc/lz4_decode_size.h against the
lock-step lane simulator with a backend that has NO destination (any access outside the stream counts as out of bounds), in both
forms -- the exact path alone, and the fast interior in front of it (stream ring of 2048 bytes, as on the device, and of 1024) --
and this file checks every value against the return value of the reference library's own LZ4_decompress_safe, called with a real
buffer of cap + 64 bytes.  Zero mismatches, nothing skipped, every test asserts its case count."""
import ctypes as C

import pytest

from size_common import (SEAM_SIZES, caps_for, edge_streams, long_literal_stream, ref_size, rng_for, seam_streams, stream_set,
                         valid_streams)
from support import build_sim

FORMS = ((0, 2048), (1, 2048), (1, 1024))   # (fast interior, stream ring bytes): exact only; what the kernel runs; a smaller ring


def load_sim():
    l = build_sim("hostsim_size")
    l.sim_decoded_size.restype = C.c_int
    l.sim_decoded_size.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    return l


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def want(ref):
    return ref_size(ref)


class Checker:
    def __init__(self, sim, want):
        self.sim, self.want, self.n = sim, want, 0

    def check(self, s, cap, what="", forms=FORMS):
        w = self.want(s, cap)
        for fast, ks in forms:
            got = self.sim.sim_decoded_size(bytes(s), len(s), cap, fast, ks, None)
            assert got != -1000000, ("out of bounds", what, fast, ks, len(s), cap)
            assert got == w, (what, fast, ks, len(s), cap, got, w)
            self.n += 1
        return w


@pytest.fixture()
def chk(sim, want):
    return Checker(sim, want)


def test_size_stream_set_every_capacity(chk, ref, O):
    """Calgary, App. F and book1 blocks by the fast and the HC compressor, overlapping matches, 1 .. 3 byte flips, every cut of a
    short stream and random bytes, each with the whole capacity list"""
    cases = stream_set(ref, O, rng_for(11))
    assert len(cases) > 3800
    for name, s, d in cases:
        for cap in caps_for(d, len(s)):
            chk.check(s, cap, name, forms=FORMS if len(s) < 20000 else FORMS[:2])
    assert chk.n > 3800 * 13 * 2


def test_size_fast_interior_does_the_block(sim, want, ref, O):
    """on a valid block the exact code sees only the ends and the long runs: the fast interior takes the rest (an interior that took
    nothing would still return the right value)"""
    n = 0
    for name, s, d in valid_streams(ref, O):
        if d < 60000 or name.startswith("zeros"):
            continue
        exact, fast = C.c_longlong(), C.c_longlong()
        assert sim.sim_decoded_size(s, len(s), d + 700, 0, 2048, C.byref(exact)) == d == want(s, d + 700)
        assert sim.sim_decoded_size(s, len(s), d + 700, 1, 2048, C.byref(fast)) == d
        assert fast.value * 8 < exact.value, (name, fast.value, exact.value)
        n += 1
    assert n >= 14


def test_size_seams_of_window_and_ring(chk):
    """token, length-extension runs (literal and match, 1 .. 3 bytes), offset bytes and the end of the block at S - 2 .. S + 2 and
    2 S - 2 .. 2 S + 2 for S = the loop's window (256) and its stream ring (2048)"""
    cases = seam_streams(rng_for(12))
    assert len(cases) == len(SEAM_SIZES) * 2 * 5 * 5 * 2
    for name, s, d in cases:
        assert chk.want(s, d + 700) == d, name       # the hand-built block is valid
        for cap in caps_for(d, len(s)):
            chk.check(s, cap, name)
    assert chk.n >= 200 * 13 * 3


def test_size_offsets_at_the_block_start(chk):
    """an offset equal to op decodes; op + 1 fails with liblz4's code; 0 is accepted (liblz4 1.9.3 does not look) -- in the exact code
    and in the fast interior"""
    cases = edge_streams(rng_for(13))
    assert len(cases) == 6
    for name, s, d in cases:
        w = chk.check(s, d + 700, name)
        if "op + 1" in name:
            assert w < 0, name
        else:
            assert w == d, name
        for cap in caps_for(d, len(s)):
            chk.check(s, cap, name)
    assert chk.n >= 6 * 14 * 3


def test_size_trivial_inputs(chk, sim):
    """empty input, the one-byte stream 00, and negative sizes (-1: the engine's rule, the reference is not called with them)"""
    for cap in (0, 1, 63, 64, 65, 700):
        assert chk.check(b"", cap) == -1
        assert chk.check(b"\x00", cap) == 0
        chk.check(b"\x10a", cap)
        chk.check(b"\xff" * 20, cap)
    assert chk.n == 6 * 4 * 3
    for fast, ks in FORMS:
        assert sim.sim_decoded_size(b"\x10a", -1, 10, fast, ks, None) == -1
        assert sim.sim_decoded_size(b"\x10a", 2, -1, fast, ks, None) == -1


def test_size_long_literal_run(chk):
    """a literal length whose extension bytes sum past 2^31: the 32-bit sum and the length cap behave as in decode_block"""
    s, _ = long_literal_stream()
    for cap in (0, 63, 64, 65, 104, 1000, 8 << 20):
        assert chk.check(s, cap, "long literals", forms=FORMS[:2]) < 0
    assert chk.n == 14
