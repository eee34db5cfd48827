"""The dictionary decoder (LZ4_decompress_safe_usingDict, external dictionary) on the CPU: tests/hostsim/hostsim_dict.cpp compiles
decode_block's DICT switch (lz4-java_amd/csrc/lz4_decode_core.h) against the lock-step lane simulator -- the exact tiers alone (a build
that never enters the interior loop) and every interior loop the dictionary kernels run in front of them: plain, staged with 4 lanes,
deep with 8 (and the pipelined loop behind it), pipelined alone -- and this file checks return value and bytes of every stream x capacity
x dictionary of tests/dict_common.py against the reference library's own LZ4_decompress_safe_usingDict.  The simulator flags every
access outside the stream, the dictionary and [dst, dst + cap); each case runs in both arena layouts (hostsim_dict.cpp), so a read past
either end of the dictionary is caught."""
import ctypes as C

import pytest

from dict_common import DICT_LENS, RefDict, book1, caps_for, case_set, hand_streams, rng_for
from support import build_sim

# (library, form, lanes): the exact tiers alone; plain; staged (decode_dict_kernel<4, 0, true>); deep (decode_dict_deep_kernel<8>); pipelined
FORMS = (("exact", 0, 4), ("exact", 0, 8), ("full", 0, 4), ("full", 0, 8), ("full", 1, 4), ("full", 2, 8), ("full", 3, 8))


def load_sims():
    libs = {}
    for name, variant, flags in (("full", "", ()), ("exact", "_exact", ("-DLZ4HIP_DECODE_INTERIOR=0",))):
        l = build_sim("hostsim_dict", variant, flags)
        l.sim_decompress_dict.restype = C.c_int
        l.sim_decompress_dict.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        libs[name] = l
    return libs


@pytest.fixture(scope="module")
def sims():
    return load_sims()


@pytest.fixture(scope="module")
def rd(ref):
    return RefDict(ref)


@pytest.fixture(scope="module")
def cases(rd):
    return case_set(rd, rng_for(11))


def sim_dict(sims, s, cap, d, lib, form, gl, layout):
    out = C.create_string_buffer(max(cap, 0) + 1)
    r = sims[lib].sim_decompress_dict(bytes(s), len(s), out, cap, bytes(d), len(d), form, gl, layout)
    return r, out.raw[:max(r, 0)]


class Checker:
    def __init__(self, sims, rd):
        self.sims, self.rd, self.n, self.bad = sims, rd, 0, []

    def check(self, s, cap, d, what="", forms=FORMS):
        want = self.rd.decode(s, cap, d)
        for lib, form, gl in forms:
            for layout in (0, 1):
                got = sim_dict(self.sims, s, cap, d, lib, form, gl, layout)
                if got != want:
                    self.bad.append((what, lib, form, gl, layout, len(s), cap, len(d), got[0], want[0]))
                self.n += 1
        return want[0]


def test_dict_set_really_uses_the_dictionary(rd, cases):
    """at least 90 % of the valid streams of every dictionary of 4096 bytes and more are rejected by the plain LZ4_decompress_safe"""
    valid, _ = cases
    for L in DICT_LENS:
        if L < 4096:
            continue
        mine = [c for c in valid if c[3] == L]
        rejected = sum(1 for _, s, d, _ in mine if rd.plain(s, d) != d)
        print("L = %d: %d of %d valid streams rejected without the dictionary" % (L, rejected, len(mine)))
        assert len(mine) >= 20 and rejected >= 0.9 * len(mine), (L, rejected, len(mine))


def test_dict_hand_built_streams_cover_the_rules(rd):
    """what the hand-built streams are for, said by the reference: both kinds of straddle, op + L decodes and op + L + 1 is an error
    at the offset, a dictionary match may end at cap - 5 and not at cap - 4"""
    b = book1()
    hs = hand_streams(rng_for(5))
    names = [h[0] for h in hs]
    assert any("overlap" in n for n in names) and any(n.startswith("straddle") and "overlap" not in n for n in names)
    s, d, L = next((s, d, L) for n, s, d, L in hs if n == "the issue's example")
    r, out = rd.decode(s, d, b[:L])
    assert r == d == 13 and out[1:5] == bytes([b[L - 1], out[0], b[L - 1], out[0]])
    for n, s, d, L in hs:
        if n.startswith("offset == op + L + 1"):
            lit = s[0] >> 4                                    # token, literals, offset: the error is reported behind the offset
            r = rd.decode(s, d, b[:L])[0]                      # (near the stream's end an extended length is read first)
            assert r == -(lit + 4) if n.endswith("ml=6") else -(lit + 8) <= r <= -(lit + 4), (n, r)
        if n.startswith("offset == op + L,"):
            assert rd.decode(s, d, b[:L])[0] == d, n
        if n.endswith("then five literals"):
            assert rd.decode(s, d, b[:L])[0] == d, n            # the match ends at cap - 5
            r = rd.decode(s, d - 1, b[:L])[0]                   # ... at cap - 4: an error AT THE MATCH, not at the last literals
            tok_pos = len(s) - 6
            assert r < 0 and -r - 1 <= tok_pos, (n, r)
    s, d = next((s, d) for n, s, d, L in hs if n == "offset == op + L + 1, ml=6" and L == 100 and (s[0] >> 4) == 1)
    assert rd.decode(s, d, b[:100])[0] == -5                    # the issue's example: a 1-literal sequence, offset dict_len + 2


def test_dict_every_stream_capacity_and_dictionary(sims, rd, cases):
    """zero mismatches in value and bytes over the whole set, in every form and both arena layouts"""
    b = book1()
    _, all_cases = cases
    chk = Checker(sims, rd)
    n_cases = 0
    for name, s, d, L in all_cases:
        for cap in caps_for(d, len(s)):
            chk.check(s, cap, b[:L], name)
            n_cases += 1
    print("%d streams, %d stream x capacity cases, %d simulator runs, %d mismatches" % (len(all_cases), n_cases, chk.n, len(chk.bad)))
    assert not chk.bad, chk.bad[:10]
    assert len(all_cases) > 1500 and n_cases > 15000 and chk.n == n_cases * len(FORMS) * 2


def test_dict_len_0_is_the_plain_decoder(sims, rd, ref):
    """dict_len == 0: LZ4_decompress_safe's value and bytes, on valid and damaged streams"""
    b = book1()
    rng = rng_for(3)
    chk = Checker(sims, rd)
    for v in (b[:5000], b[300000:365536], b"abcd      abcdefghij"):
        s = ref.compress_fast(v)
        for t in [s] + [bytes(x if rng.random() > 0.002 else rng.randrange(256) for x in s) for _ in range(4)]:
            for cap in (len(v) - 1, len(v), len(v) + 70):
                want = chk.check(t, cap, b"", "no dictionary")
                assert want == rd.plain(t, cap)
    assert not chk.bad, chk.bad[:10]


def test_dict_edge_values(sims, rd):
    """capacity 0, the empty stream, negative sizes (-1: the engine's rule; the reference is not called with them)"""
    b = book1()
    chk = Checker(sims, rd)
    for s in (b"", b"\x00", b"\x10a", b"\xff" * 20):
        for cap in (0, 5):
            chk.check(s, cap, b[:100], "edge")
    assert not chk.bad, chk.bad
    for lib, form, gl in FORMS:
        assert sim_dict(sims, b"\x10a", -1, b[:100], lib, form, gl, 0)[0] == -1
        assert sims[lib].sim_decompress_dict(b"\x10a", -1, C.create_string_buffer(16), 10, b[:100], 100, form, gl, 0) == -1
