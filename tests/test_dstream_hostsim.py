"""The stream decoder (LZ4_decompress_safe_continue in every mode of liblz4's LZ4_streamDecode_t) on the CPU: tests/hostsim/hostsim_dstream.cpp
compiles the stream walk (lz4-java_amd/csrc/lz4_decode_stream.h) and decode_block's PREFIX && DICT switch against the lock-step lane
simulator -- the exact tiers alone, the plain loop, the pipelined loop, and the deep loop with the pipelined loop behind it on 8 lanes,
the form decode_stream_kernel runs -- and this file checks every block's return value, every state record and, where a layout keeps a
block's slot clear of the history it can reach, every byte of the streams of tests/dstream_common.py against the reference library's
own stream decoder.  Every stream is cut into calls at every block boundary and at random ones, the state threaded through.  The
simulator flags every access outside the streams, the window and the history pieces, every write outside the current block's capacity,
and a changed guard, dictionary or stream byte; each stream runs in both arena layouts (hostsim_dstream.cpp)."""
import collections
import ctypes as C

import pytest

from chain_common import Chain
from conftest import lz4_seq
from dstream_common import (BRANCHES, CHAIN_STOPPED, DICT, FILL, Block, RefStream, Stream, book1, hostile_set, layout_set, lit_block, make_stream, random_cuts,
                            rng_for, same_state)
from support import build_sim

# (library, form, lanes): the exact tiers alone; plain; pipelined; deep with the pipelined loop behind it (decode_stream_kernel<8>)
FORMS = (("exact", 0, 8), ("full", 0, 8), ("full", 1, 8), ("full", 2, 8))
DICT_END = 1 << 62


def load_sims():
    libs = {}
    for name, variant, flags in (("full", "", ()), ("exact", "_exact", ("-DLZ4HIP_DECODE_INTERIOR=0",))):
        l = build_sim("hostsim_dstream", variant, flags)
        l.sim_dstream.restype = C.c_int
        l.sim_dstream.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                  C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.sim_double_dict.restype = C.c_int
        l.sim_double_dict.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint8,
                                      C.c_void_p, C.c_void_p]
        l.sim_dstream_deep_trips.restype = C.c_uint64
        libs[name] = l
    return libs


@pytest.fixture(scope="module")
def sims():
    return load_sims()


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


@pytest.fixture(scope="module")
def streams(rs):
    """about 300 streams over the layouts, the hostile ones among them"""
    rng = rng_for(31)
    return layout_set(rs, rng, 30) + hostile_set(rs, rng, 12)


def run_stream(sims, rs, s, cuts, lib, form, gl, layout):
    """stream s through the simulator, cut into calls at `cuts`, against the reference cut the same way -> mismatches"""
    w = rs.decode(s, cuts)
    window = C.create_string_buffer(bytes([FILL]) * s.win_len, max(s.win_len, 1))
    model = bytearray([FILL]) * s.win_len
    state = (C.c_uint64 * 4)(*[DICT_END if v == DICT else v for v in s.state])
    d = s.dictionary or b""
    bad, k = [], 0
    for ci, cut in enumerate(cuts):
        if k in s.before:      # the caller's own move and LZ4_setStreamDecode (layout c)
            moves, (se, sn) = s.before[k]
            for d_, s_, n_ in moves:
                chunk = window.raw[s_:s_ + n_]
                C.memmove(C.addressof(window) + d_, chunk, n_)
                model[d_:d_ + n_] = chunk
            state[0], state[1], state[2], state[3] = se, sn, 0, 0
        blocks = s.blocks[k:cut]
        n = len(blocks)
        src = b"".join(b.comp for b in blocks)
        off, p = [], 0
        for b in blocks:
            off.append(p); p += len(b.comp)
        out = (C.c_int32 * max(n, 1))(*([12345] * max(n, 1)))
        st = sims[lib].sim_dstream(src, len(src), (C.c_uint64 * max(n, 1))(*off), (C.c_int32 * max(n, 1))(*[b.src_len for b in blocks]),
                                   (C.c_uint64 * max(n, 1))(*[b.off for b in blocks]), (C.c_int32 * max(n, 1))(*[b.cap for b in blocks]), n, window,
                                   s.win_len, d, len(d), 1 if s.lead else 0, state, form, gl, layout, out)
        tag = (s.name, lib, form, gl, layout, "call %d" % ci)
        if st != 0:
            return [tag + ("out of bounds / guard",)]
        if list(out[:n]) != w.out[k:cut]:
            return [tag + ("results", list(out[:n])[:8], w.out[k:cut][:8])]
        got = tuple(DICT if (v == DICT_END and i in (0, 2)) else v for i, v in enumerate(state))
        if not same_state(got, w.states[ci]):
            return [tag + ("state", got, w.states[ci])]
        for j, b in enumerate(blocks):
            r = w.out[k + j]
            if r > 0:
                model[b.off:b.off + r] = w.data[k + j]
            elif r < 0 and r != CHAIN_STOPPED and b.cap > 0:
                model[b.off:b.off + b.cap] = window.raw[b.off:b.off + b.cap]
        if s.exact and window.raw[:s.win_len] != bytes(model):
            return [tag + ("bytes",)]
        if not s.exact:
            model[:] = window.raw[:s.win_len]
        k = cut
    return bad


def cut_sets(s, rng):
    n = len(s.blocks)
    every = list(range(1, n + 1))
    if s.before:              # (layout c: its caller moves the history between every two blocks)
        return [every]
    return [every, random_cuts(n, 3, rng), [n]]


def test_dstream_reference_takes_every_branch(rs, streams):
    """the reference takes each of the five branches of LZ4_decompress_safe_continue at least ten times over the set, and 0-byte
    blocks fall at jumps"""
    cnt = collections.Counter()
    zero_jumps = 0
    for s in streams:
        w = rs.decode(s, [len(s.blocks)])
        cnt.update(b for b in w.branch if b)
        zero_jumps += sum(1 for b, br, r in zip(s.blocks, w.branch, w.out) if b.size == 0 and br == "extdict" and r == 0)
    print(dict(cnt), zero_jumps)
    assert all(cnt[b] >= 10 for b in BRANCHES), cnt
    assert zero_jumps >= 100


def test_dstream_every_stream(sims, rs, streams):
    """zero mismatches in results, states and bytes over about 300 streams, each cut at every block boundary, at random ones and not
    at all, in every form and both arena layouts; no access outside window, history pieces and streams"""
    rng = rng_for(32)
    t0 = sims["full"].sim_dstream_deep_trips()
    bad, runs = [], 0
    for t, s in enumerate(streams):
        for ci, cuts in enumerate(cut_sets(s, rng)):
            # (every form sees every stream; the arena layouts and cut sets alternate over the forms, so that every pair occurs)
            for fi, (lib, form, gl) in enumerate(FORMS):
                bad += run_stream(sims, rs, s, cuts, lib, form, gl, (t + ci + fi) & 1)
                runs += 1
    print("%d streams, %d blocks, %d simulator runs, %d mismatches" % (len(streams), sum(len(s.blocks) for s in streams), runs, len(bad)))
    assert not bad, bad[:10]
    assert len(streams) >= 280
    assert sims["full"].sim_dstream_deep_trips() - t0 > 1000   # the deep loop really ran (layout e's blocks of up to 60000 bytes)


def test_dstream_double_dict_block(sims, rs):
    """decode_block's PREFIX && DICT instance alone against LZ4_decompress_safe_continue in its doubleDict branch: a match that
    straddles the external dictionary's end and the prefix's start, one that straddles the prefix's end and the block's start, one
    wholly in each part -- at every distance around the joints, in every form"""
    rng = rng_for(33)
    cases = []
    for E, P in ((300, 40), (70000, 100), (65536, 7), (50, 3000)):
        lit = 3
        for name, off, ml in (("ext->prefix", lit + P + 5, 5 + 9), ("ext->prefix->block", lit + P + 4, 4 + P + 20), ("prefix->block", lit + 6, 40),
                              ("in ext", lit + P + min(E, 60000), 12), ("in prefix", lit + P - 1, 4 if P < 8 else 6), ("in block", 2, 30),
                              ("ext end exactly", lit + P + 8, 8), ("one past ext", lit + P + E + 1, 8)):
            if not 1 <= off <= 65535:
                continue
            comp = lz4_seq(lit, ml, off, rng) + bytes([6 << 4]) + rng.randbytes(6)
            cases.append(("%s E=%d P=%d" % (name, E, P), E, P, comp, lit + ml + 6))
        # a long block around the joints: the interior loops see dictionary matches too
        seqs = b"".join(lz4_seq(rng.randrange(0, 20), rng.randrange(4, 40), rng.randrange(1, min(65535, P + E)), rng) for _ in range(400))
        cases.append(("long E=%d P=%d" % (E, P), E, P, seqs + bytes([6 << 4]) + rng.randbytes(6), None))
    bad = 0
    for name, E, P, comp, size in cases:
        cap = size if size is not None else 40000
        # the reference: ext far up in a window, the prefix at its start (a jump), the block behind the prefix (doubleDict)
        blocks = [Block(lit_block(E, rng), P + cap + 64, E, E), Block(lit_block(P, rng), 0, P, P)]
        ext, pre = blocks[0].comp[-E:], blocks[1].comp[-P:]
        s = Stream(name, "h", P + cap + 64 + E, blocks + [Block(comp, P, cap)], True)
        w = rs.decode(s, [3])
        assert w.branch[2] == "doubledict"
        for lib, form, gl in FORMS:
            out = C.create_string_buffer(max(cap, 1))
            status = C.c_int(0)
            r = sims[lib].sim_double_dict(comp, len(comp), pre, P, ext, E, cap, form, gl, FILL, out, C.byref(status))
            if status.value != 0 or r != w.out[2] or (r > 0 and out.raw[:r] != w.data[2]) or (r > 0 and out.raw[r:cap] != bytes([FILL]) * (cap - r)):
                bad += 1
                print("MISMATCH", name, lib, form, status.value, r, w.out[2])
    assert not bad
    assert any(size is not None and n.startswith("ext->prefix->block") for n, _, _, _, size in cases)


def test_dstream_contiguous_equals_chain_walk(sims, rs, ref):
    """layout a, from a fresh state and from a state that was set (a dictionary directly in front of the window): the results, and the
    bytes, are chain_walk's"""
    from test_chain_hostsim import load_sims as load_chain_sims, sim_chain
    csims = load_chain_sims()
    rng = rng_for(34)
    data = book1()
    for t in range(12):
        if t & 1:
            s = make_stream(rs, "a", rng, data, tag="chain #%d" % t, zero_at_jump=False)
        else:
            s = rs.write("set #%d" % t, "f", 40000, [data[o:o + 3000] for o in range(50000, 80000, 3000)], lambda k, n_, pos: pos, True,
                         dictionary=data[40000 - (70000, 5000, 9)[t % 3]:40000], lead=True, zero_at_jump=False)
        ch = Chain(s.name, [(b.comp, False, b.cap) for b in s.blocks], history=s.dictionary or b"", ccap=s.win_len)
        st, o, done, region = sim_chain(csims, ch, "full", 2, 8, 0)
        assert st == 0
        w = rs.decode(s, [len(s.blocks)])
        assert o == w.out and done == sum(w.out)
        assert not run_stream(sims, rs, s, [len(s.blocks)], "full", 2, 8, 0)
        assert region[:done] == b"".join(w.data)
