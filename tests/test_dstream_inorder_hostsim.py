"""The in-order tier of the stream decoder on the CPU: tests/hostsim/hostsim_dstream_inorder.cpp compiles lz4_decode_inorder.h and the
INORDER walk of lz4_decode_stream.h against the lock-step lane simulator, in the form decode_stream_inorder_kernel runs (8 lanes, the
deep loop for the blocks whose slots are clear) and in the other forms of the existing simulator, and this file holds it to the
reference library and to the plain definition (dstream_inorder_common) on the layouts where a block's slot overlaps the history the
block can reach: liblz4's minimal rings, rings in step with the writer's, and a grid of hand-built two-block streams.

The simulator flags every access outside streams, window and history pieces, every write outside the current block's slot -- for a
block decoded in order: every write at or behind d + r -- and a changed guard, dictionary or stream byte.  Its backend lets a store of
an in-order block reach memory only at the core's next wait (order()) and at the block's end, so a load that depends on a store
without a wait between them reads the old byte and the comparison fails.  A stream is compared byte for
byte (the whole window against the replay of the reference's decoded bytes, block by block in order) up to its first negative result:
a failed slot's bytes are nobody's, and in these layouts they may be history afterwards."""
import ctypes as C

import pytest

from dstream_common import CHAIN_STOPPED, DICT, FILL, RefStream, hostile_set, layout_set, random_cuts, rng_for, same_state
from dstream_inorder_common import (GRID_WIN, behind_grid, count_overlaps, grid, grid_expected, hostile_overlap_set, overlap_set, slot_overlaps)
from support import build_sim
from test_dstream_hostsim import load_sims as load_old_sims
from test_dstream_inorder_plain import SEED_GRID, SEED_STREAMS

DICT_END = 1 << 62
VARIANTS = (("full", "", ()), ("exact", "_exact", ("-DLZ4HIP_DECODE_INTERIOR=0",)),
            ("lits-rounded-up", "_mutant1", ("-DLZ4HIP_INORDER_MUTANT=1",)), ("early-load", "_nosync", ("-DLZ4HIP_INORDER_NO_SYNC=1",)))
# (library, form): the exact tiers alone; plain; pipelined; deep with the pipelined loop behind it (the kernel's) -- for the blocks whose slots are clear
FORMS = (("exact", 0), ("full", 0), ("full", 1), ("full", 2))


@pytest.fixture(scope="module")
def sims():
    libs = {}
    for name, variant, flags in VARIANTS:
        l = build_sim("hostsim_dstream_inorder", variant, flags)
        l.sim_dstream_inorder.restype = C.c_int
        l.sim_dstream_inorder.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        libs[name] = l
    assert libs["lits-rounded-up"].sim_dstream_inorder_mutant() == 1 and libs["early-load"].sim_dstream_inorder_mutant() == 2
    assert libs["full"].sim_dstream_inorder_mutant() == 0
    return libs


@pytest.fixture(scope="module")
def old_sims():
    return load_old_sims()


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


class Run:
    """one stream going through the simulators call after call: the window, the state, the model of what the window must hold"""

    def __init__(self, s, w):
        self.s, self.w = s, w
        self.window = C.create_string_buffer(bytes([FILL]) * s.win_len, max(s.win_len, 1))
        self.model = bytearray([FILL]) * s.win_len
        self.state = (C.c_uint64 * 4)(*[DICT_END if v == DICT else v for v in s.state])
        self.k = self.ci = 0
        self.compare = True          # (False behind the stream's first negative result)
        self.n_inorder = self.n_orders = 0

    def tuple_state(self):
        return tuple(DICT if (v == DICT_END and i in (0, 2)) else v for i, v in enumerate(self.state))

    def call(self, cut, engine, tag=()):
        """blocks [k, cut) through engine = ("new", library, form, every, arena layout) or ("old", library, form, arena layout) -> mismatches"""
        s, w, k = self.s, self.w, self.k
        if k in s.before:      # the caller's own move and LZ4_setStreamDecode (layout c)
            moves, (se, sn) = s.before[k]
            for d_, s_, n_ in moves:
                chunk = self.window.raw[s_:s_ + n_]
                C.memmove(C.addressof(self.window) + d_, chunk, n_)
                self.model[d_:d_ + n_] = chunk
            self.state[0], self.state[1], self.state[2], self.state[3] = se, sn, 0, 0
        blocks = s.blocks[k:cut]
        n = len(blocks)
        src = b"".join(b.comp for b in blocks)
        off, p = [], 0
        for b in blocks:
            off.append(p); p += len(b.comp)
        arr = lambda t, v: (t * max(n, 1))(*v)
        out = arr(C.c_int32, [12345] * max(n, 1))
        d = s.dictionary or b""
        head = (src, len(src), arr(C.c_uint64, off), arr(C.c_int32, [b.src_len for b in blocks]), arr(C.c_uint64, [b.off for b in blocks]),
                arr(C.c_int32, [b.cap for b in blocks]), n, self.window, s.win_len, d, len(d), 1 if s.lead else 0, self.state)
        if engine[0] == "new":
            _, lib, form, every, layout = engine
            ni, no = C.c_uint64(0), C.c_uint64(0)
            st = lib.sim_dstream_inorder(*head, form, 8, layout, every, out, C.byref(ni), C.byref(no))
            self.n_inorder += ni.value; self.n_orders += no.value
        else:
            _, lib, form, layout = engine
            st = lib.sim_dstream(*head, form, 8, layout, out)
        tag = tuple(tag) + (s.name, engine[0], engine[2], "call %d" % self.ci)
        self.k, self.ci = cut, self.ci + 1
        if st != 0:
            return [tag + ("out of bounds / guard / a write at or behind d + r",)]
        if list(out[:n]) != w.out[k:cut]:
            return [tag + ("results", list(out[:n])[:8], w.out[k:cut][:8])]
        if not same_state(self.tuple_state(), w.states[self.ci - 1]):
            return [tag + ("state", self.tuple_state(), w.states[self.ci - 1])]
        for j, b in enumerate(blocks):
            r = w.out[k + j]
            if r > 0:
                self.model[b.off:b.off + r] = w.data[k + j]
            elif r < 0 and r != CHAIN_STOPPED:
                if s.layout in "msg":            # an overlap layout: the failed slot's bytes, nobody's, may be history from here on
                    self.compare = False
                elif b.cap > 0:                  # the failed slot is the one place left open
                    self.model[b.off:b.off + b.cap] = self.window.raw[b.off:b.off + b.cap]
        if self.compare and s.exact and self.window.raw[:s.win_len] != bytes(self.model):
            x = next(i for i in range(s.win_len) if self.window.raw[i] != self.model[i])
            return [tag + ("bytes", x)]
        if not (self.compare and s.exact):
            self.model[:] = self.window.raw[:s.win_len]
        return []


def run_stream(rs, s, cuts, engine_for, tag=()):
    """stream s cut into calls at `cuts`, call ci through engine_for(ci, run, cut) -> (mismatches, the Run)"""
    run = Run(s, rs.decode(s, cuts))
    for ci, cut in enumerate(cuts):
        bad = run.call(cut, engine_for(ci, run, cut), tag)
        if bad:
            return bad, run
    return [], run


def cut_sets(s, rng):
    """at random boundaries, as one call, and at EVERY block boundary -- for a stream of more than 150 blocks: at every boundary from
    four blocks in front of each wrap to four behind it (the wrap is where the state changes kind), the runs between them one call each"""
    n = len(s.blocks)
    if s.before:
        return [list(range(1, n + 1))]
    sets = [random_cuts(n, 3, rng), [n], random_cuts(n, 12, rng)]
    if n <= 150:
        return sets + [list(range(1, n + 1))]
    wraps = [k for k in range(1, n) if s.blocks[k].off < s.blocks[k - 1].off]
    assert wraps, s.name
    near = sorted({c for k in wraps for c in range(max(1, k - 4), min(n, k + 5) + 1)} | {n})
    return sets + [near]


def test_inorder_every_overlap_stream(sims, rs):
    """minimal rings (fit / max, exact and full capacities, max_block 4096 / 1024 / 64) and rings in step with the writer's: results, states
    and windows in every form and both arena layouts, cut at every block boundary (streams of up to 150 blocks), at random ones and as
    one call, the knob at 0 and at 1.  At 0 exactly the blocks whose slots overlap take the in-order tier; at 1 every block does"""
    rng = rng_for(SEED_STREAMS)
    streams = overlap_set(rs, rng, 2)
    bad, runs, ino0, blocks = [], 0, 0, 0
    for t, s in enumerate(streams):
        for ci, cuts in enumerate(cut_sets(s, rng)):
            for fi, (lib, form) in enumerate(FORMS):
                every = (t + ci + fi) & 1
                b, run = run_stream(rs, s, cuts, lambda *_: ("new", sims[lib], form, every, (t + ci + (fi >> 1)) & 1), (lib, "every=%d" % every))
                bad += b
                runs += 1
                if not b:
                    want = len(s.blocks) if every else count_overlaps(s, run.w)
                    if run.n_inorder != want:
                        bad.append((s.name, "blocks in order", run.n_inorder, want))
                    if not every:
                        ino0 += run.n_inorder; blocks += len(s.blocks)
    print("%d streams, %d simulator runs, %d mismatches; knob 0: %d of %d blocks decoded in order" % (len(streams), runs, len(bad), ino0, blocks))
    assert not bad, bad[:10]
    assert ino0 > 1000


def test_inorder_alternates_with_the_existing_walk(sims, old_sims, rs):
    """the two entry forms alternate on one stream from call to call: a call none of whose slots overlaps goes to the existing walk or
    to the new one in turn, a call with an overlapping slot to the new one -- results, states and windows as if one of them had run"""
    rng = rng_for(SEED_STREAMS + 1)
    streams = overlap_set(rs, rng, 1, blocks=(4096, 1024)) + [s for s in layout_set(rs, rng, 2) if s.exact]
    bad, calls = [], {"old": 0, "new": 0}
    for t, s in enumerate(streams):
        cuts = list(range(1, len(s.blocks) + 1)) if s.before or len(s.blocks) <= 150 else random_cuts(len(s.blocks), 40, rng)

        def engine(ci, run, cut):
            st = tuple(run.tuple_state())
            clear = DICT in st
            if not clear:
                clear, blocks = True, s.blocks[run.k:cut]
                for b, r in zip(blocks, run.w.out[run.k:cut]):
                    clear = clear and not slot_overlaps(st, b.off, b.cap)
                    pe, pl, ee, el = st
                    grows = pl != 0 and pe == b.off
                    if pl != 0 and not grows:
                        ee, el = pe, pl
                    if r > 0:
                        pe, pl = (pe + r, pl + r) if grows else (b.off + r, r)
                    st = (pe, pl, ee, el)
            which = "old" if clear and (ci + t) & 1 else "new"
            calls[which] += 1
            return ("old", old_sims["full"], 2, ci & 1) if which == "old" else ("new", sims["full"], 2, 0, ci & 1)
        bad += run_stream(rs, s, cuts, engine)[0]
    print(calls)
    assert not bad, bad[:10]
    assert calls["old"] > 200 and calls["new"] > 200


def test_inorder_is_liblz4_and_the_existing_walk_on_the_exact_layouts(sims, old_sims, rs):
    """layouts a .. f and the hostile set with the knob at 1 -- every block through the in-order tier: results, states and bytes are the
    reference's, and the windows are byte for byte the existing walk's"""
    rng = rng_for(SEED_STREAMS + 2)
    streams = [s for s in layout_set(rs, rng, 6) if s.layout != "g"] + hostile_set(rs, rng, 4)
    bad = []
    for t, s in enumerate(streams):
        cuts = list(range(1, len(s.blocks) + 1)) if s.before else random_cuts(len(s.blocks), 3, rng)
        b, new = run_stream(rs, s, cuts, lambda ci, *_: ("new", sims[FORMS[t & 3][0]], FORMS[t & 3][1], 1, t & 1))
        bad += b
        b, old = run_stream(rs, s, cuts, lambda ci, *_: ("old", old_sims["full"], 2, t & 1))
        bad += b
        if s.exact and new.window.raw != old.window.raw and not any(r < 0 and r != CHAIN_STOPPED for r in new.w.out):   # (a failed slot's bytes are nobody's)
            bad.append((s.name, "differs from the existing walk"))
        if new.n_inorder == 0 and any(r != CHAIN_STOPPED and b_.src_len >= 0 and b_.cap >= 0 for r, b_ in zip(new.w.out, s.blocks)):
            bad.append((s.name, "no block took the in-order tier"))
    print("%d streams, %d mismatches" % (len(streams), len(bad)))
    assert not bad, bad[:10]
    assert len(streams) >= 60


def test_inorder_hostile_overlap_streams(sims, rs):
    """a flipped byte, a capacity one short, a negative length in streams of the overlap layouts: results, states, guards -- and the bytes
    up to the first failure"""
    rng = rng_for(SEED_STREAMS + 3)
    streams = hostile_overlap_set(rs, rng, 2)
    bad, failed = [], 0
    for t, s in enumerate(streams):
        for cuts in (random_cuts(len(s.blocks), 4, rng), [len(s.blocks)]):
            lib, form = FORMS[t & 3]
            b, run = run_stream(rs, s, cuts, lambda *_: ("new", sims[lib], form, t & 1, (t >> 1) & 1))
            bad += b
            failed += any(r < 0 and r != CHAIN_STOPPED for r in run.w.out)
    print("%d streams, %d runs met a negative result" % (len(streams), failed))
    assert not bad, bad[:10]
    assert failed >= len(streams) // 2


# ---- the grid ----
@pytest.fixture(scope="module")
def grid_cases(rs):
    cases = grid(rng_for(SEED_GRID))
    return [(c, grid_expected(c), rs.decode(c.stream, [2])) for c in cases]


@pytest.fixture(scope="module")
def behind_cases(rs):
    """the match source 1 .. 100 bytes BEHIND its destination inside the overlapped dictionary, the match longer than that"""
    cases = behind_grid(rng_for(SEED_GRID + 1))
    return [(c, grid_expected(c), rs.decode(c.stream, [2])) for c in cases]


def grid_failures(run_case, grid_cases):
    """-> the cases whose window (all of it, the FILL around the blocks included) is not the plain definition's, or whose results are not"""
    failed = []
    for c, (want, rr), w in grid_cases:
        assert w.out == rr
        bad, run = run_case(c, w)
        if bad or run.window.raw[:GRID_WIN] != want:
            failed.append(c)
    return failed


def sim_grid_case(engine):
    def run_case(c, w):
        run = Run(c.stream, w)
        run.compare = False          # (the expected bytes are the plain definition's: compared by the caller)
        return run.call(2, engine), run
    return run_case


def test_inorder_grid_is_the_plain_definition(sims, grid_cases, behind_cases):
    """every grid case -- all three tails, the source 1 .. 200 bytes ahead -- and every case with the source 1 .. 100 bytes BEHIND its
    destination (the pattern copy below the chunk of 8, the copy in pieces behind waits from 8 on), in the kernel's form and on the exact
    tiers, the knob at 0 and at 1: the window is the plain definition's, byte for byte; every block decoded in order waited at least once"""
    for lib, form in (("full", 2), ("exact", 0)):
        for every in (0, 1):
            waits = []

            def run_case(c, w):
                bad, run = sim_grid_case(("new", sims[lib], form, every, every))(c, w)
                waits.append((run.n_orders, run.n_inorder))
                return bad, run
            failed = grid_failures(run_case, grid_cases + behind_cases)
            assert not failed, (lib, form, every, len(failed), failed[0].stream.name)
            assert all(o >= 1 for o, i in waits if i) and sum(1 for o, i in waits if i) >= (len(waits) if every else 8000)   # (knob 0: a few slots end in front of block 0)
    assert len(grid_cases) == 19 * 11 * 13 * 3
    ks = {-c.ahead for c, _, _ in behind_cases}
    assert len(behind_cases) >= 120 and min(ks) == 1 and {7, 8, 9} <= ks and max(ks) >= 64


def test_existing_walk_on_the_grid(old_sims, grid_cases, rs):
    """THE HAZARD: the existing walk (the exact tiers alone, the plain, pipelined and deep forms) on the grid.  Its wild literal copies
    leave the plain definition where the source lies 1 or 2 bytes ahead; how far ahead the source must lie before they stop doing so is
    printed per form.  Every form fails the grid; no form fails a case from 7 bytes ahead on (DESIGN.md 2.2 has the figures)."""
    report = {}
    for name, lib, form in (("exact", "exact", 0), ("plain", "full", 0), ("pipelined", "full", 1), ("deep", "full", 2)):
        failed = grid_failures(sim_grid_case(("old", old_sims[lib], form, 0)), grid_cases)
        by = {}
        for c in failed:
            by[c.ahead] = by.get(c.ahead, 0) + 1
        report[name] = (len(failed), sum(v for a, v in by.items() if a >= 31), max(by) if by else 0)
        print("existing walk, %-9s: %4d of %d grid cases differ from the plain definition; %d of them with the source 31 bytes or more ahead; "
              "farthest: %d ahead" % (name, len(failed), len(grid_cases), report[name][1], report[name][2]))
    assert all(n > 0 for n, _, _ in report.values()), report
    # (for the record, not asserted: on the encoder-written overlap streams the existing forms' over-stores stay inside liblz4's own
    # 14-byte margin -- the windows are the reference's; it is the near sources of the grid that show what "unspecified" means)
    streams = overlap_set(rs, rng_for(SEED_STREAMS), 2)
    differ = sum(1 for s in streams if run_stream(rs, s, [len(s.blocks)], lambda *_: ("old", old_sims["full"], 2, 0))[0])
    print("existing walk, deep: %d of %d encoder-written overlap streams differ from the reference" % (differ, len(streams)))


@pytest.mark.parametrize("mutant", ["lits-rounded-up", "early-load"])
def test_wrong_builds_fail_the_grid(sims, grid_cases, behind_cases, mutant):
    """two deliberate faults fail the grid: a backend whose literal copy rounds its last store up to the chunk, and the CORE built
    without its wait (-DLZ4HIP_INORDER_NO_SYNC=1), which loads a match source before the stores in front of it have landed"""
    failed = grid_failures(sim_grid_case(("new", sims[mutant], 2, 1, 0)), grid_cases + behind_cases)
    print("%s: %d of %d grid cases fail" % (mutant, len(failed), len(grid_cases) + len(behind_cases)))
    assert len(failed) > 0
