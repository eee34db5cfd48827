"""The decoders' end-of-block margins in the lane simulator: the boundary streams of tests/margin_common.py -- a near-maximal simple
sequence placed at the byte at which an interior loop decides to stay or leave (ip <= iend - 306, op <= oend - 606:
LZ4HIP_DECODE_IN_MARGIN / LZ4HIP_DECODE_OUT_MARGIN of lz4-java_amd/csrc/lz4_decode_core.h) -- through every loop form the simulator
has, against the reference library's return codes and bytes.  The simulator fails a decode on any access outside the block's slots.

The two sensitivity tests build the simulator with one margin weakened to one byte less than a simple sequence produces (541) or
consumes (273) and expect the same cases to FAIL; profiles/decode_margin_audit.txt has, loop by loop, the largest weakened value
they still catch (tools/margin_probe.py)."""
import os
import subprocess
import sys

import pytest

import margin_common as M
from conftest import ROOT
from test_hostsim import load_sim, sim_decode, wave_flag

# every loop form of sim_decompress: the flag lists of test_hostsim.py and test_fast_contract_hostsim.py
LOOPS = {"plain 4": 4, "plain 8": 8, "plain 16": 16, "plain 64": 64, "pipelined 8": 8 | 0x100, "pipelined 64": 64 | 0x100,
         "staged 4": 4 | 0x200, "staged 8": 8 | 0x200, "staged 16": 16 | 0x200, "staged 64": 64 | 0x200,
         "deep 4": 4 | 0x400, "deep 8": 8 | 0x400, "deep 16": 16 | 0x400}
LOOPS.update({"ring (%d, %d)" % (gl, 1 << rl): gl | 0x800 | (rl << 12) for gl, rl in ((1, 8), (1, 9), (4, 9), (4, 10), (4, 11), (8, 9), (8, 12), (16, 12))})
for _log in (12, 13, 14, 15, 16):
    LOOPS.update({"wave %d" % _log: wave_flag(_log), "par %d" % _log: wave_flag(_log, par=True), "pair %d" % _log: wave_flag(_log, par="pair"),
                  "trio %d" % _log: wave_flag(_log, par="trio")})
LOOPS.update({"wave 13 1K": wave_flag(13, True), "par 13 1K": wave_flag(13, True, par=True)})
# one form of every family: these run every case; in the others every third case of mode a (exact capacity: 3009 cases in which no end
# arrives early -- the modes that tell a margin's value, b, h and i, run whole in every form), which keeps the file under ten minutes
FAMILIES = ("plain 4", "plain 64", "pipelined 8", "staged 8", "deep 8", "ring (4, 2048)", "wave 13", "par 13", "pair 14", "trio 13")
SHIFTS = (0, 1, 3, 64, 127)
SWEEP_SHIFTS = tuple(9 * k % 64 for k in range(16))   # every address residue (mod 16) of a slot's end: the staged loop's last flush runs to the next lane boundary of the ADDRESS


@pytest.fixture(scope="module")
def cs(ref, O):
    return M.CaseSet(ref, O)


@pytest.fixture(scope="module")
def sim():
    return load_sim()


SIM_MODES = "abcdhi"


def run_loop(sim, cs, flag, modes=SIM_MODES, stride=1, salt=0, stride_a=1):
    """the cases of modes a .. d, h and i through one loop form -> the mismatches [(mode, tag, got, want)] (-1000000: an access outside the slots)"""
    bad = []
    for k, (c, w) in enumerate(zip(cs.cases, cs.want)):
        if c.mode not in modes or c.mode not in SIM_MODES or (k + salt) % stride or (c.mode == "a" and (k + salt) % stride_a):
            continue
        src, safe = M.source(c)
        # (the sweep of mode b at sixteen alignments: a loop that stores whole ADDRESS-ALIGNED steps overruns by what the address makes of it)
        for shift in (SWEEP_SHIFTS if c.tag[0] == "sweep" else (SHIFTS[(k + salt) % len(SHIFTS)],)):
            r, d = sim_decode(sim, src, c.cap, int(safe), flag, shift=shift)
            ok = r == w[0] and (r < 0 or d[:r if safe else c.cap] == w[1])
            if not ok:
                bad.append((c.mode, c.tag, r, w[0]))
                break
    return bad


def test_margin_case_set(cs):
    """no grid point dropped: the counts of every mode, and how many placements no valid stream has (they sit as near as one has)"""
    print(cs.counts, "clamped", cs.clamped)
    assert len(M.grid()) == M.GRID_POINTS == 2529
    assert cs.counts == {"a": 3009, "b": 2209, "c": 1689, "d": 1689, "e": 1263, "f": 480, "g": 480, "h": 350, "i": 350} and cs.clamped == 270
    a = {c.tag[0] for c in cs.by_mode["a"]}
    assert sum(c.tag[0] == "sweep" for c in cs.by_mode["b"]) == 2 * 2 * 65 * 2
    assert a == set(range(M.GRID_POINTS))                     # every grid point has its exact-capacity stream(s)
    for m, n in (("b", 9), ("c", 3), ("d", 3)):               # every cut / surplus / src_cap surplus is in use
        assert len({c.tag[2] if m != "d" else c.aux - len(c.s.data) for c in cs.by_mode[m] if c.tag[0] != "sweep"}) == n, m
    for c in cs.cases:                                         # the probe is where the case says, and every loop is running in front of it
        assert c.s.p_ip > 2048 and c.s.p_op > 4096 and len(c.s.data) - c.s.p_ip == c.s.in_tail and c.s.n - c.s.p_op == c.s.out_tail
    far = [c for c in cs.by_mode["b"] if c.tag[2] == M.FAR_SHORT]
    assert len(far) > 100 and all(c.s.in_tail >= 2048 + M.IN_MARGIN for c in far)   # (the deep loop wants 2 KB of stream ahead)


@pytest.mark.parametrize("loop", list(LOOPS))
def test_margin_streams_in_every_loop(cs, sim, loop):
    """modes a (exact capacity), b (capacity short: the reference's negative code), c (capacity long), d (the fast decoder against the
    oracle's bounded one), h and i (the stream cut behind the probe, safe and fast): every case, the destination slot at five alignments
    in rotation (mode a: every third case in the forms outside FAMILIES)"""
    bad = run_loop(sim, cs, LOOPS[loop], salt=len(loop), stride_a=1 if loop in FAMILIES else 3)
    assert not bad, (loop, len(bad), bad[:6])


def test_margin_partial(cs, ref):
    """mode e: the target at the probe's start + d, through the forms the partial kernels run"""
    import test_partial_hostsim as P
    psim = P.load_sim()
    n = 0
    for c, w in zip(cs.cases, cs.want):
        if c.mode != "e":
            continue
        for form, gl in P.FORMS:
            got = P.sim_partial(psim, c.s.data, c.aux, c.cap, form, gl)
            assert got[0] == w[0] and P.same_bytes(got[1], w[1], c.s.data, w[0], min(c.aux, c.cap)), (c.tag, form, gl, got[0], w[0])
            n += 1
    assert n == 1263 * len(P.FORMS)


def test_margin_dictionary(cs):
    """mode f: the block behind a dictionary of 400 or 70000 bytes, the probe's match wholly inside it or straddling the block's start"""
    import test_dict_hostsim as D
    sims = D.load_sims()
    n = 0
    for c, w in zip(cs.cases, cs.want):
        if c.mode != "f":
            continue
        for lib, form, gl in D.FORMS:
            for layout in (0, 1):
                got = D.sim_dict(sims, c.s.data, c.cap, cs.dicts[c.aux], lib, form, gl, layout)
                assert got == w, (c.tag, c.aux, lib, form, gl, layout, got[0], w[0])
                n += 1
    assert n == 480 * len(D.FORMS) * 2


def test_margin_chain(cs):
    """mode g: the block as the second of a chain, the probe's match starting in the first block"""
    import test_chain_hostsim as K
    sims = K.load_sims()
    n = 0
    for c, w in zip(cs.cases, cs.want):
        if c.mode != "g":
            continue
        bad = K.run(sims, cs.chain(c), w)
        assert not bad, (c.tag, bad[:3])
        n += 1
    assert n == 480


def test_margin_size_query(cs):
    """the decoded-size query on modes a, b, c and h: the reference's return value, no destination touched"""
    import test_size_hostsim as S
    ssim = S.load_sim()
    n = 0
    for c, w in zip(cs.cases, cs.want):
        if c.mode not in "abch":
            continue
        src = M.source(c)[0]
        for fast, ks in S.FORMS:
            got = ssim.sim_decoded_size(src, len(src), c.cap, fast, ks, None)
            assert got == w[0], (c.mode, c.tag, fast, ks, got, w[0])
            n += 1
    assert n == (3009 + 2209 + 1689 + 350) * len(S.FORMS)


def _probe(flags, *args):
    env = dict(os.environ, LZ4HIP_SIM_FLAGS=flags)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "margin_probe.py")] + list(args), timeout=900, env=env).decode()
    res = {}
    for line in out.splitlines():
        if line.startswith("loop "):
            name, _, rest = line[5:].partition(" : ")
            res[name] = int(rest.split()[rest.split().index("bad") + 1])
    return res, out


# one loop of every family (tools/margin_probe.py runs these when asked for "families")
def test_output_margin_541_fails_the_cases():
    """A simulator built with LZ4HIP_DECODE_OUT_MARGIN = 541, one byte less than a simple sequence produces: the loop runs a sequence
    that ends past the capacity (mode b tells).  Every loop family must fail cases (the weakened build exists in the simulator alone)."""
    res, out = _probe("out541:-DLZ4HIP_DECODE_OUT_MARGIN=541", "--modes=b", "families")
    assert len(res) >= 9 and all(b > 0 for b in res.values()), out[-1500:]


def test_input_margin_273_fails_the_cases():
    """A simulator built with LZ4HIP_DECODE_IN_MARGIN = 273, one byte less than a simple sequence consumes: the loop runs a sequence
    whose end the stream does not hold.  Only modes h and i can tell: a valid stream ends six bytes or more behind its last sequence, so
    in modes a .. g no sequence of 274 bytes starts where this build and the unmodified one decide differently."""
    res, out = _probe("in273:-DLZ4HIP_DECODE_IN_MARGIN=273", "--modes=hi", "families")
    assert len(res) >= 9 and all(b > 0 for b in res.values()), out[-1500:]
