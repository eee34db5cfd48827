"""The backend layer on the build machine: every probe family of tests/backend/probes.h through its HOST instantiation
(tests/hostsim/hostsim_backend.cpp: the lane simulator's WaveHost / GroupHost).

Two things are checked.  The case tables themselves: NO case may set the backend's oob flag -- every access of every case stays
inside its slot and its LDS layout; tests/test_gpu_backend.py runs the same cases on the device, so this is also what keeps a wrong
precondition from reaching the GPU.  And the host results against plain definitions written in numpy / Python
(tests/backend_cases.py expect_*): byte-forward LZ4 match copy, memcpy, a serial prefix sum, the walk's definition, a byte-wise
ring model -- a third leg beside the two backends.  Bytes that a wild copy may touch past its length are compared between the
two backends only.

That the comparison SEES a difference: one deliberately wrong variant of the host file per family (-DBACKEND_WRONG_SCAN,
-DBACKEND_WRONG_REPLICATE, -DBACKEND_WRONG_MIRROR) must fail it."""
import functools

import numpy as np
import pytest

import backend_cases as bc
from support import build_sim


@functools.lru_cache(maxsize=None)
def sim(wrong=""):
    return build_sim("hostsim_backend", variant="_" + wrong.lower() if wrong else "", flags=("-DBACKEND_WRONG_" + wrong,) if wrong else ())


def check(L, expect, lib=None):
    """the host instantiation on the launch L: no oob, every defined byte as the definition says, the guards intact"""
    out, oob = bc.run_host(lib or sim(), L)
    bc.assert_no_oob(L, oob)
    want, mask = expect(L)
    bc.assert_same(L, out, want, mask, "the host backend departs from the definition")
    return out


def test_the_case_tables_use_the_backends_own_constants():
    bc.assert_constants(sim(), "hb_constants")


def test_wave_values_against_their_definitions():
    """ballot / lanes, mbcnt, lanemask_lt, excl_scan (a serial prefix sum), shfl*, bcast*, set_lane, writelane, alignbyte, clz64, ctz64v,
    div255, shr, vmin, vmax, select: 2000 random vectors and the all-zero, all-ones, lane-index and one-hot vectors"""
    L = bc.wave_value_cases()
    assert L.n > 14000
    check(L, bc.expect_wave_value)


def test_wave_memory_against_memcpy():
    """ld8/32/64, ldu*, sld32, st8/16/32 with masks at every alignment mod 8, st_lanes / ld_lanes, st_hdr / ld_hdr, and copy for every
    length 0 .. 1100 at source and destination alignments 0, 1, 3, 15"""
    L = bc.wave_mem_cases()
    lens = {int(r[4]) for r in L.rec if r[0] == bc.W_COPY}
    assert lens == set(range(1101))
    check(L, bc.expect_wave_mem)


def test_wave_lds_table_and_the_atomic_max():
    """lds_fill / lds_wr / lds_rd / lds_rdu / lds_max for both entry widths: the table images against the definition, lds_max's
    returned old values against the definition of an atomic max under ANY order of the colliding lanes"""
    L = bc.wave_lds_cases()
    seen = bc.lds_max_collisions(L)     # active lanes on one slot: none colliding, exactly 2, exactly 3, all 64 -- in both entry widths
    assert all({1, 2, 3, 64} <= seen[u16] for u16 in (True, False)), seen
    out = check(L, bc.expect_wave_lds)
    bc.check_lds_max_old(L, out, "host")


@pytest.mark.parametrize("gl", bc.GLS)
def test_group_copies_against_byte_forward_copy(gl):
    """copy_match (wild and not), copy_match_wide, copy_lits (wild and not), copy_lits_wide, seq_load + seq_store"""
    L = bc.group_copy_cases(gl)
    check(L, bc.expect_group_copy)


@pytest.mark.parametrize("gl", bc.GLS)
def test_group_staging_scripts(gl):
    """st_begin / st_lits / st_match / st_flush_lines / st_flush_all: scripts of up to 12 operations -- the destination below fl is
    the script's logical output, fl follows the flush rule"""
    L = bc.group_stage_cases(gl)
    assert int(L.rec[:, 1].max()) <= 12 and L.n >= 200
    check(L, bc.expect_group_stage)


@pytest.mark.parametrize("cfg", bc.WAVE_CFG, ids=lambda c: "%dx%d" % c)
def test_block_wave_lane_primitives(cfg):
    """vwalk and vwalk_par beside the walk's definition (the interpreter test's 3000 tables, tables with 60 .. 64 and 84 starts, the
    single start), vexcl_scan, vshfl, valignbyte, vmin, vreadlane, vwritelane, vlanes, vballot"""
    L = bc.bwave_lane_cases(cfg)
    starts = {len(bc.walk_definition(list(L.inp[i, :256]))) for i in np.flatnonzero(L.rec[:, 0] == bc.B_WALK)}
    assert {1, 60, 61, 62, 63, 64} <= starts
    check(L, bc.expect_bwave_lane)


@pytest.mark.parametrize("cfg", bc.WAVE_CFG, ids=lambda c: "%dx%d" % c)
def test_block_wave_rings_against_a_byte_wise_model(cfg):
    """vs_win / vs_ld32 across the stream ring's end, wv_get_* + wv_put at the output ring's ends, vcopy_run<PRED> in its three tiers
    and its step-by-step form (vcopy, vput), observed through wv_read_al + wv_store"""
    L = bc.bwave_ring_cases(cfg)
    run = L.rec[:, 0] == bc.B_RUN
    assert run.sum() == 2 * 3 * 300 + 2 * 44
    out = check(L, bc.expect_bwave_ring)
    # the rounds' forms were all there: the usual round in every tier, the step-by-step form, far lanes: none, one, all
    odd = np.array([bool((int(out[i, 256 + 1024:256 + 1028].view(np.uint32)[0]) | int(out[i, 256 + 1028:256 + 1032].view(np.uint32)[0]) << 32)
                         & (int(L.rec[i, 2]) | int(L.rec[i, 3]) << 32)) for i in np.flatnonzero(run)])
    assert 0.2 < odd.mean() < 0.5, odd.mean()


WRONG = [("SCAN", bc.wave_value_cases, bc.expect_wave_value, None),
         ("REPLICATE", bc.group_copy_cases, bc.expect_group_copy, 16),
         ("MIRROR", bc.bwave_ring_cases, bc.expect_bwave_ring, bc.WAVE_CFG[0])]


@pytest.mark.parametrize("wrong,cases,expect,param", WRONG, ids=[w[0].lower() for w in WRONG])
def test_a_wrong_backend_fails_the_comparison(wrong, cases, expect, param):
    """one deliberately wrong variant per family: the definition check fails on it, and so does the byte-for-byte comparison with the
    right backend's image (the comparison the GPU test makes)"""
    L = cases() if param is None else cases(param)
    good, _ = bc.run_host(sim(), L)
    bad, _ = bc.run_host(sim(wrong), L)
    with pytest.raises(AssertionError, match="departs from the definition"):
        want, mask = expect(L)
        bc.assert_same(L, bad, want, mask, "the host backend departs from the definition")
    with pytest.raises(AssertionError, match="the two backends differ"):
        bc.assert_same(L, bad, good, bc.unspecified(L))
