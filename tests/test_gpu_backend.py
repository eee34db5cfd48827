"""The device backends' primitives beside the lane simulator's, on the GPU: the probes of tests/backend/probes.h compiled once
against csrc's WaveDev / GroupDev<GL> / BlockWaveDev<KW, KS> (tests/backend/libdevprobe.so) and once against
tests/hostsim's WaveHost / GroupHost (hostsim_backend.cpp), on the same cases (tests/backend_cases.py), compared byte for byte.

Per test: build the cases, run the host instantiation, assert that no case is oob (a wrong precondition must not reach the GPU),
run the device library, assert that the HIP code is 0, compare the COMPLETE output images -- every slot has at least 64 guard
bytes of 0xA5 on each side in both images, so the comparison also shows that neither backend wrote outside its slot.  Nothing is
excluded but what is documented as unspecified: lane 63 of shfl_down1, and lds_max's returned old values (the hardware's order
among colliding lanes), which are checked against the definition of an atomic max instead.  tests/test_backend_hostsim.py holds
the third leg (the host images against plain definitions) and shows that the comparison sees a deliberately wrong backend."""
import functools
import time

import pytest

import backend_cases as bc
from support import build_devprobe, build_sim

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def libs():
    return build_sim("hostsim_backend"), build_devprobe()


def both(L):
    """-> the device's image, after the byte-for-byte comparison with the host's"""
    host, dev = libs()
    t0 = time.time()
    want, oob = bc.run_host(host, L)
    bc.assert_no_oob(L, oob)
    t1 = time.time()
    code, got = bc.run_dev(dev, L)
    t2 = time.time()
    print("family %s%s: %d cases, %d MB of images, host %.2f s, device %.2f s" %
          (L.family, "" if L.param is None else " %s" % (L.param,), L.n, (L.inp.nbytes + L.out.nbytes) >> 20, t1 - t0, t2 - t1))
    assert code == 0, "HIP error %d from the device probes of %s" % (code, L.describe(0))
    bc.assert_same(L, got, want, bc.unspecified(L))
    return got


def test_constants():
    """the device library was built with the layout and the staging size that the case tables (and their flush model) assume"""
    bc.assert_constants(libs()[1], "devprobe_constants")


def test_wave_values():
    both(bc.wave_value_cases())


def test_wave_memory():
    both(bc.wave_mem_cases())


def test_wave_lds_table():
    L = bc.wave_lds_cases()
    bc.check_lds_max_old(L, both(L), "device")


@pytest.mark.parametrize("gl", bc.GLS)
def test_group_copies(gl):
    both(bc.group_copy_cases(gl))


@pytest.mark.parametrize("gl", bc.GLS)
def test_group_staging(gl):
    both(bc.group_stage_cases(gl))


@pytest.mark.parametrize("cfg", bc.WAVE_CFG, ids=lambda c: "%dx%d" % c)
def test_block_wave_lane_primitives(cfg):
    both(bc.bwave_lane_cases(cfg))


@pytest.mark.parametrize("cfg", bc.WAVE_CFG, ids=lambda c: "%dx%d" % c)
def test_block_wave_rings(cfg):
    both(bc.bwave_ring_cases(cfg))
