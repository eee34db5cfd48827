"""The C ABI's multi-device host path on ONE GPU (-m gpu): lz4hip_init accepts a device list with repeats, so [0, 0] / [0, 0, 0]
drive csrc/api.cpp's D > 1 branch -- contiguous block ranges per listed device, one thread + staging set each (SURVEY.md 8(e);
block independence: /root/reference/src/java/net/jpountz/lz4/LZ4FrameOutputStream.java:361-363) -- which no 1-GPU run reaches
otherwise.  Each case runs in its own process (lz4hip_init is once per process)."""
import pytest

from support import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [2, 3])
def test_host_batch_over_repeated_device_list(D):
    assert ("multidev ok D=%d" % D) in run_child("multidev_child.py", str(D), timeout=900)
