"""Child process of tests/test_gpu_partial.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the partial
decoder's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device) on a box with one GPU,
and checks a ragged batch -- return values, bytes and the untouched bytes behind every result -- against the reference library's
LZ4_decompress_safe_partial.  Prints 'partial multidev ok D=<D>'."""
import ctypes as C
import importlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from oracle import oracle as O  # noqa: E402
from partial_common import ref_partial  # noqa: E402

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd = importlib.import_module("lz4-java_amd")
L = amd.lib()
ids = (C.c_int * D)(*([0] * D))
assert L.lz4hip_init(ids, D) == 0, L.lz4hip_last_error()
assert L.lz4hip_device_count() == D
ref = O.ref()
lz4p = ref_partial(ref)

rng = random.Random(80 + D)
base = [O.gen_block(65536, 400 + s) for s in range(12)] + [bytes(65536), O.gen_block(300000, 9, win=4096)]
streams = [ref.compress_fast(v) for v in base] + [ref.compress_hc(base[0], 12)]
sizes = [len(v) for v in base] + [len(base[0])]
srcs, targets, caps = [], [], []
for i in range(n):
    k = i % len(streams)
    s = streams[k]
    if rng.random() < 0.2:
        s = s[:rng.randrange(len(s) + 1)]
    srcs.append(s)
    t = rng.choice([0, 1, 13, 4096, 16384, sizes[k] - 1, sizes[k], 2 * sizes[k], rng.randrange(sizes[k] + 1)])
    targets.append(t)
    caps.append(rng.choice([t, t + 100, max(t - 7, 0), sizes[k]]))
want = [lz4p(s, t, c) for s, t, c in zip(srcs, targets, caps)]
so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])[:-1]]).astype(np.uint64)
do = np.concatenate([[0], np.cumsum([c + 8 for c in caps])[:-1]]).astype(np.uint64)
dst = bytearray(b"\xee" * (int(sum(caps)) + 8 * n))
out = amd.LZ4HIPBatch.decompressSafePartial(b"".join(srcs), so, np.array([len(s) for s in srcs], dtype=np.int32), dst, do,
                                            np.array(targets, dtype=np.int32), np.array(caps, dtype=np.int32))
for i in range(n):
    r, b = want[i]
    assert int(out[i]) == r, ("result", i, len(srcs[i]), targets[i], caps[i], int(out[i]), r)
    o = int(do[i])
    assert bytes(dst[o:o + max(r, 0)]) == b, ("bytes", i)
    assert dst[o + max(r, 0):o + caps[i] + 8] == b"\xee" * (caps[i] + 8 - max(r, 0)), ("written past the result", i)
print("partial multidev ok D=%d blocks=%d" % (D, n))
