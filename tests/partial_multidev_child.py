"""Child process of tests/test_gpu_partial.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the partial
decoder's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device) on a box with one GPU,
and checks a ragged batch -- return values, bytes and the untouched bytes behind every result -- against the reference library's
LZ4_decompress_safe_partial.  Prints 'partial multidev ok D=<D>'."""
import random
import sys

import numpy as np
from support import check_slots, init_repeated, slots   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from partial_common import ref_partial

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd, L = init_repeated(D)
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
so, do, dst = slots(srcs, caps)
out = amd.LZ4HIPBatch.decompressSafePartial(b"".join(srcs), so, np.array([len(s) for s in srcs], dtype=np.int32), dst, do,
                                            np.array(targets, dtype=np.int32), np.array(caps, dtype=np.int32))
check_slots(out, dst, do, caps, want, srcs, extra=lambda i: (targets[i],))
print("partial multidev ok D=%d blocks=%d" % (D, n))
