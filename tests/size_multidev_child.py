"""Child process of tests/test_gpu_size.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the decoded-size
query's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device) on a box with one GPU,
and checks a ragged batch -- valid, cut and damaged streams at capacities around their sizes -- against the return value of the
reference library's LZ4_decompress_safe.  Prints 'size multidev ok D=<D>'."""
import random
import sys

import numpy as np
from support import init_repeated, offsets   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from size_common import ref_size

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd, L = init_repeated(D)
ref = O.ref()
want = ref_size(ref)

rng = random.Random(90 + D)
base = [O.gen_block(65536, 500 + s) for s in range(12)] + [bytes(65536), O.gen_block(300000, 9, win=4096)]
streams = [ref.compress_fast(v) for v in base] + [ref.compress_hc(base[0], 12)]
sizes = [len(v) for v in base] + [len(base[0])]
srcs, caps = [], []
for i in range(n):
    k = i % len(streams)
    s = streams[k]
    u = rng.random()
    if u < 0.2:
        s = s[:rng.randrange(len(s) + 1)]
    elif u < 0.4:
        b = bytearray(s); b[rng.randrange(len(b))] ^= 1 << rng.randrange(8); s = bytes(b)
    srcs.append(s)
    caps.append(rng.choice([0, 63, 64, 65, sizes[k] - 1, sizes[k], sizes[k] + 1, sizes[k] + 64, sizes[k] + 606, sizes[k] + 607, 2 * sizes[k]]))
w = [want(s, c) for s, c in zip(srcs, caps)]
so = offsets([len(s) for s in srcs])
out = amd.LZ4HIPBatch.decompressedLengths(b"".join(srcs) + b"\0", so, np.array([len(s) for s in srcs], dtype=np.int32), np.array(caps, dtype=np.int32))
for i in range(n):
    assert int(out[i]) == w[i], ("result", i, len(srcs[i]), caps[i], int(out[i]), w[i])
assert sum(1 for v in w if v >= 0) > n // 4 and sum(1 for v in w if v < 0) > n // 4
print("size multidev ok D=%d blocks=%d" % (D, n))
