"""Child process of tests/test_gpu_accel.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the accelerated
host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device) on a box with one GPU, and
checks a ragged batch -- sizes and bytes of every block, one-byte-short capacities included -- against the reference library's
LZ4_compress_fast.  Prints 'accel multidev ok D=<D>'."""
import ctypes as C
import random
import sys

import numpy as np
from support import init_repeated, offsets   # (first: it puts the repository root on sys.path)
from oracle import oracle as O

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd, L = init_repeated(D)
f = C.CDLL(O.ref().path).LZ4_compress_fast
f.restype = C.c_int
f.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]


def ref_fast(v, cap, a):
    out = (C.c_uint8 * max(cap, 1))()
    r = f(v, out, len(v), cap, a)
    return r, bytes(out[:max(r, 0)])


rng = random.Random(60 + D)
base = [O.gen_block(65536, 200 + s) for s in range(16)] + [rng.randbytes(65536), bytes(65536), O.gen_block(300000, 7, win=4096)]
srcs = []
for i in range(n):
    v = base[i % len(base)]
    srcs.append(v[:rng.choice([len(v), len(v), rng.randrange(0, len(v) + 1), rng.randrange(13, 2000)])])
for a in (2, 8):
    want = [ref_fast(v, len(v) + len(v) // 255 + 16, a) for v in srcs]
    caps = [len(v) + len(v) // 255 + 16 if i % 7 else max(0, want[i][0] - 1) for i, v in enumerate(srcs)]
    so = offsets([len(v) for v in srcs])
    do = offsets(caps)
    dst = bytearray(int(sum(caps)) + 1)
    out = amd.LZ4HIPBatch.compress(b"".join(srcs), so, np.array([len(v) for v in srcs], dtype=np.int32), dst, do, np.array(caps, dtype=np.int32),
                                   acceleration=a)
    for i in range(n):
        exp = want[i][0] if caps[i] >= want[i][0] else 0
        assert out[i] == exp, ("size", a, i, len(srcs[i]), caps[i], int(out[i]), exp)
        if exp > 0:
            assert bytes(dst[int(do[i]):int(do[i]) + exp]) == want[i][1], ("bytes", a, i)
print("accel multidev ok D=%d blocks=%d" % (D, n))
