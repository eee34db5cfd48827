"""Child process of tests/test_gpu_hc_destsize.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the HC destSize
host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device, consumed sizes brought back per
range) on a box with one GPU, and checks a ragged batch -- sizes, consumed sizes and bytes of every block -- against the reference
library's LZ4_compress_HC_destSize at the level given as the second argument.  Prints 'hc destsize multidev ok D=<D>'."""
import ctypes as C
import random
import sys

import numpy as np
from support import init_repeated, offsets   # (first: it puts the repository root on sys.path)
from oracle import oracle as O

D = int(sys.argv[1])
LEVEL = int(sys.argv[2])
n = 32 * D + 11
amd, L = init_repeated(D)
_ref = C.CDLL(O.ref().path)
f = _ref.LZ4_compress_HC_destSize
f.restype = C.c_int
f.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.c_int, C.c_int]
_ref.LZ4_sizeofStateHC.restype = C.c_int
STATE = C.create_string_buffer(_ref.LZ4_sizeofStateHC() + 64)


def ref_dest(v, t):
    out = (C.c_uint8 * max(t, 1))()
    sz = C.c_int(len(v))
    r = f((C.addressof(STATE) + 15) & ~15, v, out, C.byref(sz), t, LEVEL)
    return r, sz.value, bytes(out[:max(r, 0)])


rng = random.Random(70 + D)
base = [O.gen_block(65536, 300 + s) for s in range(16)] + [rng.randbytes(65536), bytes(65536), O.gen_block(150000, 8, win=4096)]
srcs, targets = [], []
for i in range(n):
    v = base[i % len(base)]
    v = v[:rng.choice([len(v), len(v), rng.randrange(0, len(v) + 1), rng.randrange(13, 2000)])]
    srcs.append(v)
    targets.append(rng.choice([4096, 16384, 1, 17, len(v) // 3 + 1, len(v) + len(v) // 255 + 16]))
want = [ref_dest(v, t) for v, t in zip(srcs, targets)]
so = offsets([len(v) for v in srcs])
do = offsets(targets)
dst = bytearray(int(sum(targets)) + 1)
out, cons = amd.LZ4HIPBatch.compressHCDestSize(b"".join(srcs), so, np.array([len(v) for v in srcs], dtype=np.int32), dst, do,
                                               np.array(targets, dtype=np.int32), LEVEL)
for i in range(n):
    assert (int(out[i]), int(cons[i])) == want[i][:2], ("size", i, len(srcs[i]), targets[i], int(out[i]), int(cons[i]), want[i][:2])
    assert bytes(dst[int(do[i]):int(do[i]) + int(out[i])]) == want[i][2], ("bytes", i)
print("hc destsize multidev ok D=%d blocks=%d" % (D, n))
