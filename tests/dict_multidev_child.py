"""Child process of tests/test_gpu_dict.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the dictionary
decoder's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device, the handle resident on
each) on a box with one GPU, and checks a batch of records -- valid, damaged and cut, with ragged capacities -- against the reference
library's LZ4_decompress_safe_usingDict: return values, bytes and the untouched bytes behind every result.  A handle created BEFORE
lz4hip_init is used too (its device copy is made on first use).  Prints 'dict multidev ok D=<D>'."""
import random
import sys

import numpy as np
from support import check_slots, init_repeated, package, slots   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from dict_common import RefDict, book1
from partial_common import damaged

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd, L = package()
b = book1()
rd = RefDict(O.ref())
for dict_len, early in ((4096, False), (70000, True)):
    d = b[:dict_len]
    if early:
        L.lz4hip_shutdown()
        handle = amd.LZ4Dictionary(d)          # no device is initialised yet on this pass
    init_repeated(D)
    if not early:
        handle = amd.LZ4Dictionary(d)
    assert len(handle) == dict_len
    rng = random.Random(90 + D + dict_len)
    srcs, caps = [], []
    for i in range(n):
        size = rng.choice([64, 300, 1000, 4096, 20000])
        o = rng.randrange(200000, len(b) - size)
        s = rd.compress(d, b[o:o + size], 9 if i % 3 == 0 else 0)
        k = rng.random()
        if k < 0.15:
            s = s[:rng.randrange(len(s) + 1)]
        elif k < 0.3:
            s = damaged(s, rng, 2)
        srcs.append(s)
        caps.append(rng.choice([size, size + 100, max(size - 7, 0), size + 1]))
    want = [rd.decode(s, c, d) for s, c in zip(srcs, caps)]
    so, do, dst = slots(srcs, caps)
    out = amd.LZ4HIPBatch.decompressSafeDict(b"".join(srcs) + b"\0", so, np.array([len(s) for s in srcs], dtype=np.int32), dst, do,
                                             np.array(caps, dtype=np.int32), handle)
    check_slots(out, dst, do, caps, want, srcs, tag=(dict_len,))
    handle.close()
print("dict multidev ok D=%d blocks=%d" % (D, n))
