"""Child process of tests/test_gpu_dictc.py: initialises liblz4hip on a device LIST WITH REPEATS ([0] * D), so that the dictionary
compressor's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per listed device, the handle's tail and
table image on each) on a box with one GPU, and checks a batch of records with ragged capacities against the reference library's
LZ4_loadDict + LZ4_compress_fast_continue: return values, bytes and the untouched bytes behind every result.  A handle created BEFORE
lz4hip_init is used too (its device copies are made on first use).  Prints 'dictc multidev ok D=<D>'."""
import random
import sys

import numpy as np
from support import check_slots, init_repeated, package, slots   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from dictc_common import RefDict, book1, bound, ref_compress

D = int(sys.argv[1])
n = 64 * D * 3 + 11
amd, L = package()
b = book1()
rd = RefDict(O.ref())
for dict_len, early in ((4096, False), (70000, True), (5, False)):
    d = b[:dict_len]
    if early:
        L.lz4hip_shutdown()
        handle = amd.LZ4Dictionary(d)          # no device is initialised yet on this pass
    init_repeated(D)
    if not early:
        handle = amd.LZ4Dictionary(d)
    assert len(handle) == dict_len
    rng = random.Random(90 + D + dict_len)
    recs, caps, want = [], [], []
    for i in range(n):
        size = rng.choice([0, 12, 64, 300, 1000, 4096, 20000, 70000])
        o = rng.randrange(200000, len(b) - size)
        rec = b[o:o + size]
        full = ref_compress(rd, d, rec)
        cap = rng.choice([bound(size), full[0], full[0] - 1, full[0] + 1])
        recs.append(rec); caps.append(cap)
        want.append(full if cap >= full[0] else ref_compress(rd, d, rec, cap))
    so, do, dst = slots(recs, caps)
    out = amd.LZ4HIPBatch.compressDict(b"".join(recs) + b"\0", so, np.array([len(s) for s in recs], dtype=np.int32), dst, do,
                                       np.array(caps, dtype=np.int32), handle)
    check_slots(out, dst, do, caps, want, recs, tag=(dict_len,))
    handle.close()
print("dictc multidev ok D=%d blocks=%d" % (D, n))
