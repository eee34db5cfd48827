"""Child process of tests/test_gpu_hcdict.py: initialises liblz4hip on the devices given on the command line, so that the dictionary HC
compressor's host batch takes the multi-device branch of csrc/api.cpp (contiguous block ranges per device, the handle's tail and HC
image on each), and checks a batch of records with ragged capacities at two levels against the reference library's LZ4_loadDictHC +
LZ4_compress_HC_continue: return values, bytes and the untouched bytes behind every result.  A handle created BEFORE lz4hip_init is
used too (its device copies are made on first use).  Prints 'hcdict multidev ok D=<D>'."""
import random
import sys

import numpy as np
from support import check_slots, init_devices, package, slots   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from hcdict_common import Ref, book1, bound

devs = [int(a) for a in sys.argv[1:]]
D = len(devs)
n = 64 * D * 2 + 11
amd, L = package()
b = book1()
R = Ref(O.ref())
for dict_len, early, level in ((4096, False, 9), (70000, True, 4), (3, False, 10)):
    d = b[:dict_len]
    if early:
        L.lz4hip_shutdown()
        handle = amd.LZ4Dictionary(d)          # no device is initialised yet on this pass
    init_devices(devs)
    if not early:
        handle = amd.LZ4Dictionary(d)
    assert len(handle) == dict_len
    rng = random.Random(90 + D + dict_len)
    recs, caps, want = [], [], []
    for i in range(n):
        size = rng.choice([0, 12, 64, 300, 1000, 4096, 20000])
        o = rng.randrange(200000, len(b) - size)
        rec = b[o:o + size]
        full = R.compress(d, rec, level)
        cap = rng.choice([bound(size), full[0], full[0] - 1, full[0] + 1])
        recs.append(rec); caps.append(cap)
        want.append(full if cap >= full[0] else R.compress(d, rec, level, cap))
    so, do, dst = slots(recs, caps)
    out = amd.LZ4HIPBatch.compressHCDict(b"".join(recs) + b"\0", so, np.array([len(s) for s in recs], dtype=np.int32), dst, do,
                                         np.array(caps, dtype=np.int32), handle, level)
    check_slots(out, dst, do, caps, want, recs, tag=(dict_len,))
    handle.close()
print("hcdict multidev ok D=%d blocks=%d" % (D, n))
