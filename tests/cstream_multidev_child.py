"""Child of tests/test_gpu_cstream.py: a set of resident compress streams divided over several engine devices.  argv[1] = D > 0: device 0
listed D times (the multi-device branch on one GPU: the set has D parts and a call is sharded at their boundaries); 0: devices 0 and
1.  40 streams, so that the parts' boundaries fall inside the calls; every stream against the reference's ONE LZ4_stream_t."""
import random
import sys

import support
from cstream_common import DevEngine, RefCChain, drive, random_life

D = int(sys.argv[1])
amd, L = support.init_repeated(D) if D else support.init_devices([0, 1])
from oracle import oracle as O   # noqa: E402  (support put the repository root on the path)

rc = RefCChain(O.ref())
rng = random.Random(81)
lives = [random_life(rng, O, "stream %d" % i, rng.randrange(2, 10), 2500, every_boundary=True) for i in range(40)]
eng = DevEngine(amd, 40)
bad, results, rounds = drive(eng, rc, lives, rng, absent=0.4)
assert not bad, (len(bad), bad[:5])
cons, stop = eng.consumed()
assert cons == [sum(len(c.data) for c in lf.calls) for lf in lives] and not any(stop)
eng.reset([0, 1, 2, 20, 39])
cons, stop = eng.consumed()
assert all(cons[i] == 0 for i in (0, 1, 2, 20, 39))
assert all(cons[i] == sum(len(c.data) for c in lives[i].calls) for i in range(40) if i not in (0, 1, 2, 20, 39))
eng.close()
L.lz4hip_shutdown()
print("cstream multidev ok")
