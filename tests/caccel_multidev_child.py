"""Child of tests/test_gpu_caccel.py: a set of resident compress streams divided over several engine devices, driven at changing
accelerations through lz4hip_compress_fast_stream_accel_batch and, at acceleration 1, the existing entry point in turn.  argv[1] = D > 0:
device 0 listed D times (the multi-device branch on one GPU: the set has D parts and a call is sharded at their boundaries); 0: devices 0
and 1.  40 streams, so that the parts' boundaries fall inside the calls; every stream against the reference's ONE LZ4_stream_t; then 40
accelerated chains in one call, sharded at chain boundaries."""
import random
import sys

import support
from caccel_common import AccelPlan, DevAccel, RefAccelChain, chain_accel_call, drive_lives
from cchain_common import CPacked, book1, chain_of
from cstream_common import random_life

D = int(sys.argv[1])
amd, L = support.init_repeated(D) if D else support.init_devices([0, 1])
from oracle import oracle as O   # noqa: E402  (support put the repository root on the path)

rc = RefAccelChain(O.ref(), AccelPlan((8, 1, 64, 1, 3)))
rng = random.Random(281)
lives = [random_life(rng, O, "stream %d" % i, rng.randrange(2, 10), 2500, every_boundary=True) for i in range(40)]
eng = DevAccel(amd, 40, rc.plan)
bad, results, rounds = drive_lives(eng, rc, lives, rng, absent=0.4)
assert not bad, (len(bad), bad[:5])
assert {1, 3, 8, 64} <= set(rc.plan.used)
cons, stop = eng.consumed()
assert cons == [sum(len(c.data) for c in lf.calls) for lf in lives] and not any(stop)
eng.close()
b = book1()
chains = [chain_of("chain %d" % i, b[3000 * i:3000 * i + 6000], [1000] * 6, history=b[3000 * i - (i % 3) * 500:3000 * i]) for i in range(1, 41)]
pk = CPacked(chains)
status, dst, out, cons = chain_accel_call(L, pk, 8)
assert status == 0 and not pk.check(dst, out, cons, [rc.at(8).compress(c) for c in chains])
L.lz4hip_shutdown()
print("caccel multidev ok")
