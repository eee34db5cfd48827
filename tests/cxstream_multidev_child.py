"""Child of tests/test_gpu_cxstream.py: a set of resident compress streams divided over several engine devices, driven through
lz4hip_compress_fast_stream_ext_batch.  argv[1] = D > 0: device 0 listed D times (the multi-device branch on one GPU: the set has D
parts and a call is sharded at their boundaries); 0: devices 0 and 1.  40 streams on rings and alternating buffers, so that the parts'
boundaries fall inside the calls; every stream against the reference's ONE LZ4_stream_t."""
import random
import sys

import support
from cxstream_common import DevX, book1, drive_x, make_xstream
from dstream_common import RefStream

D = int(sys.argv[1])
amd, L = support.init_repeated(D) if D else support.init_devices([0, 1])
from oracle import oracle as O   # noqa: E402  (support put the repository root on the path)

rs = RefStream(O.ref())
rng = random.Random(91)
data = book1()
streams = [make_xstream(("two4096", "ring8192", "ring3000", "dict4096")[i % 4], rng, data, "#%d" % i, n_blocks=rng.randrange(3, 10)) for i in range(40)]
eng = DevX(amd, 40)
bad, made, rounds = drive_x(eng, rs, streams, rng, mode="random", absent=0.4)
assert not bad, (len(bad), bad[:5])
cons, stop = eng.consumed()
assert cons == [sum(len(b.data) for b in xs.blocks) for xs in streams] and not any(stop)
eng.reset([0, 1, 2, 20, 39])
cons, stop = eng.consumed()
assert all(cons[i] == 0 for i in (0, 1, 2, 20, 39))
assert all(cons[i] == sum(len(b.data) for b in streams[i].blocks) for i in range(40) if i not in (0, 1, 2, 20, 39))
eng.close()
L.lz4hip_shutdown()
print("cxstream multidev ok")
