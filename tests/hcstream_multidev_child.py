"""Child of tests/test_gpu_hcstream.py: lz4hip_compress_hc_stream_batch sharded over several engine devices at stream boundaries.
argv[1] = D > 0: device 0 listed D times (the multi-device branch on one GPU); 0: devices 0 and 1.  200 streams on rings, alternating
buffers and behind dictionaries elsewhere, so that every call has more than 64 streams per device; every stream against the
reference's ONE LZ4_streamHC_t."""
import random
import sys

import support
from cchain_common import book1
from hcstream_common import RefHCStream, drive, make

D = int(sys.argv[1])
amd, L = support.init_repeated(D) if D else support.init_devices([0, 1])
from oracle import oracle as O   # noqa: E402  (support put the repository root on the path)

rr = RefHCStream(O.ref())
rng = random.Random(391)
data = book1()
scripts = [make(("two", "ring", "dict", "adjacent")[i % 4], data[rng.randrange(0, 600000):], rng, "#%d" % i, maxb=512, n_blocks=rng.randrange(3, 9)) for i in range(200)]
for level in (9, 10):
    bad, fleet = drive(amd, rr, scripts, level, rng)
    assert not bad, (level, len(bad), bad[:5])
L.lz4hip_shutdown()
print("hcstream multidev ok")
