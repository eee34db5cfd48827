"""Child process of tests/test_gpu_dstream.py: initialises liblz4hip on D devices -- "distinct": devices 0 .. D - 1, "repeat": the list
[0] * D, which takes the same multi-device branch of csrc/api.cpp on a box with one GPU -- so that the stream decoder's host call shards
its streams over them at stream boundaries, and checks streams of every layout, hostile ones among them, cut into three calls against
the reference library's LZ4_decompress_safe_continue: values, states, bytes, and every byte that must stay untouched.  Prints
'dstream multidev ok D=<D>'."""
import sys

from support import init_devices, init_repeated   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from dstream_common import RefStream, check_set, hostile_set, layout_set, lib_decoder, rng_for

D = int(sys.argv[1])
amd, L = init_devices(list(range(D))) if sys.argv[2] == "distinct" else init_repeated(D)
rs = RefStream(O.ref())
rng = rng_for(80 + D)
streams = layout_set(rs, rng, 24 * D) + hostile_set(rs, rng, 4)   # more than 2 x 64 streams per device: every device gets a share
streams = [s for s in streams if not s.before]
assert len(streams) >= 2 * 64 * D
bad, calls = check_set(rs, streams, 3, rng, lib_decoder(L))
assert not bad, (len(bad), bad[:5])
print("dstream multidev ok D=%d streams=%d calls=%d" % (D, len(streams), calls))
