"""Child process of tests/test_gpu_dstream_inorder.py: initialises liblz4hip on D devices -- "distinct": devices 0 .. D - 1, "repeat": the
list [0] * D, which takes the same multi-device branch of csrc/api.cpp on a box with one GPU -- so that the in-order stream decoder's
host call shards its streams over them at stream boundaries, and checks streams of the overlap layouts and of every exact layout, hostile
ones among them, cut into three calls against the reference library's LZ4_decompress_safe_continue: values, states, bytes, and every
byte that must stay untouched.  Prints 'dstream inorder multidev ok D=<D>'."""
import sys

from support import init_devices, init_repeated   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from dstream_common import RefStream, check_set, hostile_set, layout_set, rng_for
from dstream_inorder_common import inorder_decoder, layout_streams

D = int(sys.argv[1])
amd, L = init_devices(list(range(D))) if sys.argv[2] == "distinct" else init_repeated(D)
rs = RefStream(O.ref())
rng = rng_for(130 + D)
streams = [s for s in layout_set(rs, rng, 12 * D) if s.layout != "g" and not s.before] + hostile_set(rs, rng, 2)
streams = [s for s in streams if not s.before]
for kind in (("s", 1024, 1, 300), ("s", 4096, 1, 1000), ("g",), ("m", "fit", 1024, True)):
    streams += layout_streams(rs, rng, kind, 16 * D)
assert len(streams) >= 2 * 64 * D
bad, calls = check_set(rs, streams, 3, rng, inorder_decoder(L))
assert not bad, (len(bad), bad[:5])
print("dstream inorder multidev ok D=%d streams=%d calls=%d" % (D, len(streams), calls))
