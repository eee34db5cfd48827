"""Child process of tests/test_gpu_cchain.py: initialises liblz4hip on D devices -- "distinct": devices 0 .. D - 1, "repeat": the list
[0] * D, which takes the same multi-device branch of csrc/api.cpp on a box with one GPU -- so that the chain compressor's host call
shards its chains over them at chain boundaries, and checks a batch of chains of uneven length (with and without prefixes, stopped
early by tight capacities) against the reference library's LZ4_compress_fast_continue: values, consumed sizes, bytes, and every byte
that must stay untouched.  Prints 'cchain multidev ok D=<D>'."""
import random
import sys

from support import init_devices   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from cchain_common import CPacked, RefCChain, book_chains, capacity_chains, hand_chains, prefix_chains

D = int(sys.argv[1])
amd, L = init_devices(list(range(D)) if sys.argv[2] == "distinct" else [0] * D)
rc = RefCChain(O.ref())
rng = random.Random(70 + D)
pre = prefix_chains()
pool = [c for c in book_chains() + pre[9] + pre[70000] + hand_chains(rng)[::3] if len(c.data) <= 70000]
pool += [c for c in capacity_chains(rc, pool[::4]) if min(c.lens + [0]) >= 0 and min(cap for _, cap in c.blocks) >= 0]
chains = [pool[(i * 5) % len(pool)] for i in range(64 * D * 2 + 9)]   # more than 2 x 64 chains per device: every device gets a share
want = [rc.compress(c) for c in chains]
assert any(0 in w[0] for w in want)
pk = CPacked(chains)
dst = bytearray(pk.dst)
out, cons = amd.LZ4HIPBatch.compressFastChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, dst, pk.dst_off, pk.dst_cap, pk.prefix)
bad = pk.check(dst, out, cons, want)
assert not bad, (len(bad), bad[:5])
for i in range(pk.n_blocks):
    o, cap, r = pk.dst_off[i], max(pk.dst_cap[i], 0), max(out[i], 0)
    assert dst[o + r:o + cap] == bytes([pk.fill]) * (cap - r), i
print("cchain multidev ok D=%d chains=%d blocks=%d" % (D, len(chains), pk.n_blocks))
