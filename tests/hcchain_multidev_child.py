"""Child process of tests/test_gpu_hcchain.py: initialises liblz4hip on D devices -- "distinct": devices 0 .. D - 1, "repeat": the list
[0] * D, which takes the same multi-device branch of csrc/api.cpp on a box with one GPU -- so that the HC chain compressor's host call
shards its chains over them at chain boundaries, and checks a batch of chains of uneven length (with and without prefixes, with blocks
that fail in the middle) against the reference library's LZ4_compress_HC_continue at level 9: values, bytes, and every byte that must
stay untouched.  Prints 'hcchain multidev ok D=<D>'."""
import random
import sys

from support import init_devices   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from cchain_common import book_chains, hand_chains, prefix_chains
from hcchain_common import HCPacked, RefHCChain, capacity_chains

D = int(sys.argv[1])
amd, L = init_devices(list(range(D)) if sys.argv[2] == "distinct" else [0] * D)
rc = RefHCChain(O.ref())
rng = random.Random(80 + D)
pre = prefix_chains()
pool = [c for c in book_chains() + pre[9] + pre[70000] + hand_chains(rng)[::3] if len(c.data) <= 70000]
pool += [c for c in capacity_chains(rc, [c for c in pool[::4] if len(c.blocks) >= 2 and len(c.data) >= 64])
         if min(c.lens + [0]) >= 0 and min(cap for _, cap in c.blocks) >= 0]
chains = [pool[(i * 5) % len(pool)] for i in range(64 * D * 2 + 9)]   # more than 2 x 64 chains per device: every device gets a share
want = [rc.compress(c, 9) for c in chains]
assert any(0 in w[0] and any(r > 0 for r in w[0][w[0].index(0) + 1:]) for w in want)
pk = HCPacked(chains)
dst = bytearray(pk.dst)
out = amd.LZ4HIPBatch.compressHCChain(pk.src, pk.chain_src_off, pk.src_len, pk.chain_first, dst, pk.dst_off, pk.dst_cap, pk.prefix, 9)
bad = pk.check(dst, out, want)
assert not bad, (len(bad), bad[:5])
for i in range(pk.n_blocks):   # the host call brings back only what was produced
    o, cap, r = pk.dst_off[i], max(pk.dst_cap[i], 0), max(out[i], 0)
    assert dst[o + r:o + cap] == bytes([pk.fill]) * (cap - r), i
print("hcchain multidev ok D=%d chains=%d blocks=%d" % (D, len(chains), pk.n_blocks))
