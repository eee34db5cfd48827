"""Child process of tests/test_gpu_chain.py: initialises liblz4hip on D devices -- "distinct": devices 0 .. D - 1, "repeat": the list
[0] * D, which takes the same multi-device branch of csrc/api.cpp on a box with one GPU -- so that the chain decoder's host call shards
its chains over them at chain boundaries, and checks a batch of chains of uneven length (valid, damaged, with history, with stored
blocks) against the reference library's LZ4_decompress_safe_continue: values, chain lengths, bytes, and every byte that must stay
untouched.  Prints 'chain multidev ok D=<D>'."""
import sys

from support import init_devices   # (first: it puts the repository root on sys.path)
from oracle import oracle as O
from chain_common import Packed, RefChain, book_chains, damaged_chains, hand_chains, rng_for, stored_and_empty_chains

D = int(sys.argv[1])
amd, L = init_devices(list(range(D)) if sys.argv[2] == "distinct" else [0] * D)
rc = RefChain(O.ref())
rng = rng_for(70 + D)
pool = book_chains(rc) + stored_and_empty_chains(rc) + damaged_chains(rc, rng, n_flipped=10) + hand_chains(rng)[::7]
chains = [pool[(i * 5) % len(pool)] for i in range(64 * D * 2 + 9)]   # more than 2 x 64 chains per device: every device gets a share
want = [rc.decode(c) for c in chains]
pk = Packed(chains)
dst = bytearray(pk.dst)
out, cout = amd.LZ4HIPBatch.decompressSafeChain(pk.src, pk.src_off, pk.src_len, pk.dst_cap, pk.chain_first, dst, pk.chain_dst_off, pk.chain_dst_cap,
                                                pk.prefix, pk.stored)
bad = pk.check(dst, out, cout, want)
assert not bad, (len(bad), bad[:5])
for c, (outs, done, _) in enumerate(want):
    off = pk.chain_dst_off[c]
    assert dst[off + done:off + pk.chain_dst_cap[c]] == bytes([pk.fill]) * (pk.chain_dst_cap[c] - done), chains[c].name
print("chain multidev ok D=%d chains=%d blocks=%d" % (D, len(chains), pk.n_blocks))
