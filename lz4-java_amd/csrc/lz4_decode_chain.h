// lz4_decode_chain.h -- the walk over one chain of linked blocks (LZ4_decompress_safe_continue, liblz4 1.9.3), shared by
// decode_chain.hip and the CPU lane simulator (tests/hostsim/hostsim_chain.cpp).
//
// A chain is a run of blocks whose decoded forms lie back to back in one destination region; a match of block k may reach into what
// the blocks before it decoded and into the history that lay in front of the chain.  liblz4 defines block k's result as
//   LZ4_setStreamDecode(sd, chain_dst - prefix_len, prefix_len);
//   r_k = LZ4_decompress_safe_continue(sd, src_k, chain_dst + sum(r_j, j < k), src_len_k, cap_k);
// which is its rolling-prefix mode throughout (every destination is where the previous one ended): decode_block's PREFIX switch with
// hist = min(prefix_len + bytes decoded so far, 65535).  A negative result ends the chain (liblz4 leaves its stream state untouched
// there and nothing meaningful can follow): the blocks behind it get kChainStopped.  A block that decodes to 0 bytes changes nothing.
//
// ONE lane group walks a chain from its first block to its last: block k + 1 reads what the same group stored for block k, in
// program order, and `io.fence()` between two blocks makes that order explicit.  Nothing here waits for another group, wavefront or
// workgroup: a chain is serial by construction, and parallelism comes from the number of chains alone.
//
// Io: put_out(i, r) / put_chain(c, bytes): the results (one lane writes them); fence(): every store of the block just decoded is
// done before the next block's first load; begin_block(d, cap): the block about to be decoded may write [d, d + cap) and nothing
// else (the simulator's bounds; nothing on the device).
#pragma once
#include <stdint.h>
#include "kernels.h"
#include "lz4_decode_core.h"

namespace lz4hip {

// a stored (raw) block: whole 64-byte steps, then the rest byte by byte -- nothing past n is touched
template <class Grp>
LZ4HIP_DEV void chain_copy_stored(Grp& g, uint8_t* d, const uint8_t* s, uint32_t n) {
  const uint32_t whole = n & ~63u;
  g.copy_lits_wide(d, s, whole);
  g.copy_lits(d + whole, s + whole, n - whole, false);
}

// PIPE: decode_block's interior loops: 2 = the deep loop (streams of 2 KB and more) with the pipelined loop behind it, as
// decode_deep_kernel runs them; 0 = the plain loop (the simulator's exact-tier builds)
template <class Grp, class Io, int PIPE = 2>
LZ4HIP_DEV void chain_walk(Grp& g, Io& io, const ChainArgs& a, uint32_t c, uint8_t* stage) {
  uint32_t b1 = a.chain_first[c + 1], b0 = a.chain_first[c];
  if (b1 > a.n_blocks) b1 = a.n_blocks;
  if (b0 > b1) b0 = b1;
  const uint64_t doff = a.chain_dst_off[c], ccap = a.chain_dst_cap[c];
  uint8_t* const base = a.dst + doff;
  uint64_t prefix = 0;
  if (a.chain_prefix_len) { const int32_t p = a.chain_prefix_len[c]; prefix = p > 0 ? (uint64_t)p : 0u; }
  if (prefix > doff) prefix = doff;
  uint64_t done = 0;   // bytes the chain has decoded
  uint32_t i = b0;
  while (i < b1) {
    const int32_t sl = a.src_len[i], dc = a.dst_cap[i];
    int r;
    if (sl < 0 || dc < 0) {
      r = -1;
    } else {
      const uint64_t left = ccap > done ? ccap - done : 0u;
      int cap = (uint64_t)dc < left ? dc : (int)left;
      if (cap > kChainBlockCapMax) cap = kChainBlockCapMax;
      const uint8_t* s = a.src + a.src_off[i];
      uint8_t* d = base + done;
      io.begin_block(d, cap);
      if (a.stored && a.stored[i]) {
        if (sl > cap) r = -1;
        else { chain_copy_stored(g, d, s, (uint32_t)sl); r = sl; }
      } else {
        const uint64_t h = prefix + done;
        r = decode_block<Grp, true, PIPE, false, false, false, true>(g, s, sl, d, cap, stage, nullptr, 0, h > 65535u ? 65535 : (int)h);
      }
    }
    io.put_out(i, r);
    i++;
    if (r < 0) break;
    done += (uint64_t)r;
    io.fence();
  }
  for (; i < b1; i++) io.put_out(i, kChainStopped);
  io.put_chain(c, done);
}

}  // namespace lz4hip
