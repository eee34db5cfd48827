// tests/hostsim/hostsim_chain.cpp -- TEST INFRASTRUCTURE ONLY.
// The chain walk of lz4-java_amd/csrc/lz4_decode_chain.h (LZ4_decompress_safe_continue over linked blocks) and the PREFIX switch of
// lz4_decode_core.h compiled against the lock-step host backend, in a library of its own (tests/test_chain_hostsim.py), in the forms
// decode_chain_kernel runs.  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_decode_chain.h"
#include "group_host.h"

namespace {
constexpr size_t kGuard = 256;
constexpr uint8_t kGuardByte = 0xA5;

// The simulator knows ONE readable range besides the block's own slot, so stream, history and the chain's earlier output share an arena:
// layout 0 = [guard][history][region][guard][streams]: readable [history, streams' end) -- a read in front of the history or behind the
// streams is out of bounds; layout 1 = [guard][streams][history][region][guard]: readable [streams, the block's end of capacity) -- a read in front of
// the streams, or past the block's capacity, is.  A case is run in both.  Writes are legal inside the current block's [d, d + cap) only.
struct SimIo {
  hostsim::GroupHost& g;
  const lz4hip::ChainArgs& a;
  int layout;
  const uint8_t* lo; const uint8_t* hi;   // layout 0: the readable range
  void begin_block(uint8_t* d, int cap) {
    g.dst_lo = d; g.dst_hi = d + cap;
    if (layout == 0) { g.src_lo = lo; g.src_hi = hi; } else { g.src_lo = lo; g.src_hi = d + cap; }   // (one range: a read may straddle the block's start)
  }
  void put_out(uint32_t i, int r) { a.out[i] = r; }
  void put_chain(uint32_t c, uint64_t n) { a.chain_out[c] = n; }
  void fence() {}
};
}  // namespace

extern "C" {

// One chain of n blocks through chain_walk: streams src + src_off[i] (src_bytes in all), history[0 .. prefix_len) in front of a region
// of chain_cap bytes.  form 2 = the deep loop with the pipelined loop behind it (decode_chain_kernel<8>), 1 = the pipelined loop alone,
// 0 = the plain loop (or, built with -DLZ4HIP_DECODE_INTERIOR=0, the exact tiers alone); gl = lanes per chain.  The region is pre-filled
// with `fill`; out_len[n], *chain_out and region_out[chain_cap] (the whole region as the walk left it) come back.  Returns 0, or
// -1000000 if the simulated group touched memory outside its bounds, wrote a guard byte or changed the history.
int sim_chain(const uint8_t* src, uint64_t src_bytes, const uint64_t* src_off, const int32_t* src_len, const uint8_t* stored, const int32_t* dst_cap,
              uint32_t n, const uint8_t* history, int prefix_len, uint64_t chain_cap, int form, int gl, int layout, uint8_t fill,
              int32_t* out_len, uint64_t* chain_out, uint8_t* region_out) {
  const size_t ns = (size_t)src_bytes, nh = prefix_len > 0 ? (size_t)prefix_len : 0, nr = (size_t)chain_cap;
  std::vector<uint8_t> arena(kGuard + nh + nr + kGuard + ns + 1, kGuardByte);
  uint8_t *s, *h;
  if (layout == 0) { h = arena.data() + kGuard; s = h + nh + nr + kGuard; }
  else { s = arena.data() + kGuard; h = s + ns; }
  uint8_t* const region = h + nh;
  if (ns) memcpy(s, src, ns);
  if (nh) memcpy(h, history, nh);
  memset(region, fill, nr);
  const uint32_t first[2] = {0u, n};
  const uint64_t doff = (uint64_t)(region - arena.data());
  lz4hip::ChainArgs a{s, src_off, src_len, stored, dst_cap, first, arena.data(), &doff, &chain_cap, &prefix_len, out_len, chain_out, n, 1u};
  hostsim::GroupHost g(gl, s, (long)ns, region, 0);
  SimIo io{g, a, layout, layout == 0 ? h : s, s + ns};
  if (form == 2) lz4hip::chain_walk<hostsim::GroupHost, SimIo, 2>(g, io, a, 0u, g.stg_buf);
  else if (form == 1) lz4hip::chain_walk<hostsim::GroupHost, SimIo, 1>(g, io, a, 0u, nullptr);
  else lz4hip::chain_walk<hostsim::GroupHost, SimIo, 0>(g, io, a, 0u, nullptr);
  memcpy(region_out, region, nr);
  bool bad = g.oob || hostsim::GroupHost::walk_mismatch.load() != 0;
  if (nh && memcmp(h, history, nh) != 0) bad = true;
  if (ns && memcmp(s, src, ns) != 0) bad = true;
  for (size_t k = 0; k < kGuard; k++) {
    if (arena[k] != kGuardByte) bad = true;
    if (region[nr + k] != kGuardByte) bad = true;
  }
  return bad ? -1000000 : 0;
}

// the number of deep-loop trips the simulator has run (tests assert that the deep loop really ran)
uint64_t sim_chain_deep_trips() { return hostsim::GroupHost::deep_trips; }

}  // extern "C"
