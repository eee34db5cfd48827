// tests/hostsim/hostsim_hcchain.cpp -- TEST INFRASTRUCTURE ONLY.
// The HC chain compressor's cores (lz4_hc_core.h: hc_chain_build_segment = HcBuild<..., false, SEG = true>, hc_chain_parse_block =
// HcParse<..., false, false, PREFIX = true>: LZ4_compress_HC_continue over linked blocks in prefix mode) compiled against the lock-step
// host backend, in a library of its own (tests/test_hcchain_hostsim.py).  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_hc_core.h"
#include "wave_host.h"

extern "C" {

// delta[0 .. len - 3) of the chain buffer buf[0, len), built in segments of `seg` positions as hc_build_chain_kernel builds it (every
// segment from a zeroed head table); -1000 if the simulated wave read outside the buffer.  order = 1: the segments last to first
// (the kernel's workgroups draw them in any order)
int sim_hc_chain_build(const uint8_t* buf, uint64_t len, uint32_t seg, uint16_t* delta, int order, uint64_t rng_seed) {
  hostsim::WaveHost w;
  w.lds.assign(16384, 0);
  if (rng_seed) w.rng = rng_seed;
  w.bounds(buf, (size_t)len, nullptr, 0);
  const uint64_t nseg = len >= 4u ? (len - 3u + seg - 1u) / seg : 0u;
  for (uint64_t t = 0; t < nseg; t++)
    lz4hip::hc_chain_build_segment(w, buf, len, seg, (uint32_t)(order ? nseg - 1u - t : t), delta);
  return w.oob ? -1000 : 0;
}

// the block of n bytes at buf + start, behind min(65536, start) bytes of history, as hc_parse_chain_kernel parses it: the compressed
// size (0 = does not fit), or -1000 if the simulated wave read outside [start - history, start + n) or wrote outside [dst, dst + cap)
int sim_hc_chain_block(const uint8_t* buf, uint64_t start, int n, const uint16_t* delta, uint8_t* dst, int cap, int level, uint64_t rng_seed) {
  if (n < 0 || (uint32_t)n > 0x7E000000u || cap < 0) return 0;
  if (level < 1) level = 9;
  if (level > 12) level = 12;
  const uint32_t hist = start > 65536u ? 65536u : (uint32_t)start;
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(buf + start - hist, (size_t)hist + (size_t)n, dst, (size_t)cap);
  std::vector<int> opt(level >= 10 ? (size_t)lz4hip::HC_OPT_INTS : 1u, 0x55555555);
  const int r = lz4hip::hc_chain_parse_block(w, buf + start - hist, hist, n, delta + (start - hist), dst, cap, level, opt.data());
  return w.oob ? -1000 : r;
}

}  // extern "C"
