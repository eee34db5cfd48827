// tests/hostsim/hostsim_hc_destsize.cpp -- TEST INFRASTRUCTURE ONLY.
// The fill-mode HC parser (lz4_hc_core.h, HcParse<..., FILL = true>: LZ4_compress_HC_destSize) behind the unchanged delta[]
// builder, compiled against the lock-step host backend, in a library of its own (tests/test_hc_destsize_hostsim.py).  Nothing
// here is linked into liblz4hip.so.
#include <stdint.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_hc_core.h"
#include "wave_host.h"

extern "C" {

// LZ4_compress_HC_destSize(state, src, dst, &n, target, level) as hc_build_kernel + hc_parse_dest_kernel run it: returns the bytes
// written and sets *consumed, or -1000 if the simulated wave touched memory outside [src, src+n) / [dst, dst+target)
int sim_compress_hc_dest_size(const uint8_t* src, int n, uint8_t* dst, int target, int level, int* consumed, uint64_t rng_seed) {
  *consumed = n;   // liblz4 leaves *srcSizePtr untouched where it returns 0 up front
  if (target < 1 || n < 0 || (uint32_t)n > 0x7E000000u) return 0;
  if (level < 1) level = 9;
  if (level > 12) level = 12;
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(src, (size_t)n, dst, (size_t)target);
  std::vector<uint16_t> delta((size_t)n + 8, 0xFFFF);
  lz4hip::HcBuild<hostsim::WaveHost>::run(w, src, (uint32_t)n, delta.data());
  lz4hip::HcParse<hostsim::WaveHost, true> p(w, src, n, delta.data(), dst, target, level);
  std::vector<int> opt(level >= 10 ? (size_t)lz4hip::HC_OPT_INTS : 1u, 0x55555555);
  const int r = level >= 10 ? p.run_opt(level, opt.data()) : p.run();
  *consumed = p.consumed;
  if (w.oob) return -1000;
  return r;
}

}  // extern "C"
