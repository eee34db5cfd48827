// tests/hostsim/hostsim_accel.cpp -- TEST INFRASTRUCTURE ONLY.
// The accelerated one-sequence core (lz4_fast_core.h, FastCore<..., ACC = true>: LZ4_compress_fast with acceleration > 1)
// compiled against the lock-step host backend, in a library of its own (tests/test_accel_hostsim.py).  Nothing here is linked
// into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_fast_core.h"
#include "wave_host.h"
#include "block_host.h"

extern "C" {

// the block shell compress_fast_accel_cu_kernel runs (fast_block_run): returns compressed size (0 = does not fit), or -1000 if the simulated wave touched memory outside [src, src+n) / [dst, dst+cap).
// `accel` is used as given (the library clamps it to 2 .. 65537 before the kernel sees it; 1 is the plain core)
int sim_compress_fast_accel(const uint8_t* src, int n, uint8_t* dst, int cap, uint32_t accel, uint64_t* stats4, uint64_t rng_seed) {
  hostsim::WaveHost w;
  hostsim::BlockHost io(src, n, dst, cap);
  io.x.accel = accel;
  return hostsim::sim_fast_block<lz4hip::FastForm<hostsim::WaveHost, false, true, false, true>>(w, io, stats4, rng_seed);
}

// the probe offsets g_a(k0 .. k0+63) of a miss-run (lane k - k0 holds g_a(k)), as the core computes them
void sim_accel_offsets(uint32_t accel, uint32_t k0, uint32_t* out64) {
  hostsim::WaveHost w;
  lz4hip::DirectOut<hostsim::WaveHost> out(w, nullptr, 0u, nullptr, 0u);
  lz4hip::FastCore<hostsim::WaveHost, true, lz4hip::DirectOut<hostsim::WaveHost>, false, true> c(w, out, nullptr, 0u);
  c.accel = accel;
  const hostsim::WaveHost::VU g = c.g_acc(w.lane() + k0);
  for (int l = 0; l < 64; l++) out64[l] = g.v[l];
}

}  // extern "C"
