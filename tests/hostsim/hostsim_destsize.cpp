// tests/hostsim/hostsim_destsize.cpp -- TEST INFRASTRUCTURE ONLY.
// The fill-mode output policy of the one-sequence core (lz4_fast_core.h, DirectOut<..., FILL = true>: LZ4_compress_destSize)
// compiled against the lock-step host backend, in a library of its own (tests/test_destsize_hostsim.py).  Nothing here is
// linked into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_fast_core.h"
#include "wave_host.h"

extern "C" {

// LZ4_compress_destSize(src, dst, &n, target) as compress_fast_dest_cu_kernel runs it: returns the bytes written and sets
// *consumed, or -1000 if the simulated wave touched memory outside [src, src+n) / [dst, dst+target)
int sim_compress_dest_size(const uint8_t* src, int n, uint8_t* dst, int target, int* consumed, uint64_t* stats4, uint64_t rng_seed) {
  *consumed = n;   // liblz4 leaves *srcSizePtr untouched where it returns 0 up front
  if (target <= 0 || n < 0 || (uint32_t)n > 0x7E000000u) return 0;
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(src, (size_t)n, dst, (size_t)target);
  lz4hip::FastStats st = {0, 0, 0, 0};
  uint32_t r;
  lz4hip::DirectOut<hostsim::WaveHost, true> out(w, src, (uint32_t)n, dst, (uint32_t)target);
  if (n < 65547) {
    lz4hip::FastCore<hostsim::WaveHost, true, lz4hip::DirectOut<hostsim::WaveHost, true>> c(w, out, src, (uint32_t)n, &st);
    r = c.run();
  } else {
    lz4hip::FastCore<hostsim::WaveHost, false, lz4hip::DirectOut<hostsim::WaveHost, true>> c(w, out, src, (uint32_t)n, &st);
    r = c.run();
  }
  *consumed = (int)out.consumed;
  if (stats4) { stats4[0] = st.steps; stats4[1] = st.slow_steps; stats4[2] = st.false_pos; stats4[3] = st.sequences; }
  if (w.oob) return -1000;
  return (int)r;
}

}  // extern "C"
