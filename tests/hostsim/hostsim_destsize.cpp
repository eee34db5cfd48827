// tests/hostsim/hostsim_destsize.cpp -- TEST INFRASTRUCTURE ONLY.
// The fill-mode output policy of the one-sequence core (lz4_fast_core.h, DirectOut<..., FILL = true>: LZ4_compress_destSize)
// compiled against the lock-step host backend, in a library of its own (tests/test_destsize_hostsim.py).  Nothing here is
// linked into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_fast_core.h"
#include "wave_host.h"
#include "block_host.h"

extern "C" {

// LZ4_compress_destSize(src, dst, &n, target) through the block shell compress_fast_dest_cu_kernel runs (fast_block_run): returns the bytes written and sets
// *consumed, or -1000 if the simulated wave touched memory outside [src, src+n) / [dst, dst+target)
int sim_compress_dest_size(const uint8_t* src, int n, uint8_t* dst, int target, int* consumed, uint64_t* stats4, uint64_t rng_seed) {
  hostsim::WaveHost w;
  hostsim::BlockHost io(src, n, dst, target);
  const int r = hostsim::sim_fast_block<lz4hip::FastForm<hostsim::WaveHost, true, false, false, true>>(w, io, stats4, rng_seed);
  *consumed = io.used;   // (src_len where the shell returns 0 up front, as liblz4 leaves *srcSizePtr untouched)
  return r;
}

}  // extern "C"
