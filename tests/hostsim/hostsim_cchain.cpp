// tests/hostsim/hostsim_cchain.cpp -- TEST INFRASTRUCTURE ONLY.
// The linked-block compressor (lz4_fast_chain.h: cchain_walk over FastCore<..., LINK = true>, what compress_fast_chain_cu_kernel
// runs) compiled against the lock-step host backend, in a library of its own (tests/test_cchain_hostsim.py).  Nothing here is linked
// into liblz4hip.so.
//
// The bounds follow the walk block by block: while block [blk, end) of a chain runs, the simulated wave may read the chain's kept
// history and its source up to `end` -- not the bytes of the chain's later blocks, let alone what follows the chain -- and may write
// the block's slot and nothing else.
#include <stdint.h>
#include <string.h>
#include "../../lz4-java_amd/csrc/kernels.h"
#include "../../lz4-java_amd/csrc/lz4_fast_chain.h"
#include "wave_host.h"

namespace {

struct CChainIoHost {
  hostsim::WaveHost& w;
  const lz4hip::CChainArgs& a;
  static uint32_t uni(uint32_t v) { return v; }
  static uint64_t uni64(uint64_t v) { return v; }
  template <class T> static T* uni_ptr(T* p) { return p; }
  void put_out(uint32_t i, int32_t r) const { a.out[i] = r; }
  void put_chain(uint32_t c, uint64_t n) const { a.chain_consumed[c] = n; }
  void begin_block(const uint8_t* buf, uint32_t end, uint8_t* d, uint32_t cap) const { w.bounds(buf, end, d, cap); }
};

}  // namespace

extern "C" {

// the whole call of lz4hip_compress_fast_chain_batch on host arrays, chain after chain on ONE simulated wavefront whose table is
// never touched between two chains (what a wavefront of the kernel that draws several chains sees).  0, or -1000 if the simulated
// wave read or wrote outside the bounds above
int sim_cchain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                     const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out,
                     uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, uint64_t rng_seed) {
  const lz4hip::CChainArgs a{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains};
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CChainIoHost io{w, a};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    lz4hip::cchain_walk(w, io, a, c);
  }
  return w.oob ? -1000 : 0;
}

// the table a chain starts with (link_table_init) for the kept history [buf, buf + keep) -- keep == 0: the four bytes at buf are the
// chain's first -- copied out of the simulated LDS into table[0 .. 4096)
int sim_cchain_table(const uint8_t* buf, uint32_t keep, int prefixed, uint64_t* table, uint64_t rng_seed) {
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(buf, keep ? keep : 4u, nullptr, 0);
  lz4hip::link_table_init(w, buf, keep, prefixed != 0);
  memcpy(table, w.lds.data(), 4096 * sizeof(uint64_t));
  return w.oob ? -1000 : 0;
}

// the image dict_image_build writes for the same bytes (keep >= 8)
int sim_cchain_dict_image(const uint8_t* tail, uint32_t keep, uint8_t* image, uint64_t rng_seed) {
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(tail, keep, image, 32768);
  lz4hip::dict_image_build(w, tail, keep, image);
  return w.oob ? -1000 : 0;
}

}  // extern "C"
