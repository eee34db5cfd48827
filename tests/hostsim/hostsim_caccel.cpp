// tests/hostsim/hostsim_caccel.cpp -- TEST INFRASTRUCTURE ONLY.
// The three linked-block walks of lz4_fast_chain.h with their ACC switch on (cchain_walk<true>, cstream_walk<true>, cxstream_walk<true>
// over FastCore<..., ACC = true, LINK = true> and FastCore<..., ACC = true, DICT = true, LINK = true>: what the *_accel_cu_kernels of
// compress_fast.hip run) compiled against the lock-step host backend, in a library of its own (tests/test_caccel_hostsim.py).  Nothing
// here is linked into liblz4hip.so.
//
// Every entry takes the caller's acceleration as the C ABI does: it is clamped as liblz4 clamps it, and after clamping 1 runs the
// EXISTING walk (ACC = false) -- csrc/api.cpp launch_block's choice between the two kernels -- so calls of both walks alternate on one
// record and one table image.  Io and bounds are those of hostsim_cchain.cpp, hostsim_cstream.cpp and hostsim_cxstream.cpp.
#include <stdint.h>
#include <string.h>
#include "../../lz4-java_amd/csrc/kernels.h"
#include "../../lz4-java_amd/csrc/lz4_fast_chain.h"
#include "wave_host.h"

namespace {

struct CAccelIoHost {
  hostsim::WaveHost& w;
  const lz4hip::CChainArgs& a;
  static uint32_t uni(uint32_t v) { return v; }
  static uint64_t uni64(uint64_t v) { return v; }
  template <class T> static T* uni_ptr(T* p) { return p; }
  void put_out(uint32_t i, int32_t r) const { a.out[i] = r; }
  void put_chain(uint32_t c, uint64_t n) const { a.chain_consumed[c] = n; }
  void begin_block(const uint8_t* buf, uint32_t end, uint8_t* d, uint32_t cap) const { w.bounds(buf, end, d, cap); }
  void begin_xblock(const uint8_t* hist, uint32_t hn, const uint8_t* blk, uint32_t n, uint8_t* d, uint32_t cap) const {
    if (!hn) { w.bounds(blk, n, d, cap); return; }
    const uint8_t* lo = hist < blk ? hist : blk;
    const uint8_t* hi = hist + hn > blk + n ? hist + hn : blk + n;
    w.bounds(lo, (size_t)(hi - lo), d, cap);
  }
  void begin_state(uint8_t* image) const { w.bounds(image, 32768, image, 32768); }
  void end_state() const { w.bounds(nullptr, 0, nullptr, 0); }
  static void table_load(hostsim::WaveHost& w, const uint8_t* image) { if (w.in_ok(image, 32768)) memcpy(w.lds.data(), image, 32768); }
  static void table_store(hostsim::WaveHost& w, uint8_t* image) { if (w.out_ok(image, 32768)) memcpy(image, w.lds.data(), 32768); }
  static void put_rec(uint32_t* rec, uint32_t idx, uint32_t held, uint32_t flags, uint32_t span, uint64_t total) {
    rec[0] = idx; rec[1] = held; rec[2] = flags; rec[3] = span; rec[4] = (uint32_t)total; rec[5] = (uint32_t)(total >> 32);
  }
};

// liblz4's clamp (csrc/api.cpp accel_clamp)
uint32_t clamp(int a) { return a < 1 ? 1u : a > 65537 ? 65537u : (uint32_t)a; }

}  // namespace

extern "C" {

uint32_t sim_caccel_rec_words() { return lz4hip::kStreamRecWords; }
// the acceleration a call runs at
uint32_t sim_caccel_clamp(int acceleration) { return clamp(acceleration); }

// lz4hip_compress_fast_chain_accel_batch on host arrays, chain after chain on ONE simulated wavefront.  0, or -1000 if the simulated
// wave read or wrote outside the bounds
int sim_caccel_chain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                           const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out,
                           uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, uint64_t rng_seed, int acceleration) {
  const lz4hip::CChainArgs a{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains};
  const uint32_t accel = clamp(acceleration);
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CAccelIoHost io{w, a};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    if (accel >= 2u) lz4hip::cchain_walk<true>(w, io, a, c, accel);
    else lz4hip::cchain_walk(w, io, a, c);
  }
  return w.oob ? -1000 : 0;
}

// one call of lz4hip_compress_fast_stream_accel_batch: chain c continues the stream in slot[c] of the state (rec, tables)
int sim_caccel_stream_batch(const uint32_t* slot, uint32_t* rec, uint64_t* tables, const uint8_t* src, const uint64_t* chain_src_off,
                            const int32_t* chain_prefix_len, const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off,
                            const int32_t* dst_cap, int32_t* out, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, uint64_t rng_seed,
                            int acceleration) {
  const lz4hip::CStreamArgs s{{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains},
                              slot, rec, tables};
  const uint32_t accel = clamp(acceleration);
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CAccelIoHost io{w, s.c};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    if (accel >= 2u) lz4hip::cstream_walk<true>(w, io, s, c, accel);
    else lz4hip::cstream_walk(w, io, s, c);
  }
  return w.oob ? -1000 : 0;
}

// one call of lz4hip_compress_fast_stream_ext_accel_batch on the same state
int sim_caccel_xstream_batch(const uint32_t* slot, uint32_t* rec, uint64_t* tables, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                             const uint32_t* chain_first, const uint64_t* chain_hist_end, const int32_t* chain_hist_len, uint8_t* dst,
                             const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                             uint64_t rng_seed, int acceleration) {
  const lz4hip::CXStreamArgs x{{{src, nullptr, chain_hist_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains},
                                slot, rec, tables}, src_off, chain_hist_end};
  const uint32_t accel = clamp(acceleration);
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CAccelIoHost io{w, x.s.c};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    if (accel >= 2u) lz4hip::cxstream_walk<true>(w, io, x, c, accel);
    else lz4hip::cxstream_walk(w, io, x, c);
  }
  return w.oob ? -1000 : 0;
}

}  // extern "C"
