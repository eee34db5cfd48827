// tests/hostsim/hostsim_cxstream.cpp -- TEST INFRASTRUCTURE ONLY.
// The resident-stream compressor for sources that land anywhere (lz4_fast_chain.h: cxstream_walk over FastCore<..., LINK = true> and
// FastCore<..., DICT = true, LINK = true>, what compress_fast_xstream_cu_kernel runs) compiled against the lock-step host backend, in a
// library of its own (tests/test_cxstream_hostsim.py), with cstream_walk beside it so that the two walks can alternate on one record.
// Nothing here is linked into liblz4hip.so.
//
// The state of the streams is the caller's host memory, as in hostsim_cstream.cpp.  The simulator knows ONE readable range: while a
// block in prefix mode runs it is the history and the source up to the block's end; while a block in external-dictionary mode runs it
// is the span from the lower of the two pieces to the end of the higher one, so the tests lay an outside dictionary on either side of
// the window; what lies between the two pieces is guard bytes or older data of the same ring.
#include <stdint.h>
#include <string.h>
#include "../../lz4-java_amd/csrc/kernels.h"
#include "../../lz4-java_amd/csrc/lz4_fast_chain.h"
#include "wave_host.h"

namespace {

struct CXStreamIoHost {
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

}  // namespace

extern "C" {

uint32_t sim_cxstream_rec_words() { return lz4hip::kStreamRecWords; }

// one call of lz4hip_compress_fast_stream_ext_batch on host arrays: chain c continues the stream in slot[c] of the state (rec, tables),
// chain after chain on ONE simulated wavefront.  0, or -1000 if the simulated wave read or wrote outside the bounds above
int sim_cxstream_batch(const uint32_t* slot, uint32_t* rec, uint64_t* tables, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                       const uint32_t* chain_first, const uint64_t* chain_hist_end, const int32_t* chain_hist_len, uint8_t* dst,
                       const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                       uint64_t rng_seed) {
  const lz4hip::CXStreamArgs x{{{src, nullptr, chain_hist_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains},
                                slot, rec, tables}, src_off, chain_hist_end};
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CXStreamIoHost io{w, x.s.c};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    lz4hip::cxstream_walk(w, io, x, c);
  }
  return w.oob ? -1000 : 0;
}

// one call of the existing walk (cstream_walk) on the same state: the two entry points alternate on a set
int sim_cxstream_prefix_batch(const uint32_t* slot, uint32_t* rec, uint64_t* tables, const uint8_t* src, const uint64_t* chain_src_off,
                              const int32_t* chain_prefix_len, const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off,
                              const int32_t* dst_cap, int32_t* out, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, uint64_t rng_seed) {
  const lz4hip::CStreamArgs s{{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, n_blocks, n_chains},
                              slot, rec, tables};
  hostsim::WaveHost w;
  if (rng_seed) w.rng = rng_seed;
  CXStreamIoHost io{w, s.c};
  for (uint32_t c = 0; c < n_chains; c++) {
    w.bounds(nullptr, 0, nullptr, 0);
    lz4hip::cstream_walk(w, io, s, c);
  }
  return w.oob ? -1000 : 0;
}

}  // extern "C"
