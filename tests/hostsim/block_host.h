// tests/hostsim/block_host.h -- TEST INFRASTRUCTURE ONLY.
// The host's side of the block shell (lz4_fast_core.h fast_block_run; compress_fast.hip's BlockIoDev is the device's): a batch of one.
#pragma once
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_fast_core.h"
#include "wave_host.h"

namespace hostsim {

struct BlockHost {
  uint64_t off = 0;
  int32_t n, cap, r = 0, used = 0;   // (r, used: what the shell stored: the result and, FILL forms, the input consumed)
  lz4hip::BatchArgs a;      // (points into this object: not to be copied)
  lz4hip::FastBlockArgs x;  // the form's state: set what the form reads before the run
  BlockHost(const uint8_t* src, int32_t n_, uint8_t* dst, int32_t cap_) : n(n_), cap(cap_), a{src, &off, &n, dst, &off, &cap, &r, 1u} {}
  static int32_t i32(int32_t v) { return v; }
  template <class T> static T* ptr(T* p) { return p; }
  template <class W> void begin_block(W& w, const uint8_t* s, uint32_t len, uint8_t* d, uint32_t room) { w.bounds(s, len, d, room); }
  void put(uint32_t, uint32_t r_) { r = (int32_t)r_; }
  void put(uint32_t, uint32_t r_, int32_t c) { r = (int32_t)r_; used = c; }
};
// one block through the shell: the result it stored, or -1000 if the simulated wave touched memory outside what begin_block allowed
template <class Form, class W, class Io>
int sim_fast_block(W& w, Io& io, uint64_t* stats4, uint64_t rng_seed) {
  if (rng_seed) w.rng = rng_seed;
  lz4hip::FastStats st = {0, 0, 0, 0};
  io.x.st = &st;
  lz4hip::fast_block_run<Form>(w, io, io.a, 0u, io.x);
  if (stats4) { stats4[0] = st.steps; stats4[1] = st.slow_steps; stats4[2] = st.false_pos; stats4[3] = st.sequences; }
  return w.oob ? -1000 : io.r;
}

}  // namespace hostsim
