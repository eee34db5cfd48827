// tests/hostsim/hostsim_dictc.cpp -- TEST INFRASTRUCTURE ONLY.
// The dictionary compressor's core (lz4_fast_core.h, FastCore<..., DICT = true>: LZ4_loadDict + LZ4_compress_fast_continue) and its
// table-image builder (dict_image_build) compiled against the lock-step host backend, in a library of its own
// (tests/test_dictc_hostsim.py).  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/kernels.h"
#include "../../lz4-java_amd/csrc/lz4_fast_core.h"
#include "wave_host.h"
#include "block_host.h"

namespace {

// the host backend with three readable ranges -- the source, the dictionary's kept tail, the table image -- and two writable ones
struct WaveHostD : hostsim::WaveHost {
  template <bool U16> using Entry = hostsim::WaveHost::Entry<U16>;
  const uint8_t* r_lo[3] = {nullptr, nullptr, nullptr};
  const uint8_t* r_hi[3] = {nullptr, nullptr, nullptr};
  uint8_t* w_lo[2] = {nullptr, nullptr};
  uint8_t* w_hi[2] = {nullptr, nullptr};
  void readable(int i, const uint8_t* p, size_t k) { r_lo[i] = p; r_hi[i] = p + k; }
  void writable(int i, uint8_t* p, size_t k) { w_lo[i] = p; w_hi[i] = p + k; }
  bool in_ok(const uint8_t* p, size_t k) {
    for (int i = 0; i < 3; i++) if (r_lo[i] && p >= r_lo[i] && p + k <= r_hi[i]) return true;
    oob = true;
    return false;
  }
  bool out_ok(const uint8_t* p, size_t k) {
    for (int i = 0; i < 2; i++) if (w_lo[i] && p >= w_lo[i] && p + k <= w_hi[i]) return true;
    oob = true;
    return false;
  }
  VU ld8(const uint8_t* b, const VU& i, const VB& m) {
    VU r; for (int l = 0; l < 64; l++) if (m.v[l] && in_ok(b + i.v[l], 1)) r.v[l] = b[i.v[l]]; return r;
  }
  VU ld32(const uint8_t* b, const VU& i, const VB& m) {
    VU r; for (int l = 0; l < 64; l++) if (m.v[l] && in_ok(b + i.v[l], 4)) memcpy(&r.v[l], b + i.v[l], 4); return r;
  }
  VU64 ld64(const uint8_t* b, const VU& i, const VB& m) {
    VU64 r; for (int l = 0; l < 64; l++) if (m.v[l] && in_ok(b + i.v[l], 8)) memcpy(&r.v[l], b + i.v[l], 8); return r;
  }
  VU ldu8(const uint8_t* b, const VU& i) { return ld8(b, i, VB(true)); }
  VU ldu32(const uint8_t* b, const VU& i) { return ld32(b, i, VB(true)); }
  VU64 ldu64(const uint8_t* b, const VU& i) { return ld64(b, i, VB(true)); }
  VU64 ldu64_cand(const uint8_t* b, const VU& i) { return ld64(b, i, VB(true)); }
  uint32_t sld32(const uint8_t* b, uint32_t i) { uint32_t v = 0; if (in_ok(b + i, 4)) memcpy(&v, b + i, 4); return v; }
  void st8(uint8_t* b, const VU& i, const VU& v, const VB& m) {
    for (int l = 0; l < 64; l++) if (m.v[l] && out_ok(b + i.v[l], 1)) b[i.v[l]] = (uint8_t)v.v[l];
  }
  void st32(uint8_t* b, const VU& i, const VU& v, const VB& m) {
    for (int l = 0; l < 64; l++) if (m.v[l] && out_ok(b + i.v[l], 4)) memcpy(b + i.v[l], &v.v[l], 4);
  }
  void copy(uint8_t* dst, uint32_t dpos, const uint8_t* src, uint32_t spos, uint32_t len) {
    if (len && in_ok(src + spos, len) && out_ok(dst + dpos, len)) memcpy(dst + dpos, src + spos, len);
  }
};

// the block as the shell sees it (block_host.h), with the tail and the image readable as well
struct BlockHostD : hostsim::BlockHost {
  using hostsim::BlockHost::BlockHost;
  const uint8_t* tail = nullptr; uint32_t keep = 0; const uint8_t* image = nullptr;
  void begin_block(WaveHostD& w, const uint8_t* s, uint32_t len, uint8_t* d, uint32_t room) {
    w.readable(0, s, len);
    if (keep) { w.readable(1, tail, keep); w.readable(2, image, 32768); }
    w.writable(0, d, room);
  }
};

}  // namespace

extern "C" {

// what LZ4_loadDict keeps of a dictionary of `len` bytes, as the library computes it
uint32_t sim_dict_keep(int len) { return lz4hip::dict_keep(len); }

// the table image of the kept tail [tail, tail + keep), keep >= 8, into image[0 .. 32768); -1000 if the simulated wave touched memory
// outside the tail / the image
int sim_dict_image(const uint8_t* tail, uint32_t keep, uint8_t* image, uint64_t rng_seed) {
  WaveHostD w;
  if (rng_seed) w.rng = rng_seed;
  w.readable(0, tail, keep);
  w.writable(0, image, 32768);
  lz4hip::dict_image_build(w, tail, keep, image);
  return w.oob ? -1000 : 0;
}

// FastForm<.., DICT>'s block through the shell (fast_block_run; compress_fast_dict_cu_kernel keeps a copy of its own, see there):
// returns compressed size (0 = does not fit), or -1000 if the simulated wave read outside [src, src+n), the tail and the image, or
// wrote outside [dst, dst+cap).  keep == 0: no dictionary (tail and image unused)
int sim_compress_fast_dict(const uint8_t* tail, uint32_t keep, const uint8_t* image, const uint8_t* src, int n, uint8_t* dst, int cap,
                           uint64_t* stats4, uint64_t rng_seed) {
  WaveHostD w;
  BlockHostD io(src, n, dst, cap);
  io.x.dict = io.tail = tail; io.x.keep = io.keep = keep; io.x.image = io.image = image;
  return hostsim::sim_fast_block<lz4hip::FastForm<WaveHostD, false, false, true, true>>(w, io, stats4, rng_seed);
}

}  // extern "C"
