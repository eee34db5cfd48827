// tests/hostsim/hostsim_hcdict.cpp -- TEST INFRASTRUCTURE ONLY.
// The dictionary HC compressor's cores (lz4_hc_core.h: hc_dict_image_build, HcBuild<..., DICT = true>, HcParse<..., false, DICT =
// true>: LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream) compiled against the lock-step host backend, in a library of
// its own (tests/test_hcdict_hostsim.py).  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_hc_core.h"
#include "wave_host.h"

namespace {

// the host backend with two readable ranges -- the source and the dictionary's kept tail -- and one writable one
struct WaveHostH : hostsim::WaveHost {
  template <bool U16> using Entry = hostsim::WaveHost::Entry<U16>;
  const uint8_t* r_lo[2] = {nullptr, nullptr};
  const uint8_t* r_hi[2] = {nullptr, nullptr};
  void readable(int i, const uint8_t* p, size_t k) { r_lo[i] = p; r_hi[i] = p + k; }
  bool in_ok(const uint8_t* p, size_t k) {
    for (int i = 0; i < 2; i++) if (r_lo[i] && p >= r_lo[i] && p + k <= r_hi[i]) return true;
    oob = true;
    return false;
  }
  VU ld32(const uint8_t* b, const VU& i, const VB& m) {
    VU r; for (int l = 0; l < 64; l++) if (m.v[l] && in_ok(b + i.v[l], 4)) memcpy(&r.v[l], b + i.v[l], 4); return r;
  }
  VU ldu32(const uint8_t* b, const VU& i) { return ld32(b, i, VB(true)); }
  void copy(uint8_t* dst, uint32_t dpos, const uint8_t* src, uint32_t spos, uint32_t len) {
    if (len && in_ok(src + spos, len) && out_ok(dst + dpos, len)) memcpy(dst + dpos, src + spos, len);
  }
};

}  // namespace

extern "C" {

// the image of the kept tail [tail, tail + K): head[0 .. 32768) and ddelta[0 .. K); -1000 if the simulated wave read outside the tail
int sim_hc_dict_image(const uint8_t* tail, uint32_t K, uint32_t* head, uint16_t* ddelta, uint64_t rng_seed) {
  WaveHostH w;
  if (rng_seed) w.rng = rng_seed;
  w.readable(0, tail, K);
  lz4hip::hc_dict_image_build(w, tail, K, ddelta);
  memcpy(head, w.lds.data(), 32768u * sizeof(uint32_t));
  return w.oob ? -1000 : 0;
}

// LZ4_loadDictHC + LZ4_compress_HC_continue(src, dst, n, cap) at `level` on a fresh stream, as hc_build_dict_kernel +
// hc_parse_dict_kernel run it: the compressed size (0 = does not fit), or -1000 if the simulated wave read outside [src, src + n) and
// the tail or wrote outside [dst, dst + cap)
int sim_compress_hc_dict(const uint8_t* tail, uint32_t K, const uint32_t* head, const uint16_t* ddelta, const uint8_t* src, int n,
                         uint8_t* dst, int cap, int level, uint64_t rng_seed) {
  if (n < 0 || (uint32_t)n > 0x7E000000u || cap < 0) return 0;
  if (level < 1) level = 9;
  if (level > 12) level = 12;
  WaveHostH w;
  if (rng_seed) w.rng = rng_seed;
  w.bounds(src, (size_t)n, dst, (size_t)cap);
  w.readable(0, src, (size_t)n);
  w.readable(1, tail, K);
  memcpy(w.lds.data(), head, 32768u * sizeof(uint32_t));
  std::vector<uint16_t> delta((size_t)n + 8, 0xFFFF);
  lz4hip::HcBuild<WaveHostH, true>::run(w, src, (uint32_t)n, delta.data(), lz4hip::HC_BIAS + K);
  lz4hip::HcParse<WaveHostH, false, true> p(w, src, n, delta.data(), dst, cap, level);
  p.s.dend = tail + K;
  p.s.ddelta_end = ddelta + K;
  p.s.K = (int)K;
  std::vector<int> opt(level >= 10 ? (size_t)lz4hip::HC_OPT_INTS : 1u, 0x55555555);
  const int r = level >= 10 ? p.run_opt(level, opt.data()) : p.run();
  if (w.oob) return -1000;
  return r;
}

}  // extern "C"
