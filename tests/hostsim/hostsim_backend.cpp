// tests/hostsim/hostsim_backend.cpp -- TEST INFRASTRUCTURE ONLY.
// The HOST instantiation of tests/backend/probes.h: every probe on the lane simulator's backends (wave_host.h, group_host.h), for
// ctypes.  tests/backend/devprobe.hip is the same probes on the device backends; the slot layouts below are its layouts too.
// Besides the output image each entry returns the backend's oob flag per case.
//
// One deliberately wrong variant per family, each behind a switch of its own, shows that the comparison sees a difference
// (tests/test_backend_hostsim.py builds them; wave_host.h / group_host.h stay as they are):
//   -DBACKEND_WRONG_SCAN       family A: the prefix sum made inclusive
//   -DBACKEND_WRONG_REPLICATE  family B: the replicate copy without r = l % offset
//   -DBACKEND_WRONG_MIRROR     family C: a piece store that leaves the mirror copy out
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "group_host.h"
#include "../backend/probes.h"

namespace {

struct HostHarness {
  static uint32_t uni(uint32_t x) { return x; }
  static void put32(uint32_t* p, uint32_t v) { *p = v; }
  static void poison_stage(uint8_t*) {}   // (st_begin / wv_begin fill the simulator's LDS bytes with 0xEE themselves)
  static void poison_wave(uint8_t*) {}
};

struct WaveProbed : hostsim::WaveHost {
#ifdef BACKEND_WRONG_SCAN
  static VU excl_scan(const VU& a) { VU r; uint32_t acc = 0; for (int l = 0; l < 64; l++) { acc += a.v[l]; r.v[l] = acc; } return r; }
#endif
};

struct GroupProbed : hostsim::GroupHost {
  using hostsim::GroupHost::GroupHost;
#ifdef BACKEND_WRONG_REPLICATE
  void copy_match(uint8_t* dst, uint32_t op, uint32_t offset, uint32_t len, bool wild) {
    if ((wild && offset >= 4u * GL) || offset == 0) { hostsim::GroupHost::copy_match(dst, op, offset, len, wild); return; }
    uint8_t* d = dst + op;
    const uint8_t* m = d - offset;
    uint32_t r[64];
    for (int l = 0; l < GL; l++) r[l] = (uint32_t)l;      // (group_host.h: l < offset ? l : l % offset)
    const uint32_t stp = (uint32_t)GL < offset ? (uint32_t)GL : (uint32_t)GL % offset;
    for (uint32_t base = 0; base < len; base += GL) {
      uint8_t v[64]; bool act[64];
      for (int l = 0; l < GL; l++) { uint32_t i = base + l; act[l] = i < len; v[l] = 0; if (act[l] && rd_ok(m + r[l], 1)) v[l] = m[r[l]]; }
      for (int l = 0; l < GL; l++) {
        uint32_t i = base + l;
        if (act[l] && wr_ok(d + i, 1)) d[i] = v[l];
        r[l] += stp; if (r[l] >= offset) r[l] -= offset;
      }
    }
  }
#endif
#ifdef BACKEND_WRONG_MIRROR
  void wv_put(uint32_t w, const WPiece& c) {
    for (int l = 0; l < GL; l++) {
      const uint32_t t = (w + 4u + c.dl[l]) & (kWv - 1u);
      if (rl_ok((wrb - 4) + t, 4)) memcpy((wrb - 4) + t, c.b[l], 4);
    }
  }
#endif
};

// the images are copied to 256-byte aligned memory: a destination's address mod 128 / mod 256 is part of a case
struct Aligned {
  uint8_t* p;
  uint8_t* user;
  size_t n;
  Aligned(uint8_t* u, size_t bytes) : p((uint8_t*)aligned_alloc(256, (bytes + 255u) & ~(size_t)255u)), user(u), n(bytes) { memcpy(p, u, n); }
  ~Aligned() { memcpy(user, p, n); free(p); }
};

const uint32_t kWaveCfg[4][2] = {{8192, 1024}, {16384, 2048}, {32768, 2048}, {65536, 2048}};   // decode_wave.hip's launch table

}  // namespace

extern "C" {

void hb_constants(uint32_t* out8) { probes::constants<hostsim::GroupHost::kStage>(out8); }

// family A.  output slot: [64 guard | payload | 64 guard]
int hb_wave(const uint32_t* rec, int n, const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride, uint8_t* oob) {
  WaveProbed w;
  for (int i = 0; i < n; i++) {
    w.oob = false;
    uint8_t* pay = out + (size_t)i * out_stride + probes::kGuard;
    w.bounds(in + (size_t)i * in_stride, in_stride, pay, out_stride - 2u * probes::kGuard);
    probes::wave_probe<WaveProbed, HostHarness>(w, rec + (size_t)i * probes::kRec, in + (size_t)i * in_stride, pay);
    oob[i] = w.oob;
  }
  return 0;
}

// family B.  output slot (256-byte aligned): dst = slot + 128 + r[7] (r[7] = its address mod 128), r[8 .. ) the staging script;
// dst's capacity is out_stride - 384; the word at slot + out_stride - 128 takes fl; everything else stays 0xA5
int hb_group(int gl, const uint32_t* rec, int n, const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride, uint8_t* oob) {
  Aligned img(out, (size_t)n * out_stride);
  for (int i = 0; i < n; i++) {
    const uint32_t* r = rec + (size_t)i * probes::kRec;
    uint8_t* slot = img.p + (size_t)i * out_stride;
    uint8_t* dst = slot + 128 + r[7];
    GroupProbed g(gl, in + (size_t)i * in_stride, (long)in_stride, dst, (long)(out_stride - 384u));
    probes::group_probe<GroupProbed, HostHarness>(g, r, in + (size_t)i * in_stride, dst, nullptr, (uint32_t*)(slot + out_stride - 128u));
    oob[i] = g.oob;
  }
  return 0;
}

// family C.  output slot (256-byte aligned): five lane vectors + headers at slot + 256, the ring's image at slot + 1792 (only when
// out_stride has room for it: the lane-parallel probes run with small slots); dst = that + r[15] (= wdb)
int hb_bwave(int cfg, const uint32_t* rec, int n, const uint8_t* common, size_t common_size, const uint8_t* in, size_t in_stride,
             uint8_t* out, size_t out_stride, uint8_t* oob) {
  Aligned img(out, (size_t)n * out_stride);
  const uint32_t KW = kWaveCfg[cfg][0], KS = kWaveCfg[cfg][1];
  for (int i = 0; i < n; i++) {
    const uint32_t* r = rec + (size_t)i * probes::kRec;
    uint8_t* slot = img.p + (size_t)i * out_stride;
    uint8_t* dump = slot + 1792;
    GroupProbed g(64, common, (long)common_size, dump, out_stride >= 1792u + KW + 64u ? (long)KW : 0l);
    g.kWv = KW; g.kWs = KS;
    probes::bwave_probe<hostsim::WaveHost, GroupProbed, HostHarness>(g, r, common, in + (size_t)i * in_stride, slot + 256, dump + (r[15] & 255u), nullptr);
    oob[i] = g.oob;
  }
  return 0;
}

}  // extern "C"
