// tests/backend/probes.h -- TEST INFRASTRUCTURE ONLY (never part of liblz4hip.so).
//
// ONE probe source for both backends of the algorithm cores: tests/hostsim/hostsim_backend.cpp instantiates it with the lane
// simulator's WaveHost / GroupHost, tests/backend/devprobe.hip with csrc's WaveDev / GroupDev<GL> / BlockWaveDev<KW, KS>, and
// the tests compare the two output images byte for byte (tests/test_backend_hostsim.py, tests/test_gpu_backend.py; the case
// tables are tests/backend_cases.py).  Written the way the cores call the backends -- typename W::VU, W::select,
// g.template vcopy_run<PRED>(...) -- so that the same text compiles against either.
//
// A probe reads a case record (kRec words), the case's input slot and the launch's common image, calls one primitive or one
// short fixed sequence of primitives, and writes everything observable to the case's output slot.  Results held in registers
// leave through the backend's own stores (st_lanes, st_hdr, wv_read_al + wv_store).  What the backends do not offer comes from
// the harness type H of each instantiation: uni (a wave-uniform value as a scalar), put32 (one word to memory) and poison_stage / poison_wave
// (what the LDS bytes of a case hold before the probe: the simulator fills them with 0xEE, the device has to be told).
// No probe waits on memory that another wavefront writes: each is a bounded sequence over its own case.
#pragma once
#include <stdint.h>

#ifndef PROBE_FN
#define PROBE_FN inline
#endif

namespace probes {

constexpr uint32_t kRec = 64;        // words of a case record; r[0] is the operation
constexpr uint32_t kGuard = 64;      // bytes of 0xA5 on each side of an output slot's payload (the tests lay the slots out)

// ---- family A: the wave backend (wave_dev.h / wave_host.h) -----------------------------------------------------------------
// input slot: four lane vectors a, b, c, d (1024 bytes), then kWaveData bytes of data; output payload: four lane vectors
// O0..O3, two headers of four words, then (at kWaveOB) the bytes of the byte stores / the table dump (the tests size the slot)
constexpr uint32_t kWaveVec = 1024, kWaveData = 1152, kWaveHdr = 1024, kWaveOB = 1088;
constexpr uint32_t kWaveTable = 32768;   // the wave backend's match table ("32 KB table of this wavefront", wave_dev.h): 8192 / 4096 entries
enum WaveOp : uint32_t {
  W_BALLOT = 0, W_SHFL = 1, W_SHFL_E = 2, W_BCAST = 3, W_SETLANE = 4, W_ARITH = 5, W_ARITH2 = 6,
  W_LD = 10, W_LDU = 11, W_ST8 = 12, W_ST32 = 13, W_ST16 = 14, W_LANES = 15, W_COPY = 16,
  W_LDS_FILL = 20, W_LDS_WR = 21, W_LDS_MAX = 22,
};

template <class W, class H, bool U16>
PROBE_FN void wave_lds_probe(W& w, const uint32_t* r, const typename W::VU& a, const typename W::VU& b, const typename W::VU& c,
                             const typename W::VU& d, uint32_t* o32, uint32_t* dump) {
  using VU = typename W::VU;
  using E = typename W::template Entry<U16>;
  const uint32_t op = H::uni(r[0]), full = kWaveTable / (U16 ? 4u : 8u), ndump = H::uni(r[5]);
  typename E::S sval;
  typename E::V v;
  if constexpr (U16) { sval = H::uni(r[3]); v = a; }
  else { sval = (uint64_t)H::uni(r[3]) | ((uint64_t)H::uni(r[4]) << 32); v = W::u64(a) | (W::u64(d) << 32); }
  const auto wr = [&](uint32_t* p, const typename E::V& x) {   // an entry vector to memory: one word per lane, or two
    if constexpr (U16) W::st_lanes(p, x);
    else { W::st_lanes(p, W::lo32(x)); W::st_lanes(p + 64, W::lo32(x >> 32)); }
  };
  if (op == W_LDS_FILL) {
    w.template lds_fill<U16>(full, (typename E::S)0);
    W::sync();
    w.template lds_fill<U16>(H::uni(r[2]), sval);
  } else if (op == W_LDS_WR) {
    w.template lds_fill<U16>(full, sval);
    W::sync();
    w.template lds_wr<U16>(b, v, (c & VU(1u)) != VU(0u));      // (the case table gives the active lanes distinct slots)
    W::sync();
    wr(o32, w.template lds_rd<U16>(d, (c & VU(2u)) != VU(0u)));
    wr(o32 + 128, w.template lds_rdu<U16>(d));
  } else {   // W_LDS_MAX
    w.template lds_fill<U16>(full, sval);
    W::sync();
    wr(o32, w.template lds_max<U16>(b, v, (c & VU(1u)) != VU(0u)));
  }
  W::sync();
  for (uint32_t k = 0; k < ndump; k += 64u) {
    const auto e = w.template lds_rdu<U16>(W::lane() + VU(k));
    if constexpr (U16) W::st_lanes(dump + k, e);
    else { W::st_lanes(dump + 2u * k, W::lo32(e)); W::st_lanes(dump + 2u * k + 64, W::lo32(e >> 32)); }
  }
}

template <class W, class H>
PROBE_FN void wave_probe(W& w, const uint32_t* r, const uint8_t* in, uint8_t* out) {
  using VU = typename W::VU;
  using VU64 = typename W::VU64;
  const uint32_t* in32 = (const uint32_t*)in;
  uint32_t* o32 = (uint32_t*)out;
  uint32_t *O0 = o32, *O1 = o32 + 64, *O2 = o32 + 128, *O3 = o32 + 192, *H0 = o32 + kWaveHdr / 4u, *H1 = H0 + 4;
  uint8_t* OB = out + kWaveOB;
  const uint8_t* data = in + kWaveVec;
  const VU a = W::ld_lanes(in32), b = W::ld_lanes(in32 + 64), c = W::ld_lanes(in32 + 128), d = W::ld_lanes(in32 + 192);
  const VU64 x = W::u64(a) | (W::u64(d) << 32);
  const auto odd = (c & VU(1u)) != VU(0u);
  const uint32_t op = H::uni(r[0]), s2 = H::uni(r[2]), s3 = H::uni(r[3]), s4 = H::uni(r[4]);
  switch (op) {
    case W_BALLOT: {
      const uint64_t m = W::ballot((a & VU(1u)) != VU(0u)), m2 = (uint64_t)s2 | ((uint64_t)s3 << 32);
      W::st_hdr(H0, (uint32_t)m, (uint32_t)(m >> 32), 0u, 0u);
      W::st_lanes(O0, W::select(W::lanes(m2), a, b));
      W::st_lanes(O1, W::mbcnt(m2));
      const VU64 lt = W::lanemask_lt();
      W::st_lanes(O2, W::lo32(lt));
      W::st_lanes(O3, W::lo32(lt >> 32));
      break;
    }
    case W_SHFL:
      W::st_lanes(O0, W::excl_scan(a));
      W::st_lanes(O1, W::shfl(a, b));
      W::st_lanes(O2, W::shfl_up1(a));
      W::st_lanes(O3, W::shfl_down1(a));          // (lane 63 is unspecified: the tests leave it out)
      break;
    case W_SHFL_E: {
      const VU64 y = W::template shfl_e<false>(x, b);
      W::st_lanes(O0, W::lo32(y));
      W::st_lanes(O1, W::lo32(y >> 32));
      W::st_lanes(O2, W::template shfl_e<true>(a, b));
      break;
    }
    case W_BCAST: {
      const uint64_t q = W::bcast64(x, (int)s2), e = W::template bcast_e<false>(x, (int)s2);
      W::st_hdr(H0, W::bcast(a, (int)s2), (uint32_t)q, (uint32_t)(q >> 32), W::template bcast_e<true>(a, (int)s2));
      W::st_hdr(H1, (uint32_t)e, (uint32_t)(e >> 32), 0u, 0u);
      break;
    }
    case W_SETLANE:
      W::st_lanes(O0, W::set_lane(a, (int)s2, s3));
      W::st_lanes(O1, W::writelane(a, s3, s2));
      break;
    case W_ARITH:
      W::st_lanes(O0, W::alignbyte(a, b, c & VU(3u)));
      W::st_lanes(O1, W::div255(a));
      W::st_lanes(O2, W::shr(a, c));
      W::st_lanes(O3, W::vmin(a, b));
      break;
    case W_ARITH2:
      W::st_lanes(O0, W::vmax(a, b));
      W::st_lanes(O1, W::clz64(x));
      W::st_lanes(O2, W::ctz64v(x));
      W::st_lanes(O3, W::select(odd, a, b));
      break;
    case W_LD: {
      W::st_lanes(O0, w.ld8(data, b, odd));
      W::st_lanes(O1, w.ld32(data, b, odd));
      const VU64 y = w.ld64(data, b, odd);
      W::st_lanes(O2, W::lo32(y));
      W::st_lanes(O3, W::lo32(y >> 32));
      break;
    }
    case W_LDU: {
      W::st_lanes(O0, w.ldu8(data, b));
      W::st_lanes(O1, w.ldu32(data, b));
      const VU64 y = w.ldu64(data, b), z = w.ldu64_cand(data, d);
      W::st_lanes(O2, W::lo32(y));
      W::st_lanes(O3, W::lo32(y >> 32) ^ W::lo32(z) ^ W::lo32(z >> 32));
      W::st_hdr(H0, w.sld32(data, s2), 0u, 0u, 0u);
      break;
    }
    case W_ST8: w.st8(OB, b, a, odd); break;        // (the case table gives the active lanes distinct, non-overlapping targets)
    case W_ST32: w.st32(OB, b, a, odd); break;
    case W_ST16: w.st16((uint16_t*)OB, b, a, odd); break;
    case W_LANES: {
      uint32_t h0, h1, h2, h3;
      W::ld_hdr(in32 + s2, h0, h1, h2, h3);
      W::st_hdr(H0, h3, h2, h1, h0);
      W::st_lanes(O0, b);
      break;
    }
    case W_COPY: w.copy(OB, s2, data, s3, s4); break;
    default:
      if (H::uni(r[1])) wave_lds_probe<W, H, true>(w, r, a, b, c, d, o32, (uint32_t*)OB);
      else wave_lds_probe<W, H, false>(w, r, a, b, c, d, o32, (uint32_t*)OB);
      break;
  }
}

// ---- family B: the lane-group backend (group_dev.h GroupDev<GL> / group_host.h) -----------------------------------------
// dst: the case's destination (its address mod 128 is the case's), in: the case's source bytes, lds: the group's kStage bytes
enum GroupOp : uint32_t { G_MATCH = 0, G_MATCH_WIDE = 1, G_LITS = 2, G_LITS_WIDE = 3, G_SEQ = 4, G_STAGE = 5 };
enum StageOp : uint32_t { S_LITS = 0, S_MATCH = 1, S_FLUSH_LINES = 2, S_FLUSH_ALL = 3 };

template <class G, class H>
PROBE_FN void group_probe(G& g, const uint32_t* r, const uint8_t* in, uint8_t* dst, uint8_t* lds, uint32_t* fl_out) {
  const uint32_t op = H::uni(r[0]), p2 = r[2], p3 = r[3], p4 = r[4], p5 = r[5], p6 = r[6];
  switch (op) {
    case G_MATCH: g.copy_match(dst, p2, p3, p4, p5 != 0u); break;            // op, offset, len, wild
    case G_MATCH_WIDE: g.copy_match_wide(dst, p2, p3, p4); break;
    case G_LITS: g.copy_lits(dst + p2, in + p3, p4, p5 != 0u); break;          // op, source position, len, wild
    case G_LITS_WIDE: g.copy_lits_wide(dst + p2, in + p3, p4); break;
    case G_SEQ: {                                                              // op, source position, lit, distance, len
      typename G::SeqRegs R;
      g.seq_load(R, in + p3, p4, dst + p2 + p4 - p5, p6);
      g.seq_store(R, dst + p2, p4, p6);
      break;
    }
    default: {   // G_STAGE: a script of r[1] operations {kind, position, x, y} from r[8] on
      H::poison_stage(lds);
      g.st_begin(lds, p2);
      const uint32_t n = H::uni(r[1]);
      for (uint32_t k = 0; k < n; k++) {
        const uint32_t* s = r + 8u + 4u * k;
        const uint32_t kind = H::uni(s[0]);
        if (kind == S_LITS) g.st_lits(dst, s[1], in + s[2], s[3]);             // position, source position, len
        else if (kind == S_MATCH) g.st_match(dst, s[1], s[2], s[3]);           // position, offset, len
        else if (kind == S_FLUSH_LINES) g.st_flush_lines(dst, s[1]);
        else g.st_flush_all(dst, s[1]);
      }
      H::put32(fl_out, g.fl);
      break;
    }
  }
}

// ---- family C: the wave loop's backend (group_dev.h BlockWaveDev<KW, KS> / group_host.h in wave mode) ---------------------
// common image: [stream KS bytes][ring KW bytes][memory kFarMem bytes]; the rings are filled from it through the backend's own
// refill and piece stores.  input slot: five lane vectors.  dst: where ring coordinates wdb start (its address mod 256 is
// wdb); the ring is observed by wv_read_al + wv_store of every step with the case's [lo, hi) window.
constexpr uint32_t kFarMem = 8192 + 128;
enum BWaveOp : uint32_t { B_WALK = 0, B_LANEOPS = 1, B_LANE_RW = 2, B_GATHER = 3, B_WIN = 4, B_PUT = 5, B_RUN = 6 };

template <class W, class G, class H>
PROBE_FN void bwave_probe(G& g, const uint32_t* r, const uint8_t* common, const uint8_t* in, uint8_t* vec_out, uint8_t* dst,
                          uint8_t* lds) {
  using VU = typename G::VU;
  const uint32_t KW = g.wv_ring(), KS = g.wv_stream();
  const uint32_t* in32 = (const uint32_t*)in;
  uint32_t* o32 = (uint32_t*)vec_out;
  uint32_t *O0 = o32, *O1 = o32 + 64, *O2 = o32 + 128, *O3 = o32 + 192, *H0 = o32 + 256;
  const VU a = W::ld_lanes(in32), b = W::ld_lanes(in32 + 64), c = W::ld_lanes(in32 + 128), d = W::ld_lanes(in32 + 192),
           e = W::ld_lanes(in32 + 256);
  const uint32_t op = H::uni(r[0]), s2 = H::uni(r[2]), s3 = H::uni(r[3]), s4 = H::uni(r[4]);
  const VU lane = g.vlane();
  if (op == B_WALK) {
    VU posv = VU(0u), posp = VU(0u);
    uint32_t T = 0u, Tp = 0u;
    G::vwalk(a, posv, T);
    G::vwalk_par(a, lane, posp, Tp);
    W::st_lanes(O0, G::vsel(lane < VU(T), posv, VU(0xFFFFFFFFu)));       // lanes [0, T) of posv
    W::st_lanes(O1, G::vsel(lane < VU(Tp), posp, VU(0xFFFFFFFFu)));
    W::st_hdr(H0, T, Tp, 0u, 0u);
    return;
  }
  if (op == B_LANEOPS) {
    W::st_lanes(O0, G::vexcl_scan(a));
    W::st_lanes(O1, G::vshfl(a, b));
    W::st_lanes(O2, G::valignbyte(a, c, d & VU(3u)));
    W::st_lanes(O3, G::vmin(a, c));
    return;
  }
  if (op == B_LANE_RW) {
    W::st_hdr(H0, G::vreadlane(a, s2), G::vreadlane(c, s2), 0u, 0u);
    W::st_lanes(O0, G::vwritelane(a, s3, s2));
    W::st_lanes(O1, G::vsel(G::vlanes((uint64_t)s3 | ((uint64_t)s4 << 32)), a, c));
    const uint64_t m = G::vballot((a & VU(1u)) != VU(0u));
    W::st_hdr(H0 + 4, (uint32_t)m, (uint32_t)(m >> 32), 0u, 0u);
    return;
  }
  if (op == B_GATHER) {   // vgather8 (the pointer doubling's gather; no core calls it by itself): every q of the 256-byte table a
    for (uint32_t q = 0; q < 256u; q += 4u)
      W::st_hdr(o32 + q, G::vgather8(a, q), G::vgather8(a, q + 1u), G::vgather8(a, q + 2u), G::vgather8(a, q + 3u));
    return;
  }
  // the ring probes: both rings filled from the common image, as a decode fills them
  const uint8_t* stream = common;
  const uint8_t* ring0 = common + KS;
  const uint8_t* mem = common + KS + KW;
  g.wv_begin(lds, dst);
  H::poison_wave(lds);
  for (uint32_t pos = 0; pos < KS; pos += 256u) g.rs_put(pos, g.rs_fetch(stream, pos));
  for (uint32_t fw = 0; fw < KW; fw += 256u) g.wv_put(fw, g.wv_get_mem(ring0 + fw, fw));
  if (op == B_WIN) {
    VU lo = VU(0u), hi = VU(0u);
    g.vs_win(s2, lo, hi);
    W::st_lanes(O0, lo);
    W::st_lanes(O1, hi);
    W::st_lanes(O2, g.vs_ld32(b));
    const uint64_t q = g.rs_ld64(s2);
    W::st_hdr(H0, (uint32_t)q, (uint32_t)(q >> 32), 0u, 0u);
    return;
  }
  if (op == B_PUT) {             // source kind, source position, destination ring index
    if (s2 == 0u) g.wv_put(s4, g.wv_get_stream(s3, s4));
    else if (s2 == 1u) g.wv_put(s4, g.wv_get_ring(s3, s4));
    else g.wv_put(s4, g.wv_get_mem(mem + s3, s4));
  } else {                       // B_RUN: dw = a, sp = b, len = c, mpos = d, from_stream = e; r[1] PRED, r[2..3] gom, r[4..5] farm, r[6] tier
    const uint64_t gom = (uint64_t)s2 | ((uint64_t)s3 << 32), farm = (uint64_t)s4 | ((uint64_t)H::uni(r[5]) << 32);
    const uint64_t oddm = g.vodd_mask(a, c);
    const uint32_t tier = H::uni(r[6]);
    W::st_hdr(H0, (uint32_t)oddm, (uint32_t)(oddm >> 32), G::vrun_tier(c, gom), 0u);
    if (H::uni(r[1])) g.template vcopy_run<true>(a, e != VU(0u), b, c, gom, mem, d, farm, oddm, tier);
    else g.template vcopy_run<false>(a, e != VU(0u), b, c, gom, mem, d, farm, oddm, tier);
  }
  // the observer: one more run, lane 1 alone, 16 bytes from the ring's last byte on -- read in one piece, that is the ring's last byte
  // and the first 15 bytes of the MIRROR behind its end (which no aligned read of the dump below would see) -- to the ring's middle
  {
    const VU odw = VU(KW / 2u), olen = VU(16u);
    g.template vcopy_run<false>(odw, VU(0u) != VU(0u), VU(KW - 1u), olen, 2ull, mem, VU(0u), 0ull, g.vodd_mask(odw, olen), 4u);
  }
  const uint32_t lo = H::uni(r[13]), hi = H::uni(r[14]);
  for (uint32_t fw = 0; fw < KW; fw += 256u) g.wv_store(dst, fw, g.wv_read_al(fw), lo, hi);
}

// what tests/backend_cases.py restates, for the tests to check (STAGE: the backend's own kStage)
template <uint32_t STAGE>
inline void constants(uint32_t* out8) {
  const uint32_t v[8] = {kRec, kGuard, kWaveVec, kWaveData, kWaveOB, kFarMem, STAGE, kWaveTable};
  for (int i = 0; i < 8; i++) out8[i] = v[i];
}

}  // namespace probes
