// lz4_fast_core.h -- wave-parallel, bit-exact LZ4 fast compressor (one 64-lane wavefront per block).
//
// Replaces, for the "HIP" family, what LZ4JNICompressor.compress reaches through the JNI shim:
// LZ4_compress_default (/root/reference/src/jni/net_jpountz_lz4_LZ4JNI.c:75), liblz4 1.9.3,
// acceleration 1, noDict; byU16 table for n < 65547, byU32 otherwise.
// Output is byte-identical to liblz4's.
//
// Why this is not a port: liblz4 walks one position at a time through a 16 KB table of positions.
// Here a wavefront evaluates 64 probe positions per step:
//   * the probe positions of a miss-run are a closed-form sequence of the run start (the skip
//     heuristic "64 probes per step increment"), so lane j computes its own position;
//   * the LDS table stores {position, 16-bit fingerprint of the 4 bytes at that position}; a lane is
//     a *tentative* hit iff the fingerprints agree, so candidate bytes (in HBM/L2, never staged) are
//     only fetched for the first tentative lane -- one global read per sequence instead of one per
//     probe;
//   * lanes up to the first tentative hit commit their inserts with one LDS atomic-max (positions
//     only ever grow, so "max" == "latest insert wins", independent of lane order inside the
//     instruction).  The value returned by the atomic reveals intra-step bucket collisions; those
//     (rare) steps are undone and resolved exactly with ballots;
//   * the two post-match table operations of liblz4 (insert ip-2, probe ip) become two extra lanes
//     in front of the next run's probes;
//   * catch-up, match length and the token/length/literal/offset stream are produced with ballots
//     and per-lane byte stores.
//
// The code is written against a "wave" backend W (wave_dev.h on the GPU; tests/hostsim/wave_host.h
// is a lock-step 64-lane simulator used ONLY by the CPU test-suite to run this very source).
// Rule: per-lane values have type W::VU / VU64 / VB; control flow branches only on wave-uniform
// scalars (ballots, broadcasts).
#pragma once
// developer probe builds only: a byU16 table of 2^LZ4HIP_PROBE_HLOG entries (13 = liblz4's; anything else is NOT bit-exact and
// exists to measure residency: 12 -> 16 KB tables, ten wavefronts per CU)
#ifndef LZ4HIP_PROBE_HLOG
#define LZ4HIP_PROBE_HLOG 13
#endif
// fingerprint bits kept per byU16 table entry (16 = the {pos16, fp16} u32 entries; narrower values exist to measure the
// false-tentative-hit cost of smaller tables: any width is bit-exact, a false tentative hit is ruled out by its candidate bytes)
#ifndef LZ4HIP_FP_BITS
#define LZ4HIP_FP_BITS 16
#endif
#define LZ4HIP_FP_MASK ((1u << LZ4HIP_FP_BITS) - 1u)
#include <stdint.h>
#include <stddef.h>
#include "kernels.h"   // BatchArgs

#ifndef LZ4HIP_DEV
#if defined(__HIPCC__)
#define LZ4HIP_DEV __device__ __forceinline__
#else
#define LZ4HIP_DEV inline
#endif
#endif
#ifndef LZ4HIP_COLD
#if defined(__HIPCC__)
#define LZ4HIP_COLD __device__ __forceinline__   /* (out-of-line calls measured 1.6x SLOWER: stack traffic around the call sites) */
#else
#define LZ4HIP_COLD inline
#endif
#endif
#define LZ4HIP_LIKELY(x) __builtin_expect(!!(x), 1)
#define LZ4HIP_UNLIKELY(x) __builtin_expect(!!(x), 0)

namespace lz4hip {

LZ4HIP_DEV int ctz64(uint64_t x) { return __builtin_ctzll(x); }
LZ4HIP_DEV int popc64(uint64_t x) { return __builtin_popcountll(x); }

struct FastStats {  // optional counters (host simulator / profiling kernel); the product kernel passes nullptr
  uint64_t steps, slow_steps, false_pos, sequences;
  uint64_t t[8];  // shader-clock cycles per phase of a step (profiling kernel only), see run()
};

// ---------------------------------------------------------------------------------------------------
// Output policies.  The match finder (FastCore) hands every sequence to an `Out`:
//   DirectOut  writes the LZ4 stream itself; a sequence found in step t is written in step t+1, after step
//              t+1 has issued its candidate loads, so the stores overlap that latency;
//   ParkOut    (lz4_fast_v2_core.h) parks {match start, length, offset} one lane per sequence and writes 64 at a time.
// (A third policy, descriptors pushed to a ring drained by a second wavefront, measured 8 % slower than DirectOut in round 1
// and was removed.)
// DirectOut<W, FILL = true> is liblz4's fillOutput (LZ4_compress_destSize): `cap` is the target size t.  The parse is the default
// one; only emission and termination differ.  A sequence that fails liblz4's literal check stops the block with the last literals
// starting at its literal start; one that fails the match check is written with a shortened match (6 bytes of room are left, a
// further sequence needs 11) and stops the block after it; the last literals are then truncated to fit.  `consumed` is the input
// that the output covers.  t >= compressBound(n) is `limited` false: the default bytes, all of the input.
// ---------------------------------------------------------------------------------------------------
template <class W, bool FILL = false>
struct DirectOut {
  using VU = typename W::VU;
  using VU64 = typename W::VU64;
  using VB = typename W::VB;
  static constexpr bool kUsesWindowRegs = true;

  W& w;
  const uint8_t* src;
  uint32_t n;
  uint8_t* dst;
  uint32_t cap;
  bool limited;
  uint32_t op = 0;
  uint32_t consumed = 0;     // (FILL) input bytes the output covers, once the block is done
  uint32_t stop_anchor = 0;  // (FILL) where the last literals start after a stop

  LZ4HIP_DEV DirectOut(W& w_, const uint8_t* s, uint32_t n_, uint8_t* d, uint32_t cap_) : w(w_), src(s), n(n_), dst(d), cap(cap_) {
    limited = cap < n + n / 255u + 16u;
  }

  // ---- small output helpers ---------------------------------------------------------------
  LZ4HIP_DEV static uint32_t ext_count(uint32_t len) { return len >= 15u ? (len - 15u) / 255u + 1u : 0u; }

  // writes `cnt` bytes of the 255-run encoding of (len-15) at dst[o..): 255,...,255,rem
  LZ4HIP_DEV void put_ext(uint32_t o, uint32_t len, uint32_t cnt) {
    const uint32_t rem = (len - 15u) - 255u * (cnt - 1u);
    for (uint32_t base = 0; base < cnt; base += 64u) {
      VU i = w.lane() + base;
      w.st8(dst, i + o, W::select(i == cnt - 1u, VU(rem), VU(255u)), i < cnt);
    }
  }

  LZ4HIP_DEV void put_ext_at(uint32_t o, uint32_t len, uint32_t cnt) { put_ext(o, len, cnt); }

  // last literals: token + run + raw bytes; returns total size or 0 (FILL: the run is truncated to fit instead)
  LZ4HIP_COLD uint32_t emit_last(uint32_t anchor) {
    uint32_t last = n - anchor;
    if (limited && (uint64_t)op + last + 1u + (last + 255u - 15u) / 255u > cap) {
      if constexpr (!FILL) return 0;
      last = cap - op - 1u;             // (op < cap: a stop leaves at least 6 bytes, the start at least 1)
      last -= (last + 256u - 15u) / 256u;
    }
    if constexpr (FILL) consumed = anchor + last;
    const uint32_t nlx = ext_count(last);
    w.st8(dst, VU(op), VU((last < 15u ? last : 15u) << 4), w.lane() == 0u);
    if (nlx) put_ext(op + 1u, last, nlx);
    w.copy(dst, op + 1u + nlx, src, anchor, last);
    return op + 1u + nlx + last;
  }

  // ---- deferred emission ---------------------------------------------------------------------
  // A sequence found in step t is written out in step t+1, AFTER step t+1 has issued its own
  // candidate loads: the token/literal/offset stores then overlap the HBM/L2 latency of those loads.
  struct Pending {
    bool have = false, check_lits = false, regs = false;
    uint32_t lit = 0, mc = 0, offset = 0, anchor = 0;
  };
  Pending pend;
  VU pend_b0;  // regs: lane l (>= 1) holds literal l-1 of the pending sequence (byte 0 of its window word)

  LZ4HIP_DEV bool emit_pending() {
    if (!pend.have) return true;
    pend.have = false;
    const uint32_t lit = pend.lit, mc = pend.mc, offset = pend.offset;
    const uint32_t token = ((lit < 15u ? lit : 15u) << 4) | (mc < 15u ? mc : 15u);
    // (FILL: no check can fire while op + 72 <= cap -- regs means at most 63 bytes and at most one match-length byte)
    if (LZ4HIP_LIKELY(pend.regs && (!limited || (FILL && op + 72u <= cap)))) {
      // The common case, branch-free, ONE store instruction, no cross-lane traffic (regs implies at most one length byte
      // each and total <= 63: no division, no loop): lane 0 writes the token; lane l >= 1 writes output byte l + nlx, so
      // the literal it needs (literal l-1) is byte 0 of its own window word; when a literal-length byte exists (nlx == 1)
      // the otherwise idle lane 63 writes it at index 1; bytes past the literals come from the 3-byte trailer word
      // {offset, ml-15}.
      const uint32_t nlx = lit >= 15u ? 1u : 0u, nmx = mc >= 15u ? 1u : 0u;
      const uint32_t off0 = 1u + nlx + lit, total = off0 + 2u + nmx;
      const uint32_t trl = offset | ((mc - 15u) << 16);  // third byte only used when nmx == 1
      const VU i = w.lane();
      const VB ext_lane = (i == 63u) & VB(nlx != 0u);
      const VU oi = W::select(ext_lane, VU(1u), W::select(i == 0u, VU(0u), i + nlx));
      const VU tb = W::shr(VU(trl), ((oi - off0) * 8u) & 31u) & 0xFFu;  // garbage for oi < off0 (never selected)
      VU b = W::select(oi >= off0, tb, pend_b0);
      b = W::select(i == 0u, VU(token), b);
      b = W::select(ext_lane, VU(lit - 15u), b);
      w.st8(dst, oi + op, b, (oi < total));
      op += total;
      return true;
    }
    return emit_checked(lit, mc, offset, token);
  }

  // everything else: a limited output buffer (liblz4's two capacity checks), literals that are not in the window registers,
  // long length runs
  LZ4HIP_COLD bool emit_checked(uint32_t lit, uint32_t mc, uint32_t offset, uint32_t token) {
    const uint32_t nlx = ext_count(lit);
    if constexpr (FILL) {
      if (limited) {
        // liblz4's fillOutput checks: the literal check (it also covers the _next_match check of a sequence without literals)
        if ((uint64_t)op + 1u + nlx + lit + 11u > cap) { stop_anchor = pend.anchor; return false; }
        const uint32_t p = op + 1u + nlx + lit + 2u;   // output position after the offset (p + 9 <= cap here)
        if ((uint64_t)p + 6u + (mc + 240u) / 255u > cap) {
          // the match description does not fit: shortened to what leaves exactly 6 bytes (never longer than mc), then stop
          const uint32_t mcs = 14u + (cap - p - 6u) * 255u;
          const uint32_t nms = ext_count(mcs);
          emit_generic(lit, mcs, offset, nlx, nms, (token & 0xF0u) | (mcs < 15u ? mcs : 15u), 1u + nlx + lit + 2u + nms);
          op += 1u + nlx + lit + 2u + nms;
          stop_anchor = pend.anchor + lit + 4u + mcs;
          return false;
        }
      }
    }
    const uint32_t nmx = ext_count(mc);
    if (!FILL && limited) {
      if (pend.check_lits && (uint64_t)op + 1u + lit + (2u + 1u + 5u) + lit / 255u > cap) return false;
      if ((uint64_t)op + 1u + nlx + lit + 2u + (1u + 5u) + (mc + 240u) / 255u > cap) return false;
    }
    const uint32_t total = 1u + nlx + lit + 2u + nmx;
    emit_generic(lit, mc, offset, nlx, nmx, token, total);
    op += total;
    return true;
  }

  // sequences whose literals are not in the window registers, or that need more than 63 bytes / long length runs
  LZ4HIP_COLD void emit_generic(uint32_t lit, uint32_t mc, uint32_t offset, uint32_t nlx, uint32_t nmx, uint32_t token, uint32_t total) {
    const VU i = w.lane();
    if (total <= 64u) {
      const uint32_t lit0 = 1u + nlx, off0 = lit0 + lit;
      VU b = w.ld8(src, i + (pend.anchor - lit0), (i >= lit0) & (i < off0));
      b = W::select(i == 0u, VU(token), b);
      if (nlx) {
        const uint32_t rem = (lit - 15u) - 255u * (nlx - 1u);
        b = W::select((i >= 1u) & (i < lit0), W::select(i == nlx, VU(rem), VU(255u)), b);
      }
      b = W::select(i == off0, VU(offset & 255u), b);
      b = W::select(i == off0 + 1u, VU(offset >> 8), b);
      if (nmx) {
        const uint32_t rem = (mc - 15u) - 255u * (nmx - 1u);
        b = W::select(i >= off0 + 2u, W::select(i == total - 1u, VU(rem), VU(255u)), b);
      }
      w.st8(dst, i + op, b, i < total);
    } else {
      w.st8(dst, VU(op), VU(token), i == 0u);
      if (nlx) put_ext(op + 1u, lit, nlx);
      w.copy(dst, op + 1u + nlx, src, pend.anchor, lit);
      const uint32_t o2 = op + 1u + nlx + lit;
      w.st8(dst, i + o2, W::select(i == 0u, VU(offset & 255u), VU(offset >> 8)), i < 2u);
      if (nmx) put_ext(o2 + 2u, mc, nmx);
    }
  }


  // ---- the Out interface ----
  LZ4HIP_DEV bool overlap_point() { return emit_pending(); }
  LZ4HIP_DEV void seq(uint32_t lit, uint32_t mc, uint32_t offset, uint32_t anchor, bool check_lits, bool regs, VU b0) {
    pend.have = true;
    pend.lit = lit;
    pend.mc = mc;
    pend.offset = offset;
    pend.anchor = anchor;
    pend.check_lits = check_lits;
    pend.regs = regs;
    pend_b0 = b0;
  }
  LZ4HIP_DEV uint32_t last(uint32_t anchor) {
    if (!emit_pending()) return stop();
    return emit_last(anchor);
  }
  // what a stop (overlap_point() or the pending sequence of last() returned false) makes of the block: 0 = it does not fit;
  // FILL: the last literals from the stop anchor, truncated to fit -- not from the finder's anchor, which is one step further on
  LZ4HIP_DEV uint32_t stop() {
    if constexpr (FILL) return emit_last(stop_anchor);
    else return 0u;
  }
};
// the result of FastCore at a stop of its output policy: 0 (did not fit) except for DirectOut's fill mode
template <class O> LZ4HIP_DEV uint32_t out_stop(O&) { return 0u; }
template <class W, bool FILL> LZ4HIP_DEV uint32_t out_stop(DirectOut<W, FILL>& o) { return o.stop(); }

// flag / mask of a packed literal length (lz4_fast_ms_core.h): bit 29 = liblz4's _next_match path (no literal-capacity check)
constexpr uint32_t SEQ_NOCHECK = 1u << 29, SEQ_LIT_MASK = (1u << 29) - 1u;

// PK (byU32 blocks of at most 4 MiB only -- the largest block of the LZ4 Frame format and its default in the reference's
// LZ4FrameOutputStream): the 4096 entries are 32 bits, {position (22 bits), fingerprint (10 bits)}, 16 KB instead of 32 -- twice the
// match-finder chains per CU (compress_fast.hip, compress_fast_v2w8_cu_kernel).  A narrower fingerprint only means more tentative hits that
// their candidate bytes rule out; what is accepted and what the table holds are liblz4's at any width.
// ACC: LZ4_compress_fast(..., acceleration) -- every miss-run starts with searchMatchNb = accel << 6 instead of 1 << 6, so probe k
// of a run sits at S + g_a(k) (see g_acc); `accel` (>= 1, clamped by the caller) is read only then.  Its steps no longer sit on
// consecutive positions beyond the first two probes, so literals always come from the source, never from the window registers.
// ACC = false is the acceleration-1 core every other kernel runs, unchanged.
// ACC with LINK, and with LINK + DICT (XLINK): LZ4_compress_fast_continue(..., acceleration) on a chain or a running stream
// (lz4_fast_chain.h, the *_accel walks).  Nothing else in those branches knows where a run's probes sit: the candidate bounds (lowidx,
// ibase, alias_hi, the 65535 distance), locate and cand_load work on one probe's position and entry.  (ACC with DICT alone -- the
// dictionary-handle form -- is not built.)
// DICT: LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream, liblz4's external-dictionary mode (byU32 at every size, 64-bit
// entries).  The table holds INDEXES: block position p is kDictBase + p, byte j of the dictionary's kept tail (its last `keep` <= 64 KB
// bytes) is kDictBase - keep + j, so a dictionary candidate is an index below kDictBase.  The table starts as the image LZ4_loadDict
// leaves (dict_image_build below) instead of cleared, position 0 is inserted explicitly, and a candidate must also lie at or above
// kDictBase - keep (liblz4's dictSmall check; it is what rejects the empty entries, index 0).  The candidate side of every comparison
// reads the tail or the source, whichever the index names: the buffer (cs, cn) is chosen per hit (locate).  A dictionary match that
// runs to the dictionary's end goes on against the block's own start.  Nothing outside the tail and [src, src + n) is read.
// DICT = false compiles to what it did before the switch existed.
// a form's own state: what the block shell (end of this file) gives a core before run(), and reads after it
struct FastBlockArgs {
  uint32_t accel = 1;                                                                // ACC: 2 .. 65537
  const uint8_t* dict = nullptr; uint32_t keep = 0; const uint8_t* image = nullptr;  // DICT: FastCore's fields; keep == 0: no dictionary
  uint32_t dense64 = 0; bool bailed = false; FastStats* st = nullptr;                // SIM: the density probe and what it did; counters
};
// (the DICT core's extra state lives in a base of its own, so that every other core is the struct it was)
template <bool DICT> struct DictState {
  // never read: the names exist so that the `if constexpr (DICT)` branches parse
  static constexpr const uint8_t* dict = nullptr; static constexpr const uint8_t* image = nullptr; static constexpr const uint8_t* cs = nullptr;
  static constexpr uint32_t keep = 0, cn = 0;
  static constexpr bool cdict = false;
};
template <> struct DictState<true> {
  // set by the caller before run(): the kept tail [dict, dict + keep), keep = 0 or 8 .. 65536, and the table image of
  // dict_image_build (4096 entries; nullptr with keep == 0)
  const uint8_t* dict = nullptr;
  uint32_t keep = 0;
  const uint8_t* image = nullptr;
  // the buffer the current candidate lives in -- the tail or the source -- and its length
  const uint8_t* cs = nullptr;
  uint32_t cn = 0;
  bool cdict = false;
};
// LINK: one block of a chain of linked blocks (LZ4_compress_fast_continue in liblz4's prefix mode; lz4_fast_chain.h walks the chain).
// `src` is the start of the chain's kept history and every position is a position in that one buffer: the block is [blk, n), the
// blocks and the history in front of it are [0, blk).  byU32 with 64-bit entries at every size; the table holds INDEXES, position p is
// ibase + p, and it is the caller's: it lives from one block of the chain to the next (link_table_init before the first block that
// probes).  A candidate must lie at or above `lowidx` (liblz4's dictSmall check; past 64 KB of history the distance check implies it)
// and within 65535 bytes; it is read from the same buffer, so a match may start in front of the block and run into it, and the
// catch-up may go back to position 0.  Position blk is inserted and never probed; mflimit and matchlimit come from n, and nothing at or
// past n is read.  LINK = false compiles to what it did before the switch existed (the state lives in a base of its own, as DictState).
template <bool LINK> struct LinkState { static constexpr uint32_t blk = 0, ibase = 0, lowidx = 0, alias_hi = 0; };
template <> struct LinkState<true> { uint32_t blk = 0, ibase = 0, lowidx = 0, alias_hi = 0; };
// LINK and DICT together: one block of a RUNNING stream in liblz4's external-dictionary mode (LZ4_compress_fast_continue on a source that
// does not follow its history; lz4_fast_chain.h cxstream_walk).  It is the DICT core with the stream's own numbers in the place of
// LZ4_loadDict's: `src` is the block, block position p is index ibase + p (ibase: the stream's index position, a run-time value where
// DICT alone has kDictBase), the history [dict, dict + keep) lies elsewhere and holds the indexes [lowidx, ibase), keep = ibase - lowidx
// (0: no history, and `dict` is not looked at), and the table is the caller's running one -- nothing is loaded or cleared here, `image`
// is unused.  blk stays 0.  alias_hi (0: off): the caller's mark that the block's bytes overlap the history's (a source written over
// the ring it came from): the fingerprint of an entry below alias_hi was taken from bytes that may be gone, so such an entry is a
// tentative hit whatever its fingerprint says, and its candidate bytes, as they are now, decide -- as liblz4's compare of them does.
template <class W, bool U16, class Out = DirectOut<W>, bool PK = false, bool ACC = false, bool DICT = false, bool LINK = false>
struct FastCore : DictState<DICT>, LinkState<LINK> {
  static_assert(!(U16 && PK), "compact entries are a byU32 layout");
  static_assert(!DICT || (!U16 && !PK && (!ACC || LINK)), "the dictionary core is byU32 with 64-bit entries; acceleration 1 unless it is a running stream's (XLINK)");
  static_assert(!LINK || (!U16 && !PK), "the linked-block core is byU32 with 64-bit entries");
  static constexpr bool XLINK = LINK && DICT;     // a running stream's block against a history that lies elsewhere
  static constexpr uint32_t kDictBase = 65536u;   // DICT: index of block position 0 (the stream's offset after LZ4_loadDict)
  static constexpr bool S32 = U16 || PK;           // entries are 32 bits
  static constexpr uint32_t kPackMaxN = 1u << 22;  // PK: positions have 22 bits
  using VU = typename W::VU;
  using VU64 = typename W::VU64;
  using VB = typename W::VB;
  using E = typename W::template Entry<S32>::S;   // scalar table entry (uint32_t / uint64_t)
  using VE = typename W::template Entry<S32>::V;  // per-lane table entry
  static constexpr int HLOG = U16 ? LZ4HIP_PROBE_HLOG : 12;
  static constexpr int PSHIFT = U16 ? 16 : (PK ? 10 : 32);
  static constexpr uint32_t FPM = PK ? 0x3FFu : 0xFFFFu;   // fingerprint bits of an entry
  static constexpr uint32_t MAXD = 65535u;
#ifndef LZ4HIP_SPEC_LANES
#define LZ4HIP_SPEC_LANES 16
#endif
  static constexpr uint32_t kSpecLanes = LZ4HIP_SPEC_LANES;  // lanes (x 8 bytes) of the speculative verify + extension compare

  W& w;
  Out& out;
  const uint8_t* src;
  uint32_t n;
  uint32_t anchor = 0;
  uint32_t mfl1, matchlimit;  // mflimitPlusOne = n-11, matchlimit = n-5
  FastStats* st;
  // Density probe (0 = off): if sequences 32..95 of the block cover fewer than `dense64` input bytes, the block is made of
  // short sequences -- the window-parallel core (lz4_fast_ms_core.h) is the faster one for it; loop() then stops with
  // `bailed` set and the caller leaves the block to that core.
  uint32_t dense64 = 0;
  uint32_t accel = 1;   // (ACC only) liblz4's acceleration, 1 .. 65537
  bool bailed = false, probe_done = false, one_done = false;
  uint32_t p_S = 0, p_ip = 0;
  using DictState<DICT>::dict; using DictState<DICT>::keep; using DictState<DICT>::image;
  using DictState<DICT>::cs; using DictState<DICT>::cn; using DictState<DICT>::cdict;
  using LinkState<LINK>::blk; using LinkState<LINK>::ibase; using LinkState<LINK>::lowidx; using LinkState<LINK>::alias_hi;
  // DICT: the index of block position 0
  LZ4HIP_DEV uint32_t dbase() const { if constexpr (XLINK) return ibase; else return kDictBase; }

  LZ4HIP_DEV FastCore(W& w_, Out& out_, const uint8_t* s, uint32_t n_, FastStats* st_ = nullptr)
      : w(w_), out(out_), src(s), n(n_), st(st_) {
    mfl1 = n - 11u;
    matchlimit = n - 5u;
  }
  template <bool SIM> LZ4HIP_DEV void setup(const FastBlockArgs& x) {   // (SIM: see FastForm)
    if constexpr (ACC) accel = x.accel;
    if constexpr (DICT) {
      if (x.keep) { dict = x.dict; keep = x.keep; image = x.image; }
    }
    if constexpr (SIM) dense64 = x.dense64;
  }

  // ---- table entry helpers ---------------------------------------------------------------
  LZ4HIP_DEV static VE mk_entry(VU pos, VU fp) {
    if constexpr (S32) return (pos << PSHIFT) | fp;
    else return (W::u64(pos) << 32) | W::u64(fp);
  }
  LZ4HIP_DEV static VU e_pos(VE e) {
    if constexpr (S32) return e >> PSHIFT;
    else return W::lo32(e >> 32);
  }
  LZ4HIP_DEV static VU e_fp(VE e) {
    if constexpr (S32) return e & FPM;
    else return W::lo32(e) & 0xFFFFu;
  }
  // byU32 fingerprint of the four bytes x (byU16 entries take theirs out of the bucket product)
  LZ4HIP_DEV static VU fp32(VU x) {
    if constexpr (PK) return ((x * 2654435761u) >> 16) & FPM;
    else return (x * 2654435761u) >> 16;
  }
  LZ4HIP_DEV static uint32_t se_pos(E e) { return (uint32_t)(e >> PSHIFT); }
  // candidate side of a comparison: the source itself unless DICT
  LZ4HIP_DEV const uint8_t* cbase() const { if constexpr (DICT) return cs; else return src; }
  LZ4HIP_DEV uint32_t climit() const { if constexpr (DICT) return cn; else return n; }
  // where the forward count of a hit stops: matchlimit unless DICT (locate)
  LZ4HIP_DEV uint32_t flimit(uint32_t lim) const { if constexpr (DICT) return lim; else return matchlimit; }
  // DICT: where the candidate of index `idx` lives.  Chooses (cs, cn), returns the candidate's offset in that buffer -- which is also how
  // far a catch-up may go back: to the tail's start or to the block's -- and sets `lim`, where a forward count from hpos stops: matchlimit,
  // or the dictionary's end.  (A tentative hit passed the lower-bound check, and LZ4_loadDict inserts only positions with 8 bytes behind
  // them.)  Without a hit the speculative loads read the block's start.
  LZ4HIP_DEV uint32_t locate(bool have_hit, uint32_t idx, uint32_t hpos, uint32_t& lim) {
    lim = matchlimit;
    if constexpr (XLINK) {   // the same with the stream's own index base
      cdict = have_hit && idx < ibase;
      if (cdict) {
        cs = dict; cn = keep;
        const uint32_t dl = ibase - idx;
        if (hpos + dl < lim) lim = hpos + dl;
        return idx - lowidx;
      }
      cs = src; cn = n;
      return have_hit ? idx - ibase : 0u;
    }
    cdict = have_hit && idx < kDictBase;
    if (cdict) {
      cs = dict; cn = keep;
      const uint32_t dl = kDictBase - idx;
      if (hpos + dl < lim) lim = hpos + dl;
      return idx - (kDictBase - keep);
    }
    cs = src; cn = n;
    return have_hit ? idx - kDictBase : 0u;
  }

  // XLINK: the speculative candidate fetch.  A running stream's history may be 4 .. 7 bytes long (LZ4_loadDict's 8-byte minimum is not
  // LZ4_saveDict's, and a stream may jump behind its first few bytes); its one possible candidate is its first byte -- index 0, the
  // empty buckets' entry while the lower bound is 0: every inserted position has 8 bytes and more behind it -- of which liblz4 reads four.
  // So do we: one 32-bit load inside the history in every lane (no lane is `full` there: the forward count stops at the history's end,
  // which count_tail reaches byte by byte).  From 8 bytes on, DICT's clamped 8-byte loads.
  LZ4HIP_DEV VU64 cand_load(VU o8s, uint32_t mpos) {
    if (LZ4HIP_UNLIKELY(cn < 8u)) return W::u64(w.ldu32(cs, VU(mpos + 4u <= cn ? mpos : cn - 4u)));
    return w.ldu64_cand(cs, W::vmin(o8s + mpos, cn - 8u));
  }

  // probe k of a miss-run starting at S sits at S + g(k): liblz4's `step = searchMatchNb++ >> 6`
  LZ4HIP_DEV static VU g(VU k) {
    VU T = k + 62u;
    VU M = T >> 6;
    return W::select(k >= 1u, VU(1u), VU(0u)) + 32u * M * (M - 1u) + M * (T - 64u * M + 1u);
  }
  // ACC: searchMatchNb starts at accel << 6, so every step after the first is accel - 1 longer: g_a(0) = 0, g_a(k) = g(k) + (a-1)(k-1).
  // (u32 throughout: a probe that is still valid has g(k) <= n and (a-1)(k-1) <= n, the 64 lanes of a step add < 64 * (a + k/64))
  LZ4HIP_DEV VU g_acc(VU k) const {
    if constexpr (ACC) return g(k) + W::select(k >= 1u, k - 1u, VU(0u)) * (accel - 1u);
    else return g(k);
  }

  // ---- match extension ------------------------------------------------------------------------
  // tail of a forward count: lane granularity ran into `limit`; at most 7 bytes are left to compare
  LZ4HIP_COLD uint32_t count_tail(uint32_t pa_t, uint32_t pb_t, uint32_t limit) {
    const uint32_t tail = pa_t < limit ? limit - pa_t : 0u;
    if (tail == 0) return 0;
    const VB act = w.lane() < tail;
    const VU ca = w.ld8(src, w.lane() + pa_t, act);
    const VU cb = w.ld8(cbase(), w.lane() + pb_t, act);
    const uint64_t bad = w.ballot(act & (ca != cb));
    return bad ? (uint32_t)ctz64(bad) : tail;
  }

  // number of equal bytes src[a+i]==src[b+i], a+i < limit (b < a); 8 bytes per lane, 512 per round
  LZ4HIP_COLD uint32_t count_fwd(uint32_t a, uint32_t b, uint32_t limit) {
    uint32_t cnt = 0;
    for (;;) {
      const VU off = w.lane() * 8u + cnt;
      const VU pa = off + a;
      const VB full = pa + 8u <= limit;
      const VU64 x = w.ldu64(src, W::vmin(pa, n - 8u)) ^ w.ldu64(cbase(), W::vmin(off + b, climit() - 8u));
      const VB diff = full & (x != VU64(0));
      const uint64_t dm = w.ballot(diff);
      const uint64_t stop = dm | w.ballot(!full);
      if (stop == 0) { cnt += 512u; continue; }
      const int f = ctz64(stop);
      cnt += 8u * (uint32_t)f;
      if ((dm >> f) & 1u) return cnt + (uint32_t)(ctz64(w.bcast64(x, f)) >> 3);
      return cnt + count_tail(a + cnt, b + cnt, limit);
    }
  }

  // catch-up beyond the first 64 bytes (rare): equal bytes before (ip, m), bounded by maxback
  LZ4HIP_COLD uint32_t count_back(uint32_t ip, uint32_t m, uint32_t maxback) {
    uint32_t back = 0;
    while (back < maxback) {
      const VU jj = w.lane() + back;
      const VB act = jj < maxback;
      const VU ca = w.ld8(src, (ip - 1u) - jj, act);
      const VU cb = w.ld8(cbase(), (m - 1u) - jj, act);
      const uint64_t am = w.ballot(act);
      const uint64_t bad = w.ballot(act & (ca != cb));
      if (bad) return back + (uint32_t)ctz64(bad);
      back += (uint32_t)popc64(am);
    }
    return back;
  }

  // ---- per-step inputs, prepared one step ahead so the window load overlaps bookkeeping ----------
  VU sp_pos;      // position of each of the 64 slots
  uint64_t sp_validm = 0, sp_probem = 0;  // lane masks (wave-uniform scalars): slot is valid / slot probes the table
  VU64 sp_x64;    // window word at the slot position (U32 mode: 8 bytes; U16 mode: low 4 bytes used)
  VU sp_x32;

  LZ4HIP_DEV void prepare_step(bool post, uint32_t S, uint32_t r, uint32_t ip) {
    const VU j = w.lane();
    const uint32_t nspecial = post ? 2u : 0u;
    const VB sp_isrun = j >= nspecial;
    const VU k = j - nspecial + r;
    VU prun, pnext;
    // probes 0..65 of a run are consecutive (ACC: only probes 0 and 1, and a step has more lanes than that)
    if (!ACC && LZ4HIP_LIKELY(r + 64u - nspecial <= 65u)) { prun = k + S; pnext = prun + 1u; }
    else { prun = g_acc(k) + S; pnext = g_acc(k + 1u) + S; }
    sp_pos = W::select(sp_isrun, prun, W::select(j == 0u, VU(ip - 2u), VU(ip)));
    // special lanes (0,1 of a post step) are always valid; lane 0 of a post step only inserts
    sp_validm = w.ballot(pnext <= mfl1) | (uint64_t)(post ? 3u : 0u);
    sp_probem = sp_validm & ~(uint64_t)(post ? 1u : 0u);
    // invalid lanes read a clamped, harmless address: no exec-mask branch around the load
    if constexpr (U16) sp_x32 = w.ldu32(src, W::vmin(sp_pos, n - 8u));
    else sp_x64 = w.ldu64(src, W::vmin(sp_pos, n - 8u));
  }

  // ---- the compressor ------------------------------------------------------------------------
  LZ4HIP_DEV uint32_t run() {
    if constexpr (LINK && !DICT) {
      anchor = blk;
      if (n - blk < 13u) return out.last(blk);  // all literals; nothing is inserted (an empty block: the single token 0x00)
      // liblz4's first insert, the block's first position (8 bytes are there: the block has 13)
      const VU64 x0 = w.ldu64(src, VU(blk));
      const VU h0 = W::lo32(((x0 << 24) * 889523592379ull) >> (64 - HLOG));
      (void)w.template lds_max<S32>(h0, mk_entry(VU(blk + ibase), fp32(W::lo32(x0))), w.lane() == 0u);
      w.sync();
      return loop<0>(false, blk + 1u, 0u, 0u);
    }
    if (n < 13u) return out.last(0u);  // all literals (n == 0: the single token 0x00)
    if constexpr (DICT) {
      // the table as LZ4_loadDict leaves it (no image: no dictionary, every entry empty = index 0, which the lower-bound check
      // rejects), then liblz4's first insert, position 0
      // (XLINK: the table is the stream's running one, as the block before left it)
      if constexpr (!XLINK) {
        if (image) {
          for (uint32_t i = 0; i < (1u << HLOG); i += 64u) {
            const VU h = w.lane() + i;
            w.template lds_wr<S32>(h, w.ldu64(image, h * 8u), VB(true));
          }
        } else {
          w.template lds_fill<S32>(1u << HLOG, (E)0);
        }
        w.sync();
      }
      const VU64 x0 = w.ldu64(src, VU(0u));
      const VU h0 = W::lo32(((x0 << 24) * 889523592379ull) >> (64 - HLOG));
      (void)w.template lds_max<S32>(h0, mk_entry(VU(dbase()), fp32(W::lo32(x0))), w.lane() == 0u);
      w.sync();
      return loop<0>(false, 1u, 0u, 0u);
    }

    // every bucket starts as {pos 0, fp(bytes at 0)}: liblz4's zeroed table makes position 0 the
    // candidate of an empty bucket, and its explicit first insert (position 0) is then implied.
    uint32_t fp0;
    {
      const uint32_t x0 = w.sld32(src, 0);
      if constexpr (U16) fp0 = ((x0 * 2654435761u) >> 3) & LZ4HIP_FP_MASK;
      else fp0 = ((x0 * 2654435761u) >> 16) & FPM;
    }
    w.template lds_fill<S32>(1u << HLOG, (E)fp0);
    w.sync();
    if (dense64 == 0u) return loop<0>(false, 1u, 0u, 0u);
    // density probe: a second copy of the loop counts the first 96 sequences, so the main loop stays untouched
    const uint32_t res = loop<1>(false, 1u, 0u, 0u);
    if (!probe_done) return res;   // the block ended (or ran out of output) before the probe did
    if (bailed) return 0u;
    return loop<0>(true, p_S, 0u, p_ip);
  }

  // the step loop from a given parser state (also entered mid-block by lz4_fast_ms_core.h when it hands a block over):
  //   post: step kind: false = run probes only; true = {insert ip-2, probe ip, run from ip+1}
  //   S, r: run start, index of the first run probe of this step;  ip: post-match position (== anchor) when post
  //   MODE: 0 = to the end of the block; 1 = density probe (see dense64); 2 = ONE sequence: returns 0 with `one_done` set and
  //         p_ip = the post-match position once a sequence has been handed to `out` (lz4_fast_v2_core.h uses this loop as the
  //         exact path for the steps its lean loop does not handle), or the block's result if the block ended first
  template <int MODE>
  LZ4HIP_DEV uint32_t loop(bool post, uint32_t S, uint32_t r, uint32_t ip) {
    constexpr bool PROBE = MODE == 1, ONE = MODE == 2;
    uint32_t probe_cd = 32u, probe_anchor = 0;  // (PROBE only) countdown to the next density-probe event
    uint32_t pf_end = PROBE ? 0u : (post ? ip : S) & ~(W::kPrefetchBytes - 1u);  // source prefetched up to here (LZ4HIP_PF_KB KB chunks, as far ahead)
    // the next chunk is due once hpos + kPrefetchBytes > pf_end, i.e. hpos >= pf_trig (never again once pf_end >= n): ONE compare per step
    uint32_t pf_trig = (n >= 16u && pf_end < n) ? (pf_end >= W::kPrefetchBytes ? pf_end - W::kPrefetchBytes + 1u : 0u) : 0xFFFFFFFFu;
    const VU j = w.lane();
    const VU o8 = j * 8u;
    const VU o8s = W::vmin(o8, VU(8u * (kSpecLanes - 1u)));
    prepare_step(post, S, r, ip);

    for (;;) {
      if (st) st->steps++;
      uint64_t tk = st ? w.tick(0u) : 0;
#define LZ4HIP_PHASE(i, dep) do { if (st) { const uint64_t t_ = w.tick(dep); st->t[i] += t_ - tk; tk = t_; } } while (0)
      // ---- [1] this step's slots were prepared (and their window words requested) one step ahead ----
      const VU pos = sp_pos;
      const uint64_t validm = sp_validm, probem = sp_probem;
      VU x32, h, fp;
      if constexpr (U16) {
        x32 = sp_x32;
        const VU prod = x32 * 2654435761u;
        h = prod >> (32 - HLOG);
        fp = (prod >> 3) & LZ4HIP_FP_MASK;
      } else {
        x32 = W::lo32(sp_x64);
        h = W::lo32(((sp_x64 << 24) * 889523592379ull) >> (64 - HLOG));
        fp = fp32(x32);
      }
      LZ4HIP_PHASE(0, w.bcast(h, 0));   // t[0]: input window arrived + hash
      // ---- [2] table lookup, tentative hits, commit ----
      const VE e = w.template lds_rdu<S32>(h);
      const VE newe = mk_entry(LINK ? pos + ibase : (DICT ? pos + kDictBase : pos), fp);
      // (ballots of plain compares are free -- the compare already writes the lane mask; the masks are combined on the scalar side)
      uint64_t tmask = w.ballot(e_fp(e) == fp) & probem;
      if constexpr (XLINK) tmask = (tmask | (w.ballot(e_pos(e) < alias_hi) & probem)) & w.ballot(e_pos(e) + MAXD >= pos + ibase) & w.ballot(e_pos(e) >= lowidx);
      else if constexpr (DICT) tmask &= w.ballot(e_pos(e) + MAXD >= pos + kDictBase) & w.ballot(e_pos(e) >= kDictBase - keep);
      else if constexpr (LINK) tmask &= w.ballot(e_pos(e) + MAXD >= pos + ibase) & w.ballot(e_pos(e) >= lowidx);
      else if constexpr (!U16) tmask &= w.ballot(e_pos(e) + MAXD >= pos);
      const uint64_t imask = ~validm;
      uint32_t k0 = tmask ? (uint32_t)ctz64(tmask) : 64u;
      const uint32_t kinv = imask ? (uint32_t)ctz64(imask) : 64u;
      uint32_t ncommit = (k0 + 1u < kinv) ? k0 + 1u : kinv;
      bool have_hit = ncommit == k0 + 1u;   // == (k0 < kinv), as a 32-bit equality (the 64-bit ctz results have no scalar "<")
      uint64_t inm = ncommit >= 64u ? ~0ull : ((1ull << ncommit) - 1ull);  // lanes that commit their insert
      LZ4HIP_PHASE(1, ncommit);          // t[1]: table read + ballots
      const VE old = w.template lds_max<S32>(h, newe, w.lanes(inm));

      // ---- [3] speculative candidate fetch: verify + forward + backward extension in ONE round trip.
      // Branch-free: without a tentative hit the loads still go out (lane 0's slot vs position 0, L1 hits). ----
      const uint32_t kk = have_hit ? k0 : 0u;
      uint32_t hpos = w.bcast(pos, (int)kk);
      uint32_t mpos = se_pos(w.template bcast_e<S32>(e, (int)kk));
      [[maybe_unused]] uint32_t midx = 0u, lim = 0u;   // DICT: the candidate's index (mpos becomes its offset in cs); where the forward count stops
      if constexpr (DICT) { midx = mpos; mpos = locate(have_hit, midx, hpos, lim); }
      if constexpr (LINK && !DICT) mpos -= ibase;   // (without a hit: any value, the loads below are clamped)
      bool hit_post = post && k0 == 1u;
      uint32_t maxback = (!have_hit || hit_post) ? 0u : ((hpos - anchor) < mpos ? (hpos - anchor) : mpos);
      // (only the first kSpecLanes lanes take part -- 8 bytes each: the candidate side is a random re-read of the block and
      // every further 128 bytes are one more cache line that mostly misses L2; longer matches take count_fwd's extra round trip)
      // (lanes past kSpecLanes repeat the last taking lane's address: same cache line, no exec-mask region around the loads)
      VU64 fa = w.ldu64(src, W::vmin(o8s + hpos, n - 8u));   // kept apart from fb: xor-ing here would wait for the loads
      VU64 fb;
      if constexpr (XLINK) fb = cand_load(o8s, mpos);
      else fb = w.ldu64_cand(cbase(), W::vmin(o8s + mpos, climit() - 8u));
      VU ba, bb;
      uint64_t bactm = maxback >= 64u ? ~0ull : ((1ull << maxback) - 1ull);
      {
        const VB bact = w.lanes(bactm);
        // (opaque index: keeps the {scalar base + 32-bit lane offset} form; the optimiser otherwise folds the subtraction into a
        // 64-bit address per lane)
        ba = w.ldu8(src, W::opaque(W::select(bact, (hpos - 1u) - j, VU(0u))));
        bb = w.ldu8(cbase(), W::opaque(W::select(bact, (mpos - 1u) - j, VU(0u))));
      }
      if (LZ4HIP_UNLIKELY(hpos >= pf_trig)) {
        w.prefetch4k(src, pf_end, n);
        pf_end += W::kPrefetchBytes;
        pf_trig = pf_end < n ? pf_end - W::kPrefetchBytes + 1u : 0xFFFFFFFFu;
      }
      LZ4HIP_PHASE(2, hpos);             // t[2]: commit issue + candidate-fetch issue

      // ---- [4] write out the previous sequence while those loads are in flight ----
      if (!out.overlap_point()) return out_stop(out);
      LZ4HIP_PHASE(3, hpos);             // t[3]: emission of the previous sequence

      // ---- [5] intra-step bucket collisions (rare): undo, resolve exactly, commit again ----
      const uint64_t det = w.ballot(old != e) & inm;
      if (LZ4HIP_UNLIKELY(det != 0)) {
        if (st) st->slow_steps++;
        const VB inrange = w.lanes(inm);
        w.template lds_wr<S32>(h, e, inrange);
        w.sync();
        VE se = e;  // candidate each lane sees under sequential semantics
        uint64_t pendm = det;
        while (pendm) {
          const int d = ctz64(pendm);
          const uint32_t hd = w.bcast(h, d);
          const VB grp = inrange & (h == hd);
          const uint64_t gm = w.ballot(grp);
          const VU64 lower = w.lanemask_lt() & VU64(gm);
          const VB has = grp & (lower != VU64(0));
          const VU srcl = VU(63u) - W::clz64(lower);
          const VE pe = w.template shfl_e<S32>(newe, srcl);
          se = W::select(has, pe, se);
          pendm &= ~gm;
        }
        uint64_t t2 = w.ballot(e_fp(se) == fp) & inm & probem;
        if constexpr (XLINK) t2 = (t2 | (w.ballot(e_pos(se) < alias_hi) & inm & probem)) & w.ballot(e_pos(se) + MAXD >= pos + ibase) & w.ballot(e_pos(se) >= lowidx);
        else if constexpr (DICT) t2 &= w.ballot(e_pos(se) + MAXD >= pos + kDictBase) & w.ballot(e_pos(se) >= kDictBase - keep);
        else if constexpr (LINK) t2 &= w.ballot(e_pos(se) + MAXD >= pos + ibase) & w.ballot(e_pos(se) >= lowidx);
        else if constexpr (!U16) t2 &= w.ballot(e_pos(se) + MAXD >= pos);
        const bool had = have_hit;
        const uint32_t hpos_old = hpos, mpos_old = mpos;
        [[maybe_unused]] const uint32_t midx_old = midx;
        if (t2) {
          k0 = (uint32_t)ctz64(t2);
          ncommit = k0 + 1u;
          have_hit = true;
        } else {
          have_hit = false;  // the tentative lane (if any) no longer matches under the sequential candidates
        }
        inm = ncommit >= 64u ? ~0ull : ((1ull << ncommit) - 1ull);
        (void)w.template lds_max<S32>(h, newe, w.lanes(inm));
        if (have_hit) {
          hpos = w.bcast(pos, (int)k0);
          mpos = se_pos(w.template bcast_e<S32>(se, (int)k0));
          if constexpr (DICT) { midx = mpos; mpos = locate(true, midx, hpos, lim); }
          if constexpr (LINK && !DICT) mpos -= ibase;
          if (!had || hpos != hpos_old || (DICT ? midx != midx_old : mpos != mpos_old)) {  // the speculation fetched the wrong candidate
            hit_post = post && k0 == 1u;
            maxback = hit_post ? 0u : ((hpos - anchor) < mpos ? (hpos - anchor) : mpos);
            fa = w.ldu64(src, W::vmin(o8s + hpos, n - 8u));
            if constexpr (XLINK) fb = cand_load(o8s, mpos);
            else fb = w.ldu64_cand(cbase(), W::vmin(o8s + mpos, climit() - 8u));
            bactm = maxback >= 64u ? ~0ull : ((1ull << maxback) - 1ull);
            const VB bact = w.lanes(bactm);
            ba = w.ldu8(src, W::select(bact, (hpos - 1u) - j, VU(0u)));
            bb = w.ldu8(cbase(), W::select(bact, (mpos - 1u) - j, VU(0u)));
          }
        }
      }
      w.sync();  // table updates of this step are ordered before the next step's reads
      LZ4HIP_PHASE(4, (uint32_t)det);    // t[4]: atomic result + collision handling

      // ---- [6] verify the tentative hit (4 bytes) ----
      const VU64 fx = fa ^ fb;
      const bool hit = have_hit & ((uint32_t)w.bcast64(fx, 0) == 0u);   // (no short circuit: one branch, and the likely side falls through)
      if (st && have_hit && !hit) st->false_pos++;
      LZ4HIP_PHASE(5, (uint32_t)hit);    // t[5]: wait for the candidate bytes
      if (LZ4HIP_UNLIKELY(!hit)) {
        if (!have_hit && kinv < 64u && kinv == ncommit) return out.last(anchor);  // liblz4's `goto _last_literals`
        // continue the run after the last committed lane
        if (post) { S = ip + 1u; r = ncommit >= 2u ? ncommit - 2u : 0u; post = false; }
        else r += ncommit;
        prepare_step(post, S, r, ip);
        continue;
      }

      // ---- [7] a match at hpos against mpos: forward length first -- it alone decides where the next step starts ----
      if (st) st->sequences++;
      uint32_t cnt;  // equal bytes from hpos on (>= 4)
      {
        constexpr uint64_t specm = (1ull << kSpecLanes) - 1ull;
        const uint64_t fullm = w.ballot(o8 + (hpos + 8u) <= flimit(lim));
        const VU64 xz = W::select(j == 0u, fx & VU64(0xFFFFFFFF00000000ull), fx);
        const uint64_t dm = w.ballot(xz != VU64(0)) & fullm & specm;
        const uint64_t stop = dm | (~fullm & specm);
        if (LZ4HIP_UNLIKELY(stop == 0)) {
          cnt = 8u * kSpecLanes + count_fwd(hpos + 8u * kSpecLanes, mpos + 8u * kSpecLanes, flimit(lim));
        } else {
          const int f = ctz64(stop);
          cnt = 8u * (uint32_t)f;
          if (LZ4HIP_LIKELY((dm >> f) & 1u)) cnt += (uint32_t)(ctz64(w.bcast64(xz, f)) >> 3);
          else if (cnt >= 4u) cnt += count_tail(hpos + cnt, mpos + cnt, flimit(lim));
          else cnt = 4u + count_tail(hpos + 4u, mpos + 4u, flimit(lim));  // lane 0 itself straddles the limit
        }
      }
      if constexpr (DICT) {
        // the match ran to the dictionary's end: liblz4 goes on comparing against the block's own start, up to matchlimit
        if (cdict && lim < matchlimit && hpos + cnt == lim) {
          cs = src; cn = n;
          cnt += count_fwd(lim, 0u, matchlimit);
          cs = dict; cn = keep;   // (the catch-up below is on the dictionary side again)
        }
      }
      const uint32_t ip_new = hpos + cnt;
      const VU b0 = x32 & 0xFFu;         // literal bytes of this step (before the slots are re-prepared)
      const bool was_post = post;
      const bool done = ip_new >= mfl1;
      if (!done && !ONE) {                // request the next step's window NOW; the rest of the bookkeeping overlaps it
        post = true;
        S = ip_new + 1u;
        r = 0;
        ip = ip_new;
        prepare_step(true, S, 0u, ip_new);
      }
      // ---- [8] catch-up, pending-sequence record ----
      uint32_t back = 0;
      if (maxback) {
        const uint64_t bad = w.ballot(ba != bb) & bactm;
        if (bad) back = (uint32_t)ctz64(bad);
        else if (LZ4HIP_LIKELY(maxback <= 64u)) back = maxback;
        else back = 64u + count_back(hpos - 64u, mpos - 64u, maxback - 64u);
      }
      const uint32_t mc = back + (cnt - 4u);
      {
        const uint32_t lit = (hpos - back) - anchor;
        // literals straight from this step's window registers: lane l (>= 1) of a post step sits on position
        // anchor + l - 1 (its run started in this step); needs at most one length byte each and lane 63 free
        // (ACC: lane l >= 4 sits further on -- the literals come from the source)
        const bool regs = !ACC && Out::kUsesWindowRegs && was_post && mc < 270u &&
                          (1u + (lit >= 15u ? 1u : 0u) + lit + 2u + (mc >= 15u ? 1u : 0u) <= 63u);
        if constexpr (DICT) out.seq(lit, mc, (hpos + dbase()) - midx, anchor, !hit_post, regs, b0);
        else out.seq(lit, mc, hpos - mpos, anchor, !hit_post, regs, b0);
      }
      anchor = ip_new;
      LZ4HIP_PHASE(6, ip_new);           // t[6]: match length + catch-up + bookkeeping
      if (done) return out.last(anchor);
      if constexpr (ONE) {
        one_done = true;
        p_ip = ip_new;
        return 0u;
      }
      if constexpr (PROBE) {
        if (--probe_cd == 0u) {
          if (probe_anchor == 0u) { probe_anchor = anchor; probe_cd = 64u; }
          else {  // sequence 96 done: the next step is a post step at ip_new
            if (!out.overlap_point()) return out_stop(out);
            probe_done = true;
            bailed = anchor - probe_anchor < dense64;
            p_S = S; p_ip = ip;
            return 0u;
          }
        }
      }
    }
#undef LZ4HIP_PHASE
  }
};

// The table LZ4_loadDict leaves, in FastCore<.., DICT>'s entry layout: tail positions 0, 3, 6, ... while p <= keep - 8 (so the last 7
// positions are never candidates), index kDictBase - keep + p, the last insert of a bucket wins (atomic max on the index, as in the
// core).  One wavefront builds it in its own table (w's LDS) and writes the 4096 entries to image[0 .. 32768).  keep >= 8.
// WRITE_OUT = false: the table is left in w's LDS and `image` is not looked at -- what the linked-block kernel starts a chain with
// (dict_table_build).
template <class W, bool WRITE_OUT = true>
LZ4HIP_DEV void dict_image_build(W& w, const uint8_t* tail, uint32_t keep, uint8_t* image) {
  using Core = FastCore<W, false, DirectOut<W>, false, false, true>;
  using VU = typename W::VU;
  using VU64 = typename W::VU64;
  using VB = typename W::VB;
  w.template lds_fill<false>(1u << Core::HLOG, (uint64_t)0);
  w.sync();
  for (uint32_t base = 0; base + 8u <= keep; base += 3u * 64u) {
    const VU p = w.lane() * 3u + base;
    const VB act = p + 8u <= keep;
    const VU64 x = w.ldu64(tail, W::vmin(p, keep - 8u));
    const VU h = W::lo32(((x << 24) * 889523592379ull) >> (64 - Core::HLOG));
    (void)w.template lds_max<false>(h, Core::mk_entry(p + (Core::kDictBase - keep), Core::fp32(W::lo32(x))), act);
  }
  w.sync();
  if constexpr (WRITE_OUT) {
    for (uint32_t i = 0; i < (1u << Core::HLOG); i += 64u) {
      const VU h = w.lane() + i;
      const VU64 e = w.template lds_rdu<false>(h);
      w.st32(image, h * 8u, W::lo32(e), VB(true));
      w.st32(image, h * 8u + 4u, W::lo32(e >> 32), VB(true));
    }
  }
}
template <class W>
LZ4HIP_DEV void dict_table_build(W& w, const uint8_t* tail, uint32_t keep) { dict_image_build<W, false>(w, tail, keep, nullptr); }

// ---------------------------------------------------------------------------------------------------
// The block shell: everything around a core's run() for ONE block, stated once for the kernels (compress_fast.hip) and the CPU lane
// simulator (tests/hostsim/block_host.h): liblz4's up-front returns, the output policy, the table layout by size (byU16 below 65547
// bytes, byU32 from there on; DICT: byU32 at every size), the form's state, run(), the results.  A new operation adds a switch to the
// core and a kernel that names its form; it does not restate this.
//   Form  FastForm<W, FILL, ACC, DICT> here, FastFormMS<W> in lz4_fast_ms_core.h.  SIM: the simulator's extras -- counters, the
//         density probe -- which the shell must not see as run-time values: a kernel's code would come out differently.
//   a, b  the batch and the block in it (dst_cap[b] is the target of a FILL form); the simulator makes a batch of one.
//   Io    i32(v) / ptr(p): a wave-uniform value back in scalar registers (identity on the host); begin_block(w, s, n, d, cap): the
//         block may read [s, s + n) and write [d, d + cap) (the simulator's bounds; nothing on the device); put(b, r) /
//         put(b, r, consumed): the results.  A FILL form's up-front 0 leaves consumed at src_len, as liblz4 leaves *srcSizePtr.
// ---------------------------------------------------------------------------------------------------
template <class W, bool FILL = false, bool ACC = false, bool DICT = false, bool SIM = false>
struct FastForm {
  using Out = DirectOut<W, FILL>;
  template <bool U16> using Core = FastCore<W, U16, Out, false, ACC, DICT>;
  static constexpr bool kFill = FILL, kDict = DICT, kSim = SIM;
};
template <class Form, class W, class Io>
LZ4HIP_DEV void fast_block_run(W& w, Io& io, const BatchArgs& a, uint32_t b, FastBlockArgs& x) {
  const int32_t n = io.i32(a.src_len[b]);
  const int32_t cap = io.i32(a.dst_cap[b]);
  uint32_t r = 0;
  int32_t used = n;
  if ((!Form::kFill || cap > 0) && n >= 0 && (uint32_t)n <= 0x7E000000u && (Form::kFill || cap >= 0)) {
    const uint8_t* s = io.ptr(a.src + a.src_off[b]);
    uint8_t* d = io.ptr(a.dst + a.dst_off[b]);
    io.begin_block(w, s, (uint32_t)n, d, (uint32_t)cap);
    typename Form::Out out(w, s, (uint32_t)n, d, (uint32_t)cap);
    if constexpr (Form::kDict) {
      typename Form::template Core<false> c(w, out, s, (uint32_t)n, Form::kSim ? x.st : nullptr);
      c.template setup<Form::kSim>(x);
      r = c.run();
      if constexpr (Form::kSim) x.bailed = c.bailed;
    } else if (n < 65547) {
      typename Form::template Core<true> c(w, out, s, (uint32_t)n, Form::kSim ? x.st : nullptr);
      c.template setup<Form::kSim>(x);
      r = c.run();
      if constexpr (Form::kSim) x.bailed = c.bailed;
    } else {
      typename Form::template Core<false> c(w, out, s, (uint32_t)n, Form::kSim ? x.st : nullptr);
      c.template setup<Form::kSim>(x);
      r = c.run();
      if constexpr (Form::kSim) x.bailed = c.bailed;
    }
    if constexpr (Form::kFill) used = (int32_t)out.consumed;
  }
  if constexpr (Form::kFill) io.put(b, r, used);
  else io.put(b, r);
}

}  // namespace lz4hip
