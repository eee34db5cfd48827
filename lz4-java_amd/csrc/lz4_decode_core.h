// lz4_decode_core.h -- LZ4 block decoder for a small lane group (G lanes of a wavefront per block).
//
// Replaces, for the "HIP" family, LZ4_decompress_safe (/root/reference/src/jni/net_jpountz_lz4_LZ4JNI.c:216,
// reached from LZ4JNISafeDecompressor.java:34-43) and LZ4_decompress_fast (LZ4JNI.c:169,
// LZ4JNIFastDecompressor.java:35-44); SURVEY.md App. C.  Return values -- decoded size / bytes
// consumed, or -(input position)-1 -- equal liblz4 1.9.3's on valid AND malformed input: liblz4
// decodes in three tiers (a fast loop while >= 64 output bytes remain, a two-stage shortcut and a
// fully checked path) and which malformed streams are accepted depends on the tier, so the tiers'
// checks are kept.  What is different is the execution shape: every lane of the group runs the
// (cheap, serial) token parse redundantly -- no cross-lane traffic, parse loads are broadcast
// loads -- and the lanes split every literal / match copy between them.  A wavefront holds 64/G
// independent blocks; thousands of groups per CU-set keep HBM busy while each parse chain waits.
//
// Match copies read the block's own output from global memory: a wavefront's vector memory
// operations execute in order, so bytes stored by an earlier instruction of the same wave are
// visible to its later loads (same CU L1, no fence needed).  Within ONE copy instruction lanes
// never read bytes written by that instruction: overlapping matches (offset < bytes per step) use
// the replicate path, which only reads bytes that precede the match.
//
// Backend `Grp` (group_dev.h on the GPU, tests/hostsim/group_host.h in the CPU test-suite):
//   ld8/ld16/ld32/ld64(p)                   uniform loads (all lanes of the group, same address)
//   copy_lits(d, s, len, wild)               d[0..len) = s[0..len); wild: may touch <= 3 bytes past len on both sides
//   copy_match(dst, op, offset, len, wild)   dst[op+i] = dst[op-offset+i], byte-forward semantics;
//                                            offset 0 zero-fills (liblz4 1.9.3 behaviour)
#pragma once
#include <stdint.h>

#ifndef LZ4HIP_DEV
#if defined(__HIPCC__)
#define LZ4HIP_DEV __device__ __forceinline__
#else
#define LZ4HIP_DEV inline
#endif
#endif

#ifndef LZ4HIP_DECODE_REENTER
#define LZ4HIP_DECODE_REENTER 1   // 0: the interior loop is entered once per block (round 1 behaviour; developer A/B builds)
#endif
#ifndef LZ4HIP_DICT_INTERIOR
#define LZ4HIP_DICT_INTERIOR 1    // 0: the interior loops leave every match that starts in the dictionary to the exact path (developer A/B builds: tools/dict_decode_sweep.py)
#endif
#ifndef LZ4HIP_DECODE_INTERIOR
#define LZ4HIP_DECODE_INTERIOR 1  // 0: the plain interior loop is never entered -- the exact tiers alone (the CPU simulator's builds)
#endif
// The interior loops' distance from a block's two ends: every one of them (the loops below and lz4_decode_deep.h .. lz4_decode_size.h)
// runs a sequence without liblz4's per-sequence checks only while ip <= iend - LZ4HIP_DECODE_IN_MARGIN and
// op <= oend - LZ4HIP_DECODE_OUT_MARGIN.  A "simple" sequence (one extension byte per length) consumes <= 274 and produces <= 542
// bytes.  What the loops need of the rest (profiles/decode_margin_audit.txt, loop by loop): 279 of the input margin -- the 8 bytes read
// at the literals' end, which is also liblz4's rule that literals end 8 bytes in front of iend -- and 547 / 549 / 557 of the output
// margin for lane groups of 16+ / 8 / 4 lanes: liblz4's five last literals, or the 3 / 7 / 15 bytes a lane's store runs past a match's end.
// The other 27 and 49 bytes are slack no loop uses.  Overridable for the lane simulator's mutant builds alone (tests/test_margin_hostsim.py).
#ifndef LZ4HIP_DECODE_IN_MARGIN
#define LZ4HIP_DECODE_IN_MARGIN 306
#endif
#ifndef LZ4HIP_DECODE_OUT_MARGIN
#define LZ4HIP_DECODE_OUT_MARGIN 606
#endif
namespace lz4hip {
// The two copies of decode_block's dictionary mode (DICT, below), in front of the interior loops that use them.  dst is where output
// position 0 lies: the block's start, or with PREFIX the start of the prefix -- where a match goes on behind the dictionary's end.
template <class Grp>
LZ4HIP_DEV int dict_match_copy(Grp& g, uint8_t* dst, int op, int back, int length, const uint8_t* dict_end) {   // back = offset - op > 0; returns op + length
  const int c = length < back ? length : back;
  g.copy_lits(dst + op, dict_end - back, (uint32_t)c, false);
  op += c;
  if (length > c) { g.copy_match(dst, (uint32_t)op, (uint32_t)op, (uint32_t)(length - c), false); op += length - c; }   // (the rest: dst[op + i] = dst[i])
  return op;
}
// a match wholly inside the dictionary, in an interior loop (>= 300 bytes of room in dst): whole steps while the step's over-read stays
// inside the dictionary, byte-exact at its end
template <class Grp>
LZ4HIP_DEV void dict_copy_interior(Grp& g, uint8_t* d, const uint8_t* dict_end, int back, int ml) {
  if (back - ml >= (int)g.slack()) g.copy_lits_wide(d, dict_end - back, (uint32_t)ml);
  else g.copy_lits(d, dict_end - back, (uint32_t)ml, false);
}
}  // namespace lz4hip
#include "lz4_decode_deep.h"
#include "lz4_decode_ring.h"
#include "lz4_decode_wave.h"
#include "lz4_decode_pair.h"
#include "lz4_decode_trio.h"
#include "lz4_decode_size.h"
namespace lz4hip {

// PARTIAL decoding: a literal or match length of `base` plus the extension bytes' 32-bit sum `ext` (liblz4 adds that unsigned sum to a
// size_t), as an int that compares with `room` as the real length does: the length itself if it is <= room, else room + 1
LZ4HIP_DEV int partial_run(uint32_t base, uint32_t ext, int room) {
  const int64_t n = (int64_t)base + (int64_t)ext;
  return n > (int64_t)room ? room + 1 : (int)n;
}

// a backend asks for liblz4's own 32-bit length sums in the full decoder (decode_block EXACT) with a member  static constexpr bool kExactLengthSum = true
template <class G, class = void> struct exact_length_sum { static constexpr bool value = false; };
template <class G> struct exact_length_sum<G, decltype((void)G::kExactLengthSum)> { static constexpr bool value = G::kExactLengthSum; };

// SAFE: LZ4_decompress_safe(src, dst, src_size, out_size) -> decoded size or negative.
// !SAFE: LZ4_decompress_fast(src, dst, out_size) -> bytes consumed or negative; `src_size` is then
//        the readable capacity of the source slot and is never exceeded (liblz4 itself trusts the
//        stream blindly; results on valid streams are identical).
// PIPE: 1 = pipelined interior loop (below).  Pays when a wavefront has to make progress on its own (few, large blocks);
//       with the GPU full of blocks the plain loop is as fast.  2 = the deep loop of lz4_decode_deep.h (stream staged in LDS at
//       `stage`, Grp::kStreamLds bytes for this block; two slots: one match source of the block waits while the next is requested); the last 2 KB of the stream
//       are left to loop 1.
//       3 = the ring loop of lz4_decode_ring.h (stream AND recent output in LDS rings at `stage`, Grp::kRingLds bytes; near matches
//       never leave the chip, far ones are pipelined through slots, output leaves as whole aligned 64-byte steps).
//       4 = the wave loop of lz4_decode_wave.h (ONE WAVEFRONT PER BLOCK, Grp = BlockWaveDev: stream ring and an output ring of 8 .. 64 KB
//       in LDS at `stage`, wave-uniform parse, one LDS round trip per sequence): launches of few blocks.
//       5 = the parallel wave loop (same file, same rings): every sequence that starts in a 256-byte window of the stream per trip.
//       7 = the pair loop of lz4_decode_pair.h (TWO WAVEFRONTS PER BLOCK: the caller is the copier, `stage` = the pair's LDS: the rings of 4 / 5 and a mailbox; a second wavefront
//       runs pair_parser_service on the same LDS).
//       8 = the trio loop of lz4_decode_trio.h (THREE WAVEFRONTS PER BLOCK: the caller is the copier; a planner and a scanner wavefront run trio_service on the same LDS).
//       9 = the size loop of lz4_decode_size.h (ONE WAVEFRONT PER BLOCK, a backend that copies nothing: `stage` = its stream ring, dst is never touched): the decoded-size query.
// STAGE: the interior loop writes through an LDS staging buffer (`stage`, Grp::kStage bytes for this block) and output leaves
//        it as whole 128-byte lines (group_dev.h st_*).
// PARTIAL (SAFE only): LZ4_decompress_safe_partial(src, dst, src_size, target, cap) with out_size = min(target, cap) -- liblz4
//        1.9.3's partialDecoding: decoding stops once out_size bytes are out, or where the input ends; a literal run or a match
//        longer than what remains is cut, not an error.  Only the end-of-block code differs: every interior loop and tier 1 stay
//        >= 32 bytes away from oend.  A match of offset 0 (no compressor emits one) that is cut zero-fills like every other offset-0
//        match here; liblz4 copies those bytes onto themselves, so its output there is whatever its buffer held.
// DICT (SAFE only, not PARTIAL): LZ4_decompress_safe_usingDict(src, dst, src_size, out_size, dict_end - dict_len, dict_len) for a dictionary
//        that is NOT contiguous with dst (liblz4 1.9.3's usingExtDict).  An offset may reach offset - op bytes before the block: it is
//        valid iff offset <= op + dict_len, and never rejected once dict_len >= 65536 (liblz4's checkOffset), tested where the plain
//        decoder tests offset > op.  Such a match takes min(length, offset - op) bytes from the dictionary's end and the rest from the
//        block's own start, byte-forward (dict_match_copy); it must end at or before oend - 5 and meets no other end-of-block rule.
//        Only [dict_end - min(dict_len, 65535), dict_end) is ever read, and never wildly.  The interior loops (plain, staged, pipelined,
//        deep) take the matches that lie wholly in the dictionary as copies from a foreign pointer, like literals; a match that
//        straddles the block's start goes to the exact code.  dict_len == 0 is the plain decoder.
// PREFIX (SAFE only, not PARTIAL, not STAGE): one block of a chain of linked blocks -- LZ4_decompress_safe_continue of liblz4 1.9.3 in its
//        rolling-prefix mode (withSmallPrefix / withPrefix64k): the `hist` bytes in front of dst are history (what the chain's earlier
//        blocks decoded, and what lay in front of the chain), hist = min(real history, 65535).  A match may start in the history: an
//        offset is valid at output position p iff offset <= p + hist, so with hist == 65535 no offset is rejected (liblz4 stops
//        checking from 65535 bytes of prefix on).  History and block are ONE contiguous run of bytes, so the block is decoded as if
//        it began `hist` bytes in front of dst with op = hist: every copy is the plain decoder's (a match that straddles the
//        block's start is one overlapping copy), every end-of-block rule is the plain decoder's (they measure the distance to oend), the
//        error codes keep their input positions, and a source in the history is an ordinary far source of the interior loops.  Only
//        loops whose output lives in memory can see the history: plain, pipelined, deep.  Nothing in front of dst is written (a copy
//        touches bytes behind its end only), nothing in front of dst - hist is read.  out_size + hist must not overflow an int.
//        hist == 0 is the plain decoder.
// PREFIX && DICT: LZ4_decompress_safe_doubleDict -- a prefix of hist < 65535 bytes in front of dst AND an external dictionary behind it
//        (the stream decoder, lz4_decode_stream.h).  The block's logical history is dictionary ++ prefix.  Output positions count from
//        the start of the prefix, as in PREFIX, so DICT's tests read unchanged with the prefix's start in the place of the block's:
//        an offset past position p is a dictionary match of offset - p bytes back from dict_end, valid iff offset <= p + dict_len
//        (never rejected once dict_len >= 65536), and a match that runs past the dictionary's end continues at the start of the
//        PREFIX -- which is where `dst` points once it has been moved back by hist, so dict_match_copy's "the block's own start" is
//        the prefix's start here.  hist == 0 is DICT, dict_len == 0 is PREFIX.
template <class Grp, bool SAFE, int PIPE = 0, bool STAGE = false, bool PARTIAL = false, bool DICT = false, bool PREFIX = false>
LZ4HIP_DEV int decode_block(Grp& g, const uint8_t* src, int src_size, uint8_t* dst, int out_size, uint8_t* stage = nullptr,
                            const uint8_t* dict_end = nullptr, int dict_len = 0, int hist = 0) {
  static_assert(!PARTIAL || SAFE, "partial decoding is a safe-decoder mode");
  static_assert(!DICT || (SAFE && !PARTIAL && PIPE <= 2), "the dictionary decoder is a safe-decoder mode of the plain, staged, pipelined and deep loops");
  static_assert(!PREFIX || (SAFE && !PARTIAL && !STAGE && PIPE <= 2), "the linked-block decoder is a safe-decoder mode of the plain, pipelined and deep loops");
  // EXACT (a backend that sets kExactLengthSum: the decoded-size query, whose value is liblz4's on EVERY input): a length's extension bytes are summed
  // in 32 bits, as liblz4 sums them, to the run's end -- the error position of a run that cannot fit is then liblz4's.  The decoders stop such a run at
  // LZ4HIP_LEN_CAP instead: also an error, reported where the cap was passed.  WRAP: the 32-bit sum, PARTIAL's too
  constexpr bool EXACT = !PARTIAL && exact_length_sum<Grp>::value, WRAP = PARTIAL || EXACT;
  const int obase = PREFIX ? hist : 0;          // (PREFIX: output positions count from the start of the history)
  if constexpr (PREFIX) dst -= obase;
  int ip = 0, op = obase;
  const int iend = src_size, oend = out_size + obase;  // iend: real end (SAFE) / read bound (!SAFE)
  const int shortiend = iend - (SAFE ? 14 : 8) - 2;
  const int shortoend = oend - (SAFE ? 14 : 8) - 18;
  uint32_t token;
  int length, offset, cpy;

#define LZ4HIP_LEN_CAP 0x7F000000  /* a run this long can never fit; stops 32-bit wrap on absurd input */
#define LZ4HIP_NEED_IN(k) do { if (!SAFE && ip + (int)(k) > iend) goto output_error; } while (0)
  /* the offset check at output position p; DICT: liblz4's checkOffset (dict_len < 64 KB) against the dictionary's start */
#define LZ4HIP_OFF_BAD(p) (DICT ? (dict_len < 65536 && offset > (p) + dict_len) : offset > (p))
  /* DICT, interior loops: the match (off, ml) at output position p starts before the block and lies wholly inside the dictionary */
#define LZ4HIP_IN_DICT(off, p, ml) (DICT && LZ4HIP_DICT_INTERIOR && (off) > (p) && (ml) <= (off) - (p) && (off) - (p) <= dict_len)
  if (out_size < 0 || src_size < 0) return -1;
  if (PARTIAL && out_size == 0) return 0;
  if (SAFE && out_size == 0) return (src_size == 1 && g.ld8(src) == 0) ? 0 : -1;
  if (!SAFE && out_size == 0) { LZ4HIP_NEED_IN(1); return g.ld8(src) == 0 ? 1 : -1; }
  if (SAFE && src_size == 0) return -1;

  if (oend - op >= 64) {
  interior:
    // ---- tier 1, interior fast loop.  While the block is far from both buffer ends (ip <= iend-306, op <= oend-606: LZ4HIP_DECODE_IN_MARGIN / _OUT_MARGIN)
    // and the sequence is "simple" -- literal and match lengths need at most ONE extension byte (<= 269 / <= 273),
    // offset <= op -- every check of liblz4's fast loop provably passes (a sequence consumes <= 274 and produces
    // <= 542 bytes), so only those few conditions are tested.  Anything else falls through, with ip/op still at the
    // sequence start, to the exact tier-1 code below, which re-decodes that sequence with all checks. ----
    // The 8 bytes fetched at the offset position also hold the NEXT sequence's token (and its first length byte), so the
    // steady state costs two dependent loads per sequence: {offset word + literals} and {match source}.
    if constexpr (PIPE == 2) {
      if (ip + 2048 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN)
        if (decode_deep_loop<Grp, DICT>(g, src, iend, dst, oend, ip, op, stage, dict_end, (uint32_t)dict_len)) goto interior;
    }
    if constexpr (PIPE == 3) {   // the ring loop (lz4_decode_ring.h): stream and recent output in LDS at `stage` (Grp::kRingLds bytes)
      // It wants 64 output bytes in front of it (its flusher stores whole aligned steps).  They are decoded HERE, by the plain
      // interior loop, and not by the exact code below one sequence per round of `goto interior`: the blocks of a wavefront need
      // different numbers of sequences for their first 64 bytes, and blocks that reach the ring loop in different rounds of an
      // enclosing loop run it one after the other, not side by side (measured: 5.4 of 16 blocks per trip, 3x the time).
      if (op < 64 && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) {
        uint32_t t4 = g.ld32(src + ip);
        do {
          int lit = (int)((t4 >> 4) & 15u), ml = (int)(t4 & 15u), hdr = 1;
          if (lit == 15) {
            const uint32_t e = (t4 >> 8) & 255u;
            if (e == 255u) break;
            lit += (int)e;
            hdr = 2;
          }
          const uint64_t o8 = g.ld64(src + ip + hdr + lit);
          const int off = (int)((uint32_t)o8 & 0xFFFFu);
          int adv = hdr + lit + 2;
          uint32_t nxt = (uint32_t)(o8 >> 16);
          if (ml == 15) {
            const uint32_t e = nxt & 255u;
            if (e == 255u) break;
            ml += (int)e;
            adv++;
            nxt = (uint32_t)(o8 >> 24);
          }
          ml += 4;
          if (off > op + lit) break;   // invalid offset: the exact path produces liblz4's error code
          g.copy_lits_wide(dst + op, src + ip + hdr, (uint32_t)lit);
          op += lit;
          g.copy_match_wide(dst, (uint32_t)op, (uint32_t)off, (uint32_t)ml);
          op += ml;
          ip += adv;
          t4 = nxt;
        } while (op < 64 && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN);
      }
      if (op >= 64 && ip + 320 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN)
        if (decode_ring_loop(g, src, iend, dst, oend, ip, op, stage)) goto interior;
    }
    if constexpr (PIPE == 4) {   // the wave loop (lz4_decode_wave.h); what it leaves at ip is done by the exact code below, which comes back
      if (ip + 1024 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) decode_wave_loop(g, src, iend, dst, oend, ip, op, stage);
    }
    if constexpr (PIPE == 5 || PIPE == 6) {   // the parallel wave loop: several sequences of the block per trip (6: one window of the stream per trip whatever the backend's ring -- the simulator's way to the form a 1 KB stream ring runs)
      if (ip + 1536 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN)
        if (decode_wave_par_loop<Grp, false>(g, src, iend, dst, oend, ip, op, stage))             // (true: the stream is full of sequences -- the loop's SHORT instance)
          if (ip + 1536 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) (void)decode_wave_par_loop<Grp, true>(g, src, iend, dst, oend, ip, op, stage);
    }
    if constexpr (PIPE == 7) {   // the pair loop (lz4_decode_pair.h): this wavefront copies, its partner wavefront parses the stream a trip or two ahead
      if (ip + 1536 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) decode_pair_loop<Grp>(g, src, iend, dst, oend, ip, op, stage);
    }
    if constexpr (PIPE == 8) {   // the trio loop (lz4_decode_trio.h): this wavefront copies, a planner and a scanner wavefront run ahead in the stream
      if (ip + 1536 <= iend && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) decode_trio_loop<Grp>(g, src, iend, dst, oend, ip, op, stage);
    }
    if constexpr (PIPE == 9) {   // the size loop (lz4_decode_size.h): it moves ip / op over every sequence that provably passes; what it leaves at ip is done by the exact code below, which comes back
      if (ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) decode_size_loop(g, src, iend, oend, ip, op, stage);
    }
    if ((PIPE == 1 || (PIPE == 2 && ip + 2048 > iend) || (PIPE == 3 && ip + 320 > iend) || (PIPE == 4 && ip + 1024 > iend) || ((PIPE == 5 || PIPE == 6 || PIPE == 7 || PIPE == 8) && ip + 1536 > iend)) && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) {   // (2 .. 8: only the tail of the stream)
      // ---- the same loop, software-pipelined.  A wavefront's memory operations retire in order, so a wait for a load also
      // waits for every OLDER store.  Here (a) the next sequence's offset word is requested as soon as this sequence's header
      // is parsed, (b) a "simple" sequence (literals and match take one step each, match source entirely before the
      // sequence's own output) is LOADED in one trip and STORED in the next, behind that trip's loads -- no wait ever covers
      // a store, and both of a trip's waits are for loads issued a trip earlier.  Two register sets alternate (a copy would
      // have to wait for the loads).  Anything not simple, or whose source reaches into bytes still waiting to be stored,
      // flushes the pending stores first. ----
      typename Grp::SeqRegs R0, R1;
      bool have_p = false, p_in0 = false;  // a loaded-not-stored sequence exists; it sits in R0 / R1
      uint32_t p_op = 0, p_lit = 0, p_ml = 0;
      uint32_t t4 = g.ld32(src + ip);
      uint64_t o8 = 0;
      bool have_o8 = false;                // o8 already holds the offset word of the sequence at ip
      auto trip = [&](typename Grp::SeqRegs& cur, typename Grp::SeqRegs& pnd, const bool cur_is0) -> bool {  // false: leave the loop
        int lit = (int)((t4 >> 4) & 15u);
        int ml = (int)(t4 & 15u);
        int hdr = 1;
        if (lit == 15) {
          const uint32_t e = (t4 >> 8) & 255u;
          if (e == 255u) return false;
          lit += (int)e;
          hdr = 2;
        }
        if (!have_o8) o8 = g.ld64(src + ip + hdr + lit);
        const int off = (int)((uint32_t)o8 & 0xFFFFu);
        int adv = hdr + lit + 2;
        uint32_t nxt = (uint32_t)(o8 >> 16);
        if (ml == 15) {
          const uint32_t e = nxt & 255u;
          if (e == 255u) { have_o8 = false; return false; }
          ml += (int)e;
          adv++;
          nxt = (uint32_t)(o8 >> 24);
        }
        ml += 4;
        if (off > op + lit) {  // invalid offset: the exact path produces liblz4's error code
          if constexpr (DICT) { if (!LZ4HIP_IN_DICT(off, op + lit, ml)) { have_o8 = false; return false; } }   // (a match wholly inside the dictionary stays here)
          else { have_o8 = false; return false; }
        }
        const uint8_t* lit_src = src + ip + hdr;
        {
          // the next sequence's header is in nxt: if it can run in this loop, request its offset word now (the address the
          // next trip computes from t4 = nxt; ip + adv <= iend - LZ4HIP_DECODE_IN_MARGIN leaves >= 306 readable bytes, the word ends <= 279 in)
          have_o8 = false;
          int lit2 = (int)((nxt >> 4) & 15u), hdr2 = 1;
          bool ok2 = ip + adv <= iend - LZ4HIP_DECODE_IN_MARGIN;
          if (lit2 == 15) {
            const uint32_t e2 = (nxt >> 8) & 255u;
            if (e2 == 255u) ok2 = false;
            lit2 += (int)e2;
            hdr2 = 2;
          }
          if (ok2) { o8 = g.ld64(src + ip + adv + hdr2 + lit2); have_o8 = true; }
        }
        // simple: one step each, and the match source [op+lit-off, +ml+slack) ends before this sequence's own output;
        // dep: the source reaches into the bytes the pending sequence has yet to store
        const uint32_t ulit = (uint32_t)lit, uml = (uint32_t)ml, uoff = (uint32_t)off, sl = g.slack();
        if constexpr (DICT) {
          if (off > op + lit) {   // wholly inside the dictionary: a source that waits for no store; simple while the step's over-read stays inside it
            const int back = off - op - lit;
            const bool dsimple = ulit <= g.step() && uml <= g.step() && (uint32_t)back >= uml + sl;
            if (have_p && !dsimple) { g.seq_store(pnd, dst + p_op, p_lit, p_ml); have_p = false; }
            if (dsimple) {
              g.seq_load(cur, lit_src, ulit, dict_end - back, uml);
              if (have_p) g.seq_store(pnd, dst + p_op, p_lit, p_ml);
              have_p = true; p_in0 = cur_is0; p_op = (uint32_t)op; p_lit = ulit; p_ml = uml;
              op += lit;
            } else {
              g.copy_lits_wide(dst + op, lit_src, ulit);
              op += lit;
              dict_copy_interior(g, dst + op, dict_end, back, ml);
            }
            op += ml;
            ip += adv;
            t4 = nxt;
            return ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN;
          }
        }
        const bool simple = ulit <= g.step() && uml <= g.step() && uoff >= ulit + uml + sl;
        const bool dep = have_p && uoff < ulit + uml + sl + p_lit + p_ml;
        if (have_p && (!simple || dep)) { g.seq_store(pnd, dst + p_op, p_lit, p_ml); have_p = false; }
        if (simple) {
          g.seq_load(cur, lit_src, ulit, dst + op + lit - off, uml);
          if (have_p) g.seq_store(pnd, dst + p_op, p_lit, p_ml);
          have_p = true; p_in0 = cur_is0; p_op = (uint32_t)op; p_lit = ulit; p_ml = uml;
          op += lit;
        } else {
          g.copy_lits_wide(dst + op, lit_src, ulit);
          op += lit;
          g.copy_match_wide(dst, (uint32_t)op, uoff, uml);
        }
        op += ml;
        ip += adv;
        t4 = nxt;
        return ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN;
      };
      while (trip(R0, R1, true) && trip(R1, R0, false)) {}
      if (have_p) g.seq_store(p_in0 ? R0 : R1, dst + p_op, p_lit, p_ml);  // the exact code below reads what is in memory
    }
    if (STAGE && !PIPE && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) {
      // ---- the plain loop below, writing through the staging buffer.  Match sources are read from memory only: a source that
      // reaches past the flushed position (rare unless offsets are short) flushes everything first, and that match is then
      // written straight to memory.  Whole lines are flushed every second sequence -- on a schedule, not when a block happens
      // to have filled a line, so that the blocks sharing a wavefront flush in the same instructions. ----
      g.st_begin(stage, (uint32_t)op);
      uint32_t t4 = g.ld32(src + ip);
      uint32_t it = 0;
      do {
        int lit = (int)((t4 >> 4) & 15u);
        int ml = (int)(t4 & 15u);
        int hdr = 1;
        if (lit == 15) {
          const uint32_t e = (t4 >> 8) & 255u;
          if (e == 255u) break;
          lit += (int)e;
          hdr = 2;
        }
        const uint64_t o8 = g.ld64(src + ip + hdr + lit);
        g.st_lits(dst, (uint32_t)op, src + ip + hdr, (uint32_t)lit);
        const int off = (int)((uint32_t)o8 & 0xFFFFu);
        int adv = hdr + lit + 2;
        uint32_t nxt = (uint32_t)(o8 >> 16);
        if (ml == 15) {
          const uint32_t e = nxt & 255u;
          if (e == 255u) break;  // (the staged literals lie beyond op: never flushed)
          ml += (int)e;
          adv++;
          nxt = (uint32_t)(o8 >> 24);
        }
        ml += 4;
        if (off > op + lit && !LZ4HIP_IN_DICT(off, op + lit, ml)) break;
        op += lit;
        if (DICT && off > op) {   // wholly inside the dictionary: staged like literals; at the dictionary's end byte-exact, straight to memory
          if (off - op - ml >= (int)g.slack()) {
            g.st_lits(dst, (uint32_t)op, dict_end - (off - op), (uint32_t)ml);
            op += ml;
          } else {
            g.st_flush_all(dst, (uint32_t)op);
            g.copy_lits(dst + op, dict_end - (off - op), (uint32_t)ml, false);
            op += ml;
            g.fl = (uint32_t)op;
          }
        } else if ((uint32_t)(op - off) + (uint32_t)ml + g.slack() > g.fl) {
          g.st_flush_all(dst, (uint32_t)op);
          g.copy_match_wide(dst, (uint32_t)op, (uint32_t)off, (uint32_t)ml);
          op += ml;
          g.fl = (uint32_t)op;
        } else {
          g.st_match(dst, (uint32_t)op, (uint32_t)off, (uint32_t)ml);
          op += ml;
        }
        ip += adv;
        t4 = nxt;
#ifndef LZ4HIP_STAGE_EVERY
#define LZ4HIP_STAGE_EVERY 2
#endif
        if (++it % LZ4HIP_STAGE_EVERY == 0u) g.st_flush_lines(dst, (uint32_t)op);
      } while (ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN);
      g.st_flush_all(dst, (uint32_t)op);  // the exact code below reads and writes memory
    }
    if (!STAGE && !PIPE && LZ4HIP_DECODE_INTERIOR && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) {
      uint32_t t4 = g.ld32(src + ip);  // {token, first literal-length byte, ...} of the sequence at ip
      do {
        int lit = (int)((t4 >> 4) & 15u);
        int ml = (int)(t4 & 15u);
        int hdr = 1;
        if (lit == 15) {
          const uint32_t e = (t4 >> 8) & 255u;
          if (e == 255u) break;
          lit += (int)e;
          hdr = 2;
        }
        const uint64_t o8 = g.ld64(src + ip + hdr + lit);  // {offset lo, hi, [match-length byte], next token, ...}
        g.copy_lits_wide(dst + op, src + ip + hdr, (uint32_t)lit);
        const int off = (int)((uint32_t)o8 & 0xFFFFu);
        int adv = hdr + lit + 2;
        uint32_t nxt = (uint32_t)(o8 >> 16);
        if (ml == 15) {
          const uint32_t e = nxt & 255u;
          if (e == 255u) break;  // (the literals just written are simply written again by the exact path)
          ml += (int)e;
          adv++;
          nxt = (uint32_t)(o8 >> 24);
        }
        ml += 4;
        if (off > op + lit && !LZ4HIP_IN_DICT(off, op + lit, ml)) break;  // invalid offset: let the exact path produce liblz4's error code
        op += lit;
        if (DICT && off > op) dict_copy_interior(g, dst + op, dict_end, off - op, ml);   // wholly inside the dictionary
        else g.copy_match_wide(dst, (uint32_t)op, (uint32_t)off, (uint32_t)ml);
        op += ml;
        ip += adv;
        t4 = nxt;
      } while (ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN);
    }
    // ---- tier 1: fast loop.  Software-pipelined: the word holding {offset, first match-length byte}
    // is requested BEFORE the literal copy, and the next sequence's token word BEFORE the match copy,
    // so a sequence costs two dependent memory round trips (literals+offset, then match source)
    // instead of four; the token fetch rides under the match-source latency. ----
    uint32_t w4;  // token + next 3 bytes when they are readable
    if (ip + 4 <= iend) { w4 = g.ld32(src + ip); } else { LZ4HIP_NEED_IN(1); w4 = g.ld8(src + ip); }
    for (;;) {
      token = w4 & 255u;
      ip++;
      length = (int)(token >> 4);
      bool wild;
      if (length == 15) {
        // read_variable_length(limit iend-15, initial+loop checks when SAFE); a limit hit inside
        // the loop is not an error in liblz4 1.9.3: the partial length is used
        if (SAFE && ip >= iend - 15) goto output_error;
        uint32_t s = (w4 >> 8) & 255u;  // readable: ip+4 <= iend held (SAFE: ip < iend-15; !SAFE: checked next)
        if (!SAFE && ip + 3 > iend) { LZ4HIP_NEED_IN(1); s = g.ld8(src + ip); }
        if (WRAP) length = 0;  // (PARTIAL: `length` sums the extension bytes in 32 bits, as liblz4 does; the 15 is added after)
        for (;;) {
          ip++;
          if (WRAP) length = (int)((uint32_t)length + s); else length += (int)s;
          if (SAFE && ip >= iend - 15) break;
          if (s != 255u) break;
          LZ4HIP_NEED_IN(1);
          s = g.ld8(src + ip);
          if (!WRAP && length > LZ4HIP_LEN_CAP) goto output_error;
        }
        if (PARTIAL) length = partial_run(15u, (uint32_t)length, iend - ip < oend - op ? iend - ip : oend - op);   // (cut at safe_literal_copy)
        else if (EXACT) { const int64_t n = (int64_t)15 + (int64_t)(uint32_t)length; if (n > (int64_t)(oend - op)) goto output_error; length = (int)n; }
        else if ((uint32_t)length > (uint32_t)(oend - op)) goto output_error;  // cannot fit: every tier rejects it at this ip
        cpy = op + length;
        if (SAFE) { if (cpy > oend - 32 || ip + length > iend - 32) goto safe_literal_copy; }
        else      { if (cpy > oend - 8) goto safe_literal_copy; }
        wild = SAFE || (ip + length + 4 <= iend);
      } else {
        cpy = op + length;
        if (SAFE && ip > iend - (16 + 1)) goto safe_literal_copy;
        wild = SAFE || (ip + length + 4 <= iend);
      }
      LZ4HIP_NEED_IN(length);
      {
        const int ipo = ip + length;  // where {offset lo, offset hi, first ML byte, ...} sit
        const bool have_off = SAFE || ipo + 2 <= iend;
        if (ipo + 4 <= iend) w4 = g.ld32(src + ipo); else if (have_off) w4 = g.ld16(src + ipo);
        g.copy_lits(dst + op, src + ip, (uint32_t)length, wild);
        ip = ipo;
        op = cpy;
        if (!have_off) goto output_error;  // the bounded fast decoder ran out of input at the offset
      }
      offset = (int)(w4 & 0xFFFFu);
      ip += 2;
      length = (int)(token & 15u);
      if (length == 15) {
        if (SAFE && LZ4HIP_OFF_BAD(op)) goto output_error;
        uint32_t s = (w4 >> 16) & 255u;
        if (ip + 2 > iend) { LZ4HIP_NEED_IN(1); s = g.ld8(src + ip); }  // (SAFE: error follows below anyway)
        if (WRAP) length = 0;
        for (;;) {  // read_variable_length(limit iend-4, loop check when SAFE)
          ip++;
          if (WRAP) length = (int)((uint32_t)length + s); else length += (int)s;
          if (SAFE && ip >= iend - 4) goto output_error;
          if (s != 255u) break;
          LZ4HIP_NEED_IN(1);
          s = g.ld8(src + ip);
          if (!WRAP && length > LZ4HIP_LEN_CAP) goto output_error;
        }
        if (PARTIAL) length = partial_run(15u, (uint32_t)length, oend - op - 4);   // (cut at safe_match_copy)
        else if (EXACT) { const int64_t n = (int64_t)15 + (int64_t)(uint32_t)length; if (n > (int64_t)(oend - op)) goto output_error; length = (int)n; }
        else if ((uint32_t)length > (uint32_t)(oend - op)) goto output_error;  // (offset <= op was checked / is checked first by liblz4 too)
        length += 4;
        if (op + length >= oend - 64) goto safe_match_copy;
      } else {
        length += 4;
        if (op + length >= oend - 64) goto safe_match_copy;
      }
      if (LZ4HIP_OFF_BAD(op)) goto output_error;  // liblz4 checks this only when SAFE; the HIP engine never reads before dst
      // next token word (SAFE: ip < iend holds after a non-final sequence)
      if (ip + 4 <= iend) { w4 = g.ld32(src + ip); } else { LZ4HIP_NEED_IN(1); w4 = g.ld8(src + ip); }
      if (DICT && offset > op) {   // the match starts in the dictionary (op + length < oend - 64 here)
        op = dict_match_copy(g, dst, op, offset - op, length, dict_end);
      } else {
        g.copy_match(dst, (uint32_t)op, (uint32_t)offset, (uint32_t)length, true);
        op += length;
      }
      // The interior loop left on a sequence it does not handle (a length run of two or more bytes, ...); that sequence has now
      // been decoded with every check: back to the interior loop while the block is still far from both ends.  (Round 1 entered
      // it once per block: data with an occasional long match or literal run fell off the fast path for the rest of the block.)
      if (LZ4HIP_DECODE_REENTER && ip <= iend - LZ4HIP_DECODE_IN_MARGIN && op <= oend - LZ4HIP_DECODE_OUT_MARGIN) goto interior;
    }
  }

  for (;;) {  // ---- tiers 2+3: shortcut and fully checked path ----
    LZ4HIP_NEED_IN(1);
    token = g.ld8(src + ip);
    ip++;
    length = (int)(token >> 4);
    if ((SAFE ? length != 15 : length <= 8) && (SAFE ? ip < shortiend : true) && op <= shortoend) {
      LZ4HIP_NEED_IN(length + 2);
      g.copy_lits(dst + op, src + ip, (uint32_t)length, false);
      op += length;
      ip += length;
      length = (int)(token & 15u);
      offset = (int)g.ld16(src + ip);
      ip += 2;
      if (length != 15 && offset >= 8 && offset <= op) {
        g.copy_match(dst, (uint32_t)op, (uint32_t)offset, (uint32_t)(length + 4), false);
        op += length + 4;
        continue;
      }
      if (!SAFE && length != 15 && offset >= 8 && offset > op) goto output_error;  // liblz4 would read before dst
      goto copy_match_label;
    }
    if (length == 15) {
      if (SAFE && ip >= iend - 15) goto output_error;
      if (WRAP) length = 0;
      for (;;) {
        LZ4HIP_NEED_IN(1);
        const uint32_t s = g.ld8(src + ip);
        ip++;
        if (WRAP) length = (int)((uint32_t)length + s); else length += (int)s;
        if (!WRAP && length > LZ4HIP_LEN_CAP) goto output_error;
        if (SAFE && ip >= iend - 15) break;
        if (s != 255u) break;
      }
      if (PARTIAL) length = partial_run(15u, (uint32_t)length, iend - ip < oend - op ? iend - ip : oend - op);
      else if (EXACT) { const int64_t n = (int64_t)15 + (int64_t)(uint32_t)length; if (n > (int64_t)(oend - op)) goto output_error; length = (int)n; }
      else if ((uint32_t)length > (uint32_t)(oend - op)) goto output_error;
    }
    cpy = op + length;
  safe_literal_copy:
    if ((SAFE && (cpy > oend - 12 || ip + length > iend - (2 + 1 + 5))) || (!SAFE && cpy > oend - 8)) {
      if constexpr (PARTIAL) {   // the run is cut to the input, then to the output; decoding goes on only if an offset can follow
        if (length > iend - ip) { length = iend - ip; cpy = op + length; }
        if (cpy > oend) { cpy = oend; length = oend - op; }
      } else {
        if (!SAFE && cpy != oend) goto output_error;
        if (SAFE && (ip + length != iend || cpy > oend)) goto output_error;
      }
      LZ4HIP_NEED_IN(length);
      g.copy_lits(dst + op, src + ip, (uint32_t)length, false);
      ip += length;
      op += length;
      if (!PARTIAL || cpy == oend || ip >= iend - 2) break;
    } else {
      LZ4HIP_NEED_IN(length);
      g.copy_lits(dst + op, src + ip, (uint32_t)length, false);
      ip += length;
      op = cpy;
    }
    LZ4HIP_NEED_IN(2);
    offset = (int)g.ld16(src + ip);
    ip += 2;
    length = (int)(token & 15u);
  copy_match_label:
    if (length == 15) {
      if (WRAP) length = 0;
      for (;;) {
        LZ4HIP_NEED_IN(1);
        const uint32_t s = g.ld8(src + ip);
        ip++;
        if (WRAP) length = (int)((uint32_t)length + s); else length += (int)s;
        if (SAFE && ip >= iend - 4) goto output_error;
        if (!WRAP && length > LZ4HIP_LEN_CAP) goto output_error;
        if (s != 255u) break;
      }
      if (PARTIAL) length = partial_run(15u, (uint32_t)length, oend - op - 4);
      else if (EXACT) { const int64_t n = (int64_t)15 + (int64_t)(uint32_t)length; if (n > (int64_t)(oend - op)) goto output_error; length = (int)n; }   // (an offset past op fails below, at this ip too)
      else if ((DICT || offset <= op) && (uint32_t)length > (uint32_t)(oend - op)) goto output_error;   // (DICT: an offset past the dictionary fails below, at this ip too)
    }
    length += 4;
  safe_match_copy:
    if (LZ4HIP_OFF_BAD(op)) goto output_error;
    if (DICT && offset > op) {   // the match starts in the dictionary: its only end-of-block rule is liblz4's last five literals
      if (length > oend - 5 - op) goto output_error;
      op = dict_match_copy(g, dst, op, offset - op, length, dict_end);
      continue;
    }
    cpy = op + length;
    if (PARTIAL && cpy > oend - 12) {   // liblz4's MATCH_SAFEGUARD_DISTANCE: copy what fits (byte-forward: overlapping matches included)
      const int mlen = length < oend - op ? length : oend - op;
      g.copy_match(dst, (uint32_t)op, (uint32_t)offset, (uint32_t)mlen, false);
      op += mlen;
      if (op == oend) break;
      continue;
    }
    if (cpy > oend - 5) goto output_error;  // the last 5 bytes are always literals
    g.copy_match(dst, (uint32_t)op, (uint32_t)offset, (uint32_t)length, false);
    op = cpy;
  }
  return SAFE ? op - obase : ip;
output_error:
  return -ip - 1;
#undef LZ4HIP_IN_DICT
#undef LZ4HIP_OFF_BAD
#undef LZ4HIP_NEED_IN
#undef LZ4HIP_LEN_CAP
}

// The decoded-size query (lz4_decode_size.h): what LZ4_decompress_safe(src, dst, src_size, cap) returns, from (src, src_size, cap) alone.
// `Grp` is a backend whose copies do nothing; dst is never touched.  FAST: the size loop in front of the exact path (`lds`: the
// backend's stream ring); !FAST: the exact path alone
template <class Grp, bool FAST>
LZ4HIP_DEV int decoded_size(Grp& g, const uint8_t* src, int src_size, int cap, uint8_t* lds = nullptr) {
  return decode_block<Grp, true, FAST ? 9 : 0>(g, src, src_size, nullptr, cap, lds);
}

}  // namespace lz4hip
