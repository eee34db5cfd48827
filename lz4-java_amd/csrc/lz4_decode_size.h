// lz4_decode_size.h -- the decoded-size query: the value LZ4_decompress_safe(src, dst, src_size, cap) returns -- the decoded size, or
// liblz4 1.9.3's -(input position)-1 -- from (src, src_size, cap) alone.  No output byte is read or written.
//
// That value never depends on what dst holds: it depends on the stream, its length and the capacity (liblz4's three tiers are chosen
// by the distance to the output's end, so which malformed streams are accepted depends on cap).  A dry run is therefore possible.
//
// EXACT PATH: decode_block<Grp, /*SAFE*/true, /*PIPE*/0> of lz4_decode_core.h as it stands, with a backend whose copy_lits* and
// copy_match* do nothing and whose ld* read the stream.  The tier rules are written once, there.
//
// FAST INTERIOR (decode_block PIPE == 9, decode_size_loop below): ONE WAVEFRONT PER BLOCK.  The stream is read coalesced, 256 bytes a
// step, into an LDS ring (the stream ring of the wave loops: group_dev.h rs_*); a trip takes every sequence that starts in a 256-byte
// window of the stream:
//  1. discovery and walk as in the parallel wave loop (lz4_decode_wave.h): every lane assumes a token at each of its four window
//     bytes and computes where the next token would lie; the chain from position 0 is walked (vwalk / vwalk_par) and its k-th start
//     goes to lane k;
//  2. A LANE PER SEQUENCE: lane k parses sequence k (token and literal-length byte out of the window registers, offset word and
//     match-length byte behind the literals out of the ring); the exclusive prefix sum of literal + match lengths is every sequence's
//     output position;
//  3. one ballot finds the first sequence that is not PROVABLY fine.  The rule is the one decode_block's interior loops use: at most
//     one extension byte per length (here: lengths below 255 + 15), ip <= iend - 306, op <= cap - 606, offset <= op + literals -- a
//     sequence that passes consumes <= 274 and produces <= 542 bytes, so every check of liblz4's fast loop passes.  The sequences in
//     front of it are taken: ip and op move, nothing else happens.
// What is not taken -- the first and last sequences of a block, long extension runs, bad offsets, a block with fewer than 606 bytes
// of room -- is left to decode_block's exact code with ip / op at that sequence's start; it does that one sequence with every check
// and comes back (decode_block's `goto interior`).  The ring's state lives in the backend, so coming back costs no refill.
// Lengths the loop sums are below 2^10 per sequence and op stays below cap: 32-bit sums are never in reach here.  In the exact code
// the size backends ask decode_block for liblz4's own 32-bit sum of a length's extension bytes (kExactLengthSum, decode_block EXACT):
// the decoders give up on a run at 0x7F000000 and report THAT position, liblz4 reads the run to its end -- the query's value is
// liblz4's there too.
//
// The query itself is decoded_size<Grp, FAST> at the end of lz4_decode_core.h (it needs decode_block).
// Backend (group_dev.h SizeWaveDev; tests/hostsim/hostsim_size.cpp on the CPU): the wave backend's stream ring and lane-parallel side,
// plus  sz_begin(lds)  and the ring's window  sz_lo, sz_avail  (the ring holds stream bytes [sz_lo, sz_avail); sz_lo > sz_avail: nothing).
#pragma once
#include <stdint.h>

namespace lz4hip {

// entry: ip <= iend - 306, op <= oend - 606.  Leaves with ip / op at the start of the first sequence it did not take.
template <class Grp>
LZ4HIP_DEV void decode_size_loop(Grp& g, const uint8_t* src, const int iend, const int oend, int& ip_io, int& op_io, uint8_t* lds) {
  typedef typename Grp::LChunk LChunk;
  typedef typename Grp::VU VU;
  typedef typename Grp::VB VB;
  constexpr uint32_t STEP = 256u;
  constexpr uint32_t AHEAD = 512u;   // stream bytes a trip may read from ip on: a sequence that starts at window position <= 250 has its offset word at <= 250 + 2 + 254 and reads 4 bytes there
  const uint32_t KS = g.wv_stream();
  uint32_t ip = (uint32_t)ip_io, op = (uint32_t)op_io;
  const uint32_t ilim = (uint32_t)iend - (uint32_t)LZ4HIP_DECODE_IN_MARGIN, olim = (uint32_t)oend - (uint32_t)LZ4HIP_DECODE_OUT_MARGIN;
  g.sz_begin(lds);
  uint32_t lo = g.sz_lo, avail = g.sz_avail;
  const VU lane = g.vlane();
  const VU p0 = lane * 4u;
  uint32_t Tprev = 0u;

  while ((ip <= ilim) & (op <= olim)) {
    // ---- the stream ring holds what this trip may read: [ip, ip + AHEAD), or the stream to its end.  It keeps everything from
    // ip & ~255 on and never more than KS bytes: steps are put below (ip & ~255) + KS only ----
    const uint32_t base = ip & ~(STEP - 1u);
    if ((base < lo) | (base > avail)) lo = avail = base;   // (first entry, or the exact code went past what the ring holds)
    while ((ip + AHEAD > avail) & (avail < (uint32_t)iend)) {
      // (room: avail < ip + 512 <= base + 767, so four steps end below base + 1791 + 256 <= base + KS for KS >= 2048; smaller rings take fewer)
      uint32_t nfull = ((uint32_t)iend - avail) >> 8;
      const uint32_t room = (base + KS - avail) >> 8;
      nfull = nfull < room ? nfull : room;
      nfull = nfull < 4u ? nfull : 4u;
      if (nfull != 0u) {   // up to four steps in flight together
        LChunk c0 = g.rs_fetch(src, avail), c1 = LChunk(), c2 = LChunk(), c3 = LChunk();
        if (nfull > 1u) c1 = g.rs_fetch(src, avail + STEP);
        if (nfull > 2u) c2 = g.rs_fetch(src, avail + 2u * STEP);
        if (nfull > 3u) c3 = g.rs_fetch(src, avail + 3u * STEP);
        g.rs_put(avail, c0);
        if (nfull > 1u) g.rs_put(avail + STEP, c1);
        if (nfull > 2u) g.rs_put(avail + 2u * STEP, c2);
        if (nfull > 3u) g.rs_put(avail + 3u * STEP, c3);
        avail += nfull * STEP;
      } else {             // the stream's last, partial step: its bytes below iend, zeros behind them
        g.rs_put(avail, g.rs_fetch_upto(src, avail, (uint32_t)iend));
        avail += STEP;
      }
    }
    // ---- refill, requested here and put into the ring at the end of the trip: two steps (a window whose starts are all taken
    // consumes more than one) while the ring has room for them ----
    uint32_t nf = 0u;
    LChunk rf0 = LChunk(), rf1 = LChunk();
    if ((avail + STEP <= (uint32_t)iend) & (avail + STEP <= base + KS)) {
      rf0 = g.rs_fetch(src, avail);
      nf = 1u;
      if ((avail + 2u * STEP <= (uint32_t)iend) & (avail + 2u * STEP <= base + KS)) {
        rf1 = g.rs_fetch(src, avail + STEP);
        nf = 2u;
      }
    }
    // ---- 1. discovery and walk (lz4_decode_wave.h): where a sequence that starts at window position p is followed by the next one,
    // a byte per position (255: not in this window, or nothing the walk may follow); posv: the k-th start, relative to ip, in lane k ----
    VU posv = VU(0u);
    uint32_t T = 0u;
    VU blo, bhi;
    g.vs_win(ip, blo, bhi);                     // stream bytes [ip + 4 l, + 8)
    {
      VU nxpack = VU(0u);
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {
        const VU w = j == 0u ? blo : ((blo >> (8 * (int)j)) | (bhi << (32 - 8 * (int)j)));   // bytes j, j + 1, ..
        const VU tl = (w >> 4) & 15u, e1 = (w >> 8) & 255u;
        const VB l15 = tl == 15u;
        // (a run of two or more length bytes makes this wrong -- and the sequence not one step 3 takes: the trip ends in front of it)
        const VU nxt = p0 + (j + 3u) + Grp::vsel(l15, VU(1u), VU(0u)) + tl + Grp::vsel(l15, e1, VU(0u)) + Grp::vsel((w & 15u) == 15u, VU(1u), VU(0u));
        nxpack = nxpack | (Grp::vsel(nxt <= 250u, nxt, VU(255u)) << (8 * (int)j));
      }
      if (Tprev >= 24u) Grp::vwalk_par(nxpack, lane, posv, T); else Grp::vwalk(nxpack, posv, T);
      Tprev = T;
    }
    // ---- 2. a lane per sequence: its header, its lengths, its output position ----
    const uint64_t actm = T >= 64u ? ~0ull : (1ull << T) - 1ull;   // (T >= 1: position 0 is a start)
    const VB act = Grp::vlanes(actm);
    const VU pv = Grp::vsel(act, posv, VU(0u));
    const VU sl = pv >> 2;
    const VU hw = Grp::valignbyte(Grp::vshfl(bhi, sl), Grp::vshfl(blo, sl), pv & 3u);
    const VU tl = (hw >> 4) & 15u, tm = hw & 15u, e1 = (hw >> 8) & 255u;
    const VB l15 = tl == 15u;
    const VU lit = tl + Grp::vsel(l15, e1, VU(0u));
    const VU lp = pv + Grp::vsel(l15, VU(2u), VU(1u));                       // where the literals start, relative to ip
    const VU ow = g.vs_ld32(lp + lit + ip);
    const VU off = ow & 0xFFFFu, e2 = (ow >> 16) & 255u;
    const VB m15 = tm == 15u;
    const VU mlx = tm + Grp::vsel(m15, e2, VU(0u));
    const VU endp = lp + lit + Grp::vsel(m15, VU(3u), VU(2u));               // where the next token lies, relative to ip
    const VU len = Grp::vsel(act, lit + mlx + 4u, VU(0u));
    const VU o = Grp::vexcl_scan(len) + op;                                   // the sequence's output position
    // ---- 3. the sequences in front of the first one that is not provably fine ----
    const uint64_t okm = actm & Grp::vballot(lit < 255u) & Grp::vballot(mlx < 255u) & Grp::vballot((pv + ip) <= VU(ilim)) & Grp::vballot(o <= VU(olim)) &
                         Grp::vballot(off <= (o + lit));
    const uint32_t Te = (uint32_t)__builtin_ctzll(~okm | (1ull << 63)) + ((okm == ~0ull) ? 1u : 0u);
    if (Te == 0u) break;                        // the sequence at ip is for the exact code
    if (Te < T) {
      op = Grp::vreadlane(o, Te);
      ip += Grp::vreadlane(pv, Te);
    } else {                                    // every start was taken: the next token lies behind the last sequence
      op = Grp::vreadlane(o, T - 1u) + Grp::vreadlane(len, T - 1u);
      ip += Grp::vreadlane(endp, T - 1u);
    }
    if (nf != 0u) {
      g.rs_put(avail, rf0);
      avail += STEP;
      if (nf == 2u) { g.rs_put(avail, rf1); avail += STEP; }
    }
    if (Te < T) break;                          // (its first sequence would end the next trip at once)
  }
  g.sz_lo = lo; g.sz_avail = avail;
  ip_io = (int)ip; op_io = (int)op;
}

}  // namespace lz4hip
