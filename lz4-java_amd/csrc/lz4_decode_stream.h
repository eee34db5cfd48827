// lz4_decode_stream.h -- the walk over one stream's blocks of a launch (LZ4_decompress_safe_continue, liblz4 1.9.3, in EVERY mode of
// its LZ4_streamDecode_t), shared by decode_stream.hip and the CPU lane simulator (tests/hostsim/hostsim_dstream.cpp).
//
// lz4_decode_chain.h decodes chains whose blocks lie back to back: liblz4's rolling-prefix mode.  Here a block may land anywhere -- a
// ring that wraps, two alternating buffers, a block area behind a save area, a stream that starts from a dictionary elsewhere -- and
// the stream's state says which of liblz4's decoders a block gets.  The state is liblz4's four fields, as offsets into the one
// destination base (kernels.h DStreamState): the prefix [prefix_end - prefix_len, prefix_end) is what was decoded contiguously last,
// the external dictionary [ext_end - ext_len, ext_end) is what the prefix was before the last jump.  For block i at d = dst_off[i]:
//   prefix_len == 0                    LZ4_decompress_safe                                    r > 0: prefix = [d, d + r)
//   prefix_end == d, prefix >= 65535   ..._withPrefix64k (ext ignored)          PREFIX        r > 0: the prefix grows by r
//                    ext_len == 0      ..._withSmallPrefix(prefix_len)          PREFIX        "
//                    else              ..._doubleDict(prefix_len, ext)          PREFIX && DICT "
//   else (a jump)                      ext = prefix, BEFORE decoding and whatever r is;
//                                      ..._forceExtDict(ext)                    DICT          r > 0: prefix = [d, d + r)
// r <= 0 leaves the prefix as it was.  (So a 0-byte block at a new place drops the old external dictionary and leaves the prefix
// standing as its own external dictionary: liblz4's behaviour, reproduced.)  A negative result ends the stream's part of the launch:
// the blocks behind it get kChainStopped and the state written back is the one in front of the failed block -- with the jump's
// ext = prefix if the failed block was a jump.  A negative src_len / dst_cap counts as a block liblz4 answered with -1.
//
// Two instances of decode_block serve the five rows: PREFIX (hist == 0 is the plain decoder) and PREFIX && DICT (hist == 0 is the
// dictionary decoder).  A stream that never jumps runs exactly the instance chain_walk runs.
//
// ONE lane group walks a stream's blocks in order, `io.fence()` between two blocks, as in chain_walk; nothing waits for another group.
// Io: get_state(c) / put_state(c, s), put_out(i, r) (one lane writes), fence(), begin_block(d, cap): the block about to be decoded may
// write [d, d + cap) and nothing else (the simulator's bounds; nothing on the device).
#pragma once
#include <stdint.h>
#include "kernels.h"
#include "lz4_decode_core.h"
#include "lz4_decode_inorder.h"

namespace lz4hip {

// INORDER walks (below): does the slot [doff, doff + cap) of a block intersect the piece of the external dictionary the block can reach --
// the last min(ext_len, 65535 - min(the prefix the block grows, 65535)) bytes in front of ext_end, from the state AFTER a jump's
// ext = prefix?  (A growing prefix ends where the slot begins: it never overlaps.  Without a prefix the block is decoded plain and
// reaches nothing.)
LZ4HIP_DEV bool dstream_slot_overlaps(const DStreamState& s, bool grows, uint64_t doff, int cap) {
  if (cap <= 0 || s.prefix_len == 0 || s.ext_len == 0) return false;
  const uint64_t pre = grows ? (s.prefix_len < 65535u ? s.prefix_len : 65535u) : 0u;
  const uint64_t reach = s.ext_len < 65535u - pre ? s.ext_len : 65535u - pre;
  return reach != 0 && doff < s.ext_end && doff + (uint64_t)cap > s.ext_end - reach;
}
template <class Grp, bool INORDER> struct dstream_plain { typedef Grp type; };
template <class Grp> struct dstream_plain<Grp, true> { typedef typename Grp::Plain type; };

// PIPE: as chain_walk's.  INORDER (Grp = InOrder<Base>, lz4_decode_inorder.h; Io has in_order(bool) beside the rest): a block whose slot
// overlaps the dictionary piece it can reach -- or every block, with `every` -- is decoded by decode_block_inorder; every other block by
// exactly the decode_block instance it gets without INORDER, on the plain backend
template <class Grp, class Io, int PIPE = 2, bool INORDER = false>
LZ4HIP_DEV void dstream_walk(Grp& g, Io& io, const DStreamArgs& a, uint32_t c, uint8_t* stage, bool every = false) {
  typedef typename dstream_plain<Grp, INORDER>::type Plain;
  Plain& pg = g;
  uint32_t b1 = a.chain_first[c + 1], b0 = a.chain_first[c];
  if (b1 > a.n_blocks) b1 = a.n_blocks;
  if (b0 > b1) b0 = b1;
  DStreamState s = io.get_state(c);
  uint32_t i = b0;
  while (i < b1) {
    const int32_t sl = a.src_len[i], dc = a.dst_cap[i];
    const uint64_t doff = a.dst_off[i];
    uint8_t* const d = a.dst + doff;
    const int cap = dc > kChainBlockCapMax ? kChainBlockCapMax : dc;
    const bool grows = s.prefix_len != 0 && s.prefix_end == doff;   // the block lands where the prefix ends
    if (s.prefix_len != 0 && !grows) { s.ext_len = s.prefix_len; s.ext_end = s.prefix_end; }   // a jump: the prefix becomes the dictionary
    int r;
    if (sl < 0 || dc < 0) {
      r = -1;
    } else {
      const uint8_t* src = a.src + a.src_off[i];
      io.begin_block(d, cap);
      bool ino = false;
      if constexpr (INORDER) { ino = every || dstream_slot_overlaps(s, grows, doff, cap); io.in_order(ino); }
      if (s.prefix_len == 0) {
        if constexpr (INORDER) { if (ino) r = decode_block_inorder<Grp, false, true>(g, src, sl, d, cap, stage, nullptr, 0, 0); }
        if (!ino) r = decode_block<Plain, true, PIPE, false, false, false, true>(pg, src, sl, d, cap, stage, nullptr, 0, 0);
      } else if (grows && (s.prefix_len >= 65535u || s.ext_len == 0)) {
        const int hist = s.prefix_len >= 65535u ? 65535 : (int)s.prefix_len;
        if constexpr (INORDER) { if (ino) r = decode_block_inorder<Grp, false, true>(g, src, sl, d, cap, stage, nullptr, 0, hist); }
        if (!ino) r = decode_block<Plain, true, PIPE, false, false, false, true>(pg, src, sl, d, cap, stage, nullptr, 0, hist);
      } else {   // doubleDict (a prefix of less than 65535 bytes in front of d) or, after a jump, forceExtDict (none)
        const int dl = s.ext_len >= 65536u ? 65536 : (int)s.ext_len;   // (from 64 KB on liblz4 rejects no offset; only the last 65535 bytes are read)
        if constexpr (INORDER) { if (ino) r = decode_block_inorder<Grp, true, true>(g, src, sl, d, cap, stage, a.dst + s.ext_end, dl, grows ? (int)s.prefix_len : 0); }
        if (!ino) r = decode_block<Plain, true, PIPE, false, false, true, true>(pg, src, sl, d, cap, stage, a.dst + s.ext_end, dl, grows ? (int)s.prefix_len : 0);
      }
    }
    io.put_out(i, r);
    i++;
    if (r < 0) break;
    if (r > 0) {
      if (grows) { s.prefix_len += (uint64_t)r; s.prefix_end += (uint64_t)r; }
      else { s.prefix_len = (uint64_t)r; s.prefix_end = doff + (uint64_t)r; }
    }
    io.fence();
  }
  for (; i < b1; i++) io.put_out(i, kChainStopped);
  io.put_state(c, s);
}

}  // namespace lz4hip
