// lz4_decode_inorder.h -- the in-order tier of the block decoder: a block whose slot overlaps the history it can reach.
//
// The stream decoder (lz4_decode_stream.h) lets a block land anywhere.  In a ring no larger than LZ4_decoderRingBufferSize(), and in
// a small ring kept in step with the encoder's, a block's slot [d, d + cap) overlaps the external dictionary the block's matches may
// read: the block overwrites, sequence by sequence, bytes that its own later sequences still need -- and must not overwrite a byte
// before every earlier sequence that reads it has read it.  decode_block's copies take liberties that are invisible while slot and
// history are disjoint (wild copies that touch bytes past a run's end, sequences loaded in one trip and stored in the next, whole
// steps of 64 bytes); here each of them can change a decoded byte.  The contract of this tier is THE PLAIN DEFINITION:
//
//   a block is decoded sequence by sequence; within a sequence the literals come first, then the match, byte by byte, forward;
//   each byte is read at the moment it is due; nothing is stored past the last byte of a sequence.
//
// which is what liblz4 1.9.3 computes wherever liblz4 itself does not overwrite a source before reading it (its 32-byte literal
// steps and 8-byte safe-loop steps do, for a source less than 31 bytes ahead of its destination: include/lz4hip.h says where).
//
// decode_block_inorder IS decode_block -- the same function, so every check, every tier's accept / reject rule and every return value
// is the core's own: control flow never depends on a copied byte -- run on a backend whose copies obey three rules:
//   (a) no early loads across sequences: a copy whose source may lie in the window (a match, a dictionary copy) is issued behind
//       Base::order(), which waits for every store issued so far -- the sequences in front of it, and the blocks in front of those;
//   (b) no over-stores: every copy is exact in extent, literals too (`wild` is ignored, the wide copies are the exact ones);
//   (c) forward copies in order: chunks of the group's width, a chunk's loads before its stores, chunks in program order
//       (Base::copy_fwd).  A source IN FRONT of its destination (the overlap case) is byte-forward by construction: chunk k reads
//       bytes that only chunks >= k overwrite.  A source less than a chunk BEHIND its destination is the pattern copy the core
//       already has (Base::copy_match's replicate path, which reads nothing but the bytes in front of the destination).  A source
//       k bytes behind its destination, a chunk <= k < the copy's length, is copied in pieces of k bytes with order() between them:
//       a piece reads what the piece before it stored.  A dictionary match that runs past dict_end continues at the block's or
//       prefix's start through dict_match_copy, as ever.
// THE ORDERING RELIED ON: none beyond order().  No copy ever loads a byte that the same copy, or a copy in front of it, stored without
// an order() between the store and the load -- Base::copy_fwd and the replicate path read only bytes that were complete when they
// began.  (The core's other tiers rely on a wavefront's memory operations executing in order; this tier does not need to.)  The lane
// simulator's backend holds the tier to exactly that: its stores reach memory only at order() and at a block's end.
// -DLZ4HIP_INORDER_NO_SYNC=1 (the lane simulator's mutant build alone) compiles the wait out.
// The plain interior loop runs too (its checks are the cheap ones); the pipelined, deep and staged loops never do (PIPE = 0).
//
// InOrder<Base> derives from the backend and shadows its four copies, so one object serves both kinds of block: the stream walk
// hands `static_cast<Base&>(g)` to decode_block for a block whose slot is clear, and `g` itself to decode_block_inorder.
// Base: csrc/group_dev.h GroupDev on the GPU, the lock-step lane simulator's backend in the CPU test-suite; beside decode_block's
// interface it has  copy_fwd(d, s, len)  (rule (c)) and, where the hardware needs a wait, a static  order().
#pragma once
#include <stdint.h>
#include "lz4_decode_core.h"

#ifndef LZ4HIP_INORDER_NO_SYNC
#define LZ4HIP_INORDER_NO_SYNC 0
#endif
namespace lz4hip {

template <class G, class = void> struct has_order { static constexpr bool value = false; };
template <class G> struct has_order<G, decltype((void)&G::order)> { static constexpr bool value = true; };

template <class Base>
struct InOrder : Base {
  typedef Base Plain;
  static constexpr bool kInOrder = true;
  using Base::Base;
  const uint8_t* lit_lo = nullptr;   // the compressed block [lit_lo, lit_hi): a copy from there is a literal run, whose source no store touches
  const uint8_t* lit_hi = nullptr;

  LZ4HIP_DEV void sync() {
    if constexpr (has_order<Base>::value && !LZ4HIP_INORDER_NO_SYNC) Base::order();
  }
  // d[0..len) = s[0..len), byte-forward, whatever lies where
  LZ4HIP_DEV void forward(uint8_t* d, const uint8_t* s, uint32_t len) {
    if (!(s >= lit_lo && s < lit_hi)) sync();
    const uint32_t chunk = (uint32_t)Base::step() / (uint32_t)Base::slack();   // lanes of the group: copy_fwd's chunk
    if (s < d && (uint32_t)(d - s) < chunk) {
      Base::copy_match(d, 0u, (uint32_t)(d - s), len, false);
    } else if (s < d && (uint32_t)(d - s) < len) {   // the source runs into what this copy stores: pieces of d - s bytes, each behind a wait
      const uint32_t k = (uint32_t)(d - s);
      for (uint32_t o = 0; o < len; o += k) {
        if (o) sync();
        Base::copy_fwd(d + o, s + o, len - o < k ? len - o : k);
      }
    } else {
      Base::copy_fwd(d, s, len);
    }
  }
  LZ4HIP_DEV void copy_lits(uint8_t* d, const uint8_t* s, uint32_t len, bool) { forward(d, s, len); }
  LZ4HIP_DEV void copy_lits_wide(uint8_t* d, const uint8_t* s, uint32_t len) { forward(d, s, len); }
  LZ4HIP_DEV void copy_match(uint8_t* dst, uint32_t op, uint32_t offset, uint32_t len, bool) {
    sync();
    Base::copy_match(dst, op, offset, len, false);
  }
  LZ4HIP_DEV void copy_match_wide(uint8_t* dst, uint32_t op, uint32_t offset, uint32_t len) { copy_match(dst, op, offset, len, false); }
};

// decode_block's arguments and decode_block<.., SAFE, .., DICT, PREFIX>'s result on every input, valid or malformed; Grp = InOrder<Base>
template <class Grp, bool DICT, bool PREFIX>
LZ4HIP_DEV int decode_block_inorder(Grp& g, const uint8_t* src, int src_size, uint8_t* dst, int out_size, uint8_t* stage = nullptr,
                                    const uint8_t* dict_end = nullptr, int dict_len = 0, int hist = 0) {
  static_assert(Grp::kInOrder, "decode_block_inorder runs on an InOrder<Base> backend");
  g.lit_lo = src;
  g.lit_hi = src + (src_size > 0 ? src_size : 0);
  return decode_block<Grp, true, 0, false, false, DICT, PREFIX>(g, src, src_size, dst, out_size, stage, dict_end, dict_len, hist);
}

}  // namespace lz4hip
