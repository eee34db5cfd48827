// container_rules.h -- ONE step of the walk over the data blocks of an LZ4 Frame body (kind 0: size words, LZ4FrameInputStream.readBlock)
// or of an lz4-java "LZ4Block" stream (kind 1: 21-byte headers, LZ4BlockInputStream.refill): the header at a position of the body is
// read, the readers' header rules are applied in the readers' order, and the step says where the next header lies and what the block
// is -- or why the walk stops here.  Free of HIP, so that the host compiles it alone (the pre-walk of lz4hip_container_decode_many_bound,
// the stand-alone rules program of the tests) and the device compiles the very same text (container_walk_many_kernel, container.hip).
// The rules and their order are container_walk_kernel's (container.hip), which states them with the reference's line numbers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4HIP_RULES_FN __host__ __device__ __forceinline__
#else
#define LZ4HIP_RULES_FN inline
#endif

namespace lz4hip {
namespace container_rules {

// why a walk stops (info[2] of the container readers; include/lz4hip.h LZ4HIP_CR_*); STEP_NEXT: it does not, a block was taken
enum : uint32_t { STOP_END = 0, STOP_MORE = 1, STOP_TRUNCATED = 2, STOP_BLOCK_TOO_BIG = 3, STOP_BLOCK_CHECKSUM = 4, STOP_DECODE = 5, STOP_CORRUPT = 6, STOP_SLOTS = 7,
                  STEP_NEXT = 0xFFFFFFFFu };

struct Block {
  uint64_t next;       // where the walk stands behind this step: behind the block (STEP_NEXT), behind the end mark (STOP_END), else unchanged
  uint64_t pay_off;    // the stored payload: body[pay_off, + pay_len)
  uint32_t pay_len;
  uint32_t stored;     // the stored checksum word (frame, with block checksums) / the header's check field (LZ4Block)
  uint32_t cap;        // what the block may decode to: the decoder's capacity (frame) / the header's original length (LZ4Block); raw: pay_len
  uint32_t raw;        // 1: stored uncompressed
  uint64_t bound;      // what the block sizes in the destination, also for a frame block whose payload is cut short (the walk looks at
                       // it); 0: the header sizes nothing
};

LZ4HIP_RULES_FN uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The step at body[p]: kind 0 / 1; flags bit 0: the frame has block checksums; max_block: the frame's block maximum (LZ4Block: the
// biggest block the caller allows, 0 = any); slot_bytes: the room a decoded block has (UINT64_MAX: the pre-walk, which is what sizes it).
LZ4HIP_RULES_FN uint32_t step(const uint8_t* body, uint64_t body_bytes, uint64_t p, int kind, uint32_t flags, uint32_t max_block, uint64_t slot_bytes, Block& b) {
  b.next = p; b.pay_off = 0; b.pay_len = 0; b.stored = 0; b.cap = 0; b.raw = 0; b.bound = 0;
  if (p == body_bytes) return STOP_MORE;
  if (kind == 0) {
    const uint32_t cks = (flags & 1u) ? 4u : 0u;
    if (p + 4u > body_bytes) return STOP_TRUNCATED;
    const uint32_t word = rd32(body + p), size = word & 0x7FFFFFFFu;
    if (size == 0u) { b.next = p + 4u; return STOP_END; }
    if (size > max_block) return STOP_BLOCK_TOO_BIG;
    b.raw = (word & 0x80000000u) ? 1u : 0u;
    // (a compressed block decodes into max_block bytes of capacity, as in the reference: a smaller one could change which check a
    // damaged stream fails first)
    b.bound = b.raw ? size : max_block;
    const uint64_t need = 4ull + size + cks;
    if (p + need > body_bytes) return STOP_TRUNCATED;
    if (b.raw && size > slot_bytes) return STOP_BLOCK_TOO_BIG;
    b.pay_off = p + 4u; b.pay_len = size;
    b.cap = b.raw ? size : (max_block < slot_bytes ? max_block : (uint32_t)slot_bytes);
    if (cks) b.stored = rd32(body + p + 4u + size);
    b.next = p + need;
    return STEP_NEXT;
  }
  if (p + 21u > body_bytes) return STOP_TRUNCATED;
  const uint8_t* h = body + p;
  const char* magic = "LZ4Block";
  bool bad = false;
  for (int i = 0; i < 8; i++) bad |= h[i] != (uint8_t)magic[i];
  const uint32_t token = h[8], method = token & 0xF0u, level = 10u + (token & 0x0Fu);
  bad |= method != 0x10u && method != 0x20u;
  const int32_t clen = (int32_t)rd32(h + 9), olen = (int32_t)rd32(h + 13);
  const uint32_t check = rd32(h + 17);
  bad |= olen > (int32_t)(1u << level) || olen < 0 || clen < 0 || (olen == 0 && clen != 0) || (olen != 0 && clen == 0) || (method == 0x10u && olen != clen);
  if (bad) return STOP_CORRUPT;
  if (olen == 0) {                       // the empty block
    if (check != 0u) return STOP_CORRUPT;
    b.next = p + 21u;
    return STOP_END;
  }
  if (max_block != 0u && (uint32_t)olen > max_block) return STOP_BLOCK_TOO_BIG;   // (bigger than the caller allows: not a stream error)
  if (p + 21u + (uint64_t)clen > body_bytes) return STOP_TRUNCATED;
  // clen bytes of LZ4 decode to at most 255 x clen bytes: a header that announces more cannot decode, and sizes nothing
  if (method == 0x20u && (uint64_t)olen > 255ull * (uint64_t)clen + 64u) return STOP_CORRUPT;
  if ((uint64_t)olen > slot_bytes) return STOP_BLOCK_TOO_BIG;                      // (the slots are too small: not a stream error)
  b.raw = method == 0x10u ? 1u : 0u;
  b.pay_off = p + 21u; b.pay_len = (uint32_t)clen;
  b.cap = (uint32_t)olen;
  b.stored = check;
  b.bound = (uint64_t)olen;
  b.next = p + 21u + (uint64_t)clen;
  return STEP_NEXT;
}

// What a walk of at most n_max blocks from the start of the body comes to; table (may be nullptr): the blocks it takes, n_max entries.
struct Walk { uint32_t blocks; uint32_t why; uint64_t pos; uint64_t dst_bytes; uint64_t slot_max; };
LZ4HIP_RULES_FN Walk walk(const uint8_t* body, uint64_t body_bytes, int kind, uint32_t flags, uint32_t max_block, uint64_t slot_bytes, uint32_t n_max, Block* table) {
  Walk w{0u, STOP_SLOTS, 0ull, 0ull, 0ull};
  while (w.blocks < n_max) {
    Block b;
    const uint32_t r = step(body, body_bytes, w.pos, kind, flags, max_block, slot_bytes, b);
    if (b.bound > w.slot_max) w.slot_max = b.bound;
    w.pos = b.next;
    if (r != STEP_NEXT) { w.why = r; break; }
    if (table) table[w.blocks] = b;
    w.dst_bytes += b.bound;
    w.blocks++;
  }
  if (w.blocks == n_max && w.pos == body_bytes) w.why = STOP_MORE;   // (every slot used and nothing left: not "more follows")
  return w;
}

}  // namespace container_rules
}  // namespace lz4hip
