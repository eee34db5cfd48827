// container_write_rules.h -- the arithmetic of WRITING the data blocks of an LZ4 Frame (kind 0: size word, payload, optional XXH32 of the
// stored payload; LZ4FrameOutputStream.writeBlock) or of an lz4-java "LZ4Block" stream (kind 1: 21-byte header, payload;
// LZ4BlockOutputStream.flushBufferedData) for an item of src_len bytes cut into pieces of block_size bytes: how many blocks the item
// has, what surrounds a block's payload, the item's worst case, the LZ4Block token's level nibble, and where block k lies inside its
// item and how long it is.  Free of HIP, so that the host compiles it alone (lz4hip_container_blocks_many_bound, the stand-alone rules
// program of the tests) and the device compiles the very same text (container_layout_many_kernel, container.hip).  The numbers are
// those of launch_container_blocks (container.hip), which the many-call equals item by item.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4HIP_WRITE_RULES_FN __host__ __device__ __forceinline__
#else
#define LZ4HIP_WRITE_RULES_FN inline
#endif

namespace lz4hip {
namespace container_write_rules {

constexpr uint32_t kMinBlockSize = 64u, kMaxBlockSize = 32u << 20;   // LZ4BlockOutputStream.java:50-51
constexpr uint64_t kMaxItemBytes = 0x7FFFFFFFull;

// flags[c]: bit 0 a block checksum follows every payload (kind 0 only), bit 1 the caller wants the item's content hash
constexpr uint32_t kFlagBlockChecksum = 1u, kFlagContentHash = 2u, kFlagsDefined = 3u;

// ceil(src_len / block_size); an item of 0 bytes has no blocks
LZ4HIP_WRITE_RULES_FN uint32_t item_blocks(uint64_t src_len, uint32_t block_size) { return (uint32_t)((src_len + block_size - 1u) / block_size); }

// the bytes around one block's payload: the size word and, with block checksums, the hash word (frame); the header (LZ4Block)
LZ4HIP_WRITE_RULES_FN uint32_t block_fixed(int kind, uint32_t flags) { return kind == 0 ? 4u + 4u * (flags & kFlagBlockChecksum) : 21u; }
// ... and the part of it that lies in front of the payload
LZ4HIP_WRITE_RULES_FN uint32_t block_header(int kind) { return kind == 0 ? 4u : 21u; }

// the worst case of a block of len bytes: it is stored as it is when compression does not gain
LZ4HIP_WRITE_RULES_FN uint64_t block_bound(int kind, uint32_t flags, uint32_t len) { return (uint64_t)block_fixed(kind, flags) + len; }

// the worst case of an item with its gaps: the bound call's item_dst_bytes[c]
LZ4HIP_WRITE_RULES_FN uint64_t item_bound(int kind, uint32_t flags, uint64_t src_len, uint32_t block_size, uint32_t gap_head, uint32_t gap_tail) {
  return (uint64_t)gap_head + src_len + (uint64_t)item_blocks(src_len, block_size) * block_fixed(kind, flags) + gap_tail;
}

// the compress slot of a block of an item with this block size: LZ4_compressBound of a whole block, on a 16-byte boundary
LZ4HIP_WRITE_RULES_FN uint32_t slot_bytes(uint32_t block_size) { return (uint32_t)(((uint64_t)block_size + block_size / 255u + 16u + 15u) & ~15ull); }

// ... and of a block of THIS item: no block of it is longer than min(block_size, src_len), so a payload much smaller than its block size
// takes a slot by what it holds -- still LZ4_compressBound of every block it has, which is all the compressors ask of a slot
LZ4HIP_WRITE_RULES_FN uint32_t item_slot_bytes(uint64_t src_len, uint32_t block_size) { return slot_bytes(src_len < block_size ? (uint32_t)src_len : block_size); }

// LZ4BlockOutputStream.compressionLevel (:57-69): max(0, ceil(log2(blockSize)) - 10), the low nibble of an LZ4Block token
LZ4HIP_WRITE_RULES_FN uint32_t level_nibble(uint32_t block_size) {
  uint32_t cl = 0;
  while (cl < 32u && (1ull << cl) < (uint64_t)block_size) cl++;
  return cl < 10u ? 0u : cl - 10u;
}

// block k of the item: where it starts inside the item and how long it is
LZ4HIP_WRITE_RULES_FN uint64_t block_offset(uint32_t block_size, uint32_t k) { return (uint64_t)k * block_size; }
LZ4HIP_WRITE_RULES_FN uint32_t block_length(uint64_t src_len, uint32_t block_size, uint32_t k) {
  const uint64_t o = block_offset(block_size, k);
  return (uint32_t)(src_len - o < block_size ? src_len - o : block_size);
}

// the item of block b: first[] is the prefix sum of the items' block counts (n_items + 1 entries); items without blocks own no b
LZ4HIP_WRITE_RULES_FN uint32_t item_of_block(const uint32_t* first, uint32_t n_items, uint32_t b) {
  uint32_t lo = 0, hi = n_items;   // the last t in [0, n_items) with first[t] <= b
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// what can be said about one item without a device -> a message, or nullptr
LZ4HIP_WRITE_RULES_FN const char* item_error(int kind, uint64_t src_len, uint32_t block_size, uint32_t flags) {
  if (block_size < kMinBlockSize || block_size > kMaxBlockSize) return "block size must be 64 .. 32 MiB";
  if (src_len > kMaxItemBytes) return "an item's src_len must be at most 2^31 - 1";
  if (flags & ~kFlagsDefined) return "container flags: only bit 0 (block checksums) and bit 1 (content hash) are defined";
  if (kind == 1 && (flags & kFlagBlockChecksum)) return "container flags: bit 0 (block checksums) belongs to kind 0 (LZ4 Frame blocks) only";
  return nullptr;
}

}  // namespace container_write_rules
}  // namespace lz4hip
