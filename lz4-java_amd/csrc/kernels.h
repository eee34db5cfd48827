// kernels.h -- host-callable launchers of the gfx950 kernels (one csrc/*.hip unit per kernel family).  All pointers are device
// pointers; launches are asynchronous on `stream`.  Return value: hipError_t as int.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace lz4hip {

struct BatchArgs {
  const uint8_t* src; const uint64_t* src_off; const int32_t* src_len;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap;
  int32_t* out; uint32_t n;
};

// compute units of the current device (cached per device; 256 where the runtime cannot say)
uint32_t device_cus();

// Fast compress, two kernels (same bytes):
//   launch_compress_fast_v2w lean finder loop (lz4_fast_v2_core.h; common step hand-scheduled, lz4_fast_v2_asm.h) with a writer
//                            wavefront per finder: bare hits parked in lanes, handed over 64 at a time: the default
//   launch_compress_fast_ms  every sequence of a 64-position window per step (lz4_fast_ms_core.h): best when sequences are short
// Both fill each CU with one workgroup of 5 finder wavefronts (5 x 32 KB tables = the CU's whole LDS) that draw blocks from a queue.
// q = three device uint32_t (queue words), n_cus = compute units of the device.
// Adaptive two-pass use: launch_compress_fast_v2w(q, routed = u32[n] device scratch, dense64) finishes the blocks with long
// sequences and lists the others in routed[] (sequences 32..95 cover fewer than dense64 bytes); launch_compress_fast_ms(q, routed,
// first = false) then does exactly those.  routed == nullptr: the kernel does every block (first = true zeroes q).
// `mail`: compress_fast_v2w_scratch_words(n_cus) words of device scratch (the finder/writer rings)
size_t compress_fast_v2w_scratch_words(uint32_t n_cus);
int launch_compress_fast_v2w(const BatchArgs& a, uint32_t* q, uint32_t* routed, uint32_t dense64, uint32_t n_cus, uint32_t* mail, void* stream);
// 1 (default): blocks of 65547 bytes .. 4 MiB run on ten pairs per CU with compact table entries (compress_fast_v2wp_cu_kernel); 0: five pairs for all
void set_compress_pack(int v);
int launch_compress_fast_ms(const BatchArgs& a, uint32_t* q, const uint32_t* routed, bool first, uint32_t n_cus, void* stream);
// LZ4_compress_fast(..., accel) for accel 2 .. 65537 (clamped by the caller; acceleration 1 is launch_compress_fast_v2w's): the
// one-sequence-per-step core of lz4_fast_core.h with its ACC switch, five wavefronts per CU drawing blocks from q = one device uint32_t
int launch_compress_fast_accel(const BatchArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream);
// What LZ4_loadDict keeps of a dictionary of `len` bytes: nothing below 8 bytes (it returns 0 and the stream has no dictionary), else
// the last 64 KB
constexpr uint32_t dict_keep(int32_t len) { return len < 8 ? 0u : (len > 65536 ? 65536u : (uint32_t)len); }
// LZ4_loadDict + LZ4_compress_fast_continue(acceleration 1) on a fresh stream per block, all blocks against one dictionary: the
// one-sequence core with its DICT switch (byU32 at every size), five wavefronts per CU drawing blocks from q = one device uint32_t.
// [dict_end - keep, dict_end) is the dictionary's kept tail in device memory and `image` its table image (launch_dict_image), both
// unused with keep == 0 (a dictionary under 8 bytes is none); keep is dict_keep()'s value: 0 or 8 .. 65536
int launch_compress_fast_dict(const BatchArgs& a, const uint8_t* dict_end, int32_t keep, const void* image, uint32_t* q, uint32_t n_cus,
                              void* stream);
// the table LZ4_loadDict leaves for the kept tail [tail, tail + keep), keep >= 8, in the DICT core's entry layout: kDictImageBytes
// bytes of device memory at `image` (dict_image_build of lz4_fast_core.h, one wavefront)
constexpr size_t kDictImageBytes = 32768;
int launch_dict_image(const uint8_t* tail, int32_t keep, void* image, void* stream);
// LZ4_compress_destSize: a.dst_cap[i] is the target size; out[i] = bytes written, consumed[i] = input consumed (src_len[i] where
// liblz4 returns 0 without touching it).  The one-sequence core with DirectOut's FILL switch, five wavefronts per CU drawing blocks
// from q = one device uint32_t
int launch_compress_dest_size(const BatchArgs& a, int32_t* consumed, uint32_t* q, uint32_t n_cus, void* stream);
#ifdef LZ4HIP_DEV_TOOLS
int launch_compress_fast_prof(const BatchArgs& a, uint64_t* prof, int core, void* stream);  // developer build only (tools/build_variant.sh dev -DLZ4HIP_DEV_TOOLS)
#endif
// HC levels 1..12: `ws` = device workspace of hc_ws_bytes(span, n, level) bytes, span = max(src_off+src_len) (launch_hc_span)
int launch_hc_span(const uint64_t* src_off, const int32_t* src_len, uint32_t n, uint64_t* out_dev, void* stream);
size_t hc_ws_bytes(uint64_t span, uint32_t n_blocks, int level);
int launch_compress_hc(const BatchArgs& a, int level, void* ws, uint64_t span, void* stream);
// LZ4_compress_HC_destSize: a.dst_cap[i] is the target size; out[i] = bytes written, consumed[i] = input consumed (src_len[i] where
// liblz4 returns 0 without touching it).  hc_build_kernel as it is, then hc_parse_dest_kernel (the parser's FILL switch); same
// workspace as launch_compress_hc.  The parse of a block stops once its target is full, so the parse time follows the input
// consumed; the delta[] build still covers the whole block.
int launch_compress_hc_dest(const BatchArgs& a, int32_t* consumed, int level, void* ws, uint64_t span, void* stream);
// LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream per block, all blocks against one dictionary (external-dictionary mode):
// hc_build_dict_kernel + hc_parse_dict_kernel, same workspace as launch_compress_hc.  [dict_end - K, dict_end) is the dictionary's
// kept tail in device memory, K = hc_dict_keep(its length) = 0 .. 65536 (K == 0: dict_end is not looked at), `image` its image:
// hc_dict_image_bytes(K) bytes of device memory filled by launch_hc_dict_image (one wavefront; the image does not depend on the level)
constexpr uint32_t hc_dict_keep(int32_t len) { return len > 65536 ? 65536u : (uint32_t)len; }
constexpr size_t hc_dict_image_bytes(uint32_t K) { return 131072u + 2u * (size_t)K; }
int launch_hc_dict_image(const uint8_t* tail, uint32_t K, void* image, void* stream);
int launch_compress_hc_dict(const BatchArgs& a, int level, void* ws, uint64_t span, const uint8_t* dict_end, uint32_t K, const void* image,
                            void* stream);
// after a compress launch: moves the out[i] > 0 useful bytes of every slot to pack + sum(out[0..i)); poff: u64[n] scratch
int launch_pack(const BatchArgs& a, uint64_t* poff, uint8_t* pack, void* stream);
// Device-side container assembly (container.hip): the data blocks of an LZ4 Frame (kind 0; block_checksum: XXH32 of each stored
// payload) or of lz4-java's LZ4Block container (kind 1) for src[0, n_bytes) cut into block_size pieces -> dst, *total = bytes
// written (if it exceeds dst_cap nothing past dst_cap was written and the caller must not use the result).  ws: device scratch of
// container_ws_bytes(); hc_level > 0: LZ4 HC at that level (hc_ws = hc_ws_bytes(n_bytes, n, level)), else the fast compressor
// (q_scratch = 3 + n + compress_fast_v2w_scratch_words(n_cus) words; core as "compress_core").
size_t container_ws_bytes(uint64_t n_bytes, uint32_t block_size);
int launch_container_blocks(int kind, int block_checksum, int hc_level, const uint8_t* src, uint64_t n_bytes, uint32_t block_size, uint8_t* dst, uint64_t dst_cap,
                            unsigned long long* total, void* ws, void* hc_ws, uint32_t* q_scratch, uint32_t dense64, uint32_t n_cus, int core, void* stream);
// Device-side container READ path (container.hip): the data blocks of an LZ4 Frame body (kind 0; block_checksum: a XXH32 word behind
// each payload) or of an LZ4Block stream (kind 1) in body[0, body_bytes) are walked, verified and decoded; block k decodes to
// dst + k * slot_bytes, sizes[k] = its decoded size, info[0..4] = {blocks delivered, body bytes consumed, stop reason, decoded bytes,
// liblz4 code of a failed decode}; ws = container_read_ws_bytes(n_max) bytes of device scratch
size_t container_read_ws_bytes(uint32_t n_max);
int launch_container_read(int kind, int block_checksum, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint8_t* dst, uint64_t slot_bytes,
                          uint32_t n_max, int32_t* sizes, unsigned long long* info, void* ws, void* stream);
// The read path over MANY containers of one kind at once (container.hip): item t's body is bodies[body_off[t], + body_len[t]) with its
// own max_block[t] and flags[t] (bit 0: block checksums); it owns the entries [first[t], first[t + 1]) of the batch arrays -- the whole
// blocks the host's pre-walk found in it plus one -- and the slots dst + dst_base[t] + k * slot[t].  Per item info[5t .. 5t + 4] as
// above; the delivered blocks' sizes lie back to back in sizes[item_first[t] ..) and their bytes in pack[item_dst_off[t] ..), item after
// item (item_first, item_dst_off: n_items + 1 entries, the last one the total).  n_max: the most blocks one item delivers; n_entries =
// first[n_items]; ws = container_many_ws_bytes(n_entries, n_items) bytes of device scratch; any_block_checksum: some flags[t] has bit 0
struct ContainerManyItems {
  const uint64_t* body_off; const uint64_t* body_len; const uint64_t* dst_base; const uint32_t* slot; const uint32_t* max_block; const uint32_t* first;
  const uint8_t* flags;
};
size_t container_many_ws_bytes(uint32_t n_entries, uint32_t n_items);
int launch_container_read_many(int kind, bool any_block_checksum, const uint8_t* bodies, const ContainerManyItems& items, uint32_t n_items, uint32_t n_entries,
                               uint32_t n_max, uint8_t* dst, uint8_t* pack, int32_t* sizes, unsigned long long* info, uint32_t* item_first,
                               unsigned long long* item_dst_off, void* ws, void* stream);
// The write sequence over MANY items of one kind at once (container.hip): item t is src[src_off[t], + src_len[t]) cut into pieces of
// block_size[t] bytes, with its own flags[t] (bit 0: block checksums, kind 0 only) and gap_head[t] / gap_tail[t] zero bytes in front of
// and behind its blocks; it owns the blocks [first[t], first[t + 1]) and the compress slots from slot_base[t] on, which are
// container_write_rules::item_slot_bytes(src_len[t], block_size[t]) bytes apart.  The items' bytes lie back to back in dst from
// item_dst_off[t] on (n_items + 1 entries, the last one the total); when any_content_hash, content_hash[t] = XXH32(seed 0) of the item's
// first hash_len[t] bytes: src_len[t] for an item that asks, 0 for one that does not.  Every array is device
// memory; ws = container_write_many_ws_bytes(n_blocks, the slots' bytes) of scratch; hc_ws, q_scratch, dense64, n_cus, core as in
// launch_container_blocks, hc_ws sized for src_span = the end of the last item's source.  n_blocks + n_items <= 2^31 - 1.
struct ContainerWriteManyItems {
  const uint64_t* src_off; const int32_t* src_len; const int32_t* hash_len; const uint64_t* slot_base; const uint32_t* block_size; const uint32_t* first;
  const uint32_t* gap_head; const uint32_t* gap_tail; const uint8_t* flags;
};
size_t container_write_many_ws_bytes(uint32_t n_blocks, uint64_t slot_bytes_total);
int launch_container_blocks_many(int kind, int hc_level, bool any_block_checksum, bool any_content_hash, const uint8_t* src, uint64_t src_span,
                                 const ContainerWriteManyItems& items, uint32_t n_items, uint32_t n_blocks, uint8_t* dst, uint64_t dst_cap,
                                 unsigned long long* item_dst_off, uint32_t* content_hash, void* ws, void* hc_ws, uint32_t* q_scratch, uint32_t dense64,
                                 uint32_t n_cus, int core, void* stream);
// lanes_per_block: lanes of a wavefront that share one block in the decoder (4..64); 0 = default
// pipe: 1 = pipelined interior loop (lz4_decode_core.h PIPE), 0 = plain, -1 = default for the batch size
// stage: 1 = the plain interior loop writes through LDS staging (whole-line output), 0 / -1 = off
// pipe 3: the ring loop (lz4_decode_ring.h); ring = bytes of its output ring (512 / 1024 / 2048 / 4096; 0 = default for the lanes)
// route_word: one device uint32_t of scratch (or nullptr): with every knob at its default, batches of more than 16 blocks per CU are routed
// on the device (decode_route_kernel): by the blocks' compressed sizes between the deep loop and the ring loop (12288 .. 40959 blocks), by
// the streams' sequence density between the lane-group loops and the wave kernel (set_route_short: average output bytes per sequence up to which a batch is text-like, 0 = never) and between the staged and the deep loop (40960 blocks and more: near sources)
void set_route_short(int bytes_per_sequence);
int last_decode_route(uint32_t* out8);   // diagnostic (8 words): {route, sampled hops, sampled stream bytes, average compressed size, offsets within 6 KB, sequences looked at, their output bytes, 0} of the current device's last routed launch (synchronises)
int launch_decompress(const BatchArgs& a, bool safe, int lanes_per_block, int pipe, int stage, int ring, void* stream, uint32_t* route_word = nullptr);
// LZ4_decompress_safe_partial: block i decodes into min(target[i], a.dst_cap[i]) bytes (-1 where one of them or src_len[i] is
// negative); out[i] = liblz4's return value.  >= 40960 blocks: decode_partial_kernel<4, 0, true> (staged), fewer:
// decode_partial_deep_kernel<8>; the decode knobs and the device-side route do not apply
int launch_decompress_partial(const BatchArgs& a, const int32_t* target, void* stream);
// LZ4_decompress_safe_usingDict (a dictionary that is not contiguous with the destination): every block decodes against the one
// dictionary [dict_end - dict_len, dict_end) in device memory, of which only the last 64 KB are read (dict_len == 0: the plain safe
// decoder, dict_end is not looked at); out[i] = liblz4's return value.  >= 40960 blocks: decode_dict_kernel<4, 0, true> (staged),
// fewer: decode_dict_deep_kernel<8>; the decode knobs and the device-side route do not apply
int launch_decompress_dict(const BatchArgs& a, const uint8_t* dict_end, int32_t dict_len, void* stream);
// LZ4_decompress_safe_continue over chains of linked blocks (decode_chain.hip, lz4_decode_chain.h).  Chain c is the blocks
// [chain_first[c], chain_first[c + 1]); their decoded forms lie back to back from dst + chain_dst_off[c] on, in at most chain_dst_cap[c]
// bytes, behind chain_prefix_len[c] bytes of history (chain_prefix_len == nullptr: none).  Block i gets the capacity
// min(dst_cap[i], what is left of the chain's, kChainBlockCapMax); stored (may be nullptr): stored[i] != 0 marks a raw block, copied
// verbatim.  out[i] = liblz4's return value (a raw block: src_len[i], or -1 if it does not fit; a negative src_len / dst_cap: -1),
// kChainStopped for the blocks behind a chain's first negative result; chain_out[c] = the bytes chain c decoded before it stopped.
// The walk trusts nothing it reads from the arrays: a chain's block range is cut to [0, n_blocks] and its history to its offset into dst.
struct ChainArgs {
  const uint8_t* src; const uint64_t* src_off; const int32_t* src_len; const uint8_t* stored; const int32_t* dst_cap;
  const uint32_t* chain_first;
  uint8_t* dst; const uint64_t* chain_dst_off; const uint64_t* chain_dst_cap; const int32_t* chain_prefix_len;
  int32_t* out; uint64_t* chain_out; uint32_t n_blocks, n_chains;
};
constexpr int32_t kChainStopped = INT32_MIN + 6;          // include/lz4hip.h LZ4HIP_CHAIN_STOPPED
constexpr int32_t kChainBlockCapMax = INT32_MAX - 65535;  // (a block's capacity plus 65535 bytes of history is counted in an int)
// decode_chain_kernel<8>: lane groups of 8 draw chains from the queue word q (one device uint32_t of scratch) and walk each chain's
// blocks in order; no group waits for another anywhere.  n_cus = compute units of the device
int launch_decompress_chain(const ChainArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// LZ4_decompress_safe_continue on streams whose blocks land anywhere (decode_stream.hip, lz4_decode_stream.h): every mode of liblz4
// 1.9.3's LZ4_streamDecode_t, not the rolling prefix alone.  Stream c is the blocks [chain_first[c], chain_first[c + 1]); block i is
// decoded to dst + dst_off[i] with the capacity min(dst_cap[i], kChainBlockCapMax).  state[c] is liblz4's four fields as offsets into
// dst (include/lz4hip.h lz4hip_dstream_state), read at the stream's first block of the launch and written back behind its last.
// out[i] = liblz4's return value (a negative src_len / dst_cap: -1), kChainStopped for the blocks behind a stream's first negative
// result.  The walk trusts nothing it reads from the arrays: a stream's block range is cut to [0, n_blocks].
struct DStreamState { uint64_t prefix_end, prefix_len, ext_end, ext_len; };
struct DStreamArgs {
  const uint8_t* src; const uint64_t* src_off; const int32_t* src_len; const uint32_t* chain_first;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap;
  DStreamState* state; int32_t* out; uint32_t n_blocks, n_chains;
};
// decode_stream_kernel<8>: decode_chain_kernel's shape -- lane groups of 8 draw streams from the queue word q (one device uint32_t
// of scratch) and walk each stream's blocks of this launch in order; no group waits for another anywhere.  n_cus = compute units
int launch_decompress_stream(const DStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// The same streams where a block's slot may overlap the history the block can reach (minimal rings; lz4_decode_inorder.h): the call's
// arrays and records, and `every`: 0 = a block is decoded in order (decode_block_inorder) iff its slot overlaps the piece of the external
// dictionary it can reach (lz4_decode_stream.h dstream_slot_overlaps), else by the instance decode_stream_kernel gives it; 1 = every block
struct DStreamInorderArgs { DStreamArgs s; uint32_t every; };
// decode_stream_inorder_kernel<8>: decode_stream_kernel's shape and queue word
int launch_decompress_stream_inorder(const DStreamInorderArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// LZ4_compress_fast_continue(acceleration 1) over chains of linked blocks (compress_fast.hip, lz4_fast_chain.h).  Chain c is the blocks
// [chain_first[c], chain_first[c + 1]); their SOURCES lie back to back from src + chain_src_off[c] on, behind chain_prefix_len[c] bytes
// of history (chain_prefix_len == nullptr: none) that the stream has loaded with LZ4_loadDict; block i owns the slot
// dst[dst_off[i] .. + dst_cap[i]).  out[i] = liblz4's return value (0: it does not fit, or src_len[i] / dst_cap[i] is negative, or the
// chain would exceed 0x7E000000 bytes), kChainStopped for the blocks behind a chain's first 0; chain_consumed[c] = the source bytes of
// the blocks that succeeded.  The walk trusts nothing it reads from the arrays: a chain's block range is cut to [0, n_blocks], a
// negative prefix counts as 0 and one longer than chain_src_off[c] is cut to it.
struct CChainArgs {
  const uint8_t* src; const uint64_t* chain_src_off; const int32_t* chain_prefix_len; const int32_t* src_len; const uint32_t* chain_first;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap;
  int32_t* out; uint64_t* chain_consumed; uint32_t n_blocks, n_chains;
};
// compress_fast_chain_cu_kernel: five wavefronts per CU, a 32 KB table each, draw chains from the queue word q (one device uint32_t of
// scratch); the table stays in LDS from one block of a chain to the next; no wavefront waits for another.  n_cus = compute units
int launch_compress_fast_chain(const CChainArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// LZ4_compress_fast_continue on streams whose state stays on the device between launches (compress_fast.hip, lz4_fast_chain.h
// cstream_walk).  Chain c of `c` is the next run of blocks of the stream in slot (slot[c] & 0x7FFFFFFF); bit 31 set: the stream is stopped
// before the walk (the host's mark of a call that failed half way).  Slot s owns the record rec[s * kStreamRecWords ..] and the table
// image tables[s * 4096 ..] (32 KB).  A record of zeros is a fresh stream.  Record words:
//   [0] the stream index of the next byte (liblz4's currentOffset)   [1] the history the stream holds, capped at 65536 (its dictSize)
//   [2] flags (kStream*)   [3] loaded history + bytes consumed, what the 0x7E000000 limit counts   [4], [5] bytes consumed, low and high
// No slot may appear twice in a launch: one wavefront owns a stream from the load of its state to the store.
constexpr uint32_t kStreamRecWords = 8;
constexpr uint32_t kStreamUsed = 1u, kStreamTable = 2u, kStreamStopped = 4u, kStreamPrefixed = 8u;   // ran before; the image is the table; stopped; began with LZ4_loadDict
constexpr uint32_t kStreamForceStop = 0x80000000u;
struct CStreamArgs {
  CChainArgs c; const uint32_t* slot; uint32_t* rec; uint64_t* tables;
};
// compress_fast_stream_cu_kernel: compress_fast_chain_cu_kernel's shape; a wavefront that draws a chain loads the stream's table into
// its LDS (or builds the fresh one), walks the call's blocks and stores table and record back
int launch_compress_fast_stream(const CStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// The same streams when their sources land anywhere -- rings, alternating buffers, a dictionary elsewhere (lz4_fast_chain.h
// cxstream_walk: liblz4's prefix and external-dictionary modes, chosen block by block).  s: as above, with s.c.chain_src_off unused
// (nullptr) and s.c.chain_prefix_len[c] = the bytes of the stream's history that are present; src_off[i]: block i's own source offset;
// chain_hist_end[c]: where stream c's history ends in s.c.src at its first block of the launch.  Same record, same image: launches of
// the two kernels alternate on a slot.  The walk trusts the offsets: the host path checks them against the stream's window.
struct CXStreamArgs {
  CStreamArgs s; const uint64_t* src_off; const uint64_t* chain_hist_end;
};
// compress_fast_xstream_cu_kernel: compress_fast_stream_cu_kernel's shape
int launch_compress_fast_xstream(const CXStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream);
// The three launches above at LZ4_compress_fast_continue's acceleration 2 .. 65537 (clamped by the caller; 1 is theirs, anything else
// is hipErrorInvalidValue), one value for every block of the launch: compress_fast_chain_accel_cu_kernel,
// compress_fast_stream_accel_cu_kernel, compress_fast_xstream_accel_cu_kernel -- the same shapes and walks with the core's ACC switch.
// Same arguments, records and table images: launches at any acceleration alternate on a slot.
int launch_compress_fast_chain_accel(const CChainArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream);
int launch_compress_fast_stream_accel(const CStreamArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream);
int launch_compress_fast_xstream_accel(const CXStreamArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream);
// LZ4_compress_HC_continue over chains of linked blocks, prefix mode (compress_hc.hip): CChainArgs as above with chain_consumed unused
// (nullptr); the history is what LZ4_loadDictHC keeps (its last 64 KB, no minimum).  out[i] = liblz4's return value; a block that
// returns 0 (it does not fit, or src_len[i] / dst_cap[i] is negative) does NOT stop its chain: its source is history for the blocks
// behind it (a negative length counts as 0 bytes).  Every block of every chain is parsed at once, a wavefront per block; the delta[]
// build runs over (chain, segment) items of `seg` positions (4096 .. 2^30; every value gives the same bytes).  `ws` = device workspace
// of hc_ws_bytes(span, n_blocks, level) bytes, span = the maximum over chains of the region's end; the regions of different chains,
// history included, must not overlap.  `scratch` = hc_chain_scratch_bytes(span, n_blocks, n_chains, seg) bytes of device memory that
// the caller keeps (not a stream-ordered allocation made for the launch).
size_t hc_chain_scratch_bytes(uint64_t span, uint32_t n_blocks, uint32_t n_chains, uint32_t seg);
int launch_compress_hc_chain(const CChainArgs& a, int level, void* ws, uint64_t span, uint32_t seg, void* scratch, uint32_t n_cus, void* stream);
// LZ4_compress_HC_continue on streams whose sources land anywhere (compress_hc.hip): the host has walked the call's state machine and laid
// every stream out as ONE buffer in liblz4's index space (host_staging.h HcsImage), so nothing here is serial.  src: the image of `span`
// bytes; per block its start in the image, the bytes of its view in front of it (0 .. 65536), liblz4's lowLimit and dictLimit as
// positions of the view (low <= dlim <= hist), its length, slot and capacity; per stream its buffer [buf_off, + buf_len) and its run
// ends ends[end_first[t] .. end_first[t + 1]) (ascending, counted from the buffer's start; n_ends in all); items: the build's
// {stream, segment} pairs of `seg` positions (4096 .. 2^30), drawn from the queue word (zeroed by the caller).  out[i] = liblz4's return value; a block
// whose length or capacity is negative, or whose numbers do not fit the image, gives 0.  `ws` = hc_ws_bytes(span, n_blocks, level).
struct HcStreamArgs {
  const uint8_t* src; const uint64_t* blk_start; const uint32_t* blk_hist; const uint32_t* blk_low; const uint32_t* blk_dlim; const int32_t* src_len;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap; int32_t* out;
  const uint64_t* buf_off; const uint64_t* buf_len; const uint32_t* end_first; const uint32_t* ends; const uint32_t* items; uint32_t* queue;
  uint64_t span; uint32_t n_blocks, n_streams, n_ends, n_items, seg;
};
// hc_build_stream_kernel (one wavefront per CU: the 128 KB head table) + hc_parse_stream_kernel (a wavefront per block)
int launch_compress_hc_stream(const HcStreamArgs& a, int level, void* ws, uint32_t n_cus, void* stream);
// The decoded-size query: out[i] = the value LZ4_decompress_safe would return for block i with capacity a.dst_cap[i] (-1 where it or
// src_len[i] is negative); a.dst and a.dst_off are ignored (may be nullptr) and no output buffer exists.  decode_size_kernel<4, 2048, true>:
// a wavefront per block; no route word, no sampler, no decode knob
int launch_decoded_size(const BatchArgs& a, void* stream);
int launch_xxh32(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed, uint32_t* out, uint32_t n, void* stream);
int launch_xxh64(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, uint64_t* out, uint32_t n, void* stream);
// streaming xxhash: `rec` = device record of xxh_stream_rec_bytes() bytes (the digest so far sits at xxh_stream_digest_offset());
// reset != 0 restarts the stream with `seed` before absorbing data[0..len)
int launch_xxh32_stream(void* rec, const uint8_t* data, uint32_t len, int reset, uint32_t seed, void* stream);
int launch_xxh64_stream(void* rec, const uint8_t* data, uint32_t len, int reset, uint64_t seed, void* stream);
size_t xxh_stream_rec_bytes(bool is64);
size_t xxh_stream_digest_offset(bool is64);
int launch_gen_blocks(uint8_t* dst, uint64_t stride, int32_t block_len, uint64_t seed, uint64_t first_idx,
                      uint32_t litmax, uint32_t win, uint32_t n_blocks, void* stream);

}  // namespace lz4hip
