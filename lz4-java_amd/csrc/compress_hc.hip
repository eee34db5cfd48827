// compress_hc.hip -- the LZ4 HC kernels of the LZ4 block engine (gfx950).
//
//   hc_build_kernel / hc_parse_kernel
//                        : LZ4 HC levels 1..12 (lz4_hc_core.h): chain deltas through a 128 KB LDS head table, then the parse.
//   hc_parse_dest_kernel : LZ4_compress_HC_destSize: hc_parse_kernel's twin with HcParse's FILL switch, behind the same
//                          hc_build_kernel.  The parse of a block ends once its target is full, so the parse time follows the
//                          input consumed; the delta[] build still covers the whole block.
//   hc_dict_image_kernel / hc_build_dict_kernel / hc_parse_dict_kernel
//                        : LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream per block.  The image kernel runs the delta[]
//                          build over a dictionary's kept tail once per handle and device and keeps its delta[] and the head table
//                          it ends with; the build's twin starts every record from that head table, the parse's twin has HcParse's
//                          DICT switch on.
//   hc_chain_layout_kernel / hc_build_chain_kernel / hc_parse_chain_kernel
//                        : LZ4_compress_HC_continue over chains of linked blocks (prefix mode).  Every block of every chain is parsed at
//                          once (HcParse's PREFIX switch) behind a delta[] built over each chain's buffer in segments that workgroups
//                          draw from a queue (HcBuild's SEG switch); the layout kernel makes the per-block offsets and the item list.
//   hc_build_stream_kernel / hc_parse_stream_kernel
//                        : LZ4_compress_HC_continue on streams whose sources land anywhere (both of its modes), over the linear image the
//                          host makes of a call (host_staging.h HcsImage): HcBuild's RUNS switch, HcParse's DICT and PREFIX switches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "wave_dev.h"
#include "lz4_hc_core.h"
#include "host_staging.h"

namespace lz4hip {

// ------------------------------------------------------------------------------------------------
// HC compress (levels 1..9): phase 1 builds delta[] (workspace `ws`, one u16 per input byte, indexed by
// the block's source offset), phase 2 parses.  One wavefront per block in both.
// ------------------------------------------------------------------------------------------------
// (`span` = u16 entries the workspace holds: a block whose source range reaches past it -- a caller-supplied span that was too
// small -- is not touched and reports LZ4HIP's generic failure 0, instead of writing chain deltas past the workspace)
__global__ __launch_bounds__(64) void hc_build_kernel(BatchArgs a, uint16_t* ws, uint64_t span) {
  __shared__ __attribute__((aligned(16))) uint32_t head[32768];  // 128 KB: liblz4's HC hashTable
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  if (n < 0 || (uint32_t)n > 0x7E000000u || a.src_off[b] + (uint64_t)n > span) return;
  WaveDev w(head);
  HcBuild<WaveDev>::run(w, a.src + a.src_off[b], (uint32_t)n, ws + a.src_off[b]);
}
__global__ __launch_bounds__(64) void hc_parse_kernel(BatchArgs a, const uint16_t* ws, int level, int* opt_ws, uint64_t span) {
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t cap = a.dst_cap[b];
  int r = 0;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0 && a.src_off[b] + (uint64_t)n <= span) {
    WaveDev w(nullptr);
    HcParse<WaveDev> p(w, a.src + a.src_off[b], n, ws + a.src_off[b], a.dst + a.dst_off[b], cap, level);
    r = level >= 10 ? p.run_opt(level, opt_ws + (size_t)b * HC_OPT_INTS) : p.run();
  }
  if (threadIdx.x == 0) a.out[b] = r;
}
// LZ4_compress_HC_destSize: the same parse with HcParse's FILL switch on (lz4_hc_core.h); dst_cap[b] is the target size, consumed[b]
// the input the output covers (src_len[b] itself where liblz4 returns 0 up front: target < 1, a block above 0x7E000000 bytes).  The
// block stops parsing when its target is full; hc_build_kernel has built delta[] for all of it.
__global__ __launch_bounds__(64) void hc_parse_dest_kernel(BatchArgs a, const uint16_t* ws, int level, int* opt_ws, uint64_t span, int32_t* consumed) {
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t target = a.dst_cap[b];
  int r = 0;
  int32_t c = n;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && target >= 1 && a.src_off[b] + (uint64_t)n <= span) {
    WaveDev w(nullptr);
    HcParse<WaveDev, true> p(w, a.src + a.src_off[b], n, ws + a.src_off[b], a.dst + a.dst_off[b], target, level);
    r = level >= 10 ? p.run_opt(level, opt_ws + (size_t)b * HC_OPT_INTS) : p.run();
    c = p.consumed;
  }
  if (threadIdx.x == 0) { a.out[b] = r; consumed[b] = c; }
}
// ------------------------------------------------------------------------------------------------
// HC compress against a dictionary.  The image: the head table (32768 x u32) the build over the kept tail ends with, then the tail's
// delta[] (u16 x K): hc_dict_image_bytes(K).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hc_dict_image_kernel(const uint8_t* tail, uint32_t K, uint32_t* image) {
  __shared__ __attribute__((aligned(16))) uint32_t head[32768];
  WaveDev w(head);
  hc_dict_image_build(w, tail, K, (uint16_t*)(image + 32768));
  w.sync();
  for (uint32_t i = threadIdx.x; i < 8192u; i += 64u) ((uint4*)image)[i] = ((const uint4*)head)[i];
}
// hc_build_kernel's twin: the head table starts as the image's (16 bytes per lane and load: 128 KB per record, whatever its size),
// and the record's first byte has index HC_BIAS + K
__global__ __launch_bounds__(64) void hc_build_dict_kernel(BatchArgs a, uint16_t* ws, uint64_t span, const uint32_t* image, uint32_t K) {
  __shared__ __attribute__((aligned(16))) uint32_t head[32768];
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  if (n < 4 || (uint32_t)n > 0x7E000000u || a.src_off[b] + (uint64_t)n > span) return;   // (under 4 bytes: nothing to insert)
  for (uint32_t i = threadIdx.x; i < 8192u; i += 64u) ((uint4*)head)[i] = ((const uint4*)image)[i];
  WaveDev w(head);
  HcBuild<WaveDev, true>::run(w, a.src + a.src_off[b], (uint32_t)n, ws + a.src_off[b], HC_BIAS + K);
}
// hc_parse_kernel's twin: [dict_end - K, dict_end) is the kept tail, image + 32768 its delta[]
__global__ __launch_bounds__(64) void hc_parse_dict_kernel(BatchArgs a, const uint16_t* ws, int level, int* opt_ws, uint64_t span,
                                                           const uint8_t* dict_end, uint32_t K, const uint32_t* image) {
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t cap = a.dst_cap[b];
  int r = 0;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0 && a.src_off[b] + (uint64_t)n <= span) {
    WaveDev w(nullptr);
    HcParse<WaveDev, false, true> p(w, a.src + a.src_off[b], n, ws + a.src_off[b], a.dst + a.dst_off[b], cap, level);
    p.s.dend = dict_end;
    p.s.ddelta_end = (const uint16_t*)(image + 32768) + K;
    p.s.K = (int)K;
    r = level >= 10 ? p.run_opt(level, opt_ws + (size_t)b * HC_OPT_INTS) : p.run();
  }
  if (threadIdx.x == 0) a.out[b] = r;
}
int launch_hc_dict_image(const uint8_t* tail, uint32_t K, void* image, void* stream) {
  hipLaunchKernelGGL(hc_dict_image_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tail, K, (uint32_t*)image);
  return (int)hipGetLastError();
}
int launch_compress_hc_dict(const BatchArgs& a, int level, void* ws, uint64_t span, const uint8_t* dict_end, uint32_t K, const void* image,
                            void* stream) {
  if (a.n == 0) return 0;
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  hipLaunchKernelGGL(hc_build_dict_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (uint16_t*)ws, span, (const uint32_t*)image, K);
  hipLaunchKernelGGL(hc_parse_dict_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (const uint16_t*)ws, level, opt, span, dict_end, K,
                     (const uint32_t*)image);
  return (int)hipGetLastError();
}

// max over blocks of (src_off + src_len): how many u16 the HC workspace needs
__global__ void hc_span_kernel(const uint64_t* src_off, const int32_t* src_len, uint32_t n, unsigned long long* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t l = src_len[i];
  atomicMax(out, (unsigned long long)(src_off[i] + (l > 0 ? (uint64_t)l : 0ull)));
}
int launch_hc_span(const uint64_t* src_off, const int32_t* src_len, uint32_t n, uint64_t* out_dev, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(hc_span_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, src_off, src_len, n, (unsigned long long*)out_dev);
  return (int)hipGetLastError();
}
// workspace: u16 delta[span] (span = max(src_off + src_len) over the batch), then -- levels 10..12 only -- the price table of
// the optimal parser, HC_OPT_INTS ints per block
size_t hc_ws_bytes(uint64_t span, uint32_t n_blocks, int level) {
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  return d + (level >= 10 ? (size_t)n_blocks * HC_OPT_INTS * sizeof(int) : 0u);
}
int launch_compress_hc(const BatchArgs& a, int level, void* ws, uint64_t span, void* stream) {
  if (a.n == 0) return 0;
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  hipLaunchKernelGGL(hc_build_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (uint16_t*)ws, span);
  hipLaunchKernelGGL(hc_parse_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (const uint16_t*)ws, level, opt, span);
  return (int)hipGetLastError();
}
// ------------------------------------------------------------------------------------------------
// HC compress over chains of linked blocks (LZ4_compress_HC_continue, prefix mode).  HC's chain table is a function of the data alone,
// and a block's parse reads only the table and the 64 KB in front of it: every block of every chain is parsed at the same time, one
// wavefront per block, behind a delta[] built over each chain's buffer (its kept history, then its sources) as ONE run of positions.
//   hc_chain_layout_kernel  chain_first / src_len / chain_src_off / chain_prefix_len -> per block its source offset and kept history,
//                           per chain its buffer, and the list of build items: (chain, segment) pairs, a segment = S positions
//   hc_build_chain_kernel   workgroups draw items from a queue word; a segment starting at position a first inserts the positions
//                           [max(0, a - 65535), a) without storing (HcBuild's SEG switch), so no build is serial in a chain's length
//   hc_parse_chain_kernel   HcParse's PREFIX switch, grid = n_blocks
// Scratch (hc_chain_scratch_bytes): HcChainScratch's arrays, in memory the caller keeps (not a stream-ordered allocation: api.cpp).
// The walk trusts nothing it reads from the arrays: a chain's block range is cut to [0, n_blocks], a negative prefix counts as 0 and
// one longer than chain_src_off[c] is cut to it; a chain whose region ends past `span` (a workspace too small) is not touched and its
// blocks report 0.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kHcChainSkip = 0xFFFFFFFFu;   // blk_hist of a block whose chain is not touched
struct HcChainScratch {
  uint64_t* blk_start;   // [n_blocks] source offset of the block
  uint64_t* chain_buf;   // [n_chains] source offset of the chain's buffer (its kept history's first byte)
  uint64_t* chain_len;   // [n_chains] bytes of the buffer
  uint2* items;          // [max_items] {chain, segment}
  uint32_t* blk_hist;    // [n_blocks] kept history in front of the block, 0 .. 65536
  uint32_t* words;       // [0] items listed, [1] the build's queue word
  uint32_t max_items;
};
// (sizes and offsets: staging::HcChainScratchLayout, host_staging.h)
size_t hc_chain_scratch_bytes(uint64_t span, uint32_t n_blocks, uint32_t n_chains, uint32_t seg) {
  return staging::HcChainScratchLayout(span, n_blocks, n_chains, seg).total;
}
static HcChainScratch hc_chain_scratch(void* p, uint64_t span, uint32_t n_blocks, uint32_t n_chains, uint32_t seg) {
  const staging::HcChainScratchLayout l(span, n_blocks, n_chains, seg);
  uint8_t* const b = (uint8_t*)p;
  HcChainScratch s;
  s.max_items = l.max_items;
  s.blk_start = (uint64_t*)(b + l.blk_start);
  s.chain_buf = (uint64_t*)(b + l.chain_buf);
  s.chain_len = (uint64_t*)(b + l.chain_len);
  s.items = (uint2*)(b + l.items);
  s.blk_hist = (uint32_t*)(b + l.blk_hist);
  s.words = (uint32_t*)(b + l.words);
  return s;
}
// inclusive prefix sum of v over the wavefront
__device__ __forceinline__ uint64_t hc_wave_scan(uint64_t v) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    if ((int)__lane_id() >= d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
// a chain's block range, kept history and offset, as the walk trusts them
struct HcChainHead { uint32_t f0, f1; uint64_t off, keep; };
__device__ __forceinline__ HcChainHead hc_chain_head(const CChainArgs& a, uint32_t c) {
  HcChainHead h;
  h.f0 = a.chain_first[c] < a.n_blocks ? a.chain_first[c] : a.n_blocks;
  h.f1 = a.chain_first[c + 1] < a.n_blocks ? a.chain_first[c + 1] : a.n_blocks;
  if (h.f1 < h.f0) h.f1 = h.f0;
  h.off = a.chain_src_off[c];
  const int32_t p = a.chain_prefix_len ? a.chain_prefix_len[c] : 0;
  h.keep = p > 0 ? (uint64_t)p : 0ull;
  if (h.keep > h.off) h.keep = h.off;
  if (h.keep > 65536u) h.keep = 65536u;
  return h;
}
// one wavefront per chain
__global__ __launch_bounds__(64) void hc_chain_layout_kernel(CChainArgs a, HcChainScratch s, uint64_t span, uint32_t seg) {
  const uint32_t c = blockIdx.x, lane = __lane_id();
  const HcChainHead h = hc_chain_head(a, c);
  uint64_t run = h.keep;   // bytes of the buffer in front of the 64 blocks at hand
  for (uint32_t base = h.f0; base < h.f1; base += 64u) {
    const uint32_t i = base + lane;
    const int32_t l = i < h.f1 ? a.src_len[i] : 0;
    const uint64_t len = l > 0 ? (uint64_t)l : 0ull;
    const uint64_t incl = hc_wave_scan(len);
    if (i < h.f1) {
      const uint64_t before = run + (incl - len);
      s.blk_start[i] = h.off - h.keep + before;
      s.blk_hist[i] = before > 65536u ? 65536u : (uint32_t)before;
    }
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63);
    run += ((uint64_t)hi << 32) | lo;
  }
  // positions 0 .. run - 4 get an entry: ceil((run - 3) / seg) segments
  const uint64_t nseg64 = run >= 4u ? (run - 3u + seg - 1u) / seg : 0ull;
  bool skip = h.off > span || h.off - h.keep + run > span || nseg64 > (uint64_t)s.max_items;
  uint32_t first_item = 0;
  if (!skip && nseg64) {
    if (lane == 0) first_item = atomicAdd(&s.words[0], (uint32_t)nseg64);
    first_item = (uint32_t)__builtin_amdgcn_readfirstlane((int)first_item);
    skip = (uint64_t)first_item + nseg64 > (uint64_t)s.max_items;   // (regions that overlap, against the contract: more items than the span has room for)
  }
  if (lane == 0) { s.chain_buf[c] = h.off - h.keep; s.chain_len[c] = skip ? 0ull : run; }
  if (skip) {
    for (uint32_t i = h.f0 + lane; i < h.f1; i += 64u) s.blk_hist[i] = kHcChainSkip;
  } else {
    for (uint32_t k = lane; k < (uint32_t)nseg64; k += 64u) s.items[first_item + k] = make_uint2(c, k);
  }
}
__global__ __launch_bounds__(64) void hc_build_chain_kernel(CChainArgs a, HcChainScratch s, uint16_t* ws, uint32_t seg) {
  __shared__ __attribute__((aligned(16))) uint32_t head[32768];  // 128 KB: liblz4's HC hashTable
  WaveDev w(head);
  uint32_t n_items = s.words[0];
  if (n_items > s.max_items) n_items = s.max_items;   // (what hc_chain_layout_kernel listed; a chain that did not fit listed nothing)
  for (;;) {
    uint32_t t = 0;
    if (__lane_id() == 0) t = atomicAdd(&s.words[1], 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= n_items) return;
    const uint2 it = s.items[t];
    if (it.x >= a.n_chains) continue;   // (an entry nobody wrote: the list starts out as all ones)
    const uint64_t buf = s.chain_buf[it.x];
    hc_chain_build_segment(w, a.src + buf, s.chain_len[it.x], seg, it.y, ws + buf);   // (a skipped chain has length 0: nothing is done)
    WaveDev::sync();   // the head table is reused: the next segment starts from its own
  }
}
__global__ __launch_bounds__(64) void hc_parse_chain_kernel(CChainArgs a, HcChainScratch s, const uint16_t* ws, int level, int* opt_ws) {
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t cap = a.dst_cap[b];
  const uint32_t hist = s.blk_hist[b];
  int r = 0;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0 && hist <= 65536u) {
    const uint64_t buf = s.blk_start[b] - hist;
    WaveDev w(nullptr);
    r = hc_chain_parse_block(w, a.src + buf, hist, n, ws + buf, a.dst + a.dst_off[b], cap, level, opt_ws + (size_t)b * HC_OPT_INTS);
  }
  if (threadIdx.x == 0) a.out[b] = r;
}
int launch_compress_hc_chain(const CChainArgs& a, int level, void* ws, uint64_t span, uint32_t seg, void* scratch, uint32_t n_cus, void* stream) {
  if (a.n_chains == 0 || a.n_blocks == 0) return 0;
  if (!scratch || seg < 4096u || seg > (1u << 30)) return (int)hipErrorInvalidValue;
  const HcChainScratch s = hc_chain_scratch(scratch, span, a.n_blocks, a.n_chains, seg);
  hipError_t e = hipMemsetAsync(s.words, 0, 2u * sizeof(uint32_t), (hipStream_t)stream);
  // (a chain that reserves more items than are left -- regions that overlap, against the contract -- lists none: no entry of the list is
  // ever read that nobody wrote)
  // (and a block that lies in no chain -- a chain_first that does not cover it -- is skipped: blk_hist lies right behind the list)
  if (e == hipSuccess) e = hipMemsetAsync(s.items, 0xFF, (size_t)s.max_items * sizeof(uint2) + (size_t)a.n_blocks * sizeof(uint32_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  hipLaunchKernelGGL(hc_chain_layout_kernel, dim3(a.n_chains), dim3(64), 0, (hipStream_t)stream, a, s, span, seg);
  // (one wavefront per CU -- the 128 KB head table -- and never more workgroups than there can be items)
  const uint32_t wgs = s.max_items < n_cus ? s.max_items : n_cus;
  hipLaunchKernelGGL(hc_build_chain_kernel, dim3(wgs ? wgs : 1u), dim3(64), 0, (hipStream_t)stream, a, s, (uint16_t*)ws, seg);
  hipLaunchKernelGGL(hc_parse_chain_kernel, dim3(a.n_blocks), dim3(64), 0, (hipStream_t)stream, a, s, (const uint16_t*)ws, level, opt);
  return (int)hipGetLastError();
}
// ------------------------------------------------------------------------------------------------
// HC compress over streams whose sources land anywhere (LZ4_compress_HC_continue in both of its modes).  The stream's bookkeeping is a
// function of addresses and lengths alone, so the host has walked it and laid every stream out in liblz4's index space (HcsImage):
//   hc_build_stream_kernel  hc_build_chain_kernel's queue and segment warm-up over the host's item list, with HcBuild's RUNS switch
//                           (the last three positions of a run that a jump ended are never inserted)
//   hc_parse_stream_kernel  HcParse's DICT and PREFIX switches together, grid = n_blocks
// Nothing that is read from the arrays is trusted to lie inside the image.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hc_build_stream_kernel(HcStreamArgs a, uint16_t* ws, uint32_t seg) {
  __shared__ __attribute__((aligned(16))) uint32_t head[32768];  // 128 KB: liblz4's HC hashTable
  WaveDev w(head);
  for (;;) {
    uint32_t t = 0;
    if (__lane_id() == 0) t = atomicAdd(a.queue, 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= a.n_items) return;
    const uint32_t c = a.items[2u * t], k = a.items[2u * t + 1u];
    if (c >= a.n_streams) continue;
    const uint64_t buf = a.buf_off[c], len = a.buf_len[c];
    const uint32_t e0 = a.end_first[c], e1 = a.end_first[c + 1];
    if (buf > a.span || len > a.span - buf || len > 0xFFFF0000ull || e0 > e1 || e1 > a.n_ends) continue;
    hc_stream_build_segment(w, a.src + buf, len, seg, k, ws + buf, a.ends + e0, e1 - e0);
    WaveDev::sync();   // the head table is reused: the next segment starts from its own
  }
}
__global__ __launch_bounds__(64) void hc_parse_stream_kernel(HcStreamArgs a, const uint16_t* ws, int level, int* opt_ws) {
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t cap = a.dst_cap[b];
  const uint32_t hist = a.blk_hist[b], low = a.blk_low[b], dlim = a.blk_dlim[b];
  const uint64_t start = a.blk_start[b];
  int r = 0;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0 && hist <= 65536u && low <= dlim && dlim <= hist && start >= hist && start <= a.span &&
      (uint64_t)n <= a.span - start) {
    const uint64_t view = start - hist;
    WaveDev w(nullptr);
    r = hc_stream_parse_block(w, a.src + view, hist, low, dlim, n, ws + view, a.dst + a.dst_off[b], cap, level, opt_ws + (size_t)b * HC_OPT_INTS);
  }
  if (threadIdx.x == 0) a.out[b] = r;
}
int launch_compress_hc_stream(const HcStreamArgs& a, int level, void* ws, uint32_t n_cus, void* stream) {
  if (a.n_blocks == 0) return 0;
  if (a.seg < 4096u || a.seg > (1u << 30)) return (int)hipErrorInvalidValue;
  const size_t d = (((size_t)a.span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  if (a.n_items) {
    const uint32_t wgs = a.n_items < n_cus ? a.n_items : n_cus;
    hipLaunchKernelGGL(hc_build_stream_kernel, dim3(wgs ? wgs : 1u), dim3(64), 0, (hipStream_t)stream, a, (uint16_t*)ws, a.seg);
  }
  hipLaunchKernelGGL(hc_parse_stream_kernel, dim3(a.n_blocks), dim3(64), 0, (hipStream_t)stream, a, (const uint16_t*)ws, level, opt);
  return (int)hipGetLastError();
}
int launch_compress_hc_dest(const BatchArgs& a, int32_t* consumed, int level, void* ws, uint64_t span, void* stream) {
  if (a.n == 0) return 0;
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  hipLaunchKernelGGL(hc_build_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (uint16_t*)ws, span);
  hipLaunchKernelGGL(hc_parse_dest_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (const uint16_t*)ws, level, opt, span, consumed);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
