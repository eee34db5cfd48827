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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "wave_dev.h"
#include "lz4_hc_core.h"

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
int launch_compress_hc_dest(const BatchArgs& a, int32_t* consumed, int level, void* ws, uint64_t span, void* stream) {
  if (a.n == 0) return 0;
  const size_t d = (((size_t)span * 2u + 64u) + 255u) & ~(size_t)255u;
  int* const opt = level >= 10 ? (int*)((uint8_t*)ws + d) : nullptr;
  hipLaunchKernelGGL(hc_build_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (uint16_t*)ws, span);
  hipLaunchKernelGGL(hc_parse_dest_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, (const uint16_t*)ws, level, opt, span, consumed);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
