// decode_lanes.hip -- the lane-group decoders of the LZ4 block engine (gfx950): GL lanes of a wavefront share one block.
//
//   decode_kernel<GL, SAFE, PIPE, STAGE>
//                        : GL lanes per block, 64/GL blocks per wavefront, algorithm in lz4_decode_core.h; PIPE = software-
//                          pipelined loop for small batches, STAGE = output through LDS as whole lines for large ones.
//   decode_partial_kernel<GL, PIPE, STAGE>, decode_partial_deep_kernel<GL>
//                        : LZ4_decompress_safe_partial: decode_kernel's and decode_deep_kernel's safe forms with the core's PARTIAL
//                          switch and a per-block target next to BatchArgs.
//   decode_dict_kernel<GL, PIPE, STAGE>, decode_dict_deep_kernel<GL>
//                        : LZ4_decompress_safe_usingDict (external dictionary): the same two safe forms with the core's DICT switch;
//                          the dictionary's end pointer and length travel next to BatchArgs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_core.h"

namespace lz4hip {

template <int GL, bool SAFE, int PIPE, bool STAGE>
__global__ __launch_bounds__(256) void decode_kernel(BatchArgs a, const uint32_t* route, uint32_t want) {
  if (route && *route != want) return;   // (the launch was routed to another decoder: launch_decompress)
  // STAGE: one staging buffer per block of the workgroup (group_dev.h st_*): 256/GL x 576 bytes; PIPE 2: the block's window of
  // the compressed stream (group_dev.h sr_*): 256/GL x (kStream + 16) bytes
  constexpr uint32_t kPer = PIPE == 2 ? GroupDev<GL>::kStreamLds : GroupDev<GL>::kStage;
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[((STAGE || PIPE == 2) ? (256 / GL) * kPer : 16) + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;  // a whole group leaves together
  GroupDev<GL> g;
  uint8_t* stage = (STAGE || PIPE == 2) ? stage_mem + (threadIdx.x / GL) * kPer : nullptr;
  const int r = decode_block<GroupDev<GL>, SAFE, PIPE, STAGE>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid], a.dst_cap[gid], stage);
  if (g.l == 0) a.out[gid] = r;
}

// the deep loop's kernel: the same body with an occupancy request (LZ4HIP_DEEP_WGS workgroups of 256 threads per CU)
#ifndef LZ4HIP_DEEP_WGS
#define LZ4HIP_DEEP_WGS 2
#endif
template <int GL, bool SAFE>
__global__ __launch_bounds__(256, LZ4HIP_DEEP_WGS) void decode_deep_kernel(BatchArgs a, const uint32_t* route, uint32_t want) {
  if (route && *route != want) return;   // (the launch was routed to another decoder: launch_decompress)
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;
  GroupDev<GL> g;
  const int r = decode_block<GroupDev<GL>, SAFE, 2, false>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid], a.dst_cap[gid],
                                                           stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds);
  if (g.l == 0) a.out[gid] = r;
}

// LZ4_decompress_safe_partial: twins of decode_kernel<GL, true, PIPE, STAGE> and decode_deep_kernel<GL, true> (same launch bounds, same
// LDS) with lz4_decode_core.h's PARTIAL switch; block i decodes into min(target[i], dst_cap[i]) bytes, and a negative size gives -1
__device__ __forceinline__ int partial_out_size(const BatchArgs& a, const int32_t* target, uint32_t i) {
  const int32_t t = target[i], c = a.dst_cap[i];
  return (t < 0 || c < 0) ? -1 : (t < c ? t : c);
}
template <int GL, int PIPE, bool STAGE>
__global__ __launch_bounds__(256) void decode_partial_kernel(BatchArgs a, const int32_t* target) {
  constexpr uint32_t kPer = PIPE == 2 ? GroupDev<GL>::kStreamLds : GroupDev<GL>::kStage;
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[((STAGE || PIPE == 2) ? (256 / GL) * kPer : 16) + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;  // a whole group leaves together
  GroupDev<GL> g;
  uint8_t* stage = (STAGE || PIPE == 2) ? stage_mem + (threadIdx.x / GL) * kPer : nullptr;
  const int r = decode_block<GroupDev<GL>, true, PIPE, STAGE, true>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid],
                                                                  partial_out_size(a, target, gid), stage);
  if (g.l == 0) a.out[gid] = r;
}
template <int GL>
__global__ __launch_bounds__(256, LZ4HIP_DEEP_WGS) void decode_partial_deep_kernel(BatchArgs a, const int32_t* target) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;
  GroupDev<GL> g;
  const int r = decode_block<GroupDev<GL>, true, 2, false, true>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid],
                                                                 partial_out_size(a, target, gid), stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds);
  if (g.l == 0) a.out[gid] = r;
}

// LZ4_decompress_safe_usingDict: twins of decode_kernel<GL, true, PIPE, STAGE> and decode_deep_kernel<GL, true> (same launch bounds, same
// LDS) with lz4_decode_core.h's DICT switch; every block of the launch decodes against the one dictionary [dict_end - dict_len, dict_end),
// of which only the last 64 KB are ever read; a negative size gives -1
template <int GL, int PIPE, bool STAGE>
__global__ __launch_bounds__(256) void decode_dict_kernel(BatchArgs a, const uint8_t* dict_end, int32_t dict_len) {
  constexpr uint32_t kPer = PIPE == 2 ? GroupDev<GL>::kStreamLds : GroupDev<GL>::kStage;
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[((STAGE || PIPE == 2) ? (256 / GL) * kPer : 16) + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;  // a whole group leaves together
  GroupDev<GL> g;
  uint8_t* stage = (STAGE || PIPE == 2) ? stage_mem + (threadIdx.x / GL) * kPer : nullptr;
  const int r = decode_block<GroupDev<GL>, true, PIPE, STAGE, false, true>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid],
                                                                         a.dst_cap[gid], stage, dict_end, dict_len);
  if (g.l == 0) a.out[gid] = r;
}
template <int GL>
__global__ __launch_bounds__(256, LZ4HIP_DEEP_WGS) void decode_dict_deep_kernel(BatchArgs a, const uint8_t* dict_end, int32_t dict_len) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= a.n) return;
  GroupDev<GL> g;
  const int r = decode_block<GroupDev<GL>, true, 2, false, false, true>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid], a.dst_cap[gid],
                                                                        stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds, dict_end, dict_len);
  if (g.l == 0) a.out[gid] = r;
}

template <int GL>
static int launch_decode_gl(const BatchArgs& a, bool safe, int pipe, bool stage, hipStream_t st, const uint32_t* route, uint32_t want) {
  const uint32_t per_wg = 256u / GL;
  const uint32_t grid = (a.n + per_wg - 1u) / per_wg;
  if (stage) {   // (staging belongs to the plain loop)
    if (safe) hipLaunchKernelGGL((decode_kernel<GL, true, 0, true>), dim3(grid), dim3(256), 0, st, a, route, 0u);
    else hipLaunchKernelGGL((decode_kernel<GL, false, 0, true>), dim3(grid), dim3(256), 0, st, a, route, 0u);
  } else if (pipe == 2 && GL <= 16) {   // (the deep loop works in 64-byte steps: groups of up to 16 lanes)
    if constexpr (GL <= 16) {
      if (safe) hipLaunchKernelGGL((decode_deep_kernel<GL, true>), dim3(grid), dim3(256), 0, st, a, route, want);
      else hipLaunchKernelGGL((decode_deep_kernel<GL, false>), dim3(grid), dim3(256), 0, st, a, route, want);
    }
  } else if (safe) {
    if (pipe) hipLaunchKernelGGL((decode_kernel<GL, true, 1, false>), dim3(grid), dim3(256), 0, st, a, route, 0u);
    else hipLaunchKernelGGL((decode_kernel<GL, true, 0, false>), dim3(grid), dim3(256), 0, st, a, route, 0u);
  } else {
    if (pipe) hipLaunchKernelGGL((decode_kernel<GL, false, 1, false>), dim3(grid), dim3(256), 0, st, a, route, 0u);
    else hipLaunchKernelGGL((decode_kernel<GL, false, 0, false>), dim3(grid), dim3(256), 0, st, a, route, 0u);
  }
  return (int)hipGetLastError();
}
int launch_decode_lanes(const BatchArgs& a, bool safe, int lanes, int pipe, bool stage, hipStream_t st, const uint32_t* route, uint32_t want) {
  switch (lanes) {
    case 4: return launch_decode_gl<4>(a, safe, pipe, stage, st, route, want);
    case 16: return launch_decode_gl<16>(a, safe, pipe, stage, st, route, want);
    case 32: return launch_decode_gl<32>(a, safe, pipe, stage, st, route, want);
    case 64: return launch_decode_gl<64>(a, safe, pipe, stage, st, route, want);
    case 8:
    default: return launch_decode_gl<8>(a, safe, pipe, stage, st, route, want);
  }
}

// LZ4_decompress_safe_partial: the two lane-group decoders an unrouted safe decode of the same batch size gets -- >= 40960 blocks:
// 4 lanes per block, the plain loop with output staging; fewer: 8 lanes, the deep loop.  No route, no wave / pair / trio / ring loop
// (each of them ends a block in code of its own) and no decode_* knob.
int launch_decompress_partial(const BatchArgs& a, const int32_t* target, void* stream) {
  if (a.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (a.n >= 40960u) hipLaunchKernelGGL((decode_partial_kernel<4, 0, true>), dim3((a.n + 63u) / 64u), dim3(256), 0, st, a, target);
  else hipLaunchKernelGGL((decode_partial_deep_kernel<8>), dim3((a.n + 31u) / 32u), dim3(256), 0, st, a, target);
  return (int)hipGetLastError();
}

// LZ4_decompress_safe_usingDict: the same two lane-group decoders by batch size as the partial decoder's.  dict_end = one past the
// dictionary's last byte in device memory (not looked at when dict_len == 0); no route, no decode_* knob.
int launch_decompress_dict(const BatchArgs& a, const uint8_t* dict_end, int32_t dict_len, void* stream) {
  if (a.n == 0) return 0;
  if (dict_len < 0 || (dict_len > 0 && !dict_end)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (a.n >= 40960u) hipLaunchKernelGGL((decode_dict_kernel<4, 0, true>), dim3((a.n + 63u) / 64u), dim3(256), 0, st, a, dict_end, dict_len);
  else hipLaunchKernelGGL((decode_dict_deep_kernel<8>), dim3((a.n + 31u) / 32u), dim3(256), 0, st, a, dict_end, dict_len);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
