// decode_wave.hip -- the decoders of the LZ4 block engine that give a block a whole wavefront (gfx950): decode_wave_kernel
// (lz4_decode_wave.h) and the decoded-size query.
//
//   decode_size_kernel<W, KS, FAST>
//                        : the decoded-size query (lz4_decode_size.h): a wavefront per block, the stream through an LDS ring, no
//                          output buffer.  Reads C, writes 4 bytes per block.
//                          Bound: HBM (reads C, writes N per block; match sources are random lines).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_core.h"

namespace lz4hip {

// the wave loop's kernel (lz4_decode_wave.h): ONE WAVEFRONT PER BLOCK, W wavefronts per workgroup, one workgroup per CU (it declares
// the LDS of its W wavefronts: a stream ring of KS bytes and an output ring of KW bytes each; workgroups that SHARE a CU get 128 KB of
// its LDS between them, a single one all 160 KB -- DESIGN.md 2.1).  No barrier: the wavefronts are independent, each takes the blocks
// blockIdx.x * W + wave, + gridDim.x * W, ... -- or, spread (wave_spread, kernels_internal.h), blockIdx.x + wave * gridDim.x, ...  The launch picks W so that the blocks of the batch spread over all CUs with the largest
// ring that fits: up to one block per CU a 64 KB ring (a 64 KiB block never leaves the chip), ... sixteen per CU an 8 KB ring.
template <int W, int KW, int KS, bool SAFE, int PIPE>
__global__ __launch_bounds__(64 * W) void decode_wave_kernel(BatchArgs a, const uint32_t* route, uint32_t want, uint32_t spread) {
  if (route && *route != want) return;   // (the launch was routed to another decoder: launch_decompress)
  typedef BlockWaveDev<KW, KS> G;
  __shared__ __attribute__((aligned(16))) uint8_t wave_mem[W * G::kWaveLds];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* lds = wave_mem + wave * G::kWaveLds;
  for (uint32_t b = spread ? blockIdx.x + wave * gridDim.x : blockIdx.x * W + wave; b < a.n; b += gridDim.x * W) {
    G g;
    const int r = decode_block<G, SAFE, PIPE, false>(g, a.src + a.src_off[b], a.src_len[b], a.dst + a.dst_off[b], a.dst_cap[b], lds);
    if (g.l == 0) a.out[b] = r;
  }
}
template <int W, int KW, int KS>
static int launch_decode_wave_w(const BatchArgs& a, bool safe, bool par, hipStream_t st, const uint32_t* route, uint32_t want) {
  const uint32_t cus = device_cus(), spread = wave_spread(a.n, W, cus), wgs = (a.n + W - 1u) / W;
  const uint32_t grid = spread ? (a.n < cus ? a.n : cus) : (wgs < cus ? wgs : cus);
  if (par) {   // (PIPE 5: several sequences of the block per trip)
    if (safe) hipLaunchKernelGGL((decode_wave_kernel<W, KW, KS, true, 5>), dim3(grid), dim3(64 * W), 0, st, a, route, want, spread);
    else hipLaunchKernelGGL((decode_wave_kernel<W, KW, KS, false, 5>), dim3(grid), dim3(64 * W), 0, st, a, route, want, spread);
  } else {
    if (safe) hipLaunchKernelGGL((decode_wave_kernel<W, KW, KS, true, 4>), dim3(grid), dim3(64 * W), 0, st, a, route, want, spread);
    else hipLaunchKernelGGL((decode_wave_kernel<W, KW, KS, false, 4>), dim3(grid), dim3(64 * W), 0, st, a, route, want, spread);
  }
  return (int)hipGetLastError();
}
// ring: bytes of the output ring (8192 / 16384 / 32768 / 65536; 0 = the largest that lets the batch spread over all CUs)
int launch_decode_wave(const BatchArgs& a, bool safe, bool par, int ring, hipStream_t st, const uint32_t* route, uint32_t want) {
  if (ring == 0) {
    const uint32_t cus = device_cus();
    ring = a.n <= 2u * cus ? 65536 : a.n <= 4u * cus ? 32768 : a.n <= 8u * cus ? 16384 : 8192;
  }
  switch (ring) {
    case 65536: return a.n <= device_cus() ? launch_decode_wave_w<1, 65536, 2048>(a, safe, par, st, route, want) : launch_decode_wave_w<2, 65536, 2048>(a, safe, par, st, route, want);
    case 32768: return launch_decode_wave_w<4, 32768, 2048>(a, safe, par, st, route, want);
    case 16384: return launch_decode_wave_w<8, 16384, 2048>(a, safe, par, st, route, want);
    case 8192: return launch_decode_wave_w<16, 8192, 1024>(a, safe, par, st, route, want);
    default: return (int)hipErrorInvalidValue;
  }
}

// The decoded-size query (lz4_decode_size.h): out[i] = what LZ4_decompress_safe(src_i, dst, src_len[i], dst_cap[i]) would return, and
// nothing else is written -- a.dst and a.dst_off are not looked at.  ONE WAVEFRONT PER BLOCK, W wavefronts per workgroup, each with a
// stream ring of KS bytes in LDS; no barrier, the wavefronts are independent and take the blocks blockIdx.x * W + wave, + gridDim.x * W,
// ... -- or, spread (wave_spread: a batch that would leave CUs empty), blockIdx.x + wave * gridDim.x, ...  A negative src_len[i] or
// dst_cap[i] gives -1 (decode_block's first test).  FAST false: the exact path alone (developer A/B builds and the tests' cross-check).
template <int W, int KS, bool FAST>
__global__ __launch_bounds__(64 * W) void decode_size_kernel(BatchArgs a, uint32_t spread) {
  typedef SizeWaveDev<KS> G;
  __shared__ __attribute__((aligned(16))) uint8_t size_mem[W * G::kSizeLds];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* lds = size_mem + wave * G::kSizeLds;
  for (uint32_t b = spread ? blockIdx.x + wave * gridDim.x : blockIdx.x * W + wave; b < a.n; b += gridDim.x * W) {
    G g;
    const int r = decoded_size<G, FAST>(g, a.src + a.src_off[b], a.src_len[b], a.dst_cap[b], lds);
    if (g.l == 0) a.out[b] = r;
  }
}
// Four wavefronts per workgroup, up to eight workgroups per CU (a wavefront's state is its 2 KB ring and a few dozen registers: the
// CU holds all 32); more blocks than that are taken in turns.
int launch_decoded_size(const BatchArgs& a, void* stream) {
  if (a.n == 0) return 0;
  constexpr uint32_t W = 4u;
  const uint32_t cus = device_cus(), spread = wave_spread(a.n, W, cus), wgs = (a.n + W - 1u) / W;
  const uint32_t grid = spread ? (a.n < cus ? a.n : cus) : (wgs < 8u * cus ? wgs : 8u * cus);
  hipLaunchKernelGGL((decode_size_kernel<4, 2048, true>), dim3(grid), dim3(64 * W), 0, (hipStream_t)stream, a, spread);
  return (int)hipGetLastError();
}
#ifdef LZ4HIP_RING_DBG
int ring_stats_take_wave(unsigned long long* sum8) { return ring_stats_take(sum8); }
#endif

}  // namespace lz4hip
