// decode_trio.hip -- the trio loop's decoder of the LZ4 block engine (gfx950): three wavefronts per block, lz4_decode_trio.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_core.h"

namespace lz4hip {

// the trio loop's kernel (lz4_decode_trio.h): THREE WAVEFRONTS PER BLOCK -- wavefront 3p of the workgroup is the COPIER of trio p (it runs
// decode_block), 3p + 1 its PLANNER, 3p + 2 its SCANNER: consecutive wavefronts of a workgroup sit on different SIMDs.  For launches of up
// to two blocks per CU (W = 1, 2: the single-call path, the smallest batches), where SIMDs idle.
// WPE: wavefronts per SIMD the kernel is compiled for (0: whatever its registers allow).  Two workgroups of four trios share a CU in the
// 8 KB-ring form (24 wavefronts = 6 per SIMD: at most 80 VGPRs each).
template <int W, int KW, int KS, bool SAFE, int WPE = 1>
__global__ __launch_bounds__(192 * W, WPE) void decode_trio_kernel(BatchArgs a, const uint32_t* route, uint32_t want, uint32_t spread) {
  if (route && *route != want) return;
  typedef BlockWaveDev<KW, KS> G;
  static_assert(G::kMailSlots == PAIR_SLOTS && G::kMailSlotBytes == PAIR_SLOT_BYTES && G::kScanSlots == TRIO_SCAN_SLOTS && G::kScanBytes == TRIO_SCAN_BYTES, "queue layout");
  __shared__ __attribute__((aligned(16))) uint8_t trio_mem[W * G::kTrioLds];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t trio = wave / 3u, role = wave - 3u * trio;
  uint8_t* lds = trio_mem + trio * G::kTrioLds;
  if (role == 0u && (threadIdx.x & 63u) < PAIR_CTL_WORDS) ((uint32_t*)(lds + G::kWaveLds + PAIR_SLOTS * PAIR_SLOT_BYTES))[threadIdx.x & 63u] = 0u;
  __syncthreads();
  if (role != 0u) {
    G g;
    trio_service(g, lds, role == 2u);
    return;
  }
  for (uint32_t b = spread ? blockIdx.x + trio * gridDim.x : blockIdx.x * W + trio; b < a.n; b += gridDim.x * W) {
    G g;
    const int r = decode_block<G, SAFE, 8, false>(g, a.src + a.src_off[b], a.src_len[b], a.dst + a.dst_off[b], a.dst_cap[b], lds);
    if (g.l == 0) a.out[b] = r;
  }
  G g;
  trio_quit(g, lds);
}
template <int W, int KW, int KS>
static int launch_decode_trio_w(const BatchArgs& a, bool safe, hipStream_t st, const uint32_t* route, uint32_t want) {
  const uint32_t cus = device_cus(), spread = wave_spread(a.n, W, cus), wgs = (a.n + W - 1u) / W;
  const uint32_t grid = spread ? (a.n < cus ? a.n : cus) : (wgs < cus ? wgs : cus);
  if (safe) hipLaunchKernelGGL((decode_trio_kernel<W, KW, KS, true>), dim3(grid), dim3(192 * W), 0, st, a, route, want, spread);
  else hipLaunchKernelGGL((decode_trio_kernel<W, KW, KS, false>), dim3(grid), dim3(192 * W), 0, st, a, route, want, spread);
  return (int)hipGetLastError();
}
// the trio loop: ring = bytes of the output ring (8192 / 16384 / 32768 / 65536; 0 = the largest that lets the batch spread over all CUs)
int launch_decode_trio(const BatchArgs& a, bool safe, int ring, hipStream_t st, const uint32_t* route, uint32_t want) {
  const uint32_t cus = device_cus();
  if (ring == 0) ring = a.n <= 2u * cus ? 65536 : a.n <= 4u * cus ? 32768 : a.n <= 5u * cus ? 16384 : 8192;
  switch (ring) {
    case 65536: return a.n <= cus ? launch_decode_trio_w<1, 65536, 2048>(a, safe, st, route, want) : launch_decode_trio_w<2, 65536, 2048>(a, safe, st, route, want);
    case 32768: return launch_decode_trio_w<4, 32768, 2048>(a, safe, st, route, want);
    case 16384: return launch_decode_trio_w<5, 16384, 2048>(a, safe, st, route, want);   // (five trios = 960 threads: what a workgroup can have)
    case 8192: {                                                                          // two workgroups of four trios per CU
      const uint32_t spread = wave_spread(a.n, 4u, 2u * cus), wgs = (a.n + 3u) / 4u, grid = spread ? (a.n < 2u * cus ? a.n : 2u * cus) : (wgs < 2u * cus ? wgs : 2u * cus);
      if (safe) hipLaunchKernelGGL((decode_trio_kernel<4, 8192, 1024, true, 6>), dim3(grid), dim3(768), 0, st, a, route, want, spread);
      else hipLaunchKernelGGL((decode_trio_kernel<4, 8192, 1024, false, 6>), dim3(grid), dim3(768), 0, st, a, route, want, spread);
      return (int)hipGetLastError();
    }
    default: return (int)hipErrorInvalidValue;
  }
}
#ifdef LZ4HIP_RING_DBG
int ring_stats_take_trio(unsigned long long* sum8) { return ring_stats_take(sum8); }
#endif

}  // namespace lz4hip
