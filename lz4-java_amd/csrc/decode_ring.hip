// decode_ring.hip -- the ring loop's decoder of the LZ4 block engine (gfx950): decode_ring_kernel<GL, KW, SAFE>, lz4_decode_ring.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_core.h"

namespace lz4hip {

// the ring loop's kernel (lz4_decode_ring.h): per block a stream ring and an output ring of KW bytes in LDS.  One wavefront per
// workgroup: the LDS a workgroup asks for is what one wavefront's 64 / GL blocks need, so the CU fills to the last wavefront
// (KW 512, 4 lanes: 16 blocks x 832 bytes = 13 KB, 12 wavefronts per CU; KW 4096, 16 lanes: 4 x 4.6 KB, 8 per CU).
template <int GL, int KW, bool SAFE>
__global__ __launch_bounds__(64) void decode_ring_kernel(BatchArgs a, const uint32_t* route, uint32_t want) {
  if (route && *route != want) return;   // (the launch was routed to another decoder: launch_decompress)
  typedef GroupDev<GL, KW> G;
  __shared__ __attribute__((aligned(16))) uint8_t ring_mem[(64 / GL) * G::kRingLds + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 64u + threadIdx.x) / GL;
  if (gid >= a.n) return;
  G g;
  const int r = decode_block<G, SAFE, 3, false>(g, a.src + a.src_off[gid], a.src_len[gid], a.dst + a.dst_off[gid], a.dst_cap[gid],
                                               ring_mem + (threadIdx.x / GL) * G::kRingLds);
  if (g.l == 0) a.out[gid] = r;
}
template <int GL, int KW>
static int launch_decode_ring_t(const BatchArgs& a, bool safe, hipStream_t st, const uint32_t* route, uint32_t want) {
  const uint32_t per_wg = 64u / GL;
  const uint32_t grid = (a.n + per_wg - 1u) / per_wg;
  if (safe) hipLaunchKernelGGL((decode_ring_kernel<GL, KW, true>), dim3(grid), dim3(64), 0, st, a, route, want);
  else hipLaunchKernelGGL((decode_ring_kernel<GL, KW, false>), dim3(grid), dim3(64), 0, st, a, route, want);
  return (int)hipGetLastError();
}
// lanes 1 / 4 / 8 / 16 with an output ring of 256 .. 4096 bytes
int launch_decode_ring(const BatchArgs& a, bool safe, int lanes, int ring, hipStream_t st, const uint32_t* route, uint32_t want) {
  switch (lanes * 100000 + ring) {
    case 100256: return launch_decode_ring_t<1, 256>(a, safe, st, route, want);   // a lane per block: 64 blocks per wavefront, 16-byte steps
    case 100512: return launch_decode_ring_t<1, 512>(a, safe, st, route, want);
    case 400512: return launch_decode_ring_t<4, 512>(a, safe, st, route, want);
    case 401024: return launch_decode_ring_t<4, 1024>(a, safe, st, route, want);
    case 402048: return launch_decode_ring_t<4, 2048>(a, safe, st, route, want);
    case 800512: return launch_decode_ring_t<8, 512>(a, safe, st, route, want);
    case 801024: return launch_decode_ring_t<8, 1024>(a, safe, st, route, want);
    case 802048: return launch_decode_ring_t<8, 2048>(a, safe, st, route, want);
    case 804096: return launch_decode_ring_t<8, 4096>(a, safe, st, route, want);
    case 1602048: return launch_decode_ring_t<16, 2048>(a, safe, st, route, want);
    case 1604096: return launch_decode_ring_t<16, 4096>(a, safe, st, route, want);
    default: return (int)hipErrorInvalidValue;
  }
}
#ifdef LZ4HIP_RING_DBG
int ring_stats_take_ring(unsigned long long* sum8) { return ring_stats_take(sum8); }
#endif

}  // namespace lz4hip
