// decode_stream.hip -- the stream decoder of the LZ4 block engine (gfx950): LZ4_decompress_safe_continue over many streams whose blocks
// land anywhere (rings, alternating buffers, save areas, dictionaries elsewhere), every mode of liblz4's LZ4_streamDecode_t.
//
//   decode_stream_kernel<GL>
//                        : decode_chain_kernel's shape (decode_chain.hip).  GL lanes of a wavefront share one STREAM
//                          (lz4_decode_stream.h): they draw it from a queue word, read its state record, walk its blocks of this
//                          launch in order -- per block the state picks decode_block's PREFIX instance (no history, a small prefix,
//                          64 KB of prefix) or its PREFIX && DICT instance (after a jump, and while a short prefix grows behind an
//                          external dictionary) -- and write the record back.  The deep loop for streams of 2 KB and more, the
//                          pipelined loop and the exact tiers below, as in the chain kernel: output stays in memory, where the
//                          history is.
// A stream is serial by construction, so it never leaves its lane group, and NO group waits for another group, wavefront or workgroup
// anywhere: parallelism comes from the number of streams alone.  Block k + 1 reads what the same lanes stored for block k: the stores
// come first in the wavefront's program order, and between two blocks the kernel waits for every outstanding store (fence).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_stream.h"

namespace lz4hip {

struct DStreamIoDev {
  const DStreamArgs& a;
  bool first;   // lane 0 of the group
  __device__ __forceinline__ DStreamState get_state(uint32_t c) const { return a.state[c]; }   // (every lane reads it: a uniform load per group)
  __device__ __forceinline__ void put_state(uint32_t c, const DStreamState& s) const { if (first) a.state[c] = s; }
  __device__ __forceinline__ void put_out(uint32_t i, int r) const { if (first) a.out[i] = r; }
  __device__ __forceinline__ void begin_block(const uint8_t*, int) const {}
  // as ChainIoDev::fence: no memory operation moves across this point in the compiled code, and the wavefront waits for its
  // outstanding vector memory operations (vmcnt(0): stores count there on gfx9)
  __device__ __forceinline__ void fence() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

#ifndef LZ4HIP_DSTREAM_WGS
#define LZ4HIP_DSTREAM_WGS 2   // workgroups of 256 threads per CU the kernel asks for (the deep loop's request, as the chain kernel's)
#endif
template <int GL>
__global__ __launch_bounds__(256, LZ4HIP_DSTREAM_WGS) void decode_stream_kernel(DStreamArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds];
  GroupDev<GL> g;
  uint8_t* const stage = stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds;
  DStreamIoDev io{a, g.l == 0};
  for (;;) {
    // One stream per group: EVERY lane takes part in the add -- the group's lane 0 adds 1 and the others 0 -- and takes lane 0's
    // result, with no branch in front of the broadcast: decode_chain.hip says what a branch there did.
    uint32_t c = atomicAdd(q, g.l == 0 ? 1u : 0u);
    c = (uint32_t)__shfl((int)c, 0, GL);
    if (c >= a.n_chains) return;
    dstream_walk(g, io, a, c, stage);
  }
}

int launch_decompress_stream(const DStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n_chains == 0) return 0;
  if (!q) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(q, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  constexpr uint32_t GL = 8u, per_wg = 256u / GL;
  const uint32_t want = (a.n_chains + per_wg - 1u) / per_wg, most = (n_cus ? n_cus : 256u) * 4u;   // (as launch_decompress_chain)
  hipLaunchKernelGGL((decode_stream_kernel<8>), dim3(want < most ? want : most), dim3(256), 0, st, a, q);
  return (int)hipGetLastError();
}

// ---- streams whose slots overlap their history (lz4_decode_inorder.h): the twin ----
//   decode_stream_inorder_kernel<GL>
//                        : decode_stream_kernel's shape -- groups of GL lanes draw streams from the queue word with every lane in the
//                          add, nobody waits for another group, a fence between two blocks.  Per block the walk tests, from the state
//                          it holds, whether the slot overlaps the piece of the external dictionary the block can reach: such a block
//                          (or every block, a.every) is decoded by decode_block_inorder, every other one by the instance
//                          decode_stream_kernel gives it.
struct DStreamInorderIoDev : DStreamIoDev {
  __device__ __forceinline__ void in_order(bool) const {}
};

template <int GL>
__global__ __launch_bounds__(256, LZ4HIP_DSTREAM_WGS) void decode_stream_inorder_kernel(DStreamInorderArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds];
  InOrder<GroupDev<GL>> g;
  uint8_t* const stage = stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds;
  DStreamInorderIoDev io{{a.s, g.l == 0}};
  const bool every = a.every != 0u;
  for (;;) {
    uint32_t c = atomicAdd(q, g.l == 0 ? 1u : 0u);   // (every lane in the add, no branch in front of the broadcast: as above)
    c = (uint32_t)__shfl((int)c, 0, GL);
    if (c >= a.s.n_chains) return;
    dstream_walk<InOrder<GroupDev<GL>>, DStreamInorderIoDev, 2, true>(g, io, a.s, c, stage, every);
  }
}

int launch_decompress_stream_inorder(const DStreamInorderArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.s.n_chains == 0) return 0;
  if (!q) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(q, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  constexpr uint32_t GL = 8u, per_wg = 256u / GL;
  const uint32_t want = (a.s.n_chains + per_wg - 1u) / per_wg, most = (n_cus ? n_cus : 256u) * 4u;   // (as launch_decompress_stream)
  hipLaunchKernelGGL((decode_stream_inorder_kernel<8>), dim3(want < most ? want : most), dim3(256), 0, st, a, q);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
