// decode_chain.hip -- the linked-block decoder of the LZ4 block engine (gfx950): LZ4_decompress_safe_continue over many chains.
//
//   decode_chain_kernel<GL>
//                        : GL lanes of a wavefront share one CHAIN (lz4_decode_chain.h): they draw it from a queue word -- chains
//                          differ in length, as the compressors' records do -- and walk its blocks in order with the core's PREFIX
//                          switch: the deep loop for streams of 2 KB and more, the pipelined loop and the exact tiers below.  Both
//                          interior loops keep their output in memory, where the history is; the LDS-staged forms cannot see it.
//                          Stored (raw) blocks are copied by the same lanes.
// One chain is serial by construction -- block k + 1 may copy from any byte block k decoded -- so a chain never leaves its lane
// group, and NO group waits for another group, wavefront or workgroup anywhere: parallelism comes from the number of chains alone
// (a single chain runs on 8 lanes of one wavefront).  Block k + 1 reads what the same lanes stored for block k: the stores come first
// in the wavefront's program order, and between two blocks the kernel waits for every outstanding store (ChainIoDev::fence), the way
// the deep loop retires its slots in front of a far read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "group_dev.h"
#include "lz4_decode_chain.h"

namespace lz4hip {

struct ChainIoDev {
  const ChainArgs& a;
  bool first;   // lane 0 of the group
  __device__ __forceinline__ void put_out(uint32_t i, int r) const { if (first) a.out[i] = r; }
  __device__ __forceinline__ void put_chain(uint32_t c, uint64_t n) const { if (first) a.chain_out[c] = n; }
  __device__ __forceinline__ void begin_block(const uint8_t*, int) const {}
  // the block's stores are complete before anything of the next block is loaded: no memory operation moves across this point in the
  // compiled code, and the wavefront waits for its outstanding vector memory operations (vmcnt(0): stores count there on gfx9)
  __device__ __forceinline__ void fence() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

#ifndef LZ4HIP_CHAIN_WGS
#define LZ4HIP_CHAIN_WGS 2   // workgroups of 256 threads per CU the kernel asks for (the deep loop's request)
#endif
template <int GL>
__global__ __launch_bounds__(256, LZ4HIP_CHAIN_WGS) void decode_chain_kernel(ChainArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * GroupDev<GL>::kStreamLds];
  GroupDev<GL> g;
  uint8_t* const stage = stage_mem + (threadIdx.x / GL) * GroupDev<GL>::kStreamLds;
  ChainIoDev io{a, g.l == 0};
  for (;;) {
    // One chain per group: EVERY lane takes part in the add -- the group's lane 0 adds 1 and the others 0 -- and takes lane 0's
    // result.  There is no branch in front of the broadcast on purpose.  With `if (lane 0) c = atomicAdd(q, 1)` the compiler gave the
    // other lanes a back edge of their own that skips the add (the condition is loop invariant) and nested the two cycles: those
    // lanes then reached the broadcast while lane 0 was masked off, read 0 from it and walked chain 0 for ever.
    uint32_t c = atomicAdd(q, g.l == 0 ? 1u : 0u);
    c = (uint32_t)__shfl((int)c, 0, GL);
    if (c >= a.n_chains) return;
    chain_walk(g, io, a, c, stage);
  }
}

int launch_decompress_chain(const ChainArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n_chains == 0) return 0;
  if (!q) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(q, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  constexpr uint32_t GL = 8u, per_wg = 256u / GL;
  const uint32_t want = (a.n_chains + per_wg - 1u) / per_wg, most = (n_cus ? n_cus : 256u) * 4u;   // (4 workgroups of 33 KB LDS fit a CU)
  hipLaunchKernelGGL((decode_chain_kernel<8>), dim3(want < most ? want : most), dim3(256), 0, st, a, q);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
