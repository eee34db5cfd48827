// tests/backend/devprobe.hip -- TEST INFRASTRUCTURE ONLY (never part of liblz4hip.so; links against the HIP runtime alone).
// The DEVICE instantiation of tests/backend/probes.h: every probe on csrc's WaveDev, GroupDev<GL> and BlockWaveDev<KW, KS>, one
// kernel per family and one host entry per family for ctypes.  An entry allocates, copies in, launches once, synchronises,
// copies out, frees, and returns the HIP error code.  tests/hostsim/hostsim_backend.cpp is the same probes on the lane
// simulator's backends and documents the slot layouts; tests/test_gpu_backend.py compares the two output images.
// One case per wavefront (WaveDev, BlockWaveDev) or per lane group (GroupDev<GL>: a wavefront's other groups run other cases).
// Every kernel is a bounded loop over its own case: none waits on memory that another wavefront writes.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I lz4-java_amd/csrc -fPIC -shared -o tests/backend/libdevprobe.so tests/backend/devprobe.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_dev.h"
#include "group_dev.h"
#define PROBE_FN __device__ inline
#include "probes.h"

#ifndef LZ4HIP_LDS_PAD
#define LZ4HIP_LDS_PAD 0   // (kernels_internal.h: the lane-group decoders' developer A/B knob)
#endif

namespace {

using namespace lz4hip;

// GL lanes share a case; BYTES: the case's LDS bytes
template <int GL, uint32_t BYTES>
struct DevHarness {
  // a value every lane of the CASE holds: a scalar for a whole wavefront; left alone where the wavefront's groups run different cases
  __device__ static uint32_t uni(uint32_t x) { return GL == 64 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)x) : x; }
  __device__ static void put32(uint32_t* p, uint32_t v) { if ((threadIdx.x & (GL - 1)) == 0) *p = v; }
  __device__ static void poison(uint8_t* lds) {
    static_assert(BYTES % 4u == 0u, "whole words");
    for (uint32_t i = (threadIdx.x & (GL - 1)) * 4u; i < BYTES; i += 4u * GL) *(uint32_t*)(lds + i) = 0xEEEEEEEEu;
  }
  __device__ static void poison_stage(uint8_t* lds) { poison(lds); }
  __device__ static void poison_wave(uint8_t* lds) { poison(lds); }
};

using probes::kWaveTable;   // WaveDev's table: 32 KB per wavefront
static_assert(GroupDev<4>::kStage == GroupDev<64>::kStage, "one staging size for every group size");

__global__ __launch_bounds__(64) void wave_kernel(const uint32_t* rec, uint32_t n, const uint8_t* in, size_t in_stride, uint8_t* out,
                                                  size_t out_stride) {
  __shared__ __attribute__((aligned(16))) uint8_t table[kWaveTable];
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  WaveDev w(table);
  probes::wave_probe<WaveDev, DevHarness<64, kWaveTable>>(w, rec + (size_t)i * probes::kRec, in + i * in_stride,
                                                           out + i * out_stride + probes::kGuard);
}

template <int GL>
__global__ __launch_bounds__(256) void group_kernel(const uint32_t* rec, uint32_t n, const uint8_t* in, size_t in_stride, uint8_t* out,
                                                    size_t out_stride) {
  constexpr uint32_t kPer = GroupDev<GL>::kStage;
  __shared__ __attribute__((aligned(16))) uint8_t stage_mem[(256 / GL) * kPer + LZ4HIP_LDS_PAD];
  const uint32_t gid = (blockIdx.x * 256u + threadIdx.x) / GL;
  if (gid >= n) return;   // a whole group leaves together
  GroupDev<GL> g;
  const uint32_t* r = rec + (size_t)gid * probes::kRec;
  uint8_t* slot = out + gid * out_stride;
  probes::group_probe<GroupDev<GL>, DevHarness<GL, kPer>>(g, r, in + gid * in_stride, slot + 128 + r[7], stage_mem + (threadIdx.x / GL) * kPer,
                                                          (uint32_t*)(slot + out_stride - 128u));
}

template <int KW, int KS>
__global__ __launch_bounds__(64) void bwave_kernel(const uint32_t* rec, uint32_t n, const uint8_t* common, const uint8_t* in, size_t in_stride,
                                                   uint8_t* out, size_t out_stride) {
  typedef BlockWaveDev<KW, KS> G;
  __shared__ __attribute__((aligned(16))) uint8_t wave_mem[G::kWaveLds];
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  G g;
  const uint32_t* r = rec + (size_t)i * probes::kRec;
  uint8_t* slot = out + i * out_stride;
  probes::bwave_probe<WaveDev, G, DevHarness<64, G::kWaveLds>>(g, r, common, in + i * in_stride, slot + 256, slot + 1792 + (r[15] & 255u), wave_mem);
}

// device copies of a launch's images; ok() is false once any HIP call failed
struct Images {
  hipError_t e = hipSuccess;
  void* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
  int k = 0;
  bool ok() const { return e == hipSuccess; }
  template <class T> T* up(const T* host, size_t bytes) {
    void* d = nullptr;
    if (ok()) e = hipMalloc(&d, bytes ? bytes : 4);
    if (ok()) { ptr[k++] = d; if (bytes) e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice); }
    return (T*)d;
  }
  int finish(uint8_t* host_out, const uint8_t* dev_out, size_t bytes) {
    if (ok()) e = hipGetLastError();
    if (ok()) e = hipDeviceSynchronize();
    if (ok()) e = hipMemcpy(host_out, dev_out, bytes, hipMemcpyDeviceToHost);
    for (int i = 0; i < k; i++) { const hipError_t f = hipFree(ptr[i]); if (ok()) e = f; }
    return (int)e;
  }
};

}  // namespace

extern "C" {

void devprobe_constants(uint32_t* out8) { probes::constants<GroupDev<4>::kStage>(out8); }

int devprobe_wave(const uint32_t* rec, int n, const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride) {
  if (n <= 0) return 0;
  Images m;
  const uint32_t* d_rec = m.up(rec, (size_t)n * probes::kRec * 4u);
  const uint8_t* d_in = m.up(in, (size_t)n * in_stride);
  uint8_t* d_out = m.up(out, (size_t)n * out_stride);
  if (m.ok()) wave_kernel<<<dim3((uint32_t)n), dim3(64)>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
  return m.finish(out, d_out, (size_t)n * out_stride);
}

int devprobe_group(int gl, const uint32_t* rec, int n, const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride) {
  if (n <= 0) return 0;
  if (gl != 4 && gl != 8 && gl != 16 && gl != 32 && gl != 64) return (int)hipErrorInvalidValue;
  Images m;
  const uint32_t* d_rec = m.up(rec, (size_t)n * probes::kRec * 4u);
  const uint8_t* d_in = m.up(in, (size_t)n * in_stride);
  uint8_t* d_out = m.up(out, (size_t)n * out_stride);
  const dim3 grid(((uint32_t)n * (uint32_t)gl + 255u) / 256u), block(256);
  if (m.ok()) {
    if (gl == 4) group_kernel<4><<<grid, block>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
    else if (gl == 8) group_kernel<8><<<grid, block>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
    else if (gl == 16) group_kernel<16><<<grid, block>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
    else if (gl == 32) group_kernel<32><<<grid, block>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
    else group_kernel<64><<<grid, block>>>(d_rec, (uint32_t)n, d_in, in_stride, d_out, out_stride);
  }
  return m.finish(out, d_out, (size_t)n * out_stride);
}

// cfg: the row of decode_wave.hip's launch table -- (KW, KS) = (8192, 1024), (16384, 2048), (32768, 2048), (65536, 2048)
int devprobe_bwave(int cfg, const uint32_t* rec, int n, const uint8_t* common, size_t common_size, const uint8_t* in, size_t in_stride,
                   uint8_t* out, size_t out_stride) {
  if (n <= 0) return 0;
  if (cfg < 0 || cfg > 3) return (int)hipErrorInvalidValue;
  Images m;
  const uint32_t* d_rec = m.up(rec, (size_t)n * probes::kRec * 4u);
  const uint8_t* d_common = m.up(common, common_size);
  const uint8_t* d_in = m.up(in, (size_t)n * in_stride);
  uint8_t* d_out = m.up(out, (size_t)n * out_stride);
  const dim3 grid((uint32_t)n), block(64);
  if (m.ok()) {
    if (cfg == 0) bwave_kernel<8192, 1024><<<grid, block>>>(d_rec, (uint32_t)n, d_common, d_in, in_stride, d_out, out_stride);
    else if (cfg == 1) bwave_kernel<16384, 2048><<<grid, block>>>(d_rec, (uint32_t)n, d_common, d_in, in_stride, d_out, out_stride);
    else if (cfg == 2) bwave_kernel<32768, 2048><<<grid, block>>>(d_rec, (uint32_t)n, d_common, d_in, in_stride, d_out, out_stride);
    else bwave_kernel<65536, 2048><<<grid, block>>>(d_rec, (uint32_t)n, d_common, d_in, in_stride, d_out, out_stride);
  }
  return m.finish(out, d_out, (size_t)n * out_stride);
}

}  // extern "C"
