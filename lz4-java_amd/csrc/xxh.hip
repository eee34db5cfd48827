// xxh.hip -- the xxhash kernels of the engine and the synthetic workload generator (gfx950).
//
//   xxh_multi_kernel<T,4>: 16 buffers per wavefront streamed through LDS, every lane an accumulator chain (xxh_core.h);
//                          xxh*_wave_kernel / xxh_stream_kernel: one wavefront per long buffer / stream.  Bound: HBM (1 B/B).
//   gen_blocks_kernel    : SURVEY.md App. F workload generator (setup only, never timed).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>
#include "kernels.h"
#include "xxh_core.h"

namespace lz4hip {

// ------------------------------------------------------------------------------------------------
// xxhash
// ------------------------------------------------------------------------------------------------
// XXH32 is a serial chain per buffer (the round is not associative), so one thread per buffer is the right shape for many
// buffers -- but a lone thread walking a LONG buffer pays a full memory round trip per 64 bytes (0.16 GB/s).  With few buffers
// each gets a wavefront instead: all 64 lanes stream the buffer through LDS in 4 KB chunks (double-buffered, coalesced 1 KB
// loads), lanes 0..3 each own one accumulator and read their word of every stripe from LDS; the chain itself is all that is left.
// Generic in the word type: lane k (mod 4) folds word k of `nst` whole stripes starting at `bulk` into its accumulator v
// (4 KB chunks through LDS, double-buffered).  Used by the long-buffer kernels and by the streaming kernels.
template <class T>
__device__ __forceinline__ T xxh_absorb(T v, const uint8_t* bulk, uint32_t nst, uint32_t (*stage)[1024], uint32_t lane) {
  constexpr uint32_t STRIPE = 4u * sizeof(T), SPC = 4096u / STRIPE;
  const uint32_t k = lane & 3u;
  const uint64_t lim = (uint64_t)nst * STRIPE;
  const uint32_t nchunks = (nst + SPC - 1u) / SPC;
  uint4 r[4];
  auto fetch = [&](uint32_t c) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint64_t o = (uint64_t)c * 4096u + (uint32_t)i * 1024u + lane * 16u;
      if (o + 16u <= lim) __builtin_memcpy(&r[i], bulk + o, 16);
    }
  };
  // the input half of the round (in * PRIME_2) does not depend on the accumulator: all 64 lanes do it here, 16 bytes each,
  // so the 4-lane serial chain is left with add, rotate, one multiply per stripe (integer multiplies are quarter rate)
  auto put = [&](uint32_t c) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      T w[16 / sizeof(T)];
      __builtin_memcpy(w, &r[i], 16);
#pragma unroll
      for (uint32_t q = 0; q < 16 / sizeof(T); q++) w[q] = XxhOps<T>::premul(w[q]);
      __builtin_memcpy(&stage[c & 1u][(uint32_t)i * 256u + lane * 4u], w, 16);
    }
  };
  if (nchunks) { fetch(0); put(0); }
  __syncthreads();
  for (uint32_t c = 0; c < nchunks; c++) {
    const bool more = c + 1u < nchunks;
    if (more) fetch(c + 1u);
    const uint8_t* st = (const uint8_t*)stage[c & 1u] + k * sizeof(T);
    const uint32_t cnt = nst - c * SPC < SPC ? nst - c * SPC : SPC;
#pragma unroll 8
    for (uint32_t s = 0; s < cnt; s++) {
      T x;
      __builtin_memcpy(&x, st + s * STRIPE, sizeof(T));
      v = XxhOps<T>::round_pre(v, x);
    }
    if (more) put(c + 1u);
    __syncthreads();
  }
  return v;
}
template <class T> __device__ __forceinline__ T xxh_lane_get(T v, int l);
template <> __device__ __forceinline__ uint32_t xxh_lane_get<uint32_t>(uint32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
template <> __device__ __forceinline__ uint64_t xxh_lane_get<uint64_t>(uint64_t v, int l) {
  // (the builtin returns int: go through uint32_t, or the low half sign-extends into the high one)
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)v, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32);
}

// Many buffers, coalesced: 64/LPB buffers per wavefront, LPB lanes each.  The one-thread-per-buffer kernels read 16 bytes from
// 64 different cache lines per load instruction; here every LPB-lane group streams its buffer through LDS with contiguous
// 16*LPB-byte loads (chunks of 256*LPB bytes, the input multiply applied while staging) and lanes 0..3 of the group run the four
// accumulator chains.  Measured on 1 Mi x 4 KiB (tools/xxh_cfg5.py): one thread per buffer 4.5 / 4.6 TB/s (XXH32 / XXH64);
// LPB = 16: 5.2 / 4.5 (only 16 of 64 lanes carry a chain: XXH64's 64-bit multiplies make that the cost); LPB = 8: 6.1 / -;
// LPB = 4 (all 64 lanes carry a chain, a buffer still reads 64 contiguous bytes per instruction): 6.2 / 6.2 TB/s.
// (lz4hip_set_option "xxh_kernel": 0 selects the one-thread-per-buffer kernels.)
template <class T, int LPB>
__global__ __launch_bounds__(64) void xxh_multi_kernel(const uint8_t* buf, const uint64_t* off, const int32_t* len, T seed, T* out, uint32_t nbuf) {
  constexpr uint32_t STRIPE = 4u * sizeof(T), CH = 256u * LPB, SPC = CH / STRIPE, NG = 64u / LPB;
  __shared__ __attribute__((aligned(16))) uint32_t stage[NG][CH / 4u];  // 16 KB
  const uint32_t lane = threadIdx.x, g = lane / LPB, gl = lane % LPB, k = lane & 3u;
  const uint32_t b = blockIdx.x * NG + g;
  const bool have = b < nbuf;
  const int32_t l = have ? len[b] : 0;
  const uint32_t n = l < 0 ? 0u : (uint32_t)l;
  const uint8_t* p = buf + (have ? off[b] : 0ull);
  const uint32_t nst = n / STRIPE;
  const uint32_t lim = nst * STRIPE;
  uint32_t nch = (nst + SPC - 1u) / SPC;
#pragma unroll
  for (int d = 32; d >= LPB; d >>= 1) nch = max(nch, (uint32_t)__shfl_xor((int)nch, d, 64));  // the wave runs the longest buffer's trip count
  T v = XxhOps<T>::init(seed, k);
  for (uint32_t c = 0; c < nch; c++) {
    uint4 r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t o = c * CH + (uint32_t)i * (16u * LPB) + gl * 16u;
      if (o + 16u <= lim) __builtin_memcpy(&r[i], p + o, 16);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
      T w[16 / sizeof(T)];
      __builtin_memcpy(w, &r[i], 16);
#pragma unroll
      for (uint32_t q = 0; q < 16 / sizeof(T); q++) w[q] = XxhOps<T>::premul(w[q]);
      __builtin_memcpy(&stage[g][(uint32_t)i * (4u * LPB) + gl * 4u], w, 16);
    }
    __syncthreads();
    const uint8_t* st = (const uint8_t*)stage[g] + k * sizeof(T);
    const uint32_t done = c * SPC;
    const uint32_t cnt = nst > done ? (nst - done < SPC ? nst - done : SPC) : 0u;
#pragma unroll 8
    for (uint32_t s = 0; s < cnt; s++) {
      T x;
      __builtin_memcpy(&x, st + s * STRIPE, sizeof(T));
      v = XxhOps<T>::round_pre(v, x);
    }
    __syncthreads();
  }
  const int base = (int)(g * LPB);
  const T v1 = __shfl(v, base, 64), v2 = __shfl(v, base + 1, 64), v3 = __shfl(v, base + 2, 64), v4 = __shfl(v, base + 3, 64);
  if (gl == 0u && have) out[b] = XxhOps<T>::finish(v1, v2, v3, v4, seed, p + lim, n - lim, n);
}

__global__ __launch_bounds__(64) void xxh32_wave_kernel(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed, uint32_t* out) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[2][1024];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  const int32_t l = len[b];
  const uint32_t n = l < 0 ? 0u : (uint32_t)l;
  const uint8_t* p = buf + off[b];
  if (n < 8192u) {
    if (lane == 0) out[b] = xxh32_one(p, n, seed);
    return;
  }
  const uint32_t nst = n / 16u;
  const uint32_t v = xxh_absorb<uint32_t>(XxhOps<uint32_t>::init(seed, lane & 3u), p, nst, stage, lane);
  const uint32_t v1 = xxh_lane_get(v, 0), v2 = xxh_lane_get(v, 1), v3 = xxh_lane_get(v, 2), v4 = xxh_lane_get(v, 3);
  if (lane == 0) out[b] = XxhOps<uint32_t>::finish(v1, v2, v3, v4, seed, p + (size_t)nst * 16u, n - nst * 16u, n);
}
int launch_xxh32(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed, uint32_t* out, uint32_t n, void* stream) {
  if (n == 0) return 0;
  if (n <= 512u) hipLaunchKernelGGL(xxh32_wave_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, buf, off, len, seed, out);
  else hipLaunchKernelGGL((xxh_multi_kernel<uint32_t, 4>), dim3((n + 15u) / 16u), dim3(64), 0, (hipStream_t)stream, buf, off, len, seed, out, n);
  return (int)hipGetLastError();
}
__global__ __launch_bounds__(64) void xxh64_wave_kernel(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, uint64_t* out) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[2][1024];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  const int32_t l = len[b];
  const uint32_t n = l < 0 ? 0u : (uint32_t)l;
  const uint8_t* p = buf + off[b];
  if (n < 8192u) {
    if (lane == 0) out[b] = xxh64_one(p, n, seed);
    return;
  }
  const uint32_t nst = n / 32u;
  const uint64_t v = xxh_absorb<uint64_t>(XxhOps<uint64_t>::init(seed, lane & 3u), p, nst, stage, lane);
  const uint64_t v1 = xxh_lane_get(v, 0), v2 = xxh_lane_get(v, 1), v3 = xxh_lane_get(v, 2), v4 = xxh_lane_get(v, 3);
  if (lane == 0) out[b] = XxhOps<uint64_t>::finish(v1, v2, v3, v4, seed, p + (size_t)nst * 32u, n - nst * 32u, n);
}

// StreamingXXHash32/64.update (XXHashJNI.c:108-121 / :218-231): one wavefront continues the stream `rec` over data[0..len).
// reset != 0: the stream is (re)started with `seed` first (XXH32_init / XXH64_init + reset, XXHashJNI.c:90-101); len may be 0.
template <class T>
__global__ __launch_bounds__(64) void xxh_stream_kernel(XxhRec<T>* rec, const uint8_t* data, uint32_t len, int reset, T seed_in) {
  constexpr uint32_t STRIPE = 4u * sizeof(T);
  __shared__ __attribute__((aligned(16))) uint32_t stage[2][1024];
  __shared__ __attribute__((aligned(16))) uint8_t memb[2 * STRIPE];
  const uint32_t lane = threadIdx.x, k = lane & 3u;
  const T seed = reset ? seed_in : rec->seed;
  T v = reset ? XxhOps<T>::init(seed, k) : rec->v[k];
  const uint32_t ms = reset ? 0u : rec->memsize;
  const uint64_t total = (reset ? 0ull : rec->total) + len;
  if (lane < ms) memb[lane] = rec->mem[lane];
  uint32_t newms;
  if (ms + len < STRIPE) {  // still no whole stripe: only buffer
    if (lane < len) memb[ms + lane] = data[lane];
    newms = ms + len;
    __syncthreads();
  } else {
    const uint32_t head = ms ? STRIPE - ms : 0u;  // bytes that complete the buffered stripe
    if (ms) {
      if (lane < head) memb[ms + lane] = data[lane];
      __syncthreads();
      v = XxhOps<T>::round(v, ((const T*)memb)[k]);
      __syncthreads();
    }
    const uint8_t* bulk = data + head;
    const uint32_t blen = len - head, nst = blen / STRIPE;
    v = xxh_absorb<T>(v, bulk, nst, stage, lane);
    newms = blen - nst * STRIPE;
    if (lane < newms) memb[lane] = bulk[(size_t)nst * STRIPE + lane];
    __syncthreads();
  }
  const T v1 = xxh_lane_get(v, 0), v2 = xxh_lane_get(v, 1), v3 = xxh_lane_get(v, 2), v4 = xxh_lane_get(v, 3);
  if (lane < 4u) rec->v[lane] = v;
  if (lane < newms) rec->mem[lane] = memb[lane];
  if (lane == 0) {
    rec->total = total;
    rec->seed = seed;
    rec->memsize = newms;
    rec->digest = XxhOps<T>::finish(v1, v2, v3, v4, seed, memb, newms, total);
  }
}
int launch_xxh32_stream(void* rec, const uint8_t* data, uint32_t len, int reset, uint32_t seed, void* stream) {
  hipLaunchKernelGGL(xxh_stream_kernel<uint32_t>, dim3(1), dim3(64), 0, (hipStream_t)stream, (XxhRec<uint32_t>*)rec, data, len, reset, seed);
  return (int)hipGetLastError();
}
int launch_xxh64_stream(void* rec, const uint8_t* data, uint32_t len, int reset, uint64_t seed, void* stream) {
  hipLaunchKernelGGL(xxh_stream_kernel<uint64_t>, dim3(1), dim3(64), 0, (hipStream_t)stream, (XxhRec<uint64_t>*)rec, data, len, reset, seed);
  return (int)hipGetLastError();
}
size_t xxh_stream_rec_bytes(bool is64) { return is64 ? sizeof(XxhRec<uint64_t>) : sizeof(XxhRec<uint32_t>); }
size_t xxh_stream_digest_offset(bool is64) { return is64 ? offsetof(XxhRec<uint64_t>, digest) : offsetof(XxhRec<uint32_t>, digest); }

int launch_xxh64(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, uint64_t* out, uint32_t n, void* stream) {
  if (n == 0) return 0;
  if (n <= 512u) hipLaunchKernelGGL(xxh64_wave_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, buf, off, len, seed, out);
  else hipLaunchKernelGGL((xxh_multi_kernel<uint64_t, 4>), dim3((n + 15u) / 16u), dim3(64), 0, (hipStream_t)stream, buf, off, len, seed, out, n);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// synthetic workload -- one thread per block, setup only
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ __launch_bounds__(64) void gen_blocks_kernel(uint8_t* dst, uint64_t stride, int32_t block_len, uint64_t seed, uint64_t first_idx,
                                                        uint32_t litmax, uint32_t win, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n_blocks) return;
  uint8_t* out = dst + (uint64_t)i * stride;
  const int64_t n = block_len;
  uint64_t s = seed ^ ((first_idx + i) * 0x9E3779B97F4A7C15ull);
  int64_t len = 0;
  while (len < n) {
    uint32_t ll = 1u + (uint32_t)(splitmix64(s) % litmax);
    while (ll > 0) {
      const uint64_t w = splitmix64(s);
      const uint32_t k = ll < 8u ? ll : 8u;
      for (uint32_t j = 0; j < k; j++) { if (len < n) out[len] = (uint8_t)(w >> (8u * j)); len++; }
      ll -= k;
    }
    if (len >= 16 && len < n) {
      const uint32_t ml = 4u + (uint32_t)(splitmix64(s) % 61u);
      const uint64_t lim = (uint64_t)len < (uint64_t)win ? (uint64_t)len : (uint64_t)win;
      const uint64_t off = 1u + splitmix64(s) % lim;
      for (uint32_t j = 0; j < ml; j++) { if (len < n) out[len] = out[len - (int64_t)off]; len++; }
    }
  }
}
int launch_gen_blocks(uint8_t* dst, uint64_t stride, int32_t block_len, uint64_t seed, uint64_t first_idx,
                      uint32_t litmax, uint32_t win, uint32_t n_blocks, void* stream) {
  if (n_blocks == 0) return 0;
  hipLaunchKernelGGL(gen_blocks_kernel, dim3((n_blocks + 63u) / 64u), dim3(64), 0, (hipStream_t)stream,
                     dst, stride, block_len, seed, first_idx, litmax, win, n_blocks);
  return (int)hipGetLastError();
}

}  // namespace lz4hip
