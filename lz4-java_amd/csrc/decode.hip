// decode.hip -- which decoder a decode launch gets: the device-side route sampler and launch_decompress, the router in front of the
// decoder family units (decode_lanes.hip, decode_ring.hip, decode_wave.hip, decode_pair.hip, decode_trio.hip).
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "group_dev.h"

namespace lz4hip {

#ifndef LZ4HIP_ROUTE_SHORT
#define LZ4HIP_ROUTE_SHORT 8   /* average output bytes per sampled sequence up to which a batch of more than 16 blocks per CU goes to the wave kernel (decode_route_kernel below) */
#endif
static std::atomic<int> g_route_short{LZ4HIP_ROUTE_SHORT};   // "decode_route_short": 0 = never the wave kernel
void set_route_short(int v) { g_route_short.store(v, std::memory_order_relaxed); }
uint32_t device_cus() {   // compute units of the current device (cached per device)
  static std::atomic<uint32_t> cus[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
  uint32_t c = cus[d].load(std::memory_order_relaxed);
  if (c == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) v = 256;
    c = (uint32_t)v;
    cus[d].store(c, std::memory_order_relaxed);
  }
  return c;
}

// Which decoder a batch of more than 16 blocks per CU gets is decided ON THE DEVICE (the launch is asynchronous and its arguments live
// in device memory): every candidate kernel is launched with the route word and the value it answers to; the ones that are not
// meant return at once.  *route =
//   1  the ring loop (lz4_decode_ring.h, 4 lanes, 2 KiB ring): a sample of the blocks averages at least `big` compressed bytes -- big
//      blocks with (typically) a short match window (BASELINE configs[2]: 847 vs 808-835 GB/s and a fabric traffic of 2.x instead of
//      3.75x the algorithmic bytes); only asked for batches of 16384 .. 40959 blocks (`big` = 0: never);
//   2  the wave kernel (lz4_decode_wave.h, a wavefront per block, W = 16): the sampled sequences are SHORT -- `seq_bytes` (8) or fewer
//      output bytes per sequence on average: text -- and NEAR: at least half of their offsets lie within 6 KB (the kernel's 8 KB ring).
//      The lane-group loops decode ~20 G sequences/s whatever the data (a match source is a memory request: text at 6 output bytes per
//      sequence is 128 GB/s where App. F data at 34 are 700); the wave kernel, its output window on chip, does text at 147 GB/s (65536
//      blocks; 8192: 140 against 60) and loses on everything longer, up to 2.5x (profiles/r06_route_sweep.txt);
//   3  the deep loop (lz4_decode_deep.h) for a batch of 40960 blocks or more whose sources are NEAR: the 4-lane staged loop -- the
//      default there since round 1, for App. F's offsets anywhere in 64 KB: 700 against 625 GB/s -- reads match sources from flushed
//      memory only and flushes everything when one reaches into staged bytes: a bitmap (run-length matches) decodes at 258 GB/s in
//      it and at 806 in the deep loop, near-offset synthetic streams gain 1 .. 15 %, text 10 %;
//   0  the lane-group default of the batch size (deep loop below 40960 blocks, 4-lane staged loop from there on).
// Round 5 sampled the HEAD of 16 streams with one lane each and took the route out again: a block's head is not its body (a text
// stream runs 16 compressed bytes per sequence in its first 512 bytes -- no history yet -- and 4.2 overall), and it looked at density
// alone.  This sampler reads the
// MIDDLE of the streams and needs no parse from the start for it: the walk of the wave loop (speculative next-token positions for
// every byte of a window, then the chain from the window's first byte) started at an ARBITRARY byte falls in with the true token
// chain within a few sequences -- chains that meet stay together -- and until it does it hops through literal bytes at about the
// data's own pace.  32 blocks spread over the batch, 1 KB from the middle of each, the first 256-byte window thrown away, hops per
// byte of the rest: Calgary book1 58 .. 69 sequences per 256 bytes (true: 61), App. F 9 .. 21 (15), 4 MiB App. F blocks 9 .. 16 (14),
// geo 4 .. 30 (7), pic 1 .. 44 (32) per SAMPLE; the route takes the sum over the 32.  One workgroup of 16 wavefronts, two blocks
// each, both 1 KB loads in flight together: ~10 us in front of launches of >= 0.9 ms.
__device__ uint32_t g_last_route[8];
__global__ __launch_bounds__(1024) void decode_route_kernel(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const int32_t* dst_cap, uint32_t n, uint32_t safe,
                                                            uint32_t big, uint32_t seq_bytes, uint32_t deep_if_near, uint32_t wave_small, uint32_t* route) {
  typedef BlockWaveDev<8192, 1024> G;   // (its hand-written walk: a static function of registers)
  constexpr uint32_t SPAN = 1024u, NS = 2u;
  __shared__ __attribute__((aligned(16))) uint8_t win[16][NS][SPAN + 32];
  __shared__ uint32_t acc[16][6];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  // ---- the blocks' sizes: 64 of them, wavefront 0 (the ring loop's criterion, unchanged) ----
  uint32_t avg = 0u;
  if (wave == 0u) {
    const uint32_t step = n > 64u ? n / 64u : 1u, i = lane * step;
    uint32_t v = (i < n && src_len[i] > 0) ? (uint32_t)src_len[i] : 0u, c = i < n ? 1u : 0u;
    for (int d = 32; d >= 1; d >>= 1) { v += (uint32_t)__shfl_xor((int)v, d, 64); c += (uint32_t)__shfl_xor((int)c, d, 64); }
    avg = c ? v / c : 0u;
  }
  // ---- the streams' density: wavefront w samples blocks (2 w + k) n / 32 + n / 64, k = 0, 1 ----
  uint32_t start[NS], have[NS];
#pragma unroll
  for (uint32_t k = 0; k < NS; k++) {
    const uint64_t bi = ((uint64_t)(NS * wave + k) * n) / (16u * NS) + n / (32u * NS);
    const uint32_t b = bi < n ? (uint32_t)bi : n - 1u;
    const int32_t len = uniform_i32(src_len[b]);
    // where to look: the middle of the stream.  The safe decoder is given the stream's length; the FAST decoder only a readable capacity
    // (LZ4_decompress_fast trusts the stream to end by itself) -- the middle of THAT is, for a slot of compressBound size, about where a
    // stream of ratio 2 ends (the first version of the route sampled the zeros behind the headline's streams and sent decompress_fast to
    // the wave kernel: 710 -> 442 GB/s).  There: a fifth of the OUTPUT size into the stream -- 40 % into a stream of ratio 2, 30 % into
    // text; not nearer the head: early in a block every offset is near.  Behind the end of a stream of ratio > 5 it finds what follows
    // it in the slot: zeros decode as sequences of offset 0, which no stream has -- such a sample routes nothing (below)
    uint32_t at = (uint32_t)(len > 0 ? len : 0) >> 1;
    if (!safe) { const uint32_t o5 = (uint32_t)max(uniform_i32(dst_cap[b]), 0) / 5u; at = at < o5 ? at : o5; }
    have[k] = (len >= 4096 && at >= 2048u && at + SPAN + 32u <= (uint32_t)len) ? 1u : 0u;   // (shorter streams are not sampled: their decode time is not in their interior loops)
    start[k] = have[k] ? (at & ~3u) : 0u;
    if (have[k]) {
      const uint8_t* p = uniform_ptr(src + src_off[b]) + start[k];
      // (byte loads assembled into dwords would be 16 instructions; the streams lie at any address, so: unaligned dword loads)
      uint32_t w[4];
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) __builtin_memcpy(&w[j], p + j * 256u + 4u * lane, 4);
      uint32_t tail = 0u;
      if (lane < 8u) __builtin_memcpy(&tail, p + SPAN + 4u * lane, 4);
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) *(uint32_t*)&win[wave][k][j * 256u + 4u * lane] = w[j];
      if (lane < 8u) *(uint32_t*)&win[wave][k][SPAN + 4u * lane] = tail;
    }
  }
  uint32_t seqs = 0u, bytes = 0u, near_n = 0u, off_n = 0u, out_n = 0u, zero_n = 0u;
#pragma unroll
  for (uint32_t k = 0; k < NS; k++) {
    if (!have[k]) continue;
    uint32_t ip = 0u;                             // relative to start[k]
    for (uint32_t wdw = 0; wdw < 4u && ip + 264u <= SPAN + 32u; wdw++) {
      const uint32_t* q = (const uint32_t*)&win[wave][k][(ip & ~3u) + 4u * lane];
      const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], sh = ip & 3u;
      const uint32_t blo = __builtin_amdgcn_alignbyte(d1, d0, sh), bhi = __builtin_amdgcn_alignbyte(d2, d1, sh);
      uint32_t nxpack = 0u;
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {         // (lz4_decode_wave.h step 1: where a token at window byte 4 l + j would be followed by the next)
        const uint32_t w = j == 0u ? blo : ((blo >> (8u * j)) | (bhi << (32u - 8u * j)));
        const uint32_t tl = (w >> 4) & 15u, e1 = (w >> 8) & 255u;
        const uint32_t nxt = 4u * lane + (j + 3u) + (tl == 15u ? 1u + e1 : 0u) + tl + ((w & 15u) == 15u ? 1u : 0u);
        nxpack |= (nxt <= 250u ? nxt : 255u) << (8u * j);
      }
      uint32_t posv = 0u, T = 0u;
      G::vwalk(nxpack, posv, T);
      const uint32_t last = T > 1u ? (uint32_t)__builtin_amdgcn_readlane((int)posv, (int)(T - 1u)) : 256u;   // the last start is where the next window begins
      const uint32_t hops = T > 1u ? T - 1u : 1u;
      if (wdw != 0u) {
        seqs += hops; bytes += last;
        // the sequences that start at the first T - 1 positions: how long they are (literals + match), and how many of their sources
        // lie within 6 KB (what a wave kernel's 8 KB ring still holds; the deep loop's near reads hit in L2)
        if (T > 1u) {
          const uint8_t* wb = &win[wave][k][0];
          const uint32_t p = ip + posv;                 // (lanes >= T - 1 are masked out below)
          const uint32_t tk = wb[p], tl = tk >> 4, tm = tk & 15u;
          const uint32_t lit = tl + (tl == 15u ? wb[p + 1u] : 0u);
          const uint32_t q = p + 1u + (tl == 15u ? 1u : 0u) + lit;
          const bool mine = lane < T - 1u && q + 3u <= SPAN + 32u;
          const uint32_t off = mine ? (uint32_t)wb[q] | ((uint32_t)wb[q + 1u] << 8) : 0xFFFFu;
          const uint32_t len = mine ? lit + tm + 4u + (tm == 15u ? wb[q + 2u] : 0u) : 0u;
          uint32_t ls = len;
          for (int d = 32; d >= 1; d >>= 1) ls += (uint32_t)__shfl_xor((int)ls, d, 64);
          out_n += (uint32_t)__builtin_amdgcn_readfirstlane((int)ls);
          near_n += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && off <= 6144u));
          off_n += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine));
          zero_n += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && off == 0u));
        }
      }
      ip += last;
    }
  }
  if (lane == 0u) { acc[wave][0] = seqs; acc[wave][1] = bytes; acc[wave][2] = near_n; acc[wave][3] = off_n; acc[wave][4] = out_n; acc[wave][5] = zero_n; }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t ts = 0u, tb = 0u, tn = 0u, to = 0u, tl = 0u, tz = 0u;
    for (uint32_t w = 0; w < 16u; w++) { ts += acc[w][0]; tb += acc[w][1]; tn += acc[w][2]; to += acc[w][3]; tl += acc[w][4]; tz += acc[w][5]; }
    const bool is_big = big != 0u && avg >= big;
    const bool sampled = tb >= 2048u && to >= 64u && 16u * tz <= to;   // (a few windows, a few dozen sequences -- and streams: offset 0 does not occur in one, zeros behind a stream's end are full of it)
    const bool is_near = sampled && 2u * tn >= to;
    // the wave kernel: SHORT sequences with near sources.  The lane-group loops decode ~20 G sequences/s whatever the data, i.e. GB/s in
    // proportion to the bytes a sequence produces; the wave kernel's rate grows far more slowly with them (text, 6 bytes per sequence:
    // 147 GB/s against 128; synthetic streams of 13: 88 against 237; 21: 304 against 483 -- tools/route_sweep.py, profiles/r06_route_sweep.txt)
    const bool is_short = seq_bytes != 0u && is_near && tl <= seq_bytes * to;
    // ... and, since the wave loop takes a window in segments and ends a block by liblz4's own rule (round 6, sessions w .. af), EVERY kind of data
    // in batches of up to 32 blocks per CU -- two rounds of its 16 wavefronts per CU -- but streams that are mostly literals (less than 1.25 output
    // bytes per stream byte as the sampled sequences have it: runs of 255 and more are one-sequence steps there).  6144 / 8192 blocks, wave against
    // deep loop (profiles/r06_route_sweep.txt, second sweep): text 156 / 206 against 46 / 60 GB/s, App. F 318 / 422 : 304 / 394, its 4 KB-window form
    // 383 / 512 : 348 / 453, a bitmap 428 / 565 : 383 / 488, 4 MiB blocks 432 / 576 : 401 / 533; geo (ratio 1.07) 196 / 260 : 328 / 421.  From
    // 12288 blocks on the lane-group loops win everything but text
    const bool lit_heavy = 4ull * tl * ts < 5ull * to * tb;
    const bool small_wave = wave_small != 0u && seq_bytes != 0u && sampled && !lit_heavy;
    const uint32_t r = is_big ? 1u : (is_short || small_wave) ? 2u : (deep_if_near != 0u && is_near) ? 3u : 0u;
    *route = r;
    g_last_route[0] = r; g_last_route[1] = ts; g_last_route[2] = tb; g_last_route[3] = avg;   // (diagnostic: last_decode_route)
    g_last_route[6] = tl; g_last_route[7] = tz;
    g_last_route[4] = tn; g_last_route[5] = to;
  }
}
int last_decode_route(uint32_t* out8) {   // what the last routed decode launch of this device decided: {route, sampled hops, sampled stream bytes, average compressed size, near offsets, sequences looked at, their output bytes, 0}
  return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_last_route), 8 * sizeof(uint32_t));
}

#ifdef LZ4HIP_RING_DBG
int ring_stats_fetch(unsigned long long* out8) {   // developer build: reads and clears the ring / wave / pair / trio loops' counters (one copy per unit that counts)
  for (int i = 0; i < 8; i++) out8[i] = 0;
  int e = ring_stats_take_ring(out8);
  if (e == 0) e = ring_stats_take_wave(out8);
  if (e == 0) e = ring_stats_take_pair(out8);
  if (e == 0) e = ring_stats_take_trio(out8);
  return e;
}
#endif
int launch_decompress(const BatchArgs& a, bool safe, int lanes_per_block, int pipe, int stage, int ring, void* stream, uint32_t* route_word) {
  if (a.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (pipe == 7) return launch_decode_pair(a, safe, ring, st);   // the pair loop: two wavefronts per block (lz4_decode_pair.h)
  if (pipe == 8) return launch_decode_trio(a, safe, ring, st);   // the trio loop: three (lz4_decode_trio.h)
  if (pipe == 4 || pipe == 5) return launch_decode_wave(a, safe, pipe == 5, ring, st);   // the wave loops: a wavefront per block (lanes_per_block is 64 by construction); 5: several sequences per trip
  if (pipe == 3) {   // the ring loop: lanes 4 / 8 / 16, output ring 512 .. 4096 bytes (0 = 512 with 4 lanes, 4096 otherwise)
    const int gl = lanes_per_block == 0 ? 4 : lanes_per_block;
    return launch_decode_ring(a, safe, gl, ring ? ring : (gl == 1 ? 256 : gl == 4 ? 512 : 4096), st);   // (decode_ring.hip has the (lanes, ring) table)
  }
  // Defaults by batch size (tools/decode_matrix.sh, tools/deep_matrix.sh; App. F / text / 4 MiB blocks):
  //   >= 40960 blocks: 4 lanes x 16 bytes per block (16 blocks per wavefront), plain loop with output staging -- the GPU is
  //                    full, long-sequence data is bandwidth-bound and short-sequence data issue-bound;
  //   fewer:           8 lanes, the deep loop (lz4_decode_deep.h).  Against the two-trip pipelined loop it replaced as the
  //                    default (GB/s of output): 16384 x 4 MiB 571 -> 794-821, 4096 x 4 MiB 185 (16 lanes) -> 282; 64 KiB App. F
  //                    blocks 2048: 70 -> 111, 8192: 264 -> 403, 16384: 438 -> 590, 24576: 538 -> 584, 32768: 551 -> 546, 40000: 542 ->
  //                    616; text 2048: 17 -> 34, 8192: 65 -> 125, 16384: 105 -> 153, 32768: 127 -> 133.  (16 lanes, the old choice
  //                    below 8192 blocks, are slower than 8 with this loop: 4096 blocks 182 vs 215.)
  const bool auto_lanes = lanes_per_block == 0;
  // Round 5: launches that cannot fill the GPU with blocks -- up to 16 per CU: the 8-GPU shard of BASELINE configs[2] (2048 x 4 MiB per
  // GPU), the readers' batches, the Java single-call path -- give every block a WAVEFRONT and decode several sequences of it per
  // trip (lz4_decode_wave.h, decode_pipe 5).  Against the lane-group loops below (GB/s of output, gpurun_out/r05j): 4 MiB blocks 256:
  // 17 -> 45, 2048: 135 -> 285, 4096: 272 -> 403 (8192: 519 -> 404, so not beyond 16 per CU); 64 KiB App. F 512: 31 -> 50, 2048: 120 -> 146,
  // 4096: 213 -> 232; 64 KiB text 512: 4.2 -> 16.1, 2048: 16.4 -> 49.6, 4096: 30.7 -> 66.4; one 64 KiB block 0.71 -> 0.43 ms.
  // Round 6: up to FIVE blocks per CU a block gets THREE wavefronts -- scanner, planner, copier (lz4_decode_trio.h, decode_pipe 8): with
  // SIMDs to spare the trip's three parts run side by side (4 MiB blocks 256: 69 -> 120 GB/s, 1024: 259 -> 352, 1280: 270 -> 383; one 64 KiB
  // block 0.284 -> 0.164 ms; two wavefronts -- the pair loop, decode_pipe 7 -- 93 / 295 / 0.221).  From six blocks per CU on one wavefront
  // per block is the faster form again: two of them per SIMD each issue 52 % of their cycles, the SIMD is full, and more wavefronts per
  // block only add their queues' instructions (2048 x 4 MiB: wave loop 432, trio with 8 KB rings 350, pair 393): profiles/r06_pair_notes.txt.
  if (auto_lanes && pipe < 0 && stage < 0 && a.n <= 5u * device_cus()) return launch_decode_trio(a, safe, 0, st);
  if (auto_lanes && pipe < 0 && stage < 0 && a.n <= 16u * device_cus()) return launch_decode_wave(a, safe, true, 0, st);
  if (auto_lanes) lanes_per_block = a.n >= 40960u ? 4 : 8;
  const int p = pipe < 0 ? ((a.n < 40960u && lanes_per_block >= 8) ? (lanes_per_block <= 16 ? 2 : 1) : 0) : pipe;
  // staging (whole-line output through LDS) pays where the batch is bandwidth-bound: App. F 65536 blocks 487 -> 680 GB/s
  // (text 106 -> 111); below that the pipelined loop wins (16384 blocks: 424 vs 289 staged vs 304 plain; 32768: 545 vs 447;
  // 49152: 508 vs 597)
  const bool sg = !p && (stage < 0 ? a.n >= 40960u : stage != 0);
  if (auto_lanes && pipe < 0 && stage < 0 && route_word) {
    // every default in place and more than 16 blocks per CU: the decoder is chosen on the device (decode_route_kernel above) -- by the
    // blocks' sizes between the deep loop and the ring loop (batches that fill the GPU with the ring loop's 16 blocks per wavefront,
    // 16384 .. 40959 blocks: 8192 x 4 MiB 409 vs 533 GB/s for the deep loop; 12288: 604 vs 670; 14336: 701 vs 757; 16384: 847 vs 815), and by what the streams
    // hold between either of them and the wave kernel
    const bool ring_size = a.n >= 16384u && a.n < 40960u, staged = a.n >= 40960u, wave_small = a.n <= 32u * device_cus();
    hipLaunchKernelGGL(decode_route_kernel, dim3(1), dim3(1024), 0, st, a.src, a.src_off, a.src_len, a.dst_cap, a.n, safe ? 1u : 0u, ring_size ? 512u << 10 : 0u,
                       (uint32_t)g_route_short.load(std::memory_order_relaxed), staged ? 1u : 0u, wave_small ? 1u : 0u, route_word);
    int e = staged ? launch_decode_lanes(a, safe, 4, 0, true, st, route_word) : launch_decode_lanes(a, safe, 8, 2, false, st, route_word);
    if (e == 0 && staged) e = launch_decode_lanes(a, safe, 8, 2, false, st, route_word, 3u);
    if (e == 0 && ring_size) e = launch_decode_ring(a, safe, 4, 2048, st, route_word, 1u);
    if (e == 0) e = launch_decode_wave(a, safe, true, 8192, st, route_word, 2u);
    return e;
  }
  return launch_decode_lanes(a, safe, lanes_per_block, p, sg, st);   // (4 / 16 / 32 / 64 lanes, anything else 8)
}

}  // namespace lz4hip
