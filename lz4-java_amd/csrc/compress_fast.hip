// compress_fast.hip -- the fast-compress kernels of the LZ4 block engine, hand-written for gfx950 (CDNA4, wave64).
//
//   compress_fast_v2w_cu_kernel / compress_fast_ms_cu_kernel
//                        : one workgroup per CU with 5 finder wavefronts (5 x 32 KB tables of {position, fingerprint} entries =
//                          the CU's whole LDS), every finder draws blocks from a queue.  v2w (the default): the lean finder of
//                          lz4_fast_v2_core.h -- its common step hand-scheduled in lz4_fast_v2_asm.h, every other step replayed
//                          by the exact step of lz4_fast_core.h -- parks bare hits in lanes, 64 at a time, and a WRITER wavefront
//                          per finder (no LDS needed) takes the batches through a ring in global memory and does all the output.
//                          ms: every sequence of a 64-position window per step (lz4_fast_ms_core.h), for blocks of short sequences.
//                          Bound: the serial parse chain of a wavefront x 5 chains per CU (roofline: HBM, 1+1/ratio B/B).
//   compress_fast_accel_cu_kernel
//                        : LZ4_compress_fast with acceleration 2 .. 65537: the one-sequence-per-step core of lz4_fast_core.h with
//                          its ACC switch, 5 wavefronts per CU drawing blocks from a queue (acceleration 1 is the kernels above).
//   compress_fast_dict_cu_kernel
//                        : LZ4_loadDict + LZ4_compress_fast_continue, a fresh stream per block: the same core and shape with the DICT
//                          switch; every table starts as the dictionary's image (dict_image_kernel builds it once per handle).
//   compress_fast_dest_cu_kernel
//                        : LZ4_compress_destSize: the same core and shape with DirectOut's FILL switch; a block ends once its
//                          target is full, so the work follows the input consumed.
// No MFMA anywhere: this is byte shuffling, not a contraction.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#include "kernels.h"
#include "kernels_internal.h"
#include "wave_dev.h"
#include "lz4_fast_core.h"
#include "lz4_fast_chain.h"
#include "lz4_fast_ms_core.h"
#include "lz4_fast_v2_core.h"
#include "mail_ring.h"

namespace lz4hip {

// ------------------------------------------------------------------------------------------------
// fast compress
// ------------------------------------------------------------------------------------------------
// (uniform_ptr / uniform_i32 -- kernels_internal.h -- put values loaded after a kernel's first store back into scalar registers)
// Adaptive two-pass scheme.  q = {next_block, n_routed, next_routed} (three queue words, zeroed by the first launch) and
// `routed` (u32[n], may be null = no routing): the one-sequence kernels probe the density of each block (lz4_fast_core.h,
// dense64); a block of short sequences is left unfinished and its index appended to routed[] for the window-parallel
// kernel, which draws exactly those.
#ifndef LZ4HIP_WPC
#define LZ4HIP_WPC 5
#endif
constexpr uint32_t WAVES_PER_CU = LZ4HIP_WPC;
#ifndef LZ4HIP_TABLE_U64
#define LZ4HIP_TABLE_U64 4096   // 32 KB per wavefront (developer probe builds: 2048 with LZ4HIP_PROBE_HLOG=12)
#endif
// Residency: a wavefront needs its 32 KB table and nothing else, but LDS is allocated in 1280-byte granules, so a 32768-byte
// workgroup occupies 33280 bytes and only FOUR fit a CU (measured: 1280 single-wave workgroups run in two rounds).  One
// workgroup that owns all 163840 bytes of the CU holds FIVE tables exactly: WAVES_PER_CU wavefronts, each compressing its own
// blocks, no barrier between them.  Blocks are handed out through the queue word q[0], so a wavefront that draws short blocks
// simply draws more of them.
// (The block body is written out in the kernel, not shared through a device function: behind a function
// boundary the per-block loads lose their no-clobber marking, become vector loads, and the whole scalar parser state follows
// them into vector registers -- 42 -> 83 VGPRs, -22 %.  Inside the loop every per-block value goes back to scalar registers
// through readfirstlane for the same reason.)
// (Rounds 1 and 2 also shipped the one-sequence-per-step core and the lean core WITHOUT writer wavefronts as kernels of their own,
// and a variant with three more chains per CU whose tables lived in global memory (+6 % for 7x the memory traffic): superseded,
// removed in round 3 -- git history has them.  FastCore stays: it is the exact path of the lean core and the byU32 core.)

// ------------------------------------------------------------------------------------------------
// lean core with a WRITER wavefront per chain.  A finder's 64-sequence batch write is ~20 scattered store instructions, and a
// wavefront's memory operations retire in order: the finder's next candidate fetch waits for all of them (8.6 % of the kernel,
// profiles/r02_compress_notes.txt).  LDS -- not wave slots -- is what limits a CU to five finders, and a writer needs no LDS:
// here every finder hands its parked batches to a partner wavefront of the same workgroup through a small ring in global memory
// (single producer, single consumer; ordered at WORKGROUP scope, see below -- which is only valid because both wavefronts belong to
// one workgroup and share the CU's L1: the kernel must not be built with -mtgsplit), and the partner does all the output of the block:
// literal copies, tokens, liblz4's capacity checks, the last literals and the block's result word.
// ------------------------------------------------------------------------------------------------
#ifndef LZ4HIP_MAIL_SLEEP
#define LZ4HIP_MAIL_SLEEP 32
#endif
// The protocol itself -- MailOut (finder side), mail_writer (writer side) -- lives in mail_ring.h, written against the wave
// backend W and a memory-ordering policy M so that the CPU suite runs the same source with two host threads per pair
// (tests/hostsim, tests/test_hostsim.py::test_mail_ring_*).  MailDev is the device policy:
// finder and writer are wavefronts of ONE workgroup, so everything is ordered at WORKGROUP scope: both see the CU's L1, and a
// release / acquire is a wait for the wave's own accesses, no cache maintenance.  (At agent scope a release writes the XCD's L2
// back and an acquire invalidates the CU's L1 for everybody on it: 2.3x .. 12x slower, measured.)
struct MailDev {
  __device__ __forceinline__ static uint32_t peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  // (every 64th poll of a wait: progress does not hang on the L1)
  __device__ __forceinline__ static uint32_t peek_far(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ static void acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
  __device__ __forceinline__ static void publish(uint32_t* p, uint32_t v) {   // every lane: this wave's earlier accesses are done first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (__lane_id() == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ static void nap_finder() { __builtin_amdgcn_s_sleep(16); }
  __device__ __forceinline__ static void nap_writer() { __builtin_amdgcn_s_sleep(LZ4HIP_MAIL_SLEEP); }
  template <class T> __device__ __forceinline__ static T* uptr(T* q) { return uniform_ptr(q); }
  __device__ __forceinline__ static int32_t u32(int32_t v) { return uniform_i32(v); }
  __device__ __forceinline__ static void block_begin(WaveDev&, const uint8_t*, uint32_t, uint8_t*, uint32_t) {}
  __device__ __forceinline__ static void result(int32_t* out, uint32_t b, int32_t r) { if (__lane_id() == 0) out[b] = r; }
};
template <class W> using MailOut = MailOutT<W, MailDev>;
__device__ __forceinline__ void mail_writer(const BatchArgs& a, uint32_t* slots, uint32_t* ctr) {
  WaveDev w(nullptr);
  mail_writer_t<WaveDev, MailDev>(w, a, slots, ctr);
}

// Control words of a fast-compress launch (the first words of its `mail` scratch): which blocks go to which kernel.
//   A block of 65547 bytes .. 4 MiB can use the compact table entries of lz4_fast_core.h (PK: {position 22 bits, fingerprint 10 bits},
//   16 KB per table), and a CU then holds TEN finder / writer pairs instead of five: compress_fast_v2wp_cu_kernel takes those blocks,
//   compress_fast_v2w_cu_kernel everything else.  The lengths live in device memory, so both kernels are always launched and decide
//   from these counts on the device; the one without work returns at once (~10 us per launch).
enum : uint32_t { CTL_PK = 0, CTL_OTHER = 1, CTL_DRAW_PK = 2, CTL_WORDS = 64 };
constexpr int32_t PK_MAX_N = 1 << 22;
__device__ __forceinline__ bool pk_block(int32_t n, int32_t cap) { return n >= 65547 && n <= PK_MAX_N && cap >= 0; }
__global__ __launch_bounds__(256) void compress_classify_kernel(const int32_t* src_len, const int32_t* dst_cap, uint32_t n, uint32_t* ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n;
  const bool pk = in && pk_block(src_len[i], dst_cap[i]);
  const uint32_t c_pk = (uint32_t)__builtin_popcountll(__ballot(pk)), c_ot = (uint32_t)__builtin_popcountll(__ballot(in && !pk));
  if (__lane_id() == 0) {
    if (c_pk) atomicAdd(ctl + CTL_PK, c_pk);
    if (c_ot) atomicAdd(ctl + CTL_OTHER, c_ot);
  }
}

// ---- the default: the five LDS pairs alone ----
__global__ __launch_bounds__(64 * 2 * WAVES_PER_CU) void compress_fast_v2w_cu_kernel(BatchArgs a, uint32_t* q, uint32_t* routed, uint32_t dense64, uint32_t* mail_ctr, uint32_t* mail_slots, const uint32_t* ctl) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t pair = blockIdx.x * WAVES_PER_CU + (wv < WAVES_PER_CU ? wv : wv - WAVES_PER_CU);
  uint32_t* ctr = mail_ctr + 2u * pair;
  uint32_t* slots = mail_slots + (size_t)pair * (MAIL_RING * MAIL_SLOT_WORDS);
  if (wv >= WAVES_PER_CU) { mail_writer(a, slots, ctr); return; }
  // the finders are issue-bound (lz4_fast_v2_asm.h), the writers mostly poll: the finders go first when both want to issue
  // (117.9 -> 119.8 GB/s on 65536 x 64 KiB; polling the ring four times less often instead changes nothing)
  __builtin_amdgcn_s_setprio(3);
  uint64_t* table = tables[wv];
  WaveDev w(table);
  uint32_t head = 0, tail_seen = 0;
  // (ctl: the ten-pair kernel ran before this one and took the blocks it can take)
  const bool pk_taken = ctl != nullptr && __builtin_amdgcn_readfirstlane(ctl[CTL_PK]) != 0u;
  if (pk_taken && __builtin_amdgcn_readfirstlane(ctl[CTL_OTHER]) == 0u) {
    MailOut<WaveDev> out(w, slots, ctr, head);
    out.post(MAIL_EXIT, 0u, 0u);
    return;
  }
  for (;;) {
    uint32_t b = 0;
    if (__lane_id() == 0) b = atomicAdd(q, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b < a.n && pk_taken && pk_block(uniform_i32(a.src_len[b]), uniform_i32(a.dst_cap[b]))) continue;
    MailOut<WaveDev> out(w, slots, ctr, head);
    out.tail_seen = tail_seen;
    if (b >= a.n) { out.post(MAIL_EXIT, 0u, 0u); return; }
    out.b = b;
    const int32_t n = uniform_i32(a.src_len[b]);
    const int32_t cap = uniform_i32(a.dst_cap[b]);
    if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0) {
      const uint8_t* s = uniform_ptr(a.src + a.src_off[b]);
      out.dense64 = routed ? dense64 : 0u;
      if (n < 65547) {
        FastV2<WaveDev, MailOut<WaveDev>> c(w, out, s, (uint32_t)n);
        (void)c.run();
      } else {
        FastV2<WaveDev, MailOut<WaveDev>, false> c(w, out, s, (uint32_t)n);   // byU32 blocks (64-bit entries: any size)
        (void)c.run();
      }
      if (out.bail) {
        out.post(MAIL_ABORT, 0u, 0u);
        if (__lane_id() == 0) routed[atomicAdd(q + 1, 1u)] = b;
      }
    } else {
      if (__lane_id() == 0) a.out[b] = 0;
    }
    head = out.head; tail_seen = out.tail_seen;
    WaveDev::sync();  // the table is reused
  }
}

// ---- byU32 blocks of at most 4 MiB (the largest block of the LZ4 Frame format, the default of the reference's
// LZ4FrameOutputStream): compact entries, 16 KB per table.  Measured on 8192 x 4 MiB (profiles/r04_compress_study.txt): throughput is
// linear in the chains a CU holds -- 3 / 5 / 6 / 8 chains: 74 / 115 / 134 / 177 GB/s -- and workgroups that SHARE a CU get 128 KB of its
// LDS between them, not 160 (2 x 80 KB, 3 x 48 KB and 5 x 32 KB all leave one workgroup waiting; a single workgroup does get 160 KB).
// So: ONE workgroup per CU with all 160 KB = TEN tables, and since ten pairs would be 1280 threads, ten finders share SIX writers
// (mail_ring.h mail_writer2_t: writer j takes the rings of finders j and j + 6; a writer is busy for a tenth of the time a finder
// needs to fill a batch).  LZ4HIP_PK_FINDERS / _WRITERS / _WGS: developer builds of other shapes (4 / 4 / 2 = eight chains in pairs).
#ifndef LZ4HIP_PK_FINDERS
#define LZ4HIP_PK_FINDERS 10
#endif
#ifndef LZ4HIP_PK_WRITERS
#define LZ4HIP_PK_WRITERS 6
#endif
#ifndef LZ4HIP_PK_WGS
#define LZ4HIP_PK_WGS 1
#endif
constexpr uint32_t PK_FINDERS = LZ4HIP_PK_FINDERS, PK_WRITERS = LZ4HIP_PK_WRITERS;
constexpr uint32_t PK_WGS_PER_CU = LZ4HIP_PK_WGS;
static_assert(PK_WRITERS <= PK_FINDERS && PK_FINDERS <= 2 * PK_WRITERS && 64 * (PK_FINDERS + PK_WRITERS) <= 1024, "shape of the packed kernel");
__global__ __launch_bounds__(64 * (PK_FINDERS + PK_WRITERS)) void compress_fast_v2wp_cu_kernel(BatchArgs a, uint32_t* ctl, uint32_t* mail_ctr, uint32_t* mail_slots) {
  __shared__ __attribute__((aligned(16))) uint32_t tables[PK_FINDERS][4096];
  if (__builtin_amdgcn_readfirstlane(ctl[CTL_PK]) == 0u) return;   // (every wavefront: no such block in this batch)
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t ring0 = blockIdx.x * PK_FINDERS;                   // this workgroup's rings: one per finder
  if (wv >= PK_FINDERS) {
    const uint32_t j = wv - PK_FINDERS, k = j + PK_WRITERS;
    WaveDev w(nullptr);
    mail_writer2_t<WaveDev, MailDev>(w, a, mail_slots + (size_t)(ring0 + j) * (MAIL_RING * MAIL_SLOT_WORDS), mail_ctr + 2u * (ring0 + j),
                                     k < PK_FINDERS ? mail_slots + (size_t)(ring0 + k) * (MAIL_RING * MAIL_SLOT_WORDS) : nullptr,
                                     k < PK_FINDERS ? mail_ctr + 2u * (ring0 + k) : nullptr);
    return;
  }
  uint32_t* ctr = mail_ctr + 2u * (ring0 + wv);
  uint32_t* slots = mail_slots + (size_t)(ring0 + wv) * (MAIL_RING * MAIL_SLOT_WORDS);
  __builtin_amdgcn_s_setprio(3);
  WaveDev w((uint64_t*)tables[wv]);
  uint32_t head = 0, tail_seen = 0;
  for (;;) {
    uint32_t b = 0;
    if (__lane_id() == 0) b = atomicAdd(ctl + CTL_DRAW_PK, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b < a.n && !pk_block(uniform_i32(a.src_len[b]), uniform_i32(a.dst_cap[b]))) continue;
    MailOut<WaveDev> out(w, slots, ctr, head);
    out.tail_seen = tail_seen;
    if (b >= a.n) { out.post(MAIL_EXIT, 0u, 0u); return; }
    out.b = b;
    const int32_t n = uniform_i32(a.src_len[b]);
    const uint8_t* s = uniform_ptr(a.src + a.src_off[b]);
    // No density probe here: with ten chains per CU this kernel beats the window-parallel core (five chains, 64-bit entries) on
    // blocks of short sequences as well -- 2560 x 4 MiB of English text 57 against 32 GB/s, synthetic blocks of 2..8 literals per
    // sequence 88-127 against 24-41 (profiles/r04_compress_study.txt) -- so these blocks are never routed.
    out.dense64 = 0u;
    {
      FastV2<WaveDev, MailOut<WaveDev>, false, true> c(w, out, s, (uint32_t)n);
      (void)c.run();
    }
    head = out.head; tail_seen = out.tail_seen;
    WaveDev::sync();  // the table is reused
  }
}
// scratch words the two-wave kernels need after the three queue words: the control words, the counters of every pair (ten per CU
// at most), then (1024-byte aligned) the rings
static std::atomic<int> g_compress_pack{1};   // "compress_pack": 0 = every block on the five-pair kernel (developer A/B); an atomic like the other knobs (round-4 advisor: a plain int read by concurrent launches was a data race)
void set_compress_pack(int v) { g_compress_pack.store(v, std::memory_order_relaxed); }
size_t compress_fast_v2w_scratch_words(uint32_t n_cus) {
  const size_t pairs = (size_t)n_cus * (PK_FINDERS * PK_WGS_PER_CU > WAVES_PER_CU ? PK_FINDERS * PK_WGS_PER_CU : WAVES_PER_CU);
  return CTL_WORDS + 2u * pairs + 256u + pairs * (MAIL_RING * MAIL_SLOT_WORDS);
}
int launch_compress_fast_v2w(const BatchArgs& a, uint32_t* q, uint32_t* routed, uint32_t dense64, uint32_t n_cus, uint32_t* mail, void* stream) {
  if (a.n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  bool pack = g_compress_pack.load(std::memory_order_relaxed) != 0;
  if (pack) {   // the packed kernel is ONE workgroup of 1024 threads with 160 KB of static LDS: a device that cannot run it gets the five-pair kernel for every block
    static std::atomic<int> fits[64];   // per device: 0 = not asked yet, 1 = fits, 2 = does not
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
    int f = fits[d].load(std::memory_order_relaxed);
    if (f == 0) {
      int lds = 0;
      f = (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, d) == hipSuccess && lds >= 160 * 1024) ? 1 : 2;
      fits[d].store(f, std::memory_order_relaxed);
    }
    if (f != 1) pack = false;
  }
  const size_t pairs_max = (size_t)n_cus * (PK_FINDERS * PK_WGS_PER_CU > WAVES_PER_CU ? PK_FINDERS * PK_WGS_PER_CU : WAVES_PER_CU);
  uint32_t* ctl = mail;
  uint32_t* ctr = mail + CTL_WORDS;
  uint32_t* slots = (uint32_t*)(((uintptr_t)(ctr + 2u * pairs_max) + 1023u) & ~(uintptr_t)1023u);
  hipError_t e = hipMemsetAsync(q, 0, 3 * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(mail, 0, (CTL_WORDS + 2u * pairs_max) * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  if (pack) {
    if (getenv("LZ4HIP_OCC_DEBUG")) {
      int nb = -1;
      hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, compress_fast_v2wp_cu_kernel, 64 * (PK_FINDERS + PK_WRITERS), 0);
      fprintf(stderr, "[lz4hip] compress_fast_v2wp_cu_kernel: %d workgroups per CU (%s)\n", nb, hipGetErrorString(oe));
    }
    hipLaunchKernelGGL(compress_classify_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, st, a.src_len, a.dst_cap, a.n, ctl);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;   // (each launch checked by itself: the five-pair kernel SKIPS the blocks ctl gives to the packed one)
    const uint32_t want = (a.n + PK_FINDERS - 1u) / PK_FINDERS, most = n_cus * PK_WGS_PER_CU;
    hipLaunchKernelGGL(compress_fast_v2wp_cu_kernel, dim3(want < most ? want : most), dim3(64 * (PK_FINDERS + PK_WRITERS)), 0, st, a, ctl, ctr, slots);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    e = hipMemsetAsync(ctr, 0, 2u * pairs_max * sizeof(uint32_t), st);   // the rings start empty again
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t wgs = (a.n + WAVES_PER_CU - 1u) / WAVES_PER_CU;
  hipLaunchKernelGGL(compress_fast_v2w_cu_kernel, dim3(wgs < n_cus ? wgs : n_cus), dim3(64 * 2 * WAVES_PER_CU), 0, st, a, q, routed, dense64, ctr, slots,
                     pack ? (const uint32_t*)ctl : (const uint32_t*)nullptr);
  return (int)hipGetLastError();
}

// The one-wavefront-per-block kernels (ms, accel, dict, dest; chain draws chains): WAVES_PER_CU wavefronts per workgroup, a 32 KB table
// each, units drawn from a queue word.  A kernel is its name, its arguments, the draw loop and the FastForm it names: the block shell
// is lz4_fast_core.h's fast_block_run, which the CPU lane simulator runs as well; BlockIoDev is the device's side of it (per-block
// values back in scalar registers, kernels_internal.h uniform_*; lane 0 stores the results) and launch_queue_kernel the launch.
// (The draw loop is written out in every kernel: behind a function that takes the body as a callable the cores are optimised once
// more on their way into the kernel, and three of four kernels come out with other instructions.)
struct BlockIoDev {
  const BatchArgs& a;
  int32_t* consumed = nullptr;   // FILL forms only
  __device__ __forceinline__ static int32_t i32(int32_t v) { return uniform_i32(v); }
  template <class T> __device__ __forceinline__ static T* ptr(T* p) { return uniform_ptr(p); }
  __device__ __forceinline__ void begin_block(WaveDev&, const uint8_t*, uint32_t, uint8_t*, uint32_t) const {}
  __device__ __forceinline__ void put(uint32_t b, uint32_t r) const { if (__lane_id() == 0) a.out[b] = (int32_t)r; }
  __device__ __forceinline__ void put(uint32_t b, uint32_t r, int32_t c) const { if (__lane_id() == 0) { a.out[b] = (int32_t)r; consumed[b] = c; } }
};
// q_words: the queue words at q to zero in front of the launch (0: an earlier launch of the same pass has)
template <class... P, class... A>
static int launch_queue_kernel(void (*kernel)(P...), uint32_t units, uint32_t* q, uint32_t q_words, uint32_t n_cus, void* stream, A... args) {
  if (q_words) {
    hipError_t e = hipMemsetAsync(q, 0, q_words * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t wgs = (units + WAVES_PER_CU - 1u) / WAVES_PER_CU;
  hipLaunchKernelGGL(kernel, dim3(wgs < n_cus ? wgs : n_cus), dim3(64 * WAVES_PER_CU), 0, (hipStream_t)stream, args...);
  return (int)hipGetLastError();
}

// window-parallel core (lz4_fast_ms_core.h): every sequence of a 64-position window per step.  Draws from q[2] either the blocks
// listed in routed[0 .. q[1]) (second pass of the adaptive scheme; an empty list costs one queue draw per wavefront) or, with
// routed == nullptr, every block of the batch
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_ms_cu_kernel(BatchArgs a, uint32_t* q, const uint32_t* routed) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  BlockIoDev io{a};
  const uint32_t count = routed ? __builtin_amdgcn_readfirstlane(q[1]) : a.n;
  for (;;) {
    uint32_t i = 0;
    if (__lane_id() == 0) i = atomicAdd(q + 2, 1u);
    i = __builtin_amdgcn_readfirstlane(i);
    if (i >= count) return;
    FastBlockArgs x;
    fast_block_run<FastFormMS<WaveDev>>(w, io, a, routed ? __builtin_amdgcn_readfirstlane(routed[i]) : i, x);
    WaveDev::sync();  // the table is reused
  }
}
// `first` = this is the first launch that uses q (zero it)
int launch_compress_fast_ms(const BatchArgs& a, uint32_t* q, const uint32_t* routed, bool first, uint32_t n_cus, void* stream) {
  if (a.n == 0) return 0;
  return launch_queue_kernel(compress_fast_ms_cu_kernel, a.n, q, first ? 3u : 0u, n_cus, stream, a, q, routed);
}

// LZ4_compress_fast with acceleration 2 .. 65537: the one-sequence-per-step core with its ACC switch on, blocks drawn from q[0]
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_accel_cu_kernel(BatchArgs a, uint32_t* q, uint32_t accel) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  BlockIoDev io{a};
  for (;;) {
    uint32_t b = 0;
    if (__lane_id() == 0) b = atomicAdd(q, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= a.n) return;
    FastBlockArgs x;
    x.accel = accel;
    fast_block_run<FastForm<WaveDev, false, true>>(w, io, a, b, x);
    WaveDev::sync();  // the table is reused
  }
}
int launch_compress_fast_accel(const BatchArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n == 0) return 0;
  if (accel < 2u || accel > 65537u) return (int)hipErrorInvalidValue;   // (the caller clamps; 1 is the plain compressor's)
  return launch_queue_kernel(compress_fast_accel_cu_kernel, a.n, q, 1u, n_cus, stream, a, q, accel);
}

// LZ4_loadDict + LZ4_compress_fast_continue, a fresh stream per block: the DICT switch -- byU32 and 64-bit entries at every size, as
// liblz4's external-dictionary mode.  Per block the table is loaded from the dictionary's 32 KB image (dict_image_kernel, once per handle
// and device; L2-resident while a batch runs) instead of being cleared; keep == 0 (no dictionary) clears it.
// (This kernel keeps a block shell of its own: through fast_block_run -- FastForm<WaveDev, false, false, true>, the form the lane
// simulator runs -- it computes the same but comes out with other instructions: values that depend on `keep` alone are hoisted out
// of the draw loop.  Any change to the shell in lz4_fast_core.h is to be made here as well.)
__device__ __forceinline__ void compress_fast_dict_block(const BatchArgs& a, uint32_t b, uint64_t* table, const uint8_t* tail, uint32_t keep,
                                                         const uint8_t* image) {
  const int32_t n = uniform_i32(a.src_len[b]);
  const int32_t cap = uniform_i32(a.dst_cap[b]);
  uint32_t r = 0;
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0) {
    const uint8_t* s = uniform_ptr(a.src + a.src_off[b]);
    uint8_t* d = uniform_ptr(a.dst + a.dst_off[b]);
    WaveDev w(table);
    DirectOut<WaveDev> out(w, s, (uint32_t)n, d, (uint32_t)cap);
    FastCore<WaveDev, false, DirectOut<WaveDev>, false, false, true> c(w, out, s, (uint32_t)n);
    if (keep) { c.dict = tail; c.keep = keep; c.image = image; }
    r = c.run();
  }
  if (__lane_id() == 0) a.out[b] = (int32_t)r;
}
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_dict_cu_kernel(BatchArgs a, const uint8_t* tail, uint32_t keep, const uint8_t* image,
                                                                                  uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  uint64_t* table = tables[threadIdx.x >> 6];
  for (;;) {
    uint32_t b = 0;
    if (__lane_id() == 0) b = atomicAdd(q, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= a.n) return;
    compress_fast_dict_block(a, b, table, tail, keep, image);
    WaveDev::sync();  // the table is reused
  }
}
int launch_compress_fast_dict(const BatchArgs& a, const uint8_t* dict_end, int32_t keep, const void* image, uint32_t* q, uint32_t n_cus,
                              void* stream) {
  if (a.n == 0) return 0;
  if (keep != 0 && (keep < 8 || keep > 65536 || !dict_end || !image)) return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_dict_cu_kernel, a.n, q, 1u, n_cus, stream, a, keep ? dict_end - keep : (const uint8_t*)nullptr,
                             (uint32_t)keep, (const uint8_t*)image, q);
}
// the dictionary's table image: one wavefront, once per handle and device
__global__ __launch_bounds__(64) void dict_image_kernel(const uint8_t* tail, uint32_t keep, uint8_t* image) {
  __shared__ __attribute__((aligned(16))) uint64_t table[LZ4HIP_TABLE_U64];
  WaveDev w(table);
  dict_image_build(w, tail, keep, image);
}
int launch_dict_image(const uint8_t* tail, int32_t keep, void* image, void* stream) {
  if (keep < 8 || keep > 65536 || !tail || !image) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dict_image_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tail, (uint32_t)keep, (uint8_t*)image);
  return (int)hipGetLastError();
}

// LZ4_compress_fast_continue over chains of linked blocks: the LINK switch and the walk of lz4_fast_chain.h, with a CHAIN as the unit of
// work: a wavefront draws a chain, builds the chain's table in its 32 KB of LDS -- cleared, or LZ4_loadDict's inserts over the kept prefix
// (dict_table_build, no image in memory) -- and walks the chain's blocks in order with the table left as the previous block left it.
// One chain is serial; nothing here waits for another wavefront.
struct CChainIoDev {
  const CChainArgs& a;
  __device__ __forceinline__ static uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
  // (the builtin returns int: each half goes through uint32_t, or a low half of 2^31 and more is sign-extended over the high one)
  __device__ __forceinline__ static uint64_t uni64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
  }
  template <class T> __device__ __forceinline__ static T* uni_ptr(T* p) { return uniform_ptr(p); }
  __device__ __forceinline__ void put_out(uint32_t i, int32_t r) const { if (__lane_id() == 0) a.out[i] = r; }
  __device__ __forceinline__ void put_chain(uint32_t c, uint64_t n) const { if (__lane_id() == 0) a.chain_consumed[c] = n; }
  __device__ __forceinline__ void begin_block(const uint8_t*, uint32_t, uint8_t*, uint32_t) const {}
};
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_chain_cu_kernel(CChainArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CChainIoDev io{a};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.n_chains) return;
    cchain_walk(w, io, a, c);
    WaveDev::sync();  // the table is reused: the next chain starts from its own
  }
}
int launch_compress_fast_chain(const CChainArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n_chains == 0) return 0;
  if (!q) return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_chain_cu_kernel, a.n_chains, q, 1u, n_cus, stream, a, q);
}

// LZ4_compress_fast_continue on streams whose state is resident on the device: the chain kernel's shape and lz4_fast_chain.h's
// cstream_walk.  A wavefront that draws chain c loads the stream's 32 KB table image from device memory into its LDS (or builds the
// fresh table), walks the call's blocks and stores table and record back.  The state was written by an earlier launch and is read
// through ordinary global loads; one wavefront owns a stream for the whole launch (the host hands every slot out once), so nothing
// inside a launch needs a fence.  The image moves 16 bytes per lane, 1 KB per instruction, both ways.
struct CStreamIoDev : CChainIoDev {
  __device__ __forceinline__ void begin_state(const uint8_t*) const {}
  __device__ __forceinline__ void end_state() const {}
  __device__ __forceinline__ static void table_load(WaveDev& w, const uint8_t* image) {
    const uint4* g = (const uint4*)image;
    uint4* t = (uint4*)w.lds;
    for (uint32_t i = __lane_id(); i < LZ4HIP_TABLE_U64 / 2u; i += 64u) t[i] = g[i];
    WaveDev::sync();
  }
  __device__ __forceinline__ static void table_store(WaveDev& w, uint8_t* image) {
    uint4* g = (uint4*)image;
    const uint4* t = (const uint4*)w.lds;
    for (uint32_t i = __lane_id(); i < LZ4HIP_TABLE_U64 / 2u; i += 64u) g[i] = t[i];
  }
  __device__ __forceinline__ static void put_rec(uint32_t* rec, uint32_t idx, uint32_t held, uint32_t flags, uint32_t span, uint64_t total) {
    if (__lane_id() == 0) { rec[0] = idx; rec[1] = held; rec[2] = flags; rec[3] = span; rec[4] = (uint32_t)total; rec[5] = (uint32_t)(total >> 32); }
  }
};
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_stream_cu_kernel(CStreamArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CStreamIoDev io{{a.c}};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.c.n_chains) return;
    cstream_walk(w, io, a, c);
    WaveDev::sync();  // the table is reused: the next stream loads or builds its own
  }
}
int launch_compress_fast_stream(const CStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.c.n_chains == 0) return 0;
  if (!q || !a.slot || !a.rec || !a.tables) return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_stream_cu_kernel, a.c.n_chains, q, 1u, n_cus, stream, a, q);
}

// The resident streams when their sources land anywhere: the same shape and state, lz4_fast_chain.h's cxstream_walk.  Per block the walk
// chooses between the LINK core (the source follows its history) and the LINK + DICT core (the history lies elsewhere) on offsets and
// lengths that are read through readfirstlane (io.uni / uni64): the choice and everything it depends on stay in scalar registers, and
// both cores work on the one table in LDS.
struct CXStreamIoDev : CStreamIoDev {
  __device__ __forceinline__ void begin_xblock(const uint8_t*, uint32_t, const uint8_t*, uint32_t, uint8_t*, uint32_t) const {}
};
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_xstream_cu_kernel(CXStreamArgs a, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CXStreamIoDev io{{{a.s.c}}};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.s.c.n_chains) return;
    cxstream_walk(w, io, a, c);
    WaveDev::sync();  // the table is reused: the next stream loads or builds its own
  }
}
int launch_compress_fast_xstream(const CXStreamArgs& a, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.s.c.n_chains == 0) return 0;
  if (!q || !a.s.slot || !a.s.rec || !a.s.tables || !a.src_off || !a.chain_hist_end || !a.s.c.chain_prefix_len) return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_xstream_cu_kernel, a.s.c.n_chains, q, 1u, n_cus, stream, a, q);
}

// The three kernels above with acceleration 2 .. 65537 (LZ4_compress_fast_continue's last argument, one value for the launch): the same
// shape, Io and walks with their ACC switch on.  Kernels of their own, so that the acceleration-1 kernels keep their instructions;
// same arguments, record and image, so that launches of all six alternate on a stream.
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_chain_accel_cu_kernel(CChainArgs a, uint32_t* q, uint32_t accel) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CChainIoDev io{a};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.n_chains) return;
    cchain_walk<true>(w, io, a, c, accel);
    WaveDev::sync();  // the table is reused: the next chain starts from its own
  }
}
int launch_compress_fast_chain_accel(const CChainArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n_chains == 0) return 0;
  if (!q || accel < 2u || accel > 65537u) return (int)hipErrorInvalidValue;   // (the caller clamps; 1 is launch_compress_fast_chain's)
  return launch_queue_kernel(compress_fast_chain_accel_cu_kernel, a.n_chains, q, 1u, n_cus, stream, a, q, accel);
}
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_stream_accel_cu_kernel(CStreamArgs a, uint32_t* q, uint32_t accel) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CStreamIoDev io{{a.c}};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.c.n_chains) return;
    cstream_walk<true>(w, io, a, c, accel);
    WaveDev::sync();  // the table is reused: the next stream loads or builds its own
  }
}
int launch_compress_fast_stream_accel(const CStreamArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.c.n_chains == 0) return 0;
  if (!q || !a.slot || !a.rec || !a.tables || accel < 2u || accel > 65537u) return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_stream_accel_cu_kernel, a.c.n_chains, q, 1u, n_cus, stream, a, q, accel);
}
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_xstream_accel_cu_kernel(CXStreamArgs a, uint32_t* q, uint32_t accel) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  CXStreamIoDev io{{{a.s.c}}};
  for (;;) {
    uint32_t c = 0;
    if (__lane_id() == 0) c = atomicAdd(q, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= a.s.c.n_chains) return;
    cxstream_walk<true>(w, io, a, c, accel);
    WaveDev::sync();  // the table is reused: the next stream loads or builds its own
  }
}
int launch_compress_fast_xstream_accel(const CXStreamArgs& a, uint32_t accel, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.s.c.n_chains == 0) return 0;
  if (!q || !a.s.slot || !a.s.rec || !a.s.tables || !a.src_off || !a.chain_hist_end || !a.s.c.chain_prefix_len || accel < 2u || accel > 65537u)
    return (int)hipErrorInvalidValue;
  return launch_queue_kernel(compress_fast_xstream_accel_cu_kernel, a.s.c.n_chains, q, 1u, n_cus, stream, a, q, accel);
}

// LZ4_compress_destSize: the one-sequence-per-step core (acceleration 1) with DirectOut's FILL switch on; dst_cap[b] is the target.  A
// block whose target is full stops at the next step, so the steps spent on it follow the input it consumes, not src_len.
__global__ __launch_bounds__(64 * WAVES_PER_CU) void compress_fast_dest_cu_kernel(BatchArgs a, int32_t* consumed, uint32_t* q) {
  __shared__ __attribute__((aligned(16))) uint64_t tables[WAVES_PER_CU][LZ4HIP_TABLE_U64];
  WaveDev w(tables[threadIdx.x >> 6]);
  BlockIoDev io{a, consumed};
  for (;;) {
    uint32_t b = 0;
    if (__lane_id() == 0) b = atomicAdd(q, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= a.n) return;
    FastBlockArgs x;
    fast_block_run<FastForm<WaveDev, true>>(w, io, a, b, x);
    WaveDev::sync();  // the table is reused
  }
}
int launch_compress_dest_size(const BatchArgs& a, int32_t* consumed, uint32_t* q, uint32_t n_cus, void* stream) {
  if (a.n == 0) return 0;
  return launch_queue_kernel(compress_fast_dest_cu_kernel, a.n, q, 1u, n_cus, stream, a, consumed, q);
}

#if LZ4HIP_V2_ASM_PROF
// developer builds: reads (and clears) the phase counters of the hand-scheduled lean step
extern "C" __attribute__((visibility("default"))) int lz4hip_dev_asm_prof(unsigned long long* out16) {
  hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_asm_prof), 16 * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  unsigned long long z[16] = {0};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_asm_prof), z, sizeof(z));
}
#endif

#if LZ4HIP_ASM_DBG & 4
extern "C" __attribute__((visibility("default"))) int lz4hip_dev_asm_dbg(unsigned int* out1600) {
  return (int)hipMemcpyFromSymbol(out1600, HIP_SYMBOL(g_asm_dbg), 1600 * sizeof(unsigned int));
}
#endif

#ifdef LZ4HIP_DEV_TOOLS
// developer diagnostics: same algorithm with per-phase shader-clock accumulation; prof[b*12 + i] =
// {steps, slow_steps, false_pos, sequences, t[0..7]} of block b
template <int MS>   // 0 = lz4_fast_core.h, 1 = lz4_fast_ms_core.h, 3 = lz4_fast_v2_core.h
__global__ __launch_bounds__(64) void compress_fast_prof_kernel(BatchArgs a, uint64_t* prof) {
  __shared__ __attribute__((aligned(16))) uint64_t table[4096];
  const uint32_t b = blockIdx.x;
  const int32_t n = a.src_len[b];
  const int32_t cap = a.dst_cap[b];
  uint32_t r = 0;
  FastStats st = {};
  if (n >= 0 && (uint32_t)n <= 0x7E000000u && cap >= 0) {
    const uint8_t* s = a.src + a.src_off[b];
    uint8_t* d = a.dst + a.dst_off[b];
    WaveDev w(table);
    DirectOut<WaveDev> out(w, s, (uint32_t)n, d, (uint32_t)cap);
    if constexpr (MS == 3) {
      ParkOutRaw<WaveDev> po(w, s, (uint32_t)n, d, (uint32_t)cap);   // (the finder of the default kernel parks raw hits; here one wave also writes them)
      if (n < 65547) { FastV2<WaveDev, ParkOutRaw<WaveDev>> c(w, po, s, (uint32_t)n, &st); r = c.run(); }
      else { FastV2<WaveDev, ParkOutRaw<WaveDev>, false> c(w, po, s, (uint32_t)n, &st); r = c.run(); }
    } else if constexpr (MS == 1) {
      if (n < 65547) { FastCoreMS<WaveDev, true> c(w, out, s, (uint32_t)n, &st); r = c.run(); }
      else { FastCoreMS<WaveDev, false> c(w, out, s, (uint32_t)n, &st); r = c.run(); }
    } else {
      if (n < 65547) { FastCore<WaveDev, true> c(w, out, s, (uint32_t)n, &st); r = c.run(); }
      else { FastCore<WaveDev, false> c(w, out, s, (uint32_t)n, &st); r = c.run(); }
    }
  }
  if (threadIdx.x == 0) {
    a.out[b] = (int32_t)r;
    uint64_t* p = prof + (uint64_t)b * 12u;
    p[0] = st.steps; p[1] = st.slow_steps; p[2] = st.false_pos; p[3] = st.sequences;
    for (int i = 0; i < 8; i++) p[4 + i] = st.t[i];
  }
}
int launch_compress_fast_prof(const BatchArgs& a, uint64_t* prof, int core, void* stream) {
  if (a.n == 0) return 0;
  if (core == 3) hipLaunchKernelGGL(compress_fast_prof_kernel<3>, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, prof);
  else if (core >= 1) hipLaunchKernelGGL(compress_fast_prof_kernel<1>, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, prof);
  else hipLaunchKernelGGL(compress_fast_prof_kernel<0>, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, prof);
  return (int)hipGetLastError();
}
#endif  // LZ4HIP_DEV_TOOLS

}  // namespace lz4hip
