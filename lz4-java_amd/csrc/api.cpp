// api.cpp -- the C ABI of liblz4hip.so (include/lz4hip.h): device context, staging for the
// host-pointer batch API, contiguous-range sharding over the initialised devices, and the
// device-pointer entry points bench.py times.  There is deliberately NO CPU code path here:
// without a HIP device every compute entry point returns LZ4HIP_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <limits.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <algorithm>
#include <vector>
#include <string>
#include "../../include/lz4hip.h"
#include "kernels.h"
#include "host_staging.h"
#include "container_rules.h"
#include "container_write_rules.h"

namespace {

using staging::al16;
using staging::pos;
thread_local std::string g_err;
std::mutex g_mu;
std::vector<int> g_devs;  // HIP device ordinals the engine is initialised on
bool g_inited = false;

int fail(int status, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof buf, "%s", what);
  g_err = buf;
  return status;
}

const char* const kNullArg = "null pointer argument";

#define HIPCHK(call)                                                   \
  do {                                                                 \
    hipError_t e_ = (call);                                            \
    if (e_ != hipSuccess) return fail(LZ4HIP_E_HIP, #call, e_);        \
  } while (0)

int ensure_init() {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_inited) return g_devs.empty() ? LZ4HIP_E_NO_DEVICE : LZ4HIP_OK;
  }
  return lz4hip_init(nullptr, 0);
}

// what every compute entry point asks first: the engine is up on a device, or the status of having none (message set)
int need_device() { const int rc = ensure_init(); return rc ? fail(rc, "no HIP device: liblz4hip has no CPU fallback") : LZ4HIP_OK; }

// the HIP ordinal of engine device index `device`
int ordinal(int device, int* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (device < 0 || device >= (int)g_devs.size()) return LZ4HIP_E_ARG;
  *out = g_devs[device];
  return LZ4HIP_OK;
}

struct DeviceGuard {  // callers (e.g. PyTorch) own the thread's current device: restore it
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int ord) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (prev == ord) || hipSetDevice(ord) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// OP_COMPRESS_ACCEL: LZ4_compress_fast with acceleration 2 .. 65537 (acceleration 1 is OP_COMPRESS_FAST)
// OP_COMPRESS_DEST: LZ4_compress_destSize, dst_cap = the target size; a second per-block output array carries the consumed sizes
// OP_DECODE_PARTIAL: LZ4_decompress_safe_partial; on the host path dst_cap already holds min(target, capacity), or -1 where one of
// them is negative (partial_room), and the kernels get that array as the target too
// OP_COMPRESS_HC_DEST: LZ4_compress_HC_destSize: OP_COMPRESS_HC's level and workspace, OP_COMPRESS_DEST's target and consumed sizes
// OP_DECODED_SIZE: the value LZ4_decompress_safe would return for (src, src_len, dst_cap), and no output buffer at all
// OP_DECODE_DICT: LZ4_decompress_safe_usingDict against one dictionary per call: a handle (BlockCall::dict, resident on the device the
// launch runs on) or the caller's device memory (BlockCall::dict_dev / dict_len)
// OP_COMPRESS_DICT: LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream per block, against a handle (BlockCall::dict) -- always
// a handle: the compressor needs the dictionary's table image (dict_compress_state), not only its bytes
// OP_COMPRESS_HC_DICT: LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream per block, against a handle (BlockCall::dict):
// OP_COMPRESS_HC's level and workspace, and the handle's HC image (dict_hc_state)
// OP_DECOMPRESS_CHAIN: LZ4_decompress_safe_continue over chains of linked blocks: its arrays (per block AND per chain) are
// BlockCall::chain, the seven arrays of the other operations are not used; the host path is chain_host_shard, not host_shard
// OP_COMPRESS_CHAIN: LZ4_compress_fast_continue over chains of linked blocks: its arrays are BlockCall::cchain; the host path is
// cchain_host_shard, which brings back only the bytes produced, as every compressor's does
// OP_COMPRESS_HC_CHAIN: LZ4_compress_HC_continue over chains of linked blocks (prefix mode): OP_COMPRESS_CHAIN's arrays and host path
// (no chain_consumed: a block that returns 0 does not stop its chain), OP_COMPRESS_HC's level and workspace
// OP_COMPRESS_STREAM: LZ4_compress_fast_continue on streams whose state is resident on the device (lz4hip_cstreams): OP_COMPRESS_CHAIN's
// arrays and host path, plus the slot of every chain's stream and the device's share of the set's state (BlockCall::cs_*, StreamShare)
// OP_DECOMPRESS_STREAM: LZ4_decompress_safe_continue on streams whose blocks land anywhere (every mode of LZ4_streamDecode_t): its
// arrays and state records are BlockCall::dstream; the host path is dstream_host_shard
// OP_DECOMPRESS_STREAM_INORDER: the same streams where a block's slot may overlap the history the block can reach (minimal rings): OP_DECOMPRESS_STREAM's
// arrays, records and host path; BlockCall::param is the "dstream_inorder" knob (1: every block in order, 0: the overlapping ones)
// OP_COMPRESS_XSTREAM: the same resident streams when their sources land anywhere (liblz4's external-dictionary mode included): its
// arrays are BlockCall::cxstream, which carries the device's share of the set's state; the host path is cxstream_host_shard
// OP_COMPRESS_HC_STREAM: LZ4_compress_HC_continue on streams whose sources land anywhere, both of its modes: its arrays are
// BlockCall::hcstream, the linear image the host has made of the call (host_staging.h HcsImage); the host path is hcstream_host_shard
enum Op { OP_COMPRESS_FAST, OP_DECODE_SAFE, OP_DECODE_FAST, OP_COMPRESS_HC, OP_COMPRESS_ACCEL, OP_COMPRESS_DEST, OP_DECODE_PARTIAL, OP_COMPRESS_HC_DEST,
          OP_DECODED_SIZE, OP_DECODE_DICT, OP_COMPRESS_DICT, OP_COMPRESS_HC_DICT, OP_DECOMPRESS_CHAIN, OP_COMPRESS_CHAIN, OP_COMPRESS_HC_CHAIN, OP_COMPRESS_STREAM,
          OP_DECOMPRESS_STREAM, OP_COMPRESS_XSTREAM, OP_COMPRESS_HC_STREAM, OP_DECOMPRESS_STREAM_INORDER };
constexpr int OP_COUNT = OP_DECOMPRESS_STREAM_INORDER + 1;   // (the last enumerator)
// What an operation is, said once; everything below asks these and launch_block, nothing else compares ops.
// a compressor: on the host path only the bytes it produced come back, packed on the device (launch_pack)
constexpr bool op_compresses(Op op) { return op == OP_COMPRESS_FAST || op == OP_COMPRESS_HC || op == OP_COMPRESS_ACCEL || op == OP_COMPRESS_DEST || op == OP_COMPRESS_HC_DEST || op == OP_COMPRESS_DICT || op == OP_COMPRESS_HC_DICT || op == OP_COMPRESS_CHAIN || op == OP_COMPRESS_HC_CHAIN || op == OP_COMPRESS_STREAM || op == OP_COMPRESS_XSTREAM || op == OP_COMPRESS_HC_STREAM; }
// a second per-block result (BlockCall::consumed) travels behind out[]
constexpr bool op_has_consumed(Op op) { return op == OP_COMPRESS_DEST || op == OP_COMPRESS_HC_DEST; }
// out[i] counts SOURCE bytes read: a block that succeeded filled its whole dst_cap[i]
constexpr bool op_fills_capacity(Op op) { return op == OP_DECODE_FAST; }
// writes no output buffer: dst and dst_off may be NULL, nothing is allocated, staged or copied back for them (dst_cap is an input)
constexpr bool op_writes_no_output(Op op) { return op == OP_DECODED_SIZE; }
// needs the chain-delta workspace (BlockCall::hc_ws / hc_span)
constexpr bool op_uses_hc_ws(Op op) { return op == OP_COMPRESS_HC || op == OP_COMPRESS_HC_DEST || op == OP_COMPRESS_HC_DICT || op == OP_COMPRESS_HC_CHAIN || op == OP_COMPRESS_HC_STREAM; }
// its arrays are BlockCall::cchain (chains of linked blocks), its host path cchain_host_shard
constexpr bool op_takes_cchain(Op op) { return op == OP_COMPRESS_CHAIN || op == OP_COMPRESS_HC_CHAIN || op == OP_COMPRESS_STREAM; }
// a block that returns 0 ends its chain (and chain_consumed[] says how far the chain came)
constexpr bool op_chain_stops(Op op) { return op == OP_COMPRESS_CHAIN || op == OP_COMPRESS_STREAM; }
// its chains continue resident streams: no 8-byte minimum on the history kept (the device knows what a stream holds), a slot per chain
constexpr bool op_resumes_streams(Op op) { return op == OP_COMPRESS_STREAM; }
// its layout kernel needs scratch beside the workspace (BlockCall::hc_scratch)
constexpr bool op_needs_chain_scratch(Op op) { return op == OP_COMPRESS_HC_CHAIN; }

// One block operation, from its entry point to launch_block.
struct BlockCall {
  Op op;
  int param = 0;                    // op_uses_hc_ws: the level (hc_level); OP_COMPRESS_ACCEL: the acceleration (accel_clamp, >= 2);
                                    // OP_COMPRESS_CHAIN, _STREAM, _XSTREAM: the acceleration (accel_clamp; 0 and 1: the acceleration-1 kernels)
                                    // OP_DECOMPRESS_STREAM_INORDER: 1 = every block in order
  const int32_t* target = nullptr;  // OP_DECODE_PARTIAL: per-block target sizes; nullptr: dst_cap already is partial_room (host path)
  int32_t* consumed = nullptr;      // op_has_consumed: the input consumed per block
  void* hc_ws = nullptr;            // op_uses_hc_ws: device workspace for hc_span bytes of source; nullptr: launch_block learns the
  uint64_t hc_span = 0;             // span and allocates one (hc_workspace)
  const lz4hip_dict* dict = nullptr;    // OP_COMPRESS_DICT, OP_COMPRESS_HC_DICT: the dictionary handle; OP_DECODE_DICT: the handle (host path, single calls) ...
  const uint8_t* dict_dev = nullptr;    // ... or, without a handle, the caller's dictionary in device memory and
  int32_t dict_len = 0;                 // its length
  const lz4hip::ChainArgs* chain = nullptr;   // OP_DECOMPRESS_CHAIN: the call's arrays on the device
  const lz4hip::CChainArgs* cchain = nullptr; // op_takes_cchain: the call's arrays on the device
  const lz4hip::DStreamArgs* dstream = nullptr;   // OP_DECOMPRESS_STREAM, _INORDER: the call's arrays and state records on the device
  const lz4hip::CXStreamArgs* cxstream = nullptr; // OP_COMPRESS_XSTREAM: the call's arrays on the device, the slots and the set's state
  const lz4hip::HcStreamArgs* hcstream = nullptr; // OP_COMPRESS_HC_STREAM: the call's linear image and its arrays on the device
  void* hc_scratch = nullptr;           // op_needs_chain_scratch: lz4hip::hc_chain_scratch_bytes of device memory
  // op_resumes_streams: the device's share of the set's state (kernels.h CStreamArgs) and, on the device, the slot of every chain
  uint32_t* cs_rec = nullptr; uint64_t* cs_tables = nullptr; const uint32_t* cs_slot = nullptr;
};
// What the host path knows of a stream set beside that, for one device's share of one call (cstreams_call makes it, the shards of
// op_resumes_streams and OP_COMPRESS_XSTREAM read it): the caller's stream ids, one per chain of the call; the id of the share's slot 0;
// the set's marks of streams to stop, by id (may be nullptr); *launched is set once a kernel of the shard is about to be enqueued
struct StreamShare {
  const uint32_t* ids = nullptr; uint32_t id0 = 0; const uint8_t* poisoned = nullptr; bool* launched = nullptr;
};
static_assert(staging::kSlotForceStop == lz4hip::kStreamForceStop, "the staging arithmetic's stop mark is the kernels'");
static_assert(lz4hip::kChainStopped == LZ4HIP_CHAIN_STOPPED, "the kernels' marker is the header's");
// the handle's bytes on the CURRENT device (uploaded on first use where lz4hip_dict_create found the device not yet initialised):
// one past the last byte, and the true length; a status (message set) on failure
int dict_resident(const lz4hip_dict* d, const uint8_t** dict_end, int32_t* dict_len);
// what the dictionary compressor needs of the handle on the CURRENT device: the end of the kept tail, its length as LZ4_loadDict keeps
// it (lz4hip::dict_keep: 0 = no dictionary) and the table image, built at the handle's first compress on the device (that one call
// waits for `st` once, so that calls on other streams find the image complete)
int dict_compress_state(const lz4hip_dict* d, hipStream_t st, const uint8_t** dict_end, int32_t* keep, const void** image);
// the same for the HC dictionary compressor: the kept tail as LZ4_loadDictHC keeps it (lz4hip::hc_dict_keep: no minimum) and the HC
// image (lz4hip::hc_dict_image_bytes), built at the handle's first HC compress on the device (that one call waits for `st` once)
int dict_hc_state(const lz4hip_dict* d, hipStream_t st, const uint8_t** dict_end, uint32_t* keep, const void** image);
// tuning knobs (lz4hip_set_option): atomics, so that a caller changing one while other threads launch is a race on the VALUE chosen,
// never undefined behaviour; every launch reads each knob once
std::atomic<int> g_decode_lanes{0};   // "decode_lanes"; 0 = kernel default
std::atomic<int> g_decode_stage{-1};  // "decode_stage": 1 = LDS output staging in the plain loop
std::atomic<int> g_decode_pipe{-1};   // "decode_pipe": 3 = ring loop, 2 = deep loop, 1/0 = pipelined interior loop on/off, -1 = kernel default
std::atomic<int> g_decode_ring{0};    // "decode_ring": bytes of the ring loop's output ring (0 = default for the lane count)
std::atomic<int> g_dstream_inorder{0};   // "dstream_inorder": lz4hip_decompress_safe_stream_inorder_batch decodes 1 = every block in order, 0 = those whose slot overlaps their history

// lz4hip_set_option "compress_core": 5 = adaptive two-pass (default): the lean core with a writer wavefront per chain finishes
// the blocks of long sequences, the window-parallel core the others; 3 = lean core only; 1 = window-parallel core only (the
// forced modes exist so that the suite can put every input through each kernel).  "compress_switch" = bytes per sequence below
// which a block counts as dense and goes to the window-parallel core (probe: sequences 32..95 of the block)
std::atomic<int> g_compress_core{5};
// lz4hip_set_option "hc_chain_segment": positions per build item of the HC chain compressor (launch_compress_hc_chain); every value
// gives the same bytes
std::atomic<int> g_hc_chain_segment{1 << 20};
std::atomic<int> g_compress_switch{16};   // (tools/switch_probe.py: 20 sent word-like data of 9 bytes per sequence to the slower core; 12 loses text)

// liblz4's level handling: < 1 -> 9, > 12 -> 12; 10..12 are the optimal parser (lz4-java levels 10..17)
int hc_level(int level, int* out) {
  if (level < 1) level = 9;
  if (level > 12) level = 12;
  *out = level;
  return LZ4HIP_OK;
}

// HC on device pointers without a workspace from the caller.  The chain-delta workspace is indexed by source offset, so its size
// depends on the batch's source span (max of src_off + src_len), which lives in device memory: it is learnt with ONE synchronisation
// of the caller's stream (stated in lz4hip.h); lz4hip_compress_hc_batch_dev_ws takes span and workspace from the caller and never
// synchronises.  Returns a status (message set); *ws is the caller's to hipFreeAsync on `st`.
int hc_workspace(const lz4hip::BatchArgs& a, int level, hipStream_t st, void** ws, uint64_t* span_out) {
  uint64_t* d_span = nullptr;
  uint64_t span = 0;
  HIPCHK(hipMallocAsync((void**)&d_span, 8, st));
  hipError_t he = hipMemsetAsync(d_span, 0, 8, st);
  int e = 0;
  if (he == hipSuccess) e = lz4hip::launch_hc_span(a.src_off, a.src_len, a.n, d_span, st);
  if (he == hipSuccess && e == 0) he = hipMemcpyAsync(&span, d_span, 8, hipMemcpyDeviceToHost, st);
  if (he == hipSuccess && e == 0) he = hipStreamSynchronize(st);
  (void)hipFreeAsync(d_span, st);   // (on every path: round 1 leaked it when a call above failed)
  if (e) return fail(LZ4HIP_E_HIP, "kernel launch", (hipError_t)e);
  if (he != hipSuccess) return fail(LZ4HIP_E_HIP, "HC span query", he);
  if (hipMallocAsync(ws, lz4hip::hc_ws_bytes(span, a.n, level), st) != hipSuccess) return fail(LZ4HIP_E_NOMEM, "HC workspace allocation failed");
  *span_out = span;
  return LZ4HIP_OK;
}

// The scratch a device entry point takes for itself -- queue words, the routed-block list, the mail rings -- comes from buffers that live
// as long as the engine, not from the stream-ordered allocator.  (It was hipMallocAsync + hipFreeAsync around every launch.  Measured
// on the MI355X, tests/test_gpu_user_streams.py: with work pending on the stream, the SECOND such call blocked the host in
// hipMallocAsync until the stream had drained -- the first call's hipFreeAsync'd block was the pool's only one, and the runtime waited
// for it instead of handing it out in stream order -- so two compress calls in a row did not "return without synchronising".  DESIGN.md
// 2.3 has the other incident with such an allocation.)  A buffer is handed to a launch on the stream that used it last -- the
// stream's own order is enough -- or once the event recorded behind its last user's kernels is complete; otherwise a new one is made.
// In the steady state that is no allocation and no wait: one buffer per stream that has launches in flight at the same time.
struct ScratchBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;      // behind the last kernel that used the buffer
  hipStream_t last = nullptr;   // the stream ev was recorded on
  bool held = false;            // between scratch_acquire and scratch_release of a host thread
};
struct ScratchPool {
  std::mutex mu;
  std::vector<ScratchBuf*> bufs;
};
ScratchPool g_scratch[64];
ScratchBuf* scratch_acquire(size_t bytes, hipStream_t st) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
  ScratchPool& P = g_scratch[d];
  std::lock_guard<std::mutex> lk(P.mu);
  ScratchBuf* pick = nullptr;
  for (ScratchBuf* b : P.bufs)
    if (!b->held && b->bytes >= bytes && b->last == st) { pick = b; break; }
  if (!pick)
    for (ScratchBuf* b : P.bufs)
      if (!b->held && b->bytes >= bytes && hipEventQuery(b->ev) == hipSuccess) { pick = b; break; }
  if (!pick) {
    size_t cap = 64u << 10;
    while (cap < bytes) cap <<= 1;
    ScratchBuf* b = new (std::nothrow) ScratchBuf();
    if (!b) return nullptr;
    if (hipMalloc(&b->p, cap) != hipSuccess) { delete b; return nullptr; }
    if (hipEventCreateWithFlags(&b->ev, hipEventDisableTiming) != hipSuccess) { (void)hipFree(b->p); delete b; return nullptr; }
    b->bytes = cap;
    try { P.bufs.push_back(b); } catch (...) { (void)hipEventDestroy(b->ev); (void)hipFree(b->p); delete b; return nullptr; }
    pick = b;
  }
  pick->held = true;
  return pick;
}
void scratch_release(ScratchBuf* b, hipStream_t st) {   // behind the launch's last kernel (also of a launch that failed half way)
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
  std::lock_guard<std::mutex> lk(g_scratch[d].mu);
  // (without its event nothing says when the buffer is free: it is not handed out again, and goes with the others at shutdown)
  if (hipEventRecord(b->ev, st) != hipSuccess) b->bytes = 0;
  b->last = st;
  b->held = false;
}
void scratch_free_all(int d) {   // lz4hip_shutdown (the device is current)
  if (d < 0 || d >= 64) return;
  std::lock_guard<std::mutex> lk(g_scratch[d].mu);
  for (ScratchBuf* b : g_scratch[d].bufs) {
    (void)hipFree(b->p);
    (void)hipEventDestroy(b->ev);
    delete b;
  }
  g_scratch[d].bufs.clear();
}

// fast compress: the cores of kernels.h, selected by "compress_core"
int launch_fast(const lz4hip::BatchArgs& a, hipStream_t st) {
  // scratch: three queue words + the routed-block list of the adaptive scheme
  const uint32_t cus = lz4hip::device_cus();
  const int core = g_compress_core.load(std::memory_order_relaxed);
  const size_t mail_words = core != 1 ? lz4hip::compress_fast_v2w_scratch_words(cus) : 0u;   // rings of the finder/writer pairs
  ScratchBuf* sb = scratch_acquire((3 + (size_t)a.n + mail_words) * sizeof(uint32_t), st);
  if (!sb) return (int)hipErrorOutOfMemory;
  uint32_t* scratch = (uint32_t*)sb->p;
  const uint32_t dense64 = 64u * (uint32_t)g_compress_switch.load(std::memory_order_relaxed);
  int le;
  if (core == 1) {
    le = lz4hip::launch_compress_fast_ms(a, scratch, nullptr, true, cus, st);
  } else if (core == 3) {
    le = lz4hip::launch_compress_fast_v2w(a, scratch, nullptr, 0u, cus, scratch + 3 + a.n, st);
  } else {   // 5: adaptive
    le = lz4hip::launch_compress_fast_v2w(a, scratch, scratch + 3, dense64, cus, scratch + 3 + a.n, st);
    if (le == 0) le = lz4hip::launch_compress_fast_ms(a, scratch, scratch + 3, false, cus, st);
  }
  scratch_release(sb, st);
  return le;
}

// liblz4's acceleration handling (LZ4_compress_fast_extState): < 1 -> 1, > LZ4_ACCELERATION_MAX -> 65537
int accel_clamp(int a) { return a < 1 ? 1 : a > 65537 ? 65537 : a; }

// the decode knobs are process-wide and set one at a time: a combination no kernel exists for is said here, by name (round-5 advisor: it
// used to surface as a bare "kernel launch: invalid value")
const char* decode_knobs_error(int lanes, int pipe, int ring) {
  const bool wave_ring = ring == 0 || ring == 8192 || ring == 16384 || ring == 32768 || ring == 65536;
  if (pipe == 4 || pipe == 5) return wave_ring ? nullptr : "decode_pipe 4 / 5 (the wave loops) take decode_ring 0, 8192, 16384, 32768 or 65536";
  if (pipe == 7) return (wave_ring && ring != 8192) ? nullptr : "decode_pipe 7 (the pair loop) takes decode_ring 0, 16384, 32768 or 65536";
  if (pipe == 8) return wave_ring ? nullptr : "decode_pipe 8 (the trio loop) takes decode_ring 0, 8192, 16384, 32768 or 65536";
  if (pipe == 3) {
    const int gl = lanes == 0 ? 4 : lanes;
    const int kw = ring ? ring : (gl == 1 ? 256 : gl == 4 ? 512 : 4096);
    const bool ok = (gl == 1 && (kw == 256 || kw == 512)) || (gl == 4 && (kw == 512 || kw == 1024 || kw == 2048)) ||
                    (gl == 8 && (kw == 512 || kw == 1024 || kw == 2048 || kw == 4096)) || (gl == 16 && (kw == 2048 || kw == 4096));
    return ok ? nullptr : "decode_pipe 3 (the ring loop) takes decode_lanes 1 (decode_ring 256 / 512), 4 (512 .. 2048), 8 (512 .. 4096) or 16 (2048 / 4096)";
  }
  if (lanes == 1) return "decode_lanes 1 exists for decode_pipe 3 (the ring loop) only";
  return nullptr;
}

// The device-side route's word: one of kRouteWords words of a per-device buffer, handed out round robin to the routed launches of ALL
// streams of the device.  (It was a stream-ordered allocation per launch: hipMallocAsync + hipFreeAsync in front of and behind EVERY
// routed launch -- tens of microseconds on the headline's 6 ms decode, measured with the route's kernels in
// profiles/r06l_bench_kernel_trace.txt.)  A word is meaningful from a launch's route kernel to the end of its LAST candidate kernel:
// every workgroup of every candidate reads it when it starts, and the later workgroups of a launch of more than 64 blocks per CU start
// while the earlier ones run.  So a slot's next use is ordered behind its previous user's last candidate kernel, on whatever stream
// either ran: each slot has an event (no timing) recorded behind the candidates, and a launch that finds its slot last used on ANOTHER
// stream makes its own stream wait for that event in front of its route kernel (on the same stream the order is the stream's; the
// pattern is xxh_stream_launch's).  No host synchronisation, no allocation per launch.  The lock is held from the slot's choice to the
// record of its event: two host threads that meet in one slot launch one behind the other.  "decode_route_slots" = how many of the
// slots are handed out (1: every routed launch reuses the one before it -- what the suite runs to exercise the wait).
constexpr uint32_t kRouteWords = 256u;
std::atomic<int> g_route_slots{(int)kRouteWords};   // "decode_route_slots"
struct RouteRing {
  uint32_t* words = nullptr;
  uint32_t next = 0;
  hipEvent_t ev[kRouteWords] = {};      // created at the slot's first use
  hipStream_t last[kRouteWords] = {};   // the stream ev was last recorded on
  bool used[kRouteWords] = {};
  std::mutex mu;
};
RouteRing g_route[64];
void route_release(int d) {   // lz4hip_shutdown (the device is current)
  if (d < 0 || d >= 64) return;
  RouteRing& r = g_route[d];
  std::lock_guard<std::mutex> lk(r.mu);
  if (r.words) { (void)hipFree(r.words); r.words = nullptr; }
  for (uint32_t i = 0; i < kRouteWords; i++) {
    if (r.ev[i]) { (void)hipEventDestroy(r.ev[i]); r.ev[i] = nullptr; }
    r.used[i] = false;
    r.last[i] = nullptr;
  }
  r.next = 0;
}

int launch_decode(const lz4hip::BatchArgs& a, bool safe, hipStream_t st) {
  const int lanes = g_decode_lanes.load(), pipe = g_decode_pipe.load(), stage = g_decode_stage.load(), ring = g_decode_ring.load();
  if (const char* why = decode_knobs_error(lanes, pipe, ring)) return fail(LZ4HIP_E_ARG, why);
  // (no route word: no device-side route, the lane-group default of the batch size -- launch_decompress routes under the same condition)
  if (!(a.n > 16u * lz4hip::device_cus() && lanes == 0 && pipe < 0 && stage < 0)) return lz4hip::launch_decompress(a, safe, lanes, pipe, stage, ring, st, nullptr);
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return lz4hip::launch_decompress(a, safe, lanes, pipe, stage, ring, st, nullptr);
  RouteRing& r = g_route[d];
  std::lock_guard<std::mutex> lk(r.mu);
  if (!r.words && hipMalloc((void**)&r.words, kRouteWords * sizeof(uint32_t)) != hipSuccess) {
    r.words = nullptr;
    return lz4hip::launch_decompress(a, safe, lanes, pipe, stage, ring, st, nullptr);
  }
  const uint32_t slots = (uint32_t)g_route_slots.load(std::memory_order_relaxed);
  const uint32_t k = r.next % slots;
  r.next = (k + 1u) % slots;
  if (!r.ev[k]) HIPCHK(hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming));
  if (r.used[k] && r.last[k] != st) HIPCHK(hipStreamWaitEvent(st, r.ev[k], 0));   // behind the slot's previous user's last candidate
  const int e = lz4hip::launch_decompress(a, safe, lanes, pipe, stage, ring, st, r.words + k);
  // (also after a failed launch: whatever part of it was enqueued reads the word)
  const hipError_t re = hipEventRecord(r.ev[k], st);
  r.used[k] = true;
  r.last[k] = st;
  if (e == 0 && re != hipSuccess) return fail(LZ4HIP_E_HIP, "hipEventRecord", re);
  return e;
}

// a queue word of scratch around a launcher: launch(q) -> the launcher's hipError_t, which is passed on
template <class Launch>
int with_queue_word(hipStream_t st, Launch launch) {
  ScratchBuf* sb = scratch_acquire(sizeof(uint32_t), st);
  if (!sb) return (int)hipErrorOutOfMemory;
  const int e = launch((uint32_t*)sb->p);
  scratch_release(sb, st);
  return e;
}

// The one place where a block operation reaches its kernels, on device arrays: the device-pointer entry points (dev_batch) and the
// host-pointer path (host_shard) both come here.  Returns 0, a launcher's hipError_t (> 0), or a status (< 0) whose message is set.
int launch_block(const BlockCall& c, const lz4hip::BatchArgs& a, hipStream_t st) {
  switch (c.op) {
    case OP_COMPRESS_FAST: return launch_fast(a, st);
    case OP_DECODE_SAFE: return launch_decode(a, true, st);
    case OP_DECODE_FAST: return launch_decode(a, false, st);
    case OP_DECODE_PARTIAL: return lz4hip::launch_decompress_partial(a, c.target ? c.target : a.dst_cap, st);
    case OP_DECODED_SIZE: return lz4hip::launch_decoded_size(a, st);
    case OP_DECODE_DICT: {
      const uint8_t* dict_end = c.dict_len > 0 ? c.dict_dev + c.dict_len : nullptr;
      int32_t dict_len = c.dict_len;
      if (c.dict) { const int rc = dict_resident(c.dict, &dict_end, &dict_len); if (rc) return rc; }
      return lz4hip::launch_decompress_dict(a, dict_end, dict_len, st);
    }
    case OP_DECOMPRESS_CHAIN:   // decode_chain_kernel draws chains from the queue word
      if (!c.chain) return fail(LZ4HIP_E_ARG, kNullArg);
      return with_queue_word(st, [&](uint32_t* q) { return lz4hip::launch_decompress_chain(*c.chain, q, lz4hip::device_cus(), st); });
    case OP_DECOMPRESS_STREAM:   // decode_stream_kernel draws streams from the queue word
      if (!c.dstream) return fail(LZ4HIP_E_ARG, kNullArg);
      return with_queue_word(st, [&](uint32_t* q) { return lz4hip::launch_decompress_stream(*c.dstream, q, lz4hip::device_cus(), st); });
    case OP_DECOMPRESS_STREAM_INORDER: {   // decode_stream_inorder_kernel draws streams from the queue word
      if (!c.dstream) return fail(LZ4HIP_E_ARG, kNullArg);
      const lz4hip::DStreamInorderArgs ia{*c.dstream, c.param ? 1u : 0u};
      return with_queue_word(st, [&](uint32_t* q) { return lz4hip::launch_decompress_stream_inorder(ia, q, lz4hip::device_cus(), st); });
    }
    case OP_COMPRESS_CHAIN:   // compress_fast_chain_cu_kernel draws chains from the queue word
      if (!c.cchain) return fail(LZ4HIP_E_ARG, kNullArg);
      return with_queue_word(st, [&](uint32_t* q) {
        return c.param >= 2 ? lz4hip::launch_compress_fast_chain_accel(*c.cchain, (uint32_t)c.param, q, lz4hip::device_cus(), st)
                            : lz4hip::launch_compress_fast_chain(*c.cchain, q, lz4hip::device_cus(), st);
      });
    case OP_COMPRESS_STREAM: {   // compress_fast_stream_cu_kernel draws chains from the queue word
      if (!c.cchain || !c.cs_rec || !c.cs_tables || !c.cs_slot) return fail(LZ4HIP_E_ARG, kNullArg);
      const lz4hip::CStreamArgs sa{*c.cchain, c.cs_slot, c.cs_rec, c.cs_tables};
      return with_queue_word(st, [&](uint32_t* q) {
        return c.param >= 2 ? lz4hip::launch_compress_fast_stream_accel(sa, (uint32_t)c.param, q, lz4hip::device_cus(), st)
                            : lz4hip::launch_compress_fast_stream(sa, q, lz4hip::device_cus(), st);
      });
    }
    case OP_COMPRESS_XSTREAM:   // compress_fast_xstream_cu_kernel draws chains from the queue word
      if (!c.cxstream) return fail(LZ4HIP_E_ARG, kNullArg);
      return with_queue_word(st, [&](uint32_t* q) {
        return c.param >= 2 ? lz4hip::launch_compress_fast_xstream_accel(*c.cxstream, (uint32_t)c.param, q, lz4hip::device_cus(), st)
                            : lz4hip::launch_compress_fast_xstream(*c.cxstream, q, lz4hip::device_cus(), st);
      });
    case OP_COMPRESS_HC_STREAM: {   // segment build over the host's item list, then the parse; the queue word is the image's own
      if (!c.hcstream || !c.hc_ws) return fail(LZ4HIP_E_ARG, kNullArg);
      return lz4hip::launch_compress_hc_stream(*c.hcstream, c.param, c.hc_ws, lz4hip::device_cus(), st);
    }
    case OP_COMPRESS_HC_CHAIN: {   // layout, segment build and parse kernels behind one scratch allocation
      if (!c.cchain) return fail(LZ4HIP_E_ARG, kNullArg);
      // (workspace and scratch are the buffer set's.  As a stream-ordered allocation made here, the scratch read as zeros in the parse
      // kernel in a third of the second calls of a process on the MI355X, behind a memset and a kernel that had written it: DESIGN.md 2.3)
      if (!c.hc_ws || !c.hc_scratch) return fail(LZ4HIP_E_ARG, kNullArg);
      const uint32_t seg = (uint32_t)g_hc_chain_segment.load(std::memory_order_relaxed);
      return lz4hip::launch_compress_hc_chain(*c.cchain, c.param, c.hc_ws, c.hc_span, seg, c.hc_scratch, lz4hip::device_cus(), st);
    }
    case OP_COMPRESS_HC:
    case OP_COMPRESS_HC_DICT:
    case OP_COMPRESS_HC_DEST: {
      const uint8_t* dict_end = nullptr;
      uint32_t keep = 0;
      const void* image = nullptr;
      if (c.op == OP_COMPRESS_HC_DICT) {
        if (!c.dict) return fail(LZ4HIP_E_ARG, kNullArg);
        const int rc = dict_hc_state(c.dict, st, &dict_end, &keep, &image);
        if (rc) return rc;
      }
      void* ws = c.hc_ws;
      uint64_t span = c.hc_span;
      if (!ws) { const int rc = hc_workspace(a, c.param, st, &ws, &span); if (rc) return rc; }
      const int e = c.op == OP_COMPRESS_HC      ? lz4hip::launch_compress_hc(a, c.param, ws, span, st)
                  : c.op == OP_COMPRESS_HC_DICT ? lz4hip::launch_compress_hc_dict(a, c.param, ws, span, dict_end, keep, image, st)
                                                : lz4hip::launch_compress_hc_dest(a, c.consumed, c.param, ws, span, st);
      if (!c.hc_ws) (void)hipFreeAsync(ws, st);
      return e;
    }
    case OP_COMPRESS_DICT:
    case OP_COMPRESS_ACCEL:   // the one-sequence kernels (compress_fast_accel_cu_kernel, compress_fast_dest_cu_kernel,
    case OP_COMPRESS_DEST: {  // compress_fast_dict_cu_kernel) draw blocks from the queue word
      const uint8_t* dict_end = nullptr;
      int32_t keep = 0;
      const void* image = nullptr;
      if (c.op == OP_COMPRESS_DICT) {
        if (!c.dict) return fail(LZ4HIP_E_ARG, kNullArg);
        const int rc = dict_compress_state(c.dict, st, &dict_end, &keep, &image);
        if (rc) return rc;
      }
      return with_queue_word(st, [&](uint32_t* q) {
        return c.op == OP_COMPRESS_DICT  ? lz4hip::launch_compress_fast_dict(a, dict_end, keep, image, q, lz4hip::device_cus(), st)
             : c.op == OP_COMPRESS_ACCEL ? lz4hip::launch_compress_fast_accel(a, (uint32_t)c.param, q, lz4hip::device_cus(), st)
                                         : lz4hip::launch_compress_dest_size(a, c.consumed, q, lz4hip::device_cus(), st);
      });
    }
  }
  return fail(LZ4HIP_E_ARG, "unknown block operation");
}

// The prologue and epilogue of every entry point that takes a device index: the engine is up, the empty batch (`empty`; false where
// the entry has none) is fine, the entry's own argument check (`arg_error`: a message, or nullptr -- which pointers may be NULL
// differs), the device's ordinal, that device current for the body and the caller's restored after it.  `body` returns what
// launch_block returns.
template <class Body>
int on_device(int device, bool empty, const char* arg_error, Body body) {
  if (const int rc = need_device()) return rc;
  if (empty) return LZ4HIP_OK;
  if (arg_error) return fail(LZ4HIP_E_ARG, arg_error);
  int ord;
  if (ordinal(device, &ord)) return fail(LZ4HIP_E_ARG, "bad device index");
  DeviceGuard g(ord);
  if (!g.ok) return fail(LZ4HIP_E_HIP, "hipSetDevice failed");
  const int e = body();
  if (e < 0) return e;   // (the message is set: decode_knobs_error, hc_workspace)
  return e ? fail(LZ4HIP_E_HIP, "kernel launch", (hipError_t)e) : LZ4HIP_OK;
}

// a block operation on device pointers; `extra_error`: the entry's check of what it takes beyond the seven arrays
int dev_batch(const BlockCall& c, const lz4hip::BatchArgs& a, int device, void* stream, const char* extra_error = nullptr) {
  const bool null_arg = !a.src || !a.src_off || !a.src_len || (!op_writes_no_output(c.op) && (!a.dst || !a.dst_off)) || !a.dst_cap || !a.out ||
                        (op_has_consumed(c.op) && !c.consumed);
  return on_device(device, a.n == 0, null_arg ? kNullArg : extra_error, [&] { return launch_block(c, a, (hipStream_t)stream); });
}
// the bytes block i of a partial decode may fill: min(target, capacity), or -1 (the kernels' -1) where one of them is negative
int32_t partial_room(int32_t target, int32_t cap) { return (target < 0 || cap < 0) ? -1 : std::min(target, cap); }

// ---- host-pointer path ---------------------------------------------------------------------------
// ---- staging of the host-pointer batch API --------------------------------------------------------------------------
// A host batch is cut into chunks (64 MiB of source for the codec calls, CHUNK_SRC for the hashes).  Each chunk is packed into a
// PINNED staging buffer (user memory is pageable: hipMemcpyAsync from it would be staged by the runtime at a fraction of the link
// rate), copied to the device, processed, and its destination slots are copied back into a second pinned buffer, from which the
// bytes each block actually produced go to the caller's slots.  Several buffer sets per device rotate, so the CPU packs chunk c+1
// and unpacks chunk c-1 while the GPU works on chunk c.  Buffers, streams and events are created once per device and kept
// (lz4hip_shutdown releases them) -- the per-call hipMalloc/hipFree/stream churn of the first version cost more than the
// work for single blocks.
constexpr size_t CHUNK_SRC = 128u << 20;   // source bytes per chunk (hash path)
inline int env_int(const char* name, int dflt, int lo, int hi) { const char* v = getenv(name); if (!v) return dflt; int x = atoi(v); return x < lo ? lo : x > hi ? hi : x; }
constexpr uint32_t CHUNK_BLOCKS = 1u << 20;
constexpr int COPY_THREADS = 16;           // host threads packing / unpacking a chunk

struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    size_t want = n + n / 4 + 4096;
    hipError_t e = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) { if (pinned) (void)hipHostFree(p); else (void)hipFree(p); }
    p = nullptr; cap = 0;
  }
};

struct ChunkSlot {
  hipStream_t st = nullptr;                       // kernels (hash path: everything)
  hipStream_t st_in = nullptr, st_out = nullptr;  // host_shard: the H2D and D2H copies run on streams that never see a kernel
  hipStream_t q_in = nullptr, q_out = nullptr;    // the copy streams of the chunk in flight (= st for a call that is one chunk)
  hipEvent_t done = nullptr, ev_in = nullptr, ev_k = nullptr;
  GrowBuf h_src, h_dst, h_meta, d_src, d_dst, d_meta, d_ws, d_pack, d_poff;
  bool packed = false;                // compress ops: only the useful bytes of the slots come back (device-side packing)
  uint32_t i0 = 0, i1 = 0;            // blocks of the chunk in flight
  size_t src_bytes = 0, dst_bytes = 0;
  std::vector<uint64_t> so, dof;      // packed offsets of the chunk's blocks
  ChunkSlot() { h_src.pinned = h_dst.pinned = h_meta.pinned = true; }
};

// One host batch in flight uses a SlotPair (two buffer sets that alternate).  Pairs are pooled per device: a caller takes a free
// pair (or creates one, up to MAX_PAIRS; beyond that it waits for one), works WITHOUT any lock held -- N callers make progress on N
// pairs, each on its own streams -- and hands the pair back.  (Round 1 held one per-device mutex for the whole batch: every
// concurrent caller of the host API ran one at a time.)
struct SlotPair {
  static constexpr int SETS = 6;   // (host_shard uses g_host_sets of them, the hash path alternates between the first two)
  ChunkSlot slot[SETS];
  hipError_t init() {
    for (auto& s : slot) {
      hipError_t e;
      for (hipStream_t* q : {&s.st, &s.st_in, &s.st_out})
        if ((e = hipStreamCreateWithFlags(q, hipStreamNonBlocking)) != hipSuccess) return e;
      for (hipEvent_t* v : {&s.done, &s.ev_in, &s.ev_k})
        if ((e = hipEventCreateWithFlags(v, hipEventDisableTiming)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void release() {
    for (auto& s : slot) {
      for (hipStream_t* q : {&s.st, &s.st_in, &s.st_out}) { if (*q) (void)hipStreamDestroy(*q); *q = nullptr; }
      for (hipEvent_t* v : {&s.done, &s.ev_in, &s.ev_k}) { if (*v) (void)hipEventDestroy(*v); *v = nullptr; }
      for (GrowBuf* g : {&s.h_src, &s.h_dst, &s.h_meta, &s.d_src, &s.d_dst, &s.d_meta, &s.d_ws, &s.d_pack, &s.d_poff}) g->release();
    }
  }
  // keeps the staging of the first pairs (the steady state of big batches), drops big staging of the pairs beyond (bursts of callers)
  void trim(size_t keep) {
    for (auto& s : slot)
      for (GrowBuf* g : {&s.h_src, &s.h_dst, &s.d_src, &s.d_dst, &s.d_ws, &s.d_pack})
        if (g->cap > keep) g->release();
  }
};
struct DevCtx {
  static constexpr size_t MAX_PAIRS = 16, KEEP_PAIRS = 2;
  std::mutex mu;                 // guards the pool only (never held while a batch runs)
  std::condition_variable cv;
  std::vector<SlotPair*> all, idle;
  SlotPair* acquire(hipError_t* err) {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      if (!idle.empty()) { SlotPair* p = idle.back(); idle.pop_back(); return p; }
      if (all.size() < MAX_PAIRS) {
        SlotPair* p = new (std::nothrow) SlotPair();
        if (!p) { *err = hipErrorOutOfMemory; return nullptr; }
        all.push_back(p);
        lk.unlock();
        if ((*err = p->init()) != hipSuccess) { lk.lock(); p->release(); all.erase(std::find(all.begin(), all.end(), p)); delete p; return nullptr; }
        return p;
      }
      cv.wait(lk);
    }
  }
  void give_back(SlotPair* p) {
    // (trimming frees pinned and device memory -- hipFree / hipHostFree synchronise the device -- so it happens BEFORE the pool
    // lock is taken: the pair still belongs to this caller, and nobody's acquire / give_back waits behind it)
    bool extra;
    { std::lock_guard<std::mutex> lk(mu); extra = std::find(all.begin(), all.end(), p) - all.begin() >= (ptrdiff_t)KEEP_PAIRS; }
    if (extra) p->trim(8u << 20);
    { std::lock_guard<std::mutex> lk(mu); idle.push_back(p); }
    cv.notify_one();
  }
  void release() {   // lz4hip_shutdown: nothing is in flight
    std::lock_guard<std::mutex> lk(mu);
    for (SlotPair* p : all) { p->release(); delete p; }
    all.clear(); idle.clear();
  }
};
DevCtx g_ctx[64];

template <class F>
void par_blocks(uint32_t i0, uint32_t i1, size_t bytes, F f) {  // f(i) for i in [i0, i1), on several threads when it is worth it
  const uint32_t n = i1 - i0;
  static const int copy_threads = env_int("LZ4HIP_HOST_COPY_THREADS", COPY_THREADS, 1, 128);
  const int T = (bytes < (4u << 20) || n < 2) ? 1 : (int)std::min<uint32_t>((uint32_t)copy_threads, n);
  if (T == 1) { for (uint32_t i = i0; i < i1; i++) f(i); return; }
  // (a helper that cannot be had -- thread or memory exhaustion -- is no error: its share is done right here; nothing is thrown
  // with threads running, which would end the process from a finisher thread)
  std::thread th[128];
  int made = 0;
  for (int t = 0; t < T; t++) {
    const uint32_t a = i0 + (uint32_t)((uint64_t)n * t / T), b = i0 + (uint32_t)((uint64_t)n * (t + 1) / T);
    bool started = false;
    if (t + 1 < T) {   // (the last share is the caller's own)
      try { th[made] = std::thread([=] { for (uint32_t i = a; i < b; i++) f(i); }); made++; started = true; } catch (...) {}
    }
    if (!started) for (uint32_t i = a; i < b; i++) f(i);
  }
  for (int t = 0; t < made; t++) th[t].join();
}

// "what: hipGetErrorString(e)" into *where (fail's formatter: g_err is this thread's) -> the status the C ABI reports for it
int hip_status(std::string* where, const char* what, hipError_t e) {
  *where = (fail(0, what, e), g_err);
  return e == hipErrorOutOfMemory ? (int)LZ4HIP_E_NOMEM : (int)LZ4HIP_E_HIP;
}

// What every shard function below has around its work: the device `ord` current, a buffer pair of its pool for as long as the scope
// lives, the shard's status (rc: once it is not LZ4HIP_OK the shard is over) with its message in *err.  When the shard ends in an
// error -- or in an exception -- the streams of the pair's buffer sets are waited for before it goes back: nothing may stay in flight
// on the cached buffers, the next caller's streams are not ordered against them.
struct ShardScope {
  std::string* err;
  const int ord;
  int rc = LZ4HIP_OK;
  SlotPair* pair = nullptr;
  ShardScope(int ord_, std::string* err_) : err(err_), ord(ord_) {
    hipError_t e = hipSuccess;
    if (ord < 0 || ord >= 64) { *err = "device ordinal out of range"; rc = LZ4HIP_E_ARG; }
    else if (ok("hipSetDevice", hipSetDevice(ord)) && !(pair = g_ctx[ord].acquire(&e))) ok("stream/event creation", e);
  }
  ~ShardScope() {
    if (!pair) return;
    if (rc != LZ4HIP_OK || std::uncaught_exceptions())
      for (ChunkSlot& s : pair->slot) {   // (the sets the shard did not touch are idle: their streams answer at once)
        for (hipStream_t q : {s.st_in, s.st, s.st_out}) (void)hipStreamSynchronize(q);
        s.i0 = s.i1 = 0;
      }
    g_ctx[ord].give_back(pair);
  }
  // every step of a shard: e is fine, or it becomes the shard's status
  bool ok(const char* what, hipError_t e) { if (e != hipSuccess) rc = hip_status(err, what, e); return e == hipSuccess; }
  bool launched(int le) {   // what launch_block returned: a status whose message is set on this thread (< 0), or a hipError_t
    if (le < 0) { *err = lz4hip_last_error(); rc = le; }
    return le >= 0 && ok("kernel launch", (hipError_t)le);
  }
  // the staging of a chunk of sb packed source bytes, db destination bytes (dst: it has a destination) and `meta` bytes of metadata
  bool reserve(ChunkSlot& s, size_t sb, bool dst, size_t db, size_t meta) {
    hipError_t e = hipSuccess;
    for (GrowBuf* g : {&s.h_src, &s.d_src}) if (e == hipSuccess) e = g->reserve(sb + 64);
    for (GrowBuf* g : {&s.h_dst, &s.d_dst}) if (e == hipSuccess && dst) e = g->reserve(db + 64);
    for (GrowBuf* g : {&s.h_meta, &s.d_meta}) if (e == hipSuccess) e = g->reserve(meta);
    return ok("staging allocation", e);
  }
  // the packed source and the metadata's inputs (and zeroed results) to the device, the metadata's results to the host: one copy each
  bool upload(ChunkSlot& s, size_t sb, const staging::MetaLayout& l, hipStream_t q) {
    return ok("H2D src", sb ? hipMemcpyAsync(s.d_src.p, s.h_src.p, sb, hipMemcpyHostToDevice, q) : hipSuccess) &&
           ok("H2D meta", hipMemcpyAsync(s.d_meta.p, s.h_meta.p, l.upload, hipMemcpyHostToDevice, q));
  }
  bool fetch_results(ChunkSlot& s, const staging::MetaLayout& l, hipStream_t q) {
    return ok("D2H out", hipMemcpyAsync((uint8_t*)s.h_meta.p + l.results, (const uint8_t*)s.d_meta.p + l.results, l.results_bytes(), hipMemcpyDeviceToHost, q));
  }
  bool wait(hipStream_t q) { return ok("hipStreamSynchronize", hipStreamSynchronize(q)); }
  // the chain- and stream-shaped shards' launch on the set's own stream: the kernel, the results to the host, and they are there
  bool run(const BlockCall& call, ChunkSlot& s, const staging::MetaLayout& l) {
    return launched(launch_block(call, lz4hip::BatchArgs{}, s.st)) && fetch_results(s, l, s.st) && wait(s.st);
  }
  // Runs of bytes (any order, overlapping ones included: joined here, host_staging.h merge_runs) that lie at the same offsets in a
  // pinned mirror and in its device buffer, one copy per joined run on s.st, `what` the step's name: from the mirror up ...
  bool upload_runs(ChunkSlot& s, const GrowBuf& host, GrowBuf& dev, std::vector<staging::Run>& runs, const char* what) {
    staging::merge_runs(runs);
    for (const staging::Run& r : runs)
      if (!ok(what, hipMemcpyAsync((uint8_t*)dev.p + r.off, (const uint8_t*)host.p + r.off, r.len, hipMemcpyHostToDevice, s.st))) return false;
    return true;
  }
  // ... and from d_dst down into h_dst, waited for
  bool fetch_runs(ChunkSlot& s, std::vector<staging::Run>& runs, const char* what) {
    staging::merge_runs(runs);
    for (const staging::Run& r : runs)
      if (!ok(what, hipMemcpyAsync((uint8_t*)s.h_dst.p + r.off, (const uint8_t*)s.d_dst.p + r.off, r.len, hipMemcpyDeviceToHost, s.st))) return false;
    return wait(s.st);
  }
  // only the bytes produced come back: entry(t) as staging::for_each_run takes it (offsets ascending)
  template <class Entry>
  bool fetch_runs(ChunkSlot& s, uint32_t n, Entry entry) {
    runs.clear();
    (void)staging::for_each_run(n, entry, [&](size_t r0, size_t r1) { runs.push_back(staging::Run{r0, r1 - r0}); return 0; });
    return fetch_runs(s, runs, "D2H dst");
  }
  // The compressors' way back, once out[] of the chunk's blocks [b0, b1) is on the host: a block produced out[i] bytes where that is a
  // size within its capacity.  Those bytes alone come down -- block b0 + t's slot lies at dso[t] of d_dst -- and go to the caller's
  // slots on several threads (db: the slots' bytes in all)
  bool hand_back_produced(ChunkSlot& s, uint32_t b0, uint32_t b1, size_t db, const std::vector<uint64_t>& dso, uint8_t* dst, const uint64_t* dst_off,
                          const int32_t* dst_cap, const int32_t* out) {
    auto produced = [=](uint32_t i) -> size_t { const int32_t r = out[i]; return r > 0 && (size_t)r <= pos(dst_cap[i]) ? (size_t)r : 0; };
    if (!fetch_runs(s, b1 - b0, [&](uint32_t t) { return staging::Run{(size_t)dso[t], produced(b0 + t)}; })) return false;
    const uint8_t* const hd = (const uint8_t*)s.h_dst.p;
    par_blocks(b0, b1, db, [=, &dso](uint32_t i) { if (const size_t r = produced(i)) memcpy(dst + dst_off[i], hd + dso[i - b0], r); });
    return true;
  }
  std::vector<staging::Run> runs;   // (fetch_runs' list, kept from chunk to chunk)
};

// ---- the frame of the shards whose unit is a chain or a stream of blocks ----
// A chunk of such a shard: the chains (streams) [c, j) of the call, their blocks [b0, b1), nc and nb of them; src, dst: what the
// chunk costs, as its shard counts it
struct ChainChunk { uint32_t c, j, b0, b1, nb, nc; size_t src, dst; };
// One device's share [c0, c1) of such a call (chain_first: the caller's), a chunk at a time through the FIRST buffer set of a pooled
// pair and on that set's stream alone -- no rotation, no finisher threads.  A chunk takes whole chains while their cost(chain) stays
// within LZ4HIP_HOST_CHUNK_MB (64) MiB of source and 512 MiB of destination, one chain at least.  chunk(sh, s, k) stages, runs and hands
// back chunk k; false: it failed (sh.rc and the message are set), which ends the shard -- through the scope, which waits for the streams.
template <class CostOf, class ChunkFn>
int chain_shard(int ord, const uint32_t* chain_first, uint32_t c0, uint32_t c1, std::string* err, CostOf cost, ChunkFn chunk) {
  if (c1 == c0) return LZ4HIP_OK;
  ShardScope sh(ord, err);
  if (sh.rc) return sh.rc;
  ChunkSlot& s = sh.pair->slot[0];
  const size_t chunk_src = (size_t)env_int("LZ4HIP_HOST_CHUNK_MB", 64, 1, 1024) << 20, chunk_dst = (size_t)512u << 20;
  for (uint32_t c = c0; c < c1;) {
    const staging::Chunk ck = staging::cut_chunk(c, c1, UINT32_MAX, chunk_src, chunk_dst, cost);
    const uint32_t j = ck.end, b0 = chain_first[c], b1 = chain_first[j];
    if (!chunk(sh, s, ChainChunk{c, j, b0, b1, b1 - b0, j - c, ck.src, ck.dst})) return sh.rc;
    c = j;
  }
  return LZ4HIP_OK;
}

// one device's share [b0, b1) of a host batch.  Three stages run side by side on LZ4HIP_HOST_SETS rotating buffer sets (default 6,
// each a pinned pair of 64 MiB of source + the destination capacity of its chunk, allocated on first use and kept in the per-device
// pool -- up to ~1 GiB of pinned host memory per cached pair at the defaults; LZ4HIP_HOST_SETS=2 / LZ4HIP_HOST_CHUNK_MB lower it):
// the calling thread PACKS chunk c + 1 into pinned memory and enqueues it, the GPU works on chunk c (its H2D, kernels and D2H on the
// set's own stream), and a finisher thread per chunk waits for chunk c - 1 and hands its bytes to the caller's slots.  (Rounds 1-2 did
// pack, the synchronous D2H of the packed bytes and the unpack one after the other on the calling thread: 44 ms per GiB, twice what
// the link needs -- tools/host_path_probe.py.)
// op_has_consumed: c.consumed (the second per-block output) travels behind out[] in the metadata and comes back with the sizes
int host_shard(const BlockCall& c, int ord, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
               const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out, uint32_t b0, uint32_t b1, std::string* err) {
  if (b1 == b0) return LZ4HIP_OK;
  ShardScope sh(ord, err);
  int& rc = sh.rc;
  if (rc) return rc;
  hipError_t e;
  const bool no_output = op_writes_no_output(c.op);   // (dst / dst_off may be NULL: no destination bytes exist on either side)
  auto dcap_of = [&](uint32_t i) -> size_t { return no_output ? 0 : pos(dst_cap[i]); };
  const bool prof = getenv("LZ4HIP_HOST_PROF") != nullptr;   // developer diagnostics: where the time of the stages goes
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  std::atomic<double> t_wait{0}, t_d2h{0}, t_unpack{0};
  auto add = [](std::atomic<double>& a, double v) { double o = a.load(); while (!a.compare_exchange_weak(o, o + v)) {} };

  // hand the results of the chunk in `s` to the caller (waits for it): runs on the chunk's finisher thread
  struct Fin { std::thread th; int rc = LZ4HIP_OK; std::string err; bool live = false; } fin[SlotPair::SETS];
  struct JoinAll {   // no finisher outlives this call, whichever way it is left (an exception of the packing code included)
    Fin* f;
    ~JoinAll() { for (int t = 0; t < SlotPair::SETS; t++) if (f[t].th.joinable()) f[t].th.join(); }
  } join_all{fin};
  auto finish = [&](ChunkSlot& s, Fin& f) -> int {
    if (s.i1 == s.i0) return LZ4HIP_OK;
    hipError_t fe;
    if ((fe = hipSetDevice(ord)) != hipSuccess) return hip_status(&f.err, "hipSetDevice", fe);
    double c0 = now();
    if ((fe = hipEventSynchronize(s.done)) != hipSuccess) return hip_status(&f.err, "hipEventSynchronize", fe);
    add(t_wait, now() - c0); c0 = now();
    const uint32_t nb = s.i1 - s.i0;
    const staging::BlockMeta m(nb, op_has_consumed(c.op));
    const int32_t* hout = m.out.in(s.h_meta.p);
    memcpy(out + s.i0, hout, m.out.bytes());
    if (op_has_consumed(c.op)) memcpy(c.consumed + s.i0, m.consumed.in(s.h_meta.p), m.consumed.bytes());
    if (s.packed) {   // the sizes are here: fetch exactly the useful bytes (already packed on the device), then hand them out
      uint64_t total = 0;
      for (uint32_t t = 0; t < nb; t++) { s.dof[t] = total; total += hout[t] > 0 ? (uint64_t)hout[t] : 0ull; }
      if (s.q_out != s.st && (fe = hipStreamWaitEvent(s.q_out, s.ev_k, 0)) != hipSuccess) return hip_status(&f.err, "hipStreamWaitEvent", fe);   // (the pack kernel)
      if (total && (fe = hipMemcpyAsync(s.h_dst.p, s.d_pack.p, (size_t)total, hipMemcpyDeviceToHost, s.q_out)) != hipSuccess) return hip_status(&f.err, "D2H packed", fe);
      if ((fe = hipStreamSynchronize(s.q_out)) != hipSuccess) return hip_status(&f.err, "hipStreamSynchronize", fe);
      s.dst_bytes = (size_t)total;
    }
    add(t_d2h, now() - c0); c0 = now();
    const bool fills = op_fills_capacity(c.op);
    if (!no_output) par_blocks(s.i0, s.i1, s.dst_bytes, [=, &s](uint32_t i) {
      int64_t produced;   // (bytes past a result stay untouched in the caller's slot)
      if (fills) produced = out[i] > 0 ? dst_cap[i] : 0;
      else produced = out[i] > 0 ? out[i] : 0;
      if (produced > 0) memcpy(dst + dst_off[i], (const uint8_t*)s.h_dst.p + s.dof[i - s.i0], (size_t)produced);
    });
    add(t_unpack, now() - c0);
    return LZ4HIP_OK;
  };
  // the buffer set is free again once its finisher is through
  auto reap = [&](int k) -> int {
    Fin& f = fin[k];
    if (!f.live) return LZ4HIP_OK;
    f.th.join();
    f.live = false;
    sh.pair->slot[k].i0 = sh.pair->slot[k].i1 = 0;
    if (f.rc != LZ4HIP_OK) *err = f.err;
    return f.rc;
  };
  auto start_finisher = [&](int k) {
    Fin& f = fin[k];
    ChunkSlot& s = sh.pair->slot[k];
    f.rc = LZ4HIP_OK;
    try {
      f.th = std::thread([&finish, &s, &f] {
        try { f.rc = finish(s, f); }
        catch (...) { f.rc = LZ4HIP_E_NOMEM; f.err = "host staging: out of memory or threads while handing a chunk back"; }
      });
      f.live = true;
    } catch (...) {   // no thread to be had: this chunk is finished on the calling thread
      f.rc = finish(s, f);
      f.live = false;
      s.i0 = s.i1 = 0;
    }
    return f.live ? LZ4HIP_OK : (f.rc != LZ4HIP_OK ? (*err = f.err, f.rc) : LZ4HIP_OK);
  };

  const int SETS = env_int("LZ4HIP_HOST_SETS", 6, 2, SlotPair::SETS);
  const size_t chunk_src = (size_t)env_int("LZ4HIP_HOST_CHUNK_MB", 64, 1, 1024) << 20;
  uint32_t i = b0;
  int k = 0;
  double t_reap = 0, t_pack = 0, t_enq = 0, t_alloc = 0;
  const double t_begin = now();
  while (i < b1 && rc == LZ4HIP_OK) {
    ChunkSlot& s = sh.pair->slot[k];
    double t0 = now();
    if ((rc = reap(k)) != LZ4HIP_OK) break;   // the chunk that used this buffer set SETS rounds ago
    t_reap += now() - t0; t0 = now();
    // the next chunk: blocks [i, j); only its source is limited
    const staging::Chunk ck = staging::cut_chunk(i, b1, CHUNK_BLOCKS, chunk_src, SIZE_MAX, [&](uint32_t t) { return staging::Cost{al16(pos(src_len[t])), al16(dcap_of(t))}; });
    const uint32_t j = ck.end, nb = j - i;
    const size_t sb = ck.src, db = ck.dst;   // packed source and destination bytes
    s.so.resize(nb); s.dof.resize(nb);
    { size_t so = 0, dofs = 0;
      for (uint32_t t = 0; t < nb; t++) { s.so[t] = so; s.dof[t] = dofs; so += al16(pos(src_len[i + t])); dofs += al16(dcap_of(i + t)); } }
    const staging::BlockMeta m(nb, op_has_consumed(c.op));
    if (!sh.reserve(s, sb, !no_output, db, m.l.total)) break;
    if ((op_uses_hc_ws(c.op) && (e = s.d_ws.reserve(lz4hip::hc_ws_bytes(sb, nb, c.param))) != hipSuccess) ||
        (op_compresses(c.op) && ((e = s.d_pack.reserve(db + 64)) != hipSuccess || (e = s.d_poff.reserve((size_t)nb * 8u)) != hipSuccess))) {
      sh.ok("staging allocation", e);
      break;
    }
    t_alloc += now() - t0; t0 = now();
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    par_blocks(i, j, sb, [=, &s](uint32_t t) { if (src_len[t] > 0) memcpy(hs + s.so[t - i], src + src_off[t], (size_t)src_len[t]); });
    memcpy(m.src_off.in(hm), s.so.data(), m.src_off.bytes());
    memcpy(m.dst_off.in(hm), s.dof.data(), m.dst_off.bytes());
    memcpy(m.src_len.in(hm), src_len + i, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), dst_cap + i, m.dst_cap.bytes());
    t_pack += now() - t0; t0 = now();
    // a call that is ONE chunk (single blocks, small batches) has nothing to overlap: one stream, no finisher thread
    const bool single = (i == b0 && j == b1);
    s.q_in = single ? s.st : s.st_in;
    s.q_out = single ? s.st : s.st_out;
    if (!sh.upload(s, sb, m.l, s.q_in)) break;
    if (!single && ((e = hipEventRecord(s.ev_in, s.q_in)) != hipSuccess || (e = hipStreamWaitEvent(s.st, s.ev_in, 0)) != hipSuccess)) { sh.ok("H2D event", e); break; }
    lz4hip::BatchArgs a{(const uint8_t*)s.d_src.p, m.src_off.in(dm), m.src_len.in(dm), no_output ? nullptr : (uint8_t*)s.d_dst.p, m.dst_off.in(dm), m.dst_cap.in(dm), m.out.in(dm), nb};
    BlockCall dc = c;   // the call on this chunk's device arrays
    if (op_has_consumed(c.op)) dc.consumed = m.consumed.in(dm);
    if (op_uses_hc_ws(c.op)) { dc.hc_ws = s.d_ws.p; dc.hc_span = sb; }
    if (!sh.launched(launch_block(dc, a, s.st))) break;   // (< 0: e.g. a decode knob combination without a kernel, launch_decode has said which)
    s.packed = op_compresses(c.op);
    // the sizes travel first; compress ops: the finisher fetches exactly the packed bytes once it has them
    if (!single && ((e = hipEventRecord(s.ev_k, s.st)) != hipSuccess || (e = hipStreamWaitEvent(s.q_out, s.ev_k, 0)) != hipSuccess)) { sh.ok("kernel event", e); break; }
    if (!sh.fetch_results(s, m.l, s.q_out)) break;
    if (s.packed) {
      if ((e = hipEventRecord(s.done, s.q_out)) != hipSuccess) { sh.ok("hipEventRecord", e); break; }   // sizes on the host
      if (!sh.launched(lz4hip::launch_pack(a, (uint64_t*)s.d_poff.p, (uint8_t*)s.d_pack.p, s.st))) break;
      if (!single && (e = hipEventRecord(s.ev_k, s.st)) != hipSuccess) { sh.ok("hipEventRecord", e); break; }   // packed bytes ready (the finisher waits for it)
    } else {
      if (db && (e = hipMemcpyAsync(s.h_dst.p, s.d_dst.p, db, hipMemcpyDeviceToHost, s.q_out)) != hipSuccess) { sh.ok("D2H dst", e); break; }
      if ((e = hipEventRecord(s.done, s.q_out)) != hipSuccess) { sh.ok("hipEventRecord", e); break; }
    }
    s.i0 = i; s.i1 = j; s.src_bytes = sb; s.dst_bytes = db;
    if (single) {
      Fin& f = fin[k];
      if ((rc = finish(s, f)) != LZ4HIP_OK) *err = f.err;
      s.i0 = s.i1 = 0;
    } else {
      rc = start_finisher(k);
    }
    i = j;
    k = (k + 1) % SETS;
    t_enq += now() - t0;
  }
  const double t_loop = now() - t_begin;
  // drain (also after an error: no finisher may outlive this call; the scope then waits for the streams)
  for (int t = 0; t < SETS; t++) {
    std::string keep = *err;
    const int r = reap((k + t) % SETS);
    if (rc == LZ4HIP_OK) rc = r; else *err = keep;   // (the first error is the one reported)
  }
  if (prof)
    fprintf(stderr, "[lz4hip host_shard op %d, %u blocks] total %.1f ms: loop %.1f (reap %.1f | alloc %.1f | pack %.1f | enqueue %.1f), drain %.1f; finishers: wait %.1f + d2h %.1f + unpack %.1f\n",
            (int)c.op, b1 - b0, 1e3 * (now() - t_begin), 1e3 * t_loop, 1e3 * t_reap, 1e3 * t_alloc, 1e3 * t_pack, 1e3 * t_enq,
            1e3 * (now() - t_begin - t_loop), 1e3 * t_wait.load(), 1e3 * t_d2h.load(), 1e3 * t_unpack.load());
  return rc;
}

// A host batch over the initialised devices: contiguous block ranges per device, a thread per device, the
// caller's current device restored, the first error reported.  Batches of fewer than 2 x per_device blocks stay on one device.
// shard(ordinal, b0, b1, &error text) does one device's share.
template <class Shard>
int fan_out(uint32_t n, uint32_t per_device, Shard shard) {
  std::vector<int> devs;
  { std::lock_guard<std::mutex> lk(g_mu); devs = g_devs; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  const uint32_t D = (uint32_t)std::min<size_t>(devs.size(), std::max<uint32_t>(1u, n / per_device));
  std::vector<int> rcs(D, 0);
  std::vector<std::string> errs(D);
  if (D == 1) {
    rcs[0] = shard(devs[0], 0u, n, &errs[0]);
  } else {
    std::vector<std::thread> th;
    for (uint32_t d = 0; d < D; d++) {
      const uint32_t b0 = (uint32_t)((uint64_t)n * d / D), b1 = (uint32_t)((uint64_t)n * (d + 1) / D);
      th.emplace_back([&, d, b0, b1] { rcs[d] = shard(devs[d], b0, b1, &errs[d]); });
    }
    for (auto& t : th) t.join();
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  for (uint32_t d = 0; d < D; d++)
    if (rcs[d]) return fail(rcs[d], errs[d].c_str());
  return LZ4HIP_OK;
}

int host_batch(const BlockCall& c, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
               const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out, uint32_t n) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!src || !src_off || !src_len || (!op_writes_no_output(c.op) && (!dst || !dst_off)) || !dst_cap || !out || (op_has_consumed(c.op) && !c.consumed))
    return fail(LZ4HIP_E_ARG, kNullArg);
  return fan_out(n, 64u, [&](int ord, uint32_t b0, uint32_t b1, std::string* err) {
    return host_shard(c, ord, src, src_off, src_len, dst, dst_off, dst_cap, out, b0, b1, err);
  });
}

// ---- chains of linked blocks on the host-pointer path ----
// The opening of every host entry point whose unit is a chain or a stream: an argument error (why: a message or nullptr) is said without
// a device too; then the engine has to be there; a call of no chains is done; everything else is rest().
template <class Rest>
int chain_entry(const char* why, uint32_t n_chains, Rest rest) {
  if (why) return fail(LZ4HIP_E_ARG, why);
  if (const int rc = need_device()) return rc;
  return n_chains == 0 ? (int)LZ4HIP_OK : rest();
}
// ... and what the entries that hold no stream set go on with: whole chains per device
template <class Shard>
int whole_chains(uint32_t n_chains, Shard shard) { return fan_out(n_chains, 64u, shard); }

// One device's share [c0, c1) of a chain batch (h: the caller's HOST arrays).  Chains are staged a chunk at a time (64 MiB of streams
// or 512 MiB of destination, one chain at least) through the first buffer set of a pooled pair: the streams and, per chain, the last
// min(prefix_len, 65536) bytes of history from the caller's dst go up; the kernel runs; the results come back, and then only the bytes
// each chain decoded (runs less than 4 KB apart travel as one copy).  On the device a chain's region is min(chain_dst_cap, the sum of
// its blocks' capacities) bytes: a block's capacity is the smaller of its own and what is left, so nothing changes.
int chain_host_shard(const lz4hip::ChainArgs& h, int ord, uint32_t c0, uint32_t c1, std::string* err) {
  auto keep_of = [&](uint32_t c) -> size_t { const int32_t p = h.chain_prefix_len ? h.chain_prefix_len[c] : 0; return p > 65536 ? 65536u : (size_t)p; };
  auto room_of = [&](uint32_t c) -> size_t {   // the chain's region on the device
    uint64_t sum = 0;
    for (uint32_t i = h.chain_first[c]; i < h.chain_first[c + 1]; i++) sum += pos(h.dst_cap[i]);
    return (size_t)std::min<uint64_t>(sum, h.chain_dst_cap[c]);
  };
  auto cost = [&](uint32_t c) { return staging::Cost{staging::chain_packed_bytes(h.chain_first, c, h.src_len), al16(keep_of(c) + room_of(c))}; };
  std::vector<uint64_t> so, cdo, room;
  return chain_shard(ord, h.chain_first, c0, c1, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, j = ck.j, b0 = ck.b0, b1 = ck.b1, nb = ck.nb, nc = ck.nc;
    const hipStream_t st = s.st;
    (void)staging::packed_offsets(h.src_len + b0, nb, so);
    cdo.resize(nc); room.resize(nc);
    { size_t o = 0; for (uint32_t t = 0; t < nc; t++) { room[t] = room_of(c + t); cdo[t] = o + keep_of(c + t); o += al16(keep_of(c + t) + room[t]); } }
    const staging::ChainMeta m(nb, nc);
    if (!sh.reserve(s, ck.src, true, ck.dst, m.l.total)) return false;
    uint8_t *const hs = (uint8_t*)s.h_src.p, *const hd = (uint8_t*)s.h_dst.p, *const dd = (uint8_t*)s.d_dst.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    par_blocks(b0, b1, ck.src, [=, &so](uint32_t i) { if (h.src_len[i] > 0) memcpy(hs + so[i - b0], h.src + h.src_off[i], (size_t)h.src_len[i]); });
    m.l.zero_results(hm);
    memcpy(m.src_off.in(hm), so.data(), m.src_off.bytes());
    memcpy(m.chain_dst_off.in(hm), cdo.data(), m.chain_dst_off.bytes());
    memcpy(m.chain_dst_cap.in(hm), room.data(), m.chain_dst_cap.bytes());
    memcpy(m.src_len.in(hm), h.src_len + b0, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), h.dst_cap + b0, m.dst_cap.bytes());
    staging::rebase_first(h.chain_first, c, nc, m.first.in(hm));
    for (uint32_t t = 0; t < nc; t++) m.prefix.in(hm)[t] = (int32_t)keep_of(c + t);
    if (h.stored) memcpy(m.stored.in(hm), h.stored + b0, nb); else memset(m.stored.in(hm), 0, nb);
    if (!sh.upload(s, ck.src, m.l, st)) return false;
    for (uint32_t t = 0; t < nc; t++) {   // the histories
      const size_t k = keep_of(c + t);
      if (!k) continue;
      memcpy(hd + cdo[t] - k, h.dst + h.chain_dst_off[c + t] - k, k);
      if (!sh.ok("H2D history", hipMemcpyAsync(dd + cdo[t] - k, hd + cdo[t] - k, k, hipMemcpyHostToDevice, st))) return false;
    }
    const lz4hip::ChainArgs a{(const uint8_t*)s.d_src.p, m.src_off.in(dm), m.src_len.in(dm), m.stored.in(dm), m.dst_cap.in(dm), m.first.in(dm), dd,
                              m.chain_dst_off.in(dm), m.chain_dst_cap.in(dm), m.prefix.in(dm), m.out.in(dm), m.chain_out.in(dm), nb, nc};
    BlockCall call{OP_DECOMPRESS_CHAIN}; call.chain = &a;
    if (!sh.run(call, s, m.l)) return false;
    memcpy(h.out + b0, m.out.in(hm), m.out.bytes());
    memcpy(h.chain_out + c, m.chain_out.in(hm), m.chain_out.bytes());
    // only the bytes decoded come back
    if (!sh.fetch_runs(s, nc, [&](uint32_t t) { return staging::Run{(size_t)cdo[t], (size_t)h.chain_out[c + t]}; })) return false;
    par_blocks(c, j, ck.dst, [=, &cdo](uint32_t t) { if (const size_t n = (size_t)h.chain_out[t]) memcpy(h.dst + h.chain_dst_off[t], hd + cdo[t - c], n); });
    return true;
  });
}

// the argument errors of a chain call that can be seen without a device; host: the arrays are the caller's host memory and are read
const char* chain_arg_error(const lz4hip::ChainArgs& a, bool host) {
  if (a.n_chains == 0 && a.n_blocks == 0) return nullptr;
  if (!a.src || !a.src_off || !a.src_len || !a.dst_cap || !a.chain_first || !a.dst || !a.chain_dst_off || !a.chain_dst_cap || !a.out || !a.chain_out) return kNullArg;
  return host ? staging::chain_shape_error(a.chain_first, a.n_chains, a.n_blocks, a.chain_prefix_len, a.chain_dst_off, true) : nullptr;
}

// ---- streams whose blocks land anywhere, on the host-pointer path ----
// the caller's HOST arrays of a stream-decode call
struct DStreamHost {
  lz4hip_dstream_state* state; const uint8_t* src; const uint64_t* src_off; const int32_t* src_len; const uint32_t* chain_first;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap; const uint64_t* win_off; const uint64_t* win_len; int32_t* out;
  uint32_t n_blocks, n_chains;
  Op op = OP_DECOMPRESS_STREAM;   // or OP_DECOMPRESS_STREAM_INORDER, with
  int every = 0;                  // its BlockCall::param
};
static_assert(sizeof(lz4hip_dstream_state) == sizeof(staging::DsState) && sizeof(lz4hip_dstream_state) == sizeof(lz4hip::DStreamState) &&
              offsetof(lz4hip_dstream_state, ext_end) == offsetof(staging::DsState, ext_end) && offsetof(lz4hip_dstream_state, ext_end) == offsetof(lz4hip::DStreamState, ext_end),
              "one state record: the header's, the staging arithmetic's, the kernels'");
// One device's share [c0, c1) of a stream-decode batch.  Streams are staged a chunk at a time (64 MiB of compressed bytes or 512 MiB of
// device image, one stream at least) through the first buffer set of a pooled pair.  The image (host_staging.h DsImage) mirrors every
// stream's window, with lead room for a prefix that ends where the window begins, and holds the outside history pieces apart, each
// once.  Up go the compressed bytes, the state records in device terms and the history pieces (the external dictionary's only while
// the prefix is shorter than 65535 bytes: behind that liblz4 never looks at it); the kernel runs; the results and records come back,
// then each block's decoded bytes (runs less than 4 KB apart travel as one copy) -- nothing else of the caller's dst is written.
int dstream_host_shard(const DStreamHost& h, int ord, uint32_t c0, uint32_t c1, std::string* err) {
  const staging::DsState* const hstate = (const staging::DsState*)h.state;
  auto cost = [&](uint32_t c) { return staging::Cost{staging::chain_packed_bytes(h.chain_first, c, h.src_len), staging::dstream_cost(hstate[c], h.win_off[c], h.win_len[c])}; };
  std::vector<uint64_t> so, ddo;
  std::vector<staging::Run> runs;
  return chain_shard(ord, h.chain_first, c0, c1, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, b0 = ck.b0, b1 = ck.b1, nb = ck.nb, nc = ck.nc;
    const hipStream_t st = s.st;
    const staging::DsImage im(hstate + c, h.win_off + c, h.win_len + c, nc);
    (void)staging::packed_offsets(h.src_len + b0, nb, so);
    ddo.resize(nb);
    for (uint32_t t = 0; t < nc; t++)
      for (uint32_t i = h.chain_first[c + t]; i < h.chain_first[c + t + 1]; i++) ddo[i - b0] = im.win[t] + (h.dst_off[i] - h.win_off[c + t]);
    const staging::DsMetaLayout m(nb, nc);
    if (!sh.reserve(s, ck.src, true, im.total, m.l.total)) return false;
    uint8_t *const hs = (uint8_t*)s.h_src.p, *const hd = (uint8_t*)s.h_dst.p, *const dd = (uint8_t*)s.d_dst.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    par_blocks(b0, b1, ck.src, [=, &so](uint32_t i) { if (h.src_len[i] > 0) memcpy(hs + so[i - b0], h.src + h.src_off[i], (size_t)h.src_len[i]); });
    memcpy(m.src_off.in(hm), so.data(), m.src_off.bytes());
    memcpy(m.dst_off.in(hm), ddo.data(), m.dst_off.bytes());
    memcpy(m.src_len.in(hm), h.src_len + b0, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), h.dst_cap + b0, m.dst_cap.bytes());
    staging::rebase_first(h.chain_first, c, nc, m.first.in(hm));
    memcpy(m.state.in(hm), im.dev.data(), m.state.bytes());
    if (!sh.upload(s, ck.src, m.l, st)) return false;
    // the history pieces: into the pinned mirror, then up as joined runs (what a joined run carries between two pieces lands in
    // window bytes no block may rely on)
    runs.clear();
    auto piece = [&](size_t dev_end, uint64_t host_end, uint64_t keep) {
      memcpy(hd + dev_end - keep, h.dst + host_end - keep, (size_t)keep);
      runs.push_back(staging::Run{dev_end - (size_t)keep, (size_t)keep});
    };
    for (uint32_t t = 0; t < nc; t++) {
      const staging::DsState& hs0 = hstate[c + t];
      if (im.prefix[t].kind == staging::DS_INSIDE || im.prefix[t].kind == staging::DS_LEAD) piece((size_t)im.dev[t].prefix_end, hs0.prefix_end, im.prefix[t].keep);
      if (im.ext[t].kind == staging::DS_INSIDE && hs0.prefix_len < staging::kDsKeep) piece((size_t)im.dev[t].ext_end, hs0.ext_end, im.ext[t].keep);
    }
    for (const staging::DsApart& a : im.apart) piece(a.dev + (size_t)a.keep, a.end, a.keep);
    if (!sh.upload_runs(s, s.h_dst, s.d_dst, runs, "H2D history")) return false;
    const lz4hip::DStreamArgs a{(const uint8_t*)s.d_src.p, m.src_off.in(dm), m.src_len.in(dm), m.first.in(dm), dd, m.dst_off.in(dm), m.dst_cap.in(dm),
                                (lz4hip::DStreamState*)m.state.in(dm), m.out.in(dm), nb, nc};
    BlockCall call{h.op, h.every}; call.dstream = &a;
    if (!sh.run(call, s, m.l)) return false;
    memcpy(h.out + b0, m.out.in(hm), m.out.bytes());
    for (uint32_t t = 0; t < nc; t++) {   // the records, in the caller's terms again
      const staging::DsState was = hstate[c + t], now = m.state.in(hm)[t];
      h.state[c + t].prefix_end = im.to_host(t, now.prefix_end, was, h.win_off[c + t], h.win_len[c + t]);
      h.state[c + t].prefix_len = now.prefix_len;
      h.state[c + t].ext_end = im.to_host(t, now.ext_end, was, h.win_off[c + t], h.win_len[c + t]);
      h.state[c + t].ext_len = now.ext_len;
    }
    // only the bytes decoded come back
    runs.clear();
    for (uint32_t i = b0; i < b1; i++) if (h.out[i] > 0) runs.push_back(staging::Run{(size_t)ddo[i - b0], (size_t)h.out[i]});
    if (!sh.fetch_runs(s, runs, "D2H dst")) return false;
    // (in block order on one thread: where two slots of a call overlap, the later block's bytes are the ones that stay, as on the device)
    for (uint32_t i = b0; i < b1; i++) if (h.out[i] > 0) memcpy(h.dst + h.dst_off[i], hd + ddo[i - b0], (size_t)h.out[i]);
    return true;
  });
}

// the argument errors of a stream-decode call, all of which can be seen without a device (the arrays are the caller's host memory)
const char* dstream_arg_error(const DStreamHost& h) {
  if (h.n_chains == 0 && h.n_blocks == 0) return nullptr;
  if (!h.state || !h.src || !h.src_off || !h.src_len || !h.chain_first || !h.dst || !h.dst_off || !h.dst_cap || !h.win_off || !h.win_len || !h.out) return kNullArg;
  return staging::dstream_shape_error((const staging::DsState*)h.state, h.chain_first, h.n_chains, h.n_blocks, h.dst_off, h.dst_cap, h.win_off, h.win_len);
}

// ---- chains of linked blocks on the host-pointer path, compressing side ----
// One device's share [c0, c1) of a chain-compress batch (h: the caller's HOST arrays).  Chains are staged a chunk at a time (64 MiB of
// source or 512 MiB of slots, one chain at least) through the first buffer set of a pooled pair: each chain's source goes up with the
// last min(prefix_len, 65536) bytes of its history in front of it; the kernel runs; the results come back, and then only the bytes
// each block produced (runs less than 4 KB apart travel as one copy).  Of a chain's source only what its blocks can consume is
// read: up to the first block with a negative length or with which the chain would exceed 0x7E000000 bytes (its result is 0).
// op_chain_stops(c.op) false (the HC chain): every block's source is read, a negative length counts as 0 bytes, a history of any
// length is kept, nothing travels in chain_consumed[], and the chunk's workspace is sized by its packed source.
// op_resumes_streams(c.op) (resident streams): chain c continues stream share.ids[c]; its slot in the device's share of the set
// travels in the metadata, with the stop mark of a stream that an earlier call left in an unknown state.
int cchain_host_shard(const BlockCall& proto, const StreamShare& share, const lz4hip::CChainArgs& h, int ord, uint32_t c0, uint32_t c1, std::string* err) {
  auto keep_of = [&](uint32_t c) -> size_t { const int32_t p = h.chain_prefix_len ? h.chain_prefix_len[c] : 0; return p > 65536 ? 65536u : (size_t)p; };
  const bool stops = op_chain_stops(proto.op), resumes = op_resumes_streams(proto.op);
  auto span_of = [&](uint32_t c) -> size_t {   // the source bytes the chain's blocks can consume
    if (!stops) {
      size_t sum = 0;
      for (uint32_t i = h.chain_first[c]; i < h.chain_first[c + 1]; i++) sum += pos(h.src_len[i]);
      return sum;
    }
    const size_t k = keep_of(c);
    // (the kernel's count: a prefix under 8 bytes is not kept.  A resident stream's count is the device's: every block that can run
    // in a stream that has consumed nothing is read)
    uint64_t pos = (k < 8u || resumes) ? 0u : k;
    const uint64_t pos0 = pos;
    for (uint32_t i = h.chain_first[c]; i < h.chain_first[c + 1]; i++) {
      if (h.src_len[i] < 0 || pos + (uint64_t)h.src_len[i] > 0x7E000000ull) break;
      pos += (uint64_t)h.src_len[i];
    }
    return (size_t)(pos - pos0);
  };
  auto cost = [&](uint32_t c) { return staging::Cost{al16(keep_of(c) + span_of(c)), staging::chain_packed_bytes(h.chain_first, c, h.dst_cap)}; };
  std::vector<uint64_t> cso, dso;
  return chain_shard(ord, h.chain_first, c0, c1, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, j = ck.j, b0 = ck.b0, nb = ck.nb, nc = ck.nc;
    cso.resize(nc);
    { size_t o = 0; for (uint32_t t = 0; t < nc; t++) { cso[t] = o + keep_of(c + t); o += al16(keep_of(c + t) + span_of(c + t)); } }
    (void)staging::packed_offsets(h.dst_cap + b0, nb, dso);
    const staging::CChainMeta m(nb, nc, resumes);
    if (!sh.reserve(s, ck.src, true, ck.dst, m.l.total)) return false;
    if (op_uses_hc_ws(proto.op) && !sh.ok("staging allocation", s.d_ws.reserve(lz4hip::hc_ws_bytes(ck.src, nb, proto.param)))) return false;
    // (the layout's scratch for the largest segment count the knob allows, in the buffer set's unused offsets buffer)
    if (op_needs_chain_scratch(proto.op) && !sh.ok("staging allocation", s.d_poff.reserve(lz4hip::hc_chain_scratch_bytes(ck.src, nb, nc, 4096u)))) return false;
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    par_blocks(c, j, ck.src, [=, &cso](uint32_t t) {
      const size_t k = keep_of(t), n = k + span_of(t);
      if (n) memcpy(hs + cso[t - c] - k, h.src + h.chain_src_off[t] - k, n);
    });
    m.l.zero_results(hm);
    memcpy(m.chain_src_off.in(hm), cso.data(), m.chain_src_off.bytes());
    memcpy(m.dst_off.in(hm), dso.data(), m.dst_off.bytes());
    memcpy(m.src_len.in(hm), h.src_len + b0, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), h.dst_cap + b0, m.dst_cap.bytes());
    staging::rebase_first(h.chain_first, c, nc, m.first.in(hm));
    for (uint32_t t = 0; t < nc; t++) m.prefix.in(hm)[t] = (int32_t)keep_of(c + t);
    if (resumes) staging::stream_slots(share.ids + c, nc, share.id0, share.poisoned, m.slot.in(hm));
    if (!sh.upload(s, ck.src, m.l, s.st)) return false;
    const lz4hip::CChainArgs a{(const uint8_t*)s.d_src.p, m.chain_src_off.in(dm), m.prefix.in(dm), m.src_len.in(dm), m.first.in(dm), (uint8_t*)s.d_dst.p,
                               m.dst_off.in(dm), m.dst_cap.in(dm), m.out.in(dm), stops ? m.consumed.in(dm) : nullptr, nb, nc};
    BlockCall call = proto; call.cchain = &a;
    if (op_uses_hc_ws(proto.op)) { call.hc_ws = s.d_ws.p; call.hc_span = ck.src; }
    if (op_needs_chain_scratch(proto.op)) call.hc_scratch = s.d_poff.p;
    if (resumes) { call.cs_slot = m.slot.in(dm); if (share.launched) *share.launched = true; }
    if (!sh.run(call, s, m.l)) return false;
    memcpy(h.out + b0, m.out.in(hm), m.out.bytes());
    if (stops) memcpy(h.chain_consumed + c, m.consumed.in(hm), m.consumed.bytes());
    return sh.hand_back_produced(s, b0, ck.b1, ck.dst, dso, h.dst, h.dst_off, h.dst_cap, h.out);
  });
}

// the argument errors of a chain-compress call that can be seen without a device; host: the arrays are the caller's host memory
const char* cchain_arg_error(const lz4hip::CChainArgs& a, bool host, bool stops) {
  if (a.n_chains == 0 && a.n_blocks == 0) return nullptr;
  if (!a.src || !a.chain_src_off || !a.src_len || !a.chain_first || !a.dst || !a.dst_off || !a.dst_cap || !a.out || (stops && !a.chain_consumed)) return kNullArg;
  return host ? staging::chain_shape_error(a.chain_first, a.n_chains, a.n_blocks, a.chain_prefix_len, a.chain_src_off, false) : nullptr;
}

// ---- HC streams whose sources land anywhere, on the host-pointer path ----
// the caller's HOST arrays of lz4hip_compress_hc_stream_batch
struct HcStreamHost {
  lz4hip_hcstream_state* state; const uint8_t* src; const uint64_t* src_off; const int32_t* src_len; const uint32_t* chain_first;
  uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap; int32_t* out; uint32_t n_blocks, n_chains;
};
static_assert(sizeof(lz4hip_hcstream_state) == sizeof(staging::HcsState) && offsetof(lz4hip_hcstream_state, index) == offsetof(staging::HcsState, index),
              "the header's state record is the staging arithmetic's");
// One device's share [c0, c1) of such a call: the frame of chain_shard (chunks of 64 MiB of image or 512 MiB of slots) around the
// linear image of host_staging.h.  The states of a chunk's streams are written back once its results are on the host.
int hcstream_host_shard(int level, const HcStreamHost& h, int ord, uint32_t c0, uint32_t c1, std::string* err) {
  const staging::HcsState* const state = (const staging::HcsState*)h.state;
  auto cost = [&](uint32_t c) { return staging::Cost{staging::hcstream_cost(state[c], h.chain_first, c, h.src_len), staging::chain_packed_bytes(h.chain_first, c, h.dst_cap)}; };
  const uint32_t seg = (uint32_t)g_hc_chain_segment.load(std::memory_order_relaxed);
  std::vector<uint64_t> dso;
  std::vector<uint32_t> items;
  return chain_shard(ord, h.chain_first, c0, c1, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, b0 = ck.b0, nb = ck.nb, nc = ck.nc;
    if (nb == 0) return true;   // (streams without blocks: their states stay as they are)
    const staging::HcsImage im(state, h.chain_first, c, nc, h.src_off, h.src_len);
    (void)staging::packed_offsets(h.dst_cap + b0, nb, dso);
    items.clear();   // positions 0 .. len - 4 get an entry: ceil((len - 3) / seg) segments per stream
    for (uint32_t t = 0; t < nc; t++)
      for (uint64_t k = 0, nk = im.buf_len[t] >= 4u ? (im.buf_len[t] - 3u + seg - 1u) / seg : 0u; k < nk; k++) { items.push_back(t); items.push_back((uint32_t)k); }
    const staging::HcStreamMeta m(nb, nc, im.ends.size(), items.size() / 2u);
    if (!sh.reserve(s, im.total, true, ck.dst, m.l.total)) return false;
    if (!sh.ok("staging allocation", s.d_ws.reserve(lz4hip::hc_ws_bytes(im.total, nb, level)))) return false;
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    par_blocks(0, (uint32_t)im.pieces.size(), im.total, [=, &im](uint32_t t) { const staging::HcsPiece& p = im.pieces[t]; memcpy(hs + p.dev, h.src + p.src, p.len); });
    m.l.zero_results(hm);
    memcpy(m.blk_start.in(hm), im.blk_start.data(), m.blk_start.bytes());
    memcpy(m.dst_off.in(hm), dso.data(), m.dst_off.bytes());
    memcpy(m.buf_off.in(hm), im.buf_off.data(), m.buf_off.bytes());
    memcpy(m.buf_len.in(hm), im.buf_len.data(), m.buf_len.bytes());
    memcpy(m.src_len.in(hm), h.src_len + b0, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), h.dst_cap + b0, m.dst_cap.bytes());
    memcpy(m.blk_hist.in(hm), im.blk_hist.data(), m.blk_hist.bytes());
    memcpy(m.blk_low.in(hm), im.blk_low.data(), m.blk_low.bytes());
    memcpy(m.blk_dlim.in(hm), im.blk_dlim.data(), m.blk_dlim.bytes());
    memcpy(m.end_first.in(hm), im.end_first.data(), m.end_first.bytes());
    if (m.ends.n) memcpy(m.ends.in(hm), im.ends.data(), m.ends.bytes());
    if (m.items.n) memcpy(m.items.in(hm), items.data(), m.items.bytes());
    if (!sh.upload(s, im.total, m.l, s.st)) return false;
    const lz4hip::HcStreamArgs a{(const uint8_t*)s.d_src.p, m.blk_start.in(dm), m.blk_hist.in(dm), m.blk_low.in(dm), m.blk_dlim.in(dm), m.src_len.in(dm),
                                 (uint8_t*)s.d_dst.p, m.dst_off.in(dm), m.dst_cap.in(dm), m.out.in(dm), m.buf_off.in(dm), m.buf_len.in(dm), m.end_first.in(dm),
                                 m.ends.in(dm), m.items.in(dm), m.queue.in(dm), (uint64_t)im.total, nb, nc, (uint32_t)im.ends.size(), (uint32_t)(items.size() / 2u), seg};
    BlockCall call{OP_COMPRESS_HC_STREAM, level};
    call.hcstream = &a; call.hc_ws = s.d_ws.p; call.hc_span = im.total;
    if (!sh.run(call, s, m.l)) return false;
    memcpy(h.out + b0, m.out.in(hm), m.out.bytes());
    if (!sh.hand_back_produced(s, b0, ck.b1, ck.dst, dso, h.dst, h.dst_off, h.dst_cap, h.out)) return false;
    memcpy(h.state + c, im.after.data(), (size_t)nc * sizeof(staging::HcsState));
    return true;
  });
}
// the argument errors of such a call that can be seen without a device
const char* hcstream_arg_error(const HcStreamHost& h) {
  if (h.n_chains == 0 && h.n_blocks == 0) return nullptr;
  if (!h.state || !h.src || !h.src_off || !h.src_len || !h.chain_first || !h.dst || !h.dst_off || !h.dst_cap || !h.out) return kNullArg;
  return staging::hcstream_shape_error((const staging::HcsState*)h.state, h.chain_first, h.n_chains, h.n_blocks, h.src_len);
}

// ---- resident streams whose sources land anywhere, on the host-pointer path ----
// the caller's HOST arrays of lz4hip_compress_fast_stream_ext_batch
struct CXStreamHost {
  const uint8_t* src; const uint64_t* src_off; const int32_t* src_len; const uint32_t* chain_first; const uint64_t* hist_end; const int32_t* hist_len;
  const uint64_t* win_off; const uint64_t* win_len; uint8_t* dst; const uint64_t* dst_off; const int32_t* dst_cap; int32_t* out; uint64_t* chain_consumed;
  uint32_t n_blocks, n_chains;
};
// One device's share [c0, c1) of such a call: the frame of chain_shard (chunks of 64 MiB of image or 512 MiB of slots; proto.cs_*
// and share: the share's state and slots) around the image of host_staging.h CxImage.  Per stream the used part of its window is
// mirrored: up go the sources that can run and the history pieces -- those inside a window or in front of it where they lie in the
// mirror, those apart once per chunk -- as runs (what a joined run carries between two pieces lands in mirror bytes nothing reads);
// the kernel gets every offset in device terms; the results come back, then only the bytes each block produced.
int cxstream_host_shard(const BlockCall& proto, const StreamShare& share, const CXStreamHost& h, int ord, uint32_t c0, uint32_t c1, std::string* err) {
  auto cost = [&](uint32_t c) {
    staging::DsPiece p;
    (void)staging::cxstream_piece(h.hist_end[c], h.hist_len[c], h.win_off[c], h.win_len[c], &p);
    return staging::Cost{staging::cxstream_cost(staging::cxstream_hull(h.chain_first, c, h.src_off, h.src_len, h.hist_end[c], p, h.win_off[c]), p),
                         staging::chain_packed_bytes(h.chain_first, c, h.dst_cap)};
  };
  std::vector<uint64_t> dso;
  std::vector<staging::Run> runs;
  return chain_shard(ord, h.chain_first, c0, c1, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, j = ck.j, b0 = ck.b0, nb = ck.nb, nc = ck.nc;
    const staging::CxImage im(h.chain_first, c, nc, h.src_off, h.src_len, h.hist_end, h.hist_len, h.win_off, h.win_len);
    (void)staging::packed_offsets(h.dst_cap + b0, nb, dso);
    const staging::CXStreamMeta m(nb, nc);
    if (!sh.reserve(s, im.total, true, ck.dst, m.l.total)) return false;
    uint8_t *const hs = (uint8_t*)s.h_src.p, *const ds = (uint8_t*)s.d_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    m.l.zero_results(hm);
    runs.clear();
    // (of a stream's sources only what its blocks can consume: up to the first block with a negative length.  The copies into the
    // pinned mirror run stream by stream on several threads; a stream's mirror is its own, so no two threads write one byte -- two
    // sources of ONE stream may overlap, and their bytes are the same bytes)
    par_blocks(c, j, im.total, [=, &im](uint32_t u) {
      const uint32_t t = u - c;
      for (uint32_t i = h.chain_first[u]; i < h.chain_first[u + 1] && h.src_len[i] >= 0; i++)
        if (h.src_len[i] > 0) memcpy(hs + (size_t)im.to_dev(t, h.src_off[i]), h.src + h.src_off[i], (size_t)h.src_len[i]);
      const staging::DsPiece& p = im.piece[t];
      if (p.kind == staging::DS_INSIDE || p.kind == staging::DS_LEAD) memcpy(hs + im.hist_dev[t] - p.keep, h.src + h.hist_end[u] - p.keep, (size_t)p.keep);
    });
    for (uint32_t t = 0; t < nc; t++) {
      for (uint32_t i = h.chain_first[c + t]; i < h.chain_first[c + t + 1] && h.src_len[i] >= 0; i++)
        if (h.src_len[i] > 0) runs.push_back(staging::Run{(size_t)im.to_dev(t, h.src_off[i]), (size_t)h.src_len[i]});
      const staging::DsPiece& p = im.piece[t];
      if (p.kind == staging::DS_INSIDE || p.kind == staging::DS_LEAD) runs.push_back(staging::Run{(size_t)(im.hist_dev[t] - p.keep), (size_t)p.keep});
    }
    for (const staging::DsApart& a : im.apart) {
      memcpy(hs + a.dev, h.src + a.end - a.keep, (size_t)a.keep);
      runs.push_back(staging::Run{a.dev, (size_t)a.keep});
    }
    for (uint32_t t = 0; t < nc; t++) {
      for (uint32_t i = h.chain_first[c + t]; i < h.chain_first[c + t + 1]; i++) m.src_off.in(hm)[i - b0] = im.to_dev(t, h.src_off[i]);
      m.hist_end.in(hm)[t] = im.hist_dev[t];
      m.hist_len.in(hm)[t] = (int32_t)im.piece[t].keep;
    }
    staging::stream_slots(share.ids + c, nc, share.id0, share.poisoned, m.slot.in(hm));
    memcpy(m.dst_off.in(hm), dso.data(), m.dst_off.bytes());
    memcpy(m.src_len.in(hm), h.src_len + b0, m.src_len.bytes());
    memcpy(m.dst_cap.in(hm), h.dst_cap + b0, m.dst_cap.bytes());
    staging::rebase_first(h.chain_first, c, nc, m.first.in(hm));
    // (the source goes up as runs: upload() carries the metadata alone)
    if (!sh.upload_runs(s, s.h_src, s.d_src, runs, "H2D src") || !sh.upload(s, 0, m.l, s.st)) return false;
    const lz4hip::CXStreamArgs a{{{ds, nullptr, m.hist_len.in(dm), m.src_len.in(dm), m.first.in(dm), (uint8_t*)s.d_dst.p, m.dst_off.in(dm), m.dst_cap.in(dm),
                                   m.out.in(dm), m.consumed.in(dm), nb, nc}, m.slot.in(dm), proto.cs_rec, proto.cs_tables}, m.src_off.in(dm), m.hist_end.in(dm)};
    BlockCall call = proto; call.cxstream = &a;
    if (share.launched) *share.launched = true;
    if (!sh.run(call, s, m.l)) return false;
    memcpy(h.out + b0, m.out.in(hm), m.out.bytes());
    memcpy(h.chain_consumed + c, m.consumed.in(hm), m.consumed.bytes());
    return sh.hand_back_produced(s, b0, ck.b1, ck.dst, dso, h.dst, h.dst_off, h.dst_cap, h.out);
  });
}

// hashes of one device's share [b0, b1) of a host batch: the same pinned, double-buffered staging as host_shard (chunks of
// <= CHUNK_SRC bytes packed by several host threads while the previous chunk is on the GPU), from the same pool of buffer pairs
template <class T>
int xxh_shard(bool is64, int ord, const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, T* out, uint32_t b0, uint32_t b1, std::string* err) {
  if (b1 == b0) return LZ4HIP_OK;
  ShardScope sh(ord, err);
  int& rc = sh.rc;
  if (rc) return rc;
  auto finish = [&](ChunkSlot& s) {   // the hashes of the chunk in `s`, if there is one, to the caller (waits for it)
    const staging::HashMeta<T> m(s.i1 - s.i0);
    if (s.i1 > s.i0 && sh.ok("hipEventSynchronize", hipEventSynchronize(s.done))) memcpy(out + s.i0, m.hash.in(s.h_meta.p), m.hash.bytes());
    s.i0 = s.i1 = 0;
    return rc == LZ4HIP_OK;
  };
  uint32_t i = b0;
  int k = 0;
  while (i < b1 && rc == LZ4HIP_OK) {
    ChunkSlot& s = sh.pair->slot[k];
    if (!finish(s)) break;
    const staging::Chunk ck = staging::cut_chunk(i, b1, CHUNK_BLOCKS, CHUNK_SRC, SIZE_MAX, [&](uint32_t t) { return staging::Cost{al16(pos(len[t])), 0}; });
    const uint32_t j = ck.end, nb = j - i;
    (void)staging::packed_offsets(len + i, nb, s.so);
    const staging::HashMeta<T> m(nb);
    if (!sh.reserve(s, ck.src, false, 0, m.l.total)) break;
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    par_blocks(i, j, ck.src, [=, &s](uint32_t t) { if (len[t] > 0) memcpy(hs + s.so[t - i], buf + off[t], (size_t)len[t]); });
    memcpy(m.off.in(s.h_meta.p), s.so.data(), m.off.bytes());
    memcpy(m.len.in(s.h_meta.p), len + i, m.len.bytes());
    void* dm = s.d_meta.p;
    if (!sh.upload(s, ck.src, m.l, s.st)) break;
    const int le = is64 ? lz4hip::launch_xxh64((const uint8_t*)s.d_src.p, m.off.in(dm), m.len.in(dm), seed, (uint64_t*)m.hash.in(dm), nb, s.st)
                        : lz4hip::launch_xxh32((const uint8_t*)s.d_src.p, m.off.in(dm), m.len.in(dm), (uint32_t)seed, (uint32_t*)m.hash.in(dm), nb, s.st);
    if (!sh.launched(le) || !sh.fetch_results(s, m.l, s.st) || !sh.ok("hipEventRecord", hipEventRecord(s.done, s.st))) break;
    s.i0 = i; s.i1 = j;
    i = j;
    k ^= 1;
  }
  for (int t = 0; t < 2 && rc == LZ4HIP_OK; t++) finish(sh.pair->slot[(k + t) & 1]);
  return rc;
}

template <class T>
int host_xxh(bool is64, const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, T* out, uint32_t n) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!buf || !off || !len || !out) return fail(LZ4HIP_E_ARG, kNullArg);
  return fan_out(n, 1024u, [&](int ord, uint32_t b0, uint32_t b1, std::string* err) {
    return xxh_shard<T>(is64, ord, buf, off, len, seed, out, b0, b1, err);
  });
}

// ---- single-block calls: coalesced ---------------------------------------------------------------------------------------
// The reference's API shape is one block per call from many threads (LZ4Compressor.compress, LZ4Compressor.java:59,82).  A GPU
// launch per block would serialise those threads on launch + PCIe latency, so concurrent single-block calls of the same kind are
// combined: a caller queues its request; whoever finds no batch in progress becomes the leader, takes EVERYTHING queued so far and
// runs it as one host batch; requests that arrive meanwhile form the next batch (led by one of their own callers).  A lone caller
// pays no waiting window; N concurrent callers share one launch.
struct Req {
  const uint8_t* src; int32_t len; uint8_t* dst; int32_t cap;
  int32_t out = 0; int rc = 0; bool done = false; std::string err;
  int32_t consumed = 0;   // (op_has_consumed)
};
struct Combiner {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Req*> q;
  bool leader = false;
};
// Calls are coalesced only with calls of the same operation, HC level and acceleration: one combiner per operation, HC's per level,
// accelerated compress's per (clamped) acceleration -- created on first use and kept (at most 65536 of them)
Combiner g_comb[OP_COUNT];
Combiner g_hc_comb[13];   // [HC level]
Combiner g_hc_dest_comb[13];   // [HC level]: LZ4_compress_HC_destSize, coalesced only with destSize calls of the same level
std::mutex g_accel_comb_mu;
std::map<int, Combiner> g_accel_comb;
Combiner* dict_combiner(const lz4hip_dict* d, bool compress);   // (the handle's own: single calls coalesce only with calls of the same operation on the same handle)
Combiner* dict_hc_combiner(const lz4hip_dict* d, int level);    // (the handle's own, per clamped HC level)
// nullptr: no combiner for this call (an operation or level outside the tables); may throw (the map's allocation)
Combiner* combiner_for(const BlockCall& c) {
  if (c.op == OP_DECODE_DICT || c.op == OP_COMPRESS_DICT) return c.dict ? dict_combiner(c.dict, c.op == OP_COMPRESS_DICT) : nullptr;
  if (c.op == OP_COMPRESS_HC_DICT) return c.dict && c.param >= 1 && c.param <= 12 ? dict_hc_combiner(c.dict, c.param) : nullptr;
  if (c.op == OP_COMPRESS_ACCEL) {
    std::lock_guard<std::mutex> lk(g_accel_comb_mu);
    return &g_accel_comb[c.param];   // (std::map: references stay valid while other entries are added)
  }
  if (c.op == OP_COMPRESS_HC) return c.param >= 1 && c.param <= 12 ? &g_hc_comb[c.param] : nullptr;
  if (c.op == OP_COMPRESS_HC_DEST) return c.param >= 1 && c.param <= 12 ? &g_hc_dest_comb[c.param] : nullptr;
  return (int)c.op >= 0 && (int)c.op < OP_COUNT ? &g_comb[c.op] : nullptr;
}

// one host batch for all of `batch`; returns its rc (every request gets its out[]); may throw (allocation of the index vectors,
// thread creation inside host_batch)
int run_batch_once(const BlockCall& c, const std::vector<Req*>& batch) {
  static uint8_t dummy_in = 0, dummy_out = 0;
  const uint32_t n = (uint32_t)batch.size();
  const uint8_t* sbase = nullptr; uint8_t* dbase = nullptr;
  for (Req* r : batch) {
    if (!r->src) r->src = &dummy_in;
    if (!r->dst) r->dst = &dummy_out;
    if (!sbase || r->src < sbase) sbase = r->src;
    if (!dbase || r->dst < dbase) dbase = r->dst;
  }
  std::vector<uint64_t> so(n), dof(n);
  std::vector<int32_t> sl(n), dc(n), out(n, 0), cons(op_has_consumed(c.op) ? n : 0u, 0);
  for (uint32_t i = 0; i < n; i++) { so[i] = (uint64_t)(batch[i]->src - sbase); dof[i] = (uint64_t)(batch[i]->dst - dbase); sl[i] = batch[i]->len; dc[i] = batch[i]->cap; }
  BlockCall bc = c;   // (the leader's call: the batch's consumed sizes go to the requests, not to the leader's caller)
  bc.consumed = cons.data();
  const int rc = host_batch(bc, sbase, so.data(), sl.data(), dbase, dof.data(), dc.data(), out.data(), n);
  for (uint32_t i = 0; i < n; i++) {
    batch[i]->rc = rc; batch[i]->out = out[i]; if (rc) batch[i]->err = g_err;
    if (op_has_consumed(c.op)) batch[i]->consumed = cons[i];
  }
  return rc;
}

// Combined callers do not share a fate: when the shared batch fails as a whole (staging could not be allocated because of ONE
// caller's huge block, a HIP error) every request is run again on its own, so only the caller whose request is the cause sees
// the failure.  Exceptions (bad_alloc of the index vectors, system_error from thread creation) become LZ4HIP_E_NOMEM for the
// requests concerned; nothing propagates into the leader's bookkeeping.
void run_combined(const BlockCall& c, std::vector<Req*>& batch) noexcept {
  int rc;
  try { rc = run_batch_once(c, batch); }
  catch (...) { rc = LZ4HIP_E_NOMEM; for (Req* r : batch) { r->rc = rc; r->out = 0; r->err = "out of memory while combining single-block calls"; } }
  if (rc == 0 || batch.size() < 2) return;
  for (Req* r : batch) {
    std::vector<Req*> one;
    try { one.push_back(r); (void)run_batch_once(c, one); }
    catch (...) { r->rc = LZ4HIP_E_NOMEM; r->out = 0; r->err = "out of memory"; }
  }
}

// c.consumed: where this caller's consumed size goes (op_has_consumed; written only on success)
int single(const BlockCall& c, const uint8_t* src, int src_len, uint8_t* dst, int dst_cap) {
  Req r{src, src_len, dst, dst_cap};
  Combiner* cp;
  try { cp = combiner_for(c); }
  catch (...) { return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  if (!cp) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, "no combiner for this operation"));
  Combiner& cb = *cp;
  {
    std::unique_lock<std::mutex> lk(cb.mu);
    try { cb.q.push_back(&r); }
    catch (...) { return fail(LZ4HIP_E_NOMEM, "out of memory"); }
    while (!r.done) {
      if (!cb.leader) {
        cb.leader = true;
        std::vector<Req*> batch;
        batch.swap(cb.q);          // (contains r: only a leader takes requests out of the queue; swap does not throw)
        lk.unlock();
        run_combined(c, batch);   // noexcept: the leader always comes back to hand the results out
        lk.lock();
        for (Req* x : batch) x->done = true;
        cb.leader = false;
        cb.cv.notify_all();
      } else {
        cb.cv.wait(lk);
      }
    }
  }
  if (r.rc) { g_err = r.err; return LZ4HIP_LIB_ERROR(r.rc); }
  if (c.consumed) *c.consumed = r.consumed;
  return r.out;
}

}  // namespace

// ---- dictionary handles (LZ4_decompress_safe_usingDict, LZ4_loadDict + LZ4_compress_fast_continue) ------------------------------------------------------------------------------
// The true length (liblz4's offset check needs it while it is below 64 KB) and the last 64 KB, which is all a decoder can reach; a
// copy of those bytes on every initialised device, made by lz4hip_dict_create, or on a device's first use where the engine was
// initialised (again) later.  The handle is immutable after creation: any number of threads may decode against it.
// A compressor also needs the table LZ4_loadDict leaves (32 KB, lz4hip::launch_dict_image): built per device at the handle's first
// compress there, never for a handle that only decodes, and freed with the handle.  The HC compressor's image (the head table and
// the chain deltas LZ4_loadDictHC leaves: 128 KB + 2 bytes per kept byte, lz4hip::launch_hc_dict_image) likewise, at the first HC
// compress; the two images are independent.
struct lz4hip_dict {
  int32_t len = 0;               // the dictionary's true length
  std::vector<uint8_t> tail;     // its last min(len, 65536) bytes
  std::mutex mu;                 // guards dev[]
  uint8_t* dev[64] = {};         // [HIP ordinal]: the tail in device memory
  void* image[64] = {};          // [HIP ordinal]: the compressor's table image (only where dict_keep(len) > 0, from the first compress on)
  Combiner comb;                 // single decode calls on this handle
  Combiner comb_c;               // single compress calls on this handle
  void* hc_image[64] = {};       // [HIP ordinal]: the HC compressor's image (from the first HC compress on)
  Combiner comb_hc[13];          // [HC level]: single HC compress calls on this handle
};
namespace {
Combiner* dict_combiner(const lz4hip_dict* d, bool compress) {
  lz4hip_dict* m = const_cast<lz4hip_dict*>(d);
  return compress ? &m->comb_c : &m->comb;
}
Combiner* dict_hc_combiner(const lz4hip_dict* d, int level) { return &const_cast<lz4hip_dict*>(d)->comb_hc[level]; }
int dict_upload(lz4hip_dict* d, int ord) {   // (d->mu held or the handle not yet published; the device is current)
  if (d->dev[ord] || d->tail.empty()) return LZ4HIP_OK;
  uint8_t* p = nullptr;
  if (hipMalloc((void**)&p, d->tail.size()) != hipSuccess) return fail(LZ4HIP_E_NOMEM, "hipMalloc of the dictionary failed");
  const hipError_t e = hipMemcpy(p, d->tail.data(), d->tail.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p); return fail(LZ4HIP_E_HIP, "dictionary upload", e); }
  d->dev[ord] = p;
  return LZ4HIP_OK;
}
int dict_resident(const lz4hip_dict* cd, const uint8_t** dict_end, int32_t* dict_len) {
  lz4hip_dict* d = const_cast<lz4hip_dict*>(cd);
  int ord = -1;
  if (hipGetDevice(&ord) != hipSuccess || ord < 0 || ord >= 64) return fail(LZ4HIP_E_HIP, "hipGetDevice failed");
  *dict_len = d->len;
  *dict_end = nullptr;
  if (d->tail.empty()) return LZ4HIP_OK;
  std::lock_guard<std::mutex> lk(d->mu);
  const int rc = dict_upload(d, ord);
  if (rc) return rc;
  *dict_end = d->dev[ord] + d->tail.size();
  return LZ4HIP_OK;
}
int dict_compress_state(const lz4hip_dict* cd, hipStream_t st, const uint8_t** dict_end, int32_t* keep, const void** image) {
  lz4hip_dict* d = const_cast<lz4hip_dict*>(cd);
  int ord = -1;
  if (hipGetDevice(&ord) != hipSuccess || ord < 0 || ord >= 64) return fail(LZ4HIP_E_HIP, "hipGetDevice failed");
  *keep = (int32_t)lz4hip::dict_keep(d->len);
  *dict_end = nullptr;
  *image = nullptr;
  if (*keep == 0) return LZ4HIP_OK;   // (under 8 bytes: LZ4_loadDict loads nothing)
  std::lock_guard<std::mutex> lk(d->mu);
  const int rc = dict_upload(d, ord);
  if (rc) return rc;
  if (!d->image[ord]) {
    void* p = nullptr;
    if (hipMalloc(&p, lz4hip::kDictImageBytes) != hipSuccess) return fail(LZ4HIP_E_NOMEM, "hipMalloc of the dictionary's table image failed");
    const int le = lz4hip::launch_dict_image(d->dev[ord] + (d->tail.size() - (size_t)*keep), *keep, p, st);
    const hipError_t e = le ? (hipError_t)le : hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(p); return fail(LZ4HIP_E_HIP, "dictionary table image", e); }
    d->image[ord] = p;
  }
  *dict_end = d->dev[ord] + d->tail.size();
  *image = d->image[ord];
  return LZ4HIP_OK;
}
int dict_hc_state(const lz4hip_dict* cd, hipStream_t st, const uint8_t** dict_end, uint32_t* keep, const void** image) {
  lz4hip_dict* d = const_cast<lz4hip_dict*>(cd);
  int ord = -1;
  if (hipGetDevice(&ord) != hipSuccess || ord < 0 || ord >= 64) return fail(LZ4HIP_E_HIP, "hipGetDevice failed");
  *keep = lz4hip::hc_dict_keep(d->len);   // (= tail.size(): LZ4_loadDictHC has no minimum length)
  *dict_end = nullptr;
  *image = nullptr;
  std::lock_guard<std::mutex> lk(d->mu);
  const int rc = dict_upload(d, ord);
  if (rc) return rc;
  if (!d->hc_image[ord]) {   // (also for an empty dictionary: the record's build starts from the image's -- empty -- head table)
    void* p = nullptr;
    if (hipMalloc(&p, lz4hip::hc_dict_image_bytes(*keep)) != hipSuccess) return fail(LZ4HIP_E_NOMEM, "hipMalloc of the dictionary's HC image failed");
    const int le = lz4hip::launch_hc_dict_image(d->dev[ord], *keep, p, st);
    const hipError_t e = le ? (hipError_t)le : hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(p); return fail(LZ4HIP_E_HIP, "dictionary HC image", e); }
    d->hc_image[ord] = p;
  }
  if (*keep) *dict_end = d->dev[ord] + d->tail.size();
  *image = d->hc_image[ord];
  return LZ4HIP_OK;
}
}  // namespace

// ---- device-side container assembly (container.hip launch_container_blocks) ------------------------------------------------------
namespace {
struct ContainerPlan { size_t cws, hcws, qwords, total; uint32_t n; };
// the largest CU count of any visible device: what a workspace must be sized for when the device is not known yet
uint32_t max_cu_count() {
  static std::atomic<uint32_t> cached{0};
  uint32_t v = cached.load(std::memory_order_relaxed);
  if (v) return v;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  for (int d = 0; d < n; d++) {
    int c = 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && (uint32_t)c > v) v = (uint32_t)c;
  }
  if (!v) v = 256;
  cached.store(v, std::memory_order_relaxed);
  return v;
}
// cus: the CU count the launch will use (device_cus() under the DeviceGuard of the launch device) or max_cu_count() for a query
ContainerPlan container_plan(uint64_t n_bytes, uint32_t block_size, int hc_lv, uint32_t cus) {
  ContainerPlan p{};
  p.n = (uint32_t)((n_bytes + block_size - 1u) / block_size);
  p.cws = (lz4hip::container_ws_bytes(n_bytes, block_size) + 255u) & ~(size_t)255u;
  p.hcws = hc_lv > 0 ? ((lz4hip::hc_ws_bytes(n_bytes, p.n, hc_lv) + 255u) & ~(size_t)255u) : 0u;
  p.qwords = 3u + (size_t)p.n + lz4hip::compress_fast_v2w_scratch_words(cus);
  p.total = p.cws + p.hcws + p.qwords * sizeof(uint32_t) + 256u;
  return p;
}
int container_args(int kind, uint64_t n_bytes, uint32_t block_size, int level, int* hc_lv) {
  *hc_lv = 0;
  if (kind != 0 && kind != 1) return fail(LZ4HIP_E_ARG, "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)");
  if (block_size < 64u || block_size > (32u << 20)) return fail(LZ4HIP_E_ARG, "block size must be 64 .. 32 MiB");   // LZ4BlockOutputStream.java:50-51
  if (n_bytes / block_size >= 0x7FFFFFFFull) return fail(LZ4HIP_E_ARG, "too many blocks");
  if (level != 0 && hc_level(level, hc_lv)) return fail(LZ4HIP_E_UNSUPPORTED, "unsupported compression level");
  return 0;
}
// the launch both container entries make: `ws` = p.total bytes of device scratch, cut up as container_plan says; the launch device is current
int launch_container(int kind, int flags, int hc_lv, const uint8_t* src, uint64_t n_bytes, uint32_t block_size, uint8_t* dst, uint64_t dst_cap,
                     uint64_t* total_dev, void* ws, const ContainerPlan& p, void* stream) {
  uint8_t* w = (uint8_t*)(((uintptr_t)ws + 255u) & ~(uintptr_t)255u);
  return lz4hip::launch_container_blocks(kind, flags & 1, hc_lv, src, n_bytes, block_size, dst, dst_cap, (unsigned long long*)total_dev, w,
                                         p.hcws ? w + p.cws : nullptr, (uint32_t*)(w + p.cws + p.hcws),
                                         64u * (uint32_t)g_compress_switch.load(std::memory_order_relaxed), lz4hip::device_cus(),
                                         g_compress_core.load(std::memory_order_relaxed), stream);
}
}  // namespace

extern "C" {
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
size_t lz4hip_container_workspace_bytes(uint64_t n_bytes, uint32_t block_size, int level) {
  int lv = 0;
  if (ensure_init() || block_size < 64u || (level != 0 && hc_level(level, &lv))) return 0;
  return container_plan(n_bytes, block_size, lv, max_cu_count()).total;   // (enough for whichever device the launch names)
}
int lz4hip_container_blocks_dev(int kind, int flags, int level, const uint8_t* src, uint64_t n_bytes, uint32_t block_size, uint8_t* dst, uint64_t dst_cap,
                                uint64_t* total_dev, void* ws, size_t ws_bytes, int device, void* stream) {
  int rc = need_device();
  if (rc) return rc;   // (the answer without a device, whatever the arguments)
  int lv;
  if ((rc = container_args(kind, n_bytes, block_size, level, &lv)) != 0) return rc;
  return on_device(device, false, (n_bytes && !src) || !dst || !total_dev || !ws ? kNullArg : nullptr, [&] {
    // (on the launch device: the plan's ring words are a function of ITS CU count)
    const ContainerPlan p = container_plan(n_bytes, block_size, lv, lz4hip::device_cus());
    if (ws_bytes < p.total) return fail(LZ4HIP_E_ARG, "container workspace too small (lz4hip_container_workspace_bytes)");
    return launch_container(kind, flags, lv, src, n_bytes, block_size, dst, dst_cap, total_dev, ws, p, stream);
  });
}
int lz4hip_container_blocks(int kind, int flags, int level, const uint8_t* src, uint64_t n_bytes, uint32_t block_size, uint8_t* dst, uint64_t dst_cap,
                            uint64_t* out_bytes) {
  int rc = need_device();
  if (rc) return rc;
  int lv;
  if ((rc = container_args(kind, n_bytes, block_size, level, &lv)) != 0) return rc;
  if ((n_bytes && !src) || !dst || !out_bytes) return fail(LZ4HIP_E_ARG, kNullArg);
  *out_bytes = 0;
  if (n_bytes == 0) return LZ4HIP_OK;
  int ord;
  if (ordinal(0, &ord)) return fail(LZ4HIP_E_NO_DEVICE, "no device");
  DeviceGuard g(ord);
  const ContainerPlan p = container_plan(n_bytes, block_size, lv, lz4hip::device_cus());
  const uint64_t worst = n_bytes + (uint64_t)p.n * (kind == 0 ? 8u : 21u);
  hipStream_t st = nullptr;
  uint8_t *d_src = nullptr, *d_dst = nullptr, *d_ws = nullptr;
  uint64_t* d_total = nullptr;
  hipError_t he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  auto done = [&](int r) {
    if (d_src) (void)hipFreeAsync(d_src, st);
    if (d_dst) (void)hipFreeAsync(d_dst, st);
    if (d_ws) (void)hipFreeAsync(d_ws, st);
    if (d_total) (void)hipFreeAsync(d_total, st);
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    return r;
  };
  if (he != hipSuccess) return fail(LZ4HIP_E_HIP, "hipStreamCreate", he);
  if ((he = hipMallocAsync((void**)&d_src, n_bytes, st)) != hipSuccess || (he = hipMallocAsync((void**)&d_dst, worst, st)) != hipSuccess ||
      (he = hipMallocAsync((void**)&d_ws, p.total, st)) != hipSuccess || (he = hipMallocAsync((void**)&d_total, 8, st)) != hipSuccess)
    return done(fail(he == hipErrorOutOfMemory ? LZ4HIP_E_NOMEM : LZ4HIP_E_HIP, "device allocation", he));
  if ((he = hipMemcpyAsync(d_src, src, n_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "H2D", he));
  const int e = launch_container(kind, flags, lv, d_src, n_bytes, block_size, d_dst, worst, d_total, d_ws, p, st);
  if (e) return done(fail(LZ4HIP_E_HIP, "kernel launch", (hipError_t)e));
  uint64_t total = 0;
  if ((he = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st)) != hipSuccess || (he = hipStreamSynchronize(st)) != hipSuccess)
    return done(fail(LZ4HIP_E_HIP, "container size", he));
  if (total > dst_cap) return done(fail(LZ4HIP_E_ARG, "destination too small for the container blocks"));
  if (total && (he = hipMemcpyAsync(dst, d_dst, total, hipMemcpyDeviceToHost, st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "D2H", he));
  if ((he = hipStreamSynchronize(st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "hipStreamSynchronize", he));
  *out_bytes = total;
  return done(LZ4HIP_OK);
}
size_t lz4hip_container_decode_workspace_bytes(uint32_t n_max) { return lz4hip::container_read_ws_bytes(n_max) + 256u; }
int lz4hip_container_decode_dev(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint8_t* dst, uint64_t slot_bytes,
                                uint32_t n_max, int32_t* sizes_dev, uint64_t* info_dev, void* ws, size_t ws_bytes, int device, void* stream) {
  const char* arg_error =
      (kind != 0 && kind != 1) ? "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)"
      : ((body_bytes && !body) || !dst || !sizes_dev || !info_dev || !ws) ? kNullArg
      : (n_max == 0 || n_max > 0x7FFFFFFFu) ? "n_max must be 1 .. 2^31 - 1"
      : (slot_bytes == 0 || slot_bytes > 0x7FFFFFFFull || (kind == 0 && (max_block == 0 || slot_bytes < max_block)))
          ? "slot_bytes must be 1 .. 2^31 - 1 and, for frame blocks, at least the frame's block maximum size"
      : ws_bytes < lz4hip_container_decode_workspace_bytes(n_max) ? "workspace too small (lz4hip_container_decode_workspace_bytes)"
      : nullptr;
  return on_device(device, false, arg_error, [&] {
    uint8_t* w = (uint8_t*)(((uintptr_t)ws + 255u) & ~(uintptr_t)255u);
    return lz4hip::launch_container_read(kind, flags & 1, body, body_bytes, max_block, dst, slot_bytes, n_max, sizes_dev,
                                         (unsigned long long*)info_dev, w, stream);
  });
}
// Host-side walk of the size words / headers of a container body IN HOST MEMORY (no device work, no decoding): how many whole blocks
// of the first n_max the body holds, how many bytes their decoded forms can need at most (frame: max_block per compressed block, the
// stored size of a raw one; LZ4Block: the header's original length) and
// the largest of those bounds (incl. the block the walk stopped at, when its header is readable).  It follows the device walk's
// positions (container_walk_kernel) and stops where that stops.  What it is for (round-4 advisor): lz4hip_container_decode sized its
// device slots -- and its callers their destination -- by max_block x n_max whatever the body held: 256 MiB for a 100-byte frame,
// gigabytes for a 21-byte LZ4Block header with level nibble 15.
static void container_prewalk(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint32_t n_max,
                              uint32_t* n_blocks, uint64_t* dst_bytes, uint64_t* slot_max) {
  auto rd32 = [](const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
  uint64_t p = 0, total = 0, smax = 0;
  uint32_t k = 0;
  while (k < n_max && p < body_bytes) {
    uint64_t need, bound;
    if (kind == 0) {
      if (p + 4u > body_bytes) break;
      const uint32_t word = rd32(body + p), size = word & 0x7FFFFFFFu;
      if (size == 0u || size > max_block) break;
      bound = (word & 0x80000000u) ? size : max_block;   // (a compressed block decodes into max_block bytes of capacity, as in the reference: a smaller one could change which check a damaged stream fails first)
      need = 4ull + size + ((flags & 1) ? 4u : 0u);
    } else {
      if (p + 21u > body_bytes) break;
      const uint8_t* h = body + p;
      if (memcmp(h, "LZ4Block", 8) != 0) break;
      const uint32_t method = h[8] & 0xF0u, level = 10u + (h[8] & 0x0Fu);
      const int32_t clen = (int32_t)rd32(h + 9), olen = (int32_t)rd32(h + 13);
      if ((method != 0x10u && method != 0x20u) || olen > (int32_t)(1u << level) || olen <= 0 || clen <= 0 || (method == 0x10u && olen != clen)) break;
      // (round-5 advisor) the device walk stops at a block bigger than the caller's max_block (CR_BLOCK_TOO_BIG: the readers take the
      // host walk, which allocates one block at a time like LZ4BlockInputStream.java:236-253), at a block whose payload is cut short
      // (CR_TRUNCATED) and at a header that announces more than its compressed bytes can decode to -- clen bytes of LZ4 are at most
      // 255 x clen bytes (CR_CORRUPT: the reference's decompressor would fail on it) -- in that order, and none of the three sizes a
      // slot.  Without these rules 256 headers {level nibble 15, olen 32 MiB, clen 1} -- 5 KB of input -- sized 8 GiB of device slots
      // and 8 GiB of destination before block 0 was found corrupt
      if ((uint64_t)olen > max_block) break;
      bound = (uint64_t)olen;
      need = 21ull + (uint64_t)clen;
      if (p + need > body_bytes) break;
      if (method == 0x20u && bound > 255ull * (uint64_t)clen + 64u) break;
    }
    if (bound > smax) smax = bound;             // (frames: also for a block whose payload is cut short: the device walk looks at it)
    if (p + need > body_bytes) break;
    total += bound; p += need; k++;
  }
  *n_blocks = k; *dst_bytes = total; *slot_max = smax;
}
int lz4hip_container_decode_bound(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint32_t n_max,
                                  uint32_t* n_blocks, uint64_t* dst_bytes) {
  if (kind != 0 && kind != 1) return fail(LZ4HIP_E_ARG, "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)");
  if ((body_bytes && !body) || !n_blocks || !dst_bytes) return fail(LZ4HIP_E_ARG, kNullArg);
  if (n_max == 0 || n_max > 0x7FFFFFFFu || max_block == 0 || max_block > 0x7FFFFFFFu) return fail(LZ4HIP_E_ARG, "n_max and max_block must be 1 .. 2^31 - 1");
  uint64_t smax = 0;
  container_prewalk(kind, flags, body, body_bytes, max_block, n_max, n_blocks, dst_bytes, &smax);
  return LZ4HIP_OK;
}
// host pointers: H2D of the container bytes, the device path above, D2H of the delivered blocks back to back into dst
int lz4hip_container_decode(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint32_t n_max, uint8_t* dst,
                            uint64_t dst_cap, int32_t* sizes, uint64_t* info) {
  if (const int rc = need_device()) return rc;
  if (kind != 0 && kind != 1) return fail(LZ4HIP_E_ARG, "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)");
  if ((body_bytes && !body) || !sizes || !info || (dst_cap && !dst)) return fail(LZ4HIP_E_ARG, kNullArg);
  if (n_max == 0 || n_max > 0x7FFFFFFFu || max_block == 0 || max_block > 0x7FFFFFFFu) return fail(LZ4HIP_E_ARG, "n_max and max_block must be 1 .. 2^31 - 1");
  for (int i = 0; i < 5; i++) info[i] = 0;
  int ord;
  if (ordinal(0, &ord)) return fail(LZ4HIP_E_NO_DEVICE, "no device");
  DeviceGuard g(ord);
  // slots and their number by what the body holds, not by what the caller allows: one slot more than the whole blocks present (the
  // device walk finds out why the run ends there), each as big as the largest decoded block can be
  uint64_t slot_need;
  {
    uint32_t nb = 0; uint64_t db = 0, smax = 0;
    container_prewalk(kind, flags, body, body_bytes, max_block, n_max, &nb, &db, &smax);
    if (nb + 1u < n_max) n_max = nb + 1u;
    slot_need = smax ? smax : 1u;
  }
  const size_t wsb = lz4hip_container_decode_workspace_bytes(n_max);
  const uint64_t slot = (slot_need + 63u) & ~63ull;
  hipStream_t st = nullptr;
  uint8_t *d_body = nullptr, *d_dst = nullptr, *d_ws = nullptr;
  int32_t* d_sizes = nullptr;
  uint64_t* d_info = nullptr;
  hipError_t he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  auto done = [&](int r) {
    if (d_body) (void)hipFreeAsync(d_body, st);
    if (d_dst) (void)hipFreeAsync(d_dst, st);
    if (d_ws) (void)hipFreeAsync(d_ws, st);
    if (d_sizes) (void)hipFreeAsync(d_sizes, st);
    if (d_info) (void)hipFreeAsync(d_info, st);
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    return r;
  };
  if (he != hipSuccess) return fail(LZ4HIP_E_HIP, "hipStreamCreate", he);
  if ((he = hipMallocAsync((void**)&d_body, body_bytes ? body_bytes : 1, st)) != hipSuccess || (he = hipMallocAsync((void**)&d_dst, slot * n_max, st)) != hipSuccess ||
      (he = hipMallocAsync((void**)&d_ws, wsb, st)) != hipSuccess || (he = hipMallocAsync((void**)&d_sizes, sizeof(int32_t) * (size_t)n_max, st)) != hipSuccess ||
      (he = hipMallocAsync((void**)&d_info, 5 * sizeof(uint64_t), st)) != hipSuccess)
    return done(fail(he == hipErrorOutOfMemory ? LZ4HIP_E_NOMEM : LZ4HIP_E_HIP, "device allocation", he));
  if (body_bytes && (he = hipMemcpyAsync(d_body, body, body_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "H2D", he));
  uint8_t* w = (uint8_t*)(((uintptr_t)d_ws + 255u) & ~(uintptr_t)255u);
  const int e = lz4hip::launch_container_read(kind, flags & 1, d_body, body_bytes, max_block, d_dst, slot, n_max, d_sizes, (unsigned long long*)d_info, w, st);
  if (e) return done(fail(LZ4HIP_E_HIP, "kernel launch", (hipError_t)e));
  if ((he = hipMemcpyAsync(info, d_info, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (he = hipMemcpyAsync(sizes, d_sizes, sizeof(int32_t) * (size_t)n_max, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (he = hipStreamSynchronize(st)) != hipSuccess)
    return done(fail(LZ4HIP_E_HIP, "container result", he));
  const uint64_t n_ok = info[0];
  if (info[3] > dst_cap) return done(fail(LZ4HIP_E_ARG, "destination too small for the decoded blocks"));
  // runs of full slots go back in one copy each (the usual case: every block but the last is a whole block)
  uint64_t o = 0;
  for (uint64_t k = 0; k < n_ok;) {
    uint64_t j = k;
    while (j < n_ok && (uint64_t)sizes[j] == slot) j++;
    if (j > k) {
      if ((he = hipMemcpyAsync(dst + o, d_dst + k * slot, (j - k) * slot, hipMemcpyDeviceToHost, st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "D2H", he));
      o += (j - k) * slot; k = j;
    } else {
      const uint64_t sz = sizes[k] > 0 ? (uint64_t)sizes[k] : 0;
      if (sz && (he = hipMemcpyAsync(dst + o, d_dst + k * slot, sz, hipMemcpyDeviceToHost, st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "D2H", he));
      o += sz; k++;
    }
  }
  if ((he = hipStreamSynchronize(st)) != hipSuccess) return done(fail(LZ4HIP_E_HIP, "hipStreamSynchronize", he));
  return done(LZ4HIP_OK);
}

// ---- many containers per call ----
// what can be said about the items of a many-call without a device -> a message, or nullptr
static const char* container_many_arg_error(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len, const uint32_t* max_block,
                                            const uint8_t* flags, uint32_t n_items, uint32_t n_max) {
  if (kind != 0 && kind != 1) return "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)";
  if (n_items && (!body_off || !body_len || !max_block || !flags)) return kNullArg;
  for (uint32_t c = 0; c < n_items; c++) if (body_len[c] && !bodies) return kNullArg;
  if (n_max == 0 || n_max > 0x7FFFFFFFu) return "n_max and max_block must be 1 .. 2^31 - 1";
  for (uint32_t c = 0; c < n_items; c++) if (max_block[c] == 0 || max_block[c] > 0x7FFFFFFFu) return "n_max and max_block must be 1 .. 2^31 - 1";
  for (uint32_t c = 0; c < n_items; c++) if (flags[c] & ~1u) return "container flags: only bit 0 (block checksums) is defined";
  return nullptr;
}
// the host pre-walk of item c (container_rules.h, the step the device walk compiles): container_prewalk's numbers
static lz4hip::container_rules::Walk container_many_prewalk(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len,
                                                            const uint32_t* max_block, const uint8_t* flags, uint32_t c, uint32_t n_max) {
  return lz4hip::container_rules::walk(body_len[c] ? bodies + body_off[c] : nullptr, body_len[c], kind, flags[c], max_block[c], UINT64_MAX, n_max, nullptr);
}
int lz4hip_container_decode_many_bound(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len, const uint32_t* max_block,
                                       const uint8_t* flags, uint32_t n_items, uint32_t n_max, uint32_t* item_blocks, uint64_t* item_dst_bytes) {
  if (const char* why = container_many_arg_error(kind, bodies, body_off, body_len, max_block, flags, n_items, n_max)) return fail(LZ4HIP_E_ARG, why);
  if (n_items && (!item_blocks || !item_dst_bytes)) return fail(LZ4HIP_E_ARG, kNullArg);
  for (uint32_t c = 0; c < n_items; c++) {
    const auto w = container_many_prewalk(kind, bodies, body_off, body_len, max_block, flags, c, n_max);
    item_blocks[c] = w.blocks; item_dst_bytes[c] = w.dst_bytes;
  }
  return LZ4HIP_OK;
}
// The items of a many-call through the shared staging, a group at a time (chain_shard: an item is its unit, the entries it owns in the
// batch arrays -- first[] -- are its "blocks"): a group is the items whose bodies fit LZ4HIP_HOST_CHUNK_MB MiB and whose slots fit 512
// MiB, one item at least.  Item c has nb[c] slots of slot[c] bytes, as lz4hip_container_decode gives that body.  A group costs one
// upload of the packed bodies and the item arrays, one launch sequence, one copy of the results and one of the delivered bytes, which
// the device has packed back to back.
static int container_many_shard(int ord, int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len, const uint32_t* max_block,
                                const uint8_t* flags, uint32_t n_items, uint32_t n_max, const uint32_t* nb, const uint32_t* slot, const uint32_t* first,
                                uint8_t* dst, uint64_t* item_dst_off, uint32_t* item_first, int32_t* sizes, uint64_t* info, std::string* err) {
  auto cost = [&](uint32_t c) { return staging::Cost{al16((size_t)body_len[c]), (size_t)nb[c] * slot[c]}; };
  uint64_t out_bytes = 0;
  uint32_t out_blocks = 0;
  std::vector<uint64_t> so;
  return chain_shard(ord, first, 0, n_items, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, nc = ck.nc, ne = ck.nb;
    const staging::ContainerManyMeta m(nc, ne);
    if (!sh.reserve(s, ck.src, true, ck.dst, m.l.total)) return false;
    if (!sh.ok("staging allocation", s.d_ws.reserve(lz4hip::container_many_ws_bytes(ne, nc) + 256u)) || !sh.ok("staging allocation", s.d_pack.reserve(ck.dst + 64u))) return false;
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    so.resize(nc);
    bool any_cks = false;
    { size_t o = 0, d = 0;
      for (uint32_t t = 0; t < nc; t++) {
        so[t] = o; o += al16((size_t)body_len[c + t]);
        m.body_off.in(hm)[t] = so[t]; m.body_len.in(hm)[t] = body_len[c + t]; m.dst_base.in(hm)[t] = d; d += (uint64_t)nb[c + t] * slot[c + t];
        m.slot.in(hm)[t] = slot[c + t]; m.max_block.in(hm)[t] = max_block[c + t]; m.flags.in(hm)[t] = flags[c + t];
        any_cks |= (flags[c + t] & 1u) != 0u;
      } }
    staging::rebase_first(first, c, nc, m.first.in(hm));
    par_blocks(c, ck.j, ck.src, [=, &so](uint32_t t) { if (body_len[t]) memcpy(hs + so[t - c], bodies + body_off[t], (size_t)body_len[t]); });
    if (!sh.upload(s, ck.src, m.l, s.st)) return false;
    const lz4hip::ContainerManyItems items{m.body_off.in(dm), m.body_len.in(dm), m.dst_base.in(dm), m.slot.in(dm), m.max_block.in(dm), m.first.in(dm), m.flags.in(dm)};
    if (!sh.launched(lz4hip::launch_container_read_many(kind, any_cks, (const uint8_t*)s.d_src.p, items, nc, ne, n_max, (uint8_t*)s.d_dst.p, (uint8_t*)s.d_pack.p,
                                                        m.sizes.in(dm), (unsigned long long*)m.info.in(dm), m.item_first.in(dm),
                                                        (unsigned long long*)m.item_dst_off.in(dm), s.d_ws.p, s.st)))
      return false;
    if (!sh.fetch_results(s, m.l, s.st) || !sh.wait(s.st)) return false;
    const uint64_t* const ido = m.item_dst_off.in(hm);
    const uint32_t* const ifi = m.item_first.in(hm);
    const uint64_t total = ido[nc];
    if (total > ck.dst || ifi[nc] > ne) { *sh.err = "container read: the device delivered more than the bodies can hold"; sh.rc = LZ4HIP_E_HIP; return false; }
    if (total) {
      if (!sh.ok("D2H dst", hipMemcpyAsync(s.h_dst.p, s.d_pack.p, (size_t)total, hipMemcpyDeviceToHost, s.st)) || !sh.wait(s.st)) return false;
      memcpy(dst + out_bytes, s.h_dst.p, (size_t)total);
    }
    memcpy(info + 5u * (size_t)c, m.info.in(hm), 5u * (size_t)nc * sizeof(uint64_t));
    if (ifi[nc]) memcpy(sizes + out_blocks, m.sizes.in(hm), (size_t)ifi[nc] * sizeof(int32_t));
    for (uint32_t t = 0; t <= nc; t++) { item_dst_off[c + t] = out_bytes + ido[t]; item_first[c + t] = out_blocks + ifi[t]; }
    out_bytes += total; out_blocks += ifi[nc];
    return true;
  });
}
int lz4hip_container_decode_many(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len, const uint32_t* max_block,
                                 const uint8_t* flags, uint32_t n_items, uint32_t n_max, uint8_t* dst, uint64_t dst_cap, uint64_t* item_dst_off,
                                 uint32_t* item_first, int32_t* sizes, uint32_t sizes_cap, uint64_t* info) {
  if (kind != 0 && kind != 1) return fail(LZ4HIP_E_ARG, "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)");
  if (!item_dst_off || !item_first || (n_items && !info) || (dst_cap && !dst) || (sizes_cap && !sizes)) return fail(LZ4HIP_E_ARG, kNullArg);
  if (const char* why = container_many_arg_error(kind, bodies, body_off, body_len, max_block, flags, n_items, n_max)) return fail(LZ4HIP_E_ARG, why);
  item_dst_off[0] = 0; item_first[0] = 0;
  if (n_items == 0) return LZ4HIP_OK;
  // slots and their number by what each body holds (lz4hip_container_decode): one entry more than the whole blocks present, where the
  // device walk finds out why the run ends; each slot as big as the item's largest decoded block can be
  std::vector<uint32_t> nb(n_items), slot(n_items), first((size_t)n_items + 1u);
  uint64_t need_bytes = 0, need_blocks = 0, entries = 0;
  for (uint32_t c = 0; c < n_items; c++) {
    const auto w = container_many_prewalk(kind, bodies, body_off, body_len, max_block, flags, c, n_max);
    nb[c] = w.blocks; slot[c] = (uint32_t)(((w.slot_max ? w.slot_max : 1u) + 63u) & ~63ull);
    first[c] = (uint32_t)entries;
    need_bytes += w.dst_bytes; need_blocks += w.blocks; entries += (uint64_t)w.blocks + 1u;
    if (entries > 0x7FFFFFFFull) return fail(LZ4HIP_E_ARG, "the items hold more than 2^31 - 1 blocks: split the call");
  }
  first[n_items] = (uint32_t)entries;
  if (dst_cap < need_bytes) return fail(LZ4HIP_E_ARG, "dst_cap is below the sum of item_dst_bytes (lz4hip_container_decode_many_bound)");
  if (sizes_cap < need_blocks) return fail(LZ4HIP_E_ARG, "sizes_cap is below the sum of item_blocks (lz4hip_container_decode_many_bound)");
  for (size_t i = 0; i < 5u * (size_t)n_items; i++) info[i] = 0;
  if (const int rc = need_device()) return rc;
  int ord;
  if (ordinal(0, &ord)) return fail(LZ4HIP_E_NO_DEVICE, "no device");
  DeviceGuard g(ord);
  std::string err;
  const int rc = container_many_shard(ord, kind, bodies, body_off, body_len, max_block, flags, n_items, n_max, nb.data(), slot.data(), first.data(), dst,
                                      item_dst_off, item_first, sizes, info, &err);
  return rc ? fail(rc, err.c_str()) : (int)LZ4HIP_OK;
}

// ---- many containers written per call ----
// what can be said about the items of a many-write without a device -> a message, or nullptr
static const char* container_write_many_arg_error(int kind, const uint64_t* src_len, const uint32_t* block_size, const uint8_t* flags, uint32_t n_items) {
  if (kind != 0 && kind != 1) return "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)";
  if (n_items && (!src_len || !block_size || !flags)) return kNullArg;
  for (uint32_t c = 0; c < n_items; c++)
    if (const char* why = lz4hip::container_write_rules::item_error(kind, src_len[c], block_size[c], flags[c])) return why;
  return nullptr;
}
int lz4hip_container_blocks_many_bound(int kind, const uint64_t* src_len, const uint32_t* block_size, const uint8_t* flags, const uint32_t* gap_head,
                                       const uint32_t* gap_tail, uint32_t n_items, uint32_t* item_blocks, uint64_t* item_dst_bytes) {
  namespace wr = lz4hip::container_write_rules;
  if (const char* why = container_write_many_arg_error(kind, src_len, block_size, flags, n_items)) return fail(LZ4HIP_E_ARG, why);
  if (n_items && (!item_blocks || !item_dst_bytes)) return fail(LZ4HIP_E_ARG, kNullArg);
  for (uint32_t c = 0; c < n_items; c++) {
    item_blocks[c] = wr::item_blocks(src_len[c], block_size[c]);
    item_dst_bytes[c] = wr::item_bound(kind, flags[c], src_len[c], block_size[c], gap_head ? gap_head[c] : 0u, gap_tail ? gap_tail[c] : 0u);
  }
  return LZ4HIP_OK;
}
// The items of a many-write through the shared staging, a group at a time (chain_shard: an item is its unit, first[] counts its blocks):
// a group is the items whose sources fit LZ4HIP_HOST_CHUNK_MB MiB and whose bounds fit 512 MiB, one item at least.  A group costs one
// upload of the packed sources and the item arrays, one launch sequence, one copy of the results and one of the finished bytes, which
// the device has laid back to back; compress slots (LZ4_compressBound of an item's largest block, per block: a payload far smaller than
// its block size takes what it holds, so the slots of a group stay below 2.01 x its sources + 32 bytes per block) and the HC workspace
// are sized by what the group holds.
static int container_write_many_shard(int ord, int kind, int hc_lv, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len,
                                      const uint32_t* block_size, const uint8_t* flags, const uint32_t* gap_head, const uint32_t* gap_tail, uint32_t n_items,
                                      const uint32_t* first, const uint64_t* bound, uint8_t* dst, uint64_t* item_dst_off, uint32_t* content_hash,
                                      std::string* err) {
  namespace wr = lz4hip::container_write_rules;
  auto cost = [&](uint32_t c) { return staging::Cost{al16((size_t)src_len[c]), (size_t)bound[c]}; };
  uint64_t out_bytes = 0;
  std::vector<uint64_t> so;
  return chain_shard(ord, first, 0, n_items, err, cost, [&](ShardScope& sh, ChunkSlot& s, const ChainChunk& ck) {
    const uint32_t c = ck.c, nc = ck.nc, nb = ck.nb;
    const staging::ContainerWriteManyMeta m(nc);
    if (!sh.reserve(s, ck.src, true, ck.dst, m.l.total)) return false;
    uint8_t* const hs = (uint8_t*)s.h_src.p;
    void *const hm = s.h_meta.p, *const dm = s.d_meta.p;
    so.resize(nc);
    bool any_cks = false, any_hash = false;
    uint64_t slots = 0;
    { size_t o = 0;
      for (uint32_t t = 0; t < nc; t++) {
        so[t] = o; o += al16((size_t)src_len[c + t]);
        m.src_off.in(hm)[t] = so[t]; m.src_len.in(hm)[t] = (int32_t)src_len[c + t]; m.slot_base.in(hm)[t] = slots;
        slots += (uint64_t)(first[c + t + 1] - first[c + t]) * wr::item_slot_bytes(src_len[c + t], block_size[c + t]);
        m.hash_len.in(hm)[t] = (flags[c + t] & wr::kFlagContentHash) ? (int32_t)src_len[c + t] : 0;
        m.block_size.in(hm)[t] = block_size[c + t]; m.flags.in(hm)[t] = flags[c + t];
        m.gap_head.in(hm)[t] = gap_head ? gap_head[c + t] : 0u; m.gap_tail.in(hm)[t] = gap_tail ? gap_tail[c + t] : 0u;
        any_cks |= (flags[c + t] & wr::kFlagBlockChecksum) != 0u; any_hash |= (flags[c + t] & wr::kFlagContentHash) != 0u;
      } }
    staging::rebase_first(first, c, nc, m.first.in(hm));
    // the device scratch of the group: the block arrays and the slots | the HC workspace | the fast compressor's queue words
    const size_t cws = (lz4hip::container_write_many_ws_bytes(nb, slots) + 256u + 255u) & ~(size_t)255u;
    const size_t hcws = hc_lv > 0 && nb ? ((lz4hip::hc_ws_bytes(ck.src, nb, hc_lv) + 255u) & ~(size_t)255u) : 0u;
    const size_t qwords = 3u + (size_t)nb + lz4hip::compress_fast_v2w_scratch_words(lz4hip::device_cus());
    if (!sh.ok("staging allocation", s.d_ws.reserve(cws + hcws + qwords * sizeof(uint32_t) + 256u))) return false;
    par_blocks(c, ck.j, ck.src, [=, &so](uint32_t t) { if (src_len[t]) memcpy(hs + so[t - c], src + src_off[t], (size_t)src_len[t]); });
    if (!sh.upload(s, ck.src, m.l, s.st)) return false;
    uint8_t* const w = (uint8_t*)s.d_ws.p;
    const lz4hip::ContainerWriteManyItems items{m.src_off.in(dm), m.src_len.in(dm), m.hash_len.in(dm), m.slot_base.in(dm), m.block_size.in(dm), m.first.in(dm),
                                                m.gap_head.in(dm), m.gap_tail.in(dm), m.flags.in(dm)};
    if (!sh.launched(lz4hip::launch_container_blocks_many(kind, hc_lv, any_cks, any_hash, (const uint8_t*)s.d_src.p, ck.src, items, nc, nb, (uint8_t*)s.d_dst.p,
                                                          ck.dst, (unsigned long long*)m.item_dst_off.in(dm), m.content_hash.in(dm), w, hcws ? w + cws : nullptr,
                                                          (uint32_t*)(w + cws + hcws), 64u * (uint32_t)g_compress_switch.load(std::memory_order_relaxed),
                                                          lz4hip::device_cus(), g_compress_core.load(std::memory_order_relaxed), s.st)))
      return false;
    if (!sh.fetch_results(s, m.l, s.st) || !sh.wait(s.st)) return false;
    const uint64_t* const ido = m.item_dst_off.in(hm);
    const uint64_t total = ido[nc];
    if (total > ck.dst) { *sh.err = "container write: the device wrote more than the items' bounds"; sh.rc = LZ4HIP_E_HIP; return false; }
    if (total) {
      if (!sh.ok("D2H dst", hipMemcpyAsync(s.h_dst.p, s.d_dst.p, (size_t)total, hipMemcpyDeviceToHost, s.st)) || !sh.wait(s.st)) return false;
      memcpy(dst + out_bytes, s.h_dst.p, (size_t)total);
    }
    for (uint32_t t = 0; t <= nc; t++) item_dst_off[c + t] = out_bytes + ido[t];
    if (content_hash) for (uint32_t t = 0; t < nc; t++) content_hash[c + t] = (flags[c + t] & wr::kFlagContentHash) ? m.content_hash.in(hm)[t] : 0u;
    out_bytes += total;
    return true;
  });
}
int lz4hip_container_blocks_many(int kind, int level, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len, const uint32_t* block_size,
                                 const uint8_t* flags, const uint32_t* gap_head, const uint32_t* gap_tail, uint32_t n_items, uint8_t* dst, uint64_t dst_cap,
                                 uint64_t* item_dst_off, uint32_t* content_hash) {
  namespace wr = lz4hip::container_write_rules;
  if (kind != 0 && kind != 1) return fail(LZ4HIP_E_ARG, "container kind must be 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks)");
  if (n_items > 0x7FFFFFFFu) return fail(LZ4HIP_E_ARG, "more than 2^31 - 1 items: split the call");   // (before any array is read)
  if (!item_dst_off || (n_items && !src_off) || (dst_cap && !dst)) return fail(LZ4HIP_E_ARG, kNullArg);
  if (const char* why = container_write_many_arg_error(kind, src_len, block_size, flags, n_items)) return fail(LZ4HIP_E_ARG, why);
  std::vector<uint32_t> first((size_t)n_items + 1u);
  std::vector<uint64_t> bound(n_items);
  uint64_t need = 0, blocks = 0;
  for (uint32_t c = 0; c < n_items; c++) {
    if (src_len[c] && !src) return fail(LZ4HIP_E_ARG, kNullArg);
    if ((flags[c] & wr::kFlagContentHash) && !content_hash) return fail(LZ4HIP_E_ARG, "an item asks for its content hash (flag bit 1) and content_hash is NULL");
    first[c] = (uint32_t)blocks;
    blocks += wr::item_blocks(src_len[c], block_size[c]);
    if (blocks > 0x7FFFFFFFull - n_items) return fail(LZ4HIP_E_ARG, "the items hold more than 2^31 - 1 - n_items blocks: split the call");
    bound[c] = wr::item_bound(kind, flags[c], src_len[c], block_size[c], gap_head ? gap_head[c] : 0u, gap_tail ? gap_tail[c] : 0u);
    if (need + bound[c] < need) return fail(LZ4HIP_E_ARG, "the sum of item_dst_bytes does not fit 64 bits: split the call");
    need += bound[c];
  }
  first[n_items] = (uint32_t)blocks;
  if (dst_cap < need) return fail(LZ4HIP_E_ARG, "dst_cap is below the sum of item_dst_bytes (lz4hip_container_blocks_many_bound)");
  int lv = 0;
  if (level != 0 && hc_level(level, &lv)) return fail(LZ4HIP_E_UNSUPPORTED, "unsupported compression level");
  item_dst_off[0] = 0;
  if (n_items == 0) return LZ4HIP_OK;
  if (content_hash) for (uint32_t c = 0; c < n_items; c++) content_hash[c] = 0;
  if (const int rc = need_device()) return rc;
  int ord;
  if (ordinal(0, &ord)) return fail(LZ4HIP_E_NO_DEVICE, "no device");
  DeviceGuard g(ord);
  std::string err;
  const int rc = container_write_many_shard(ord, kind, lv, src, src_off, src_len, block_size, flags, gap_head, gap_tail, n_items, first.data(), bound.data(),
                                            dst, item_dst_off, content_hash, &err);
  return rc ? fail(rc, err.c_str()) : (int)LZ4HIP_OK;
}
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
}  // extern "C"

// ---- resident compress streams (lz4hip_compress_fast_stream_batch) ---------------------------------------------------------
// A set of n streams whose state -- a record of lz4hip::kStreamRecWords words and a 32 KB table image each (kernels.h CStreamArgs) --
// lives in device memory between calls.  The streams are divided into contiguous id ranges over the devices the engine was initialised
// on at create; a call is sharded at those boundaries.  A record of zeros is a fresh stream, so create and reset are memsets.
struct lz4hip_cstreams {
  struct Part { int ord = 0; uint32_t lo = 0, hi = 0; uint32_t* rec = nullptr; uint64_t* tables = nullptr; };
  uint32_t n = 0;
  std::vector<Part> parts;
  // streams a call that failed after its launch has named: stopped at their next call (the slot's force-stop mark) and reported as
  // stopped, until they are reset
  std::vector<uint8_t> poisoned;
  std::mutex mu;   // calls on one set are serialised, as the streaming-xxhash handles are
};
namespace {
constexpr size_t kStreamRecBytes = lz4hip::kStreamRecWords * sizeof(uint32_t), kStreamTableBytes = 32768;
void cstreams_release(lz4hip_cstreams* set) {
  for (auto& p : set->parts) {
    DeviceGuard g(p.ord);
    if (p.rec) (void)hipFree(p.rec);
    if (p.tables) (void)hipFree(p.tables);
  }
  delete set;
}
// the argument errors of a call on a set that can be seen without a device: what does not depend on the set first (so that it is said,
// and can be tested, where no set can exist) -- the ids' array, what the call's own arrays say (arrays() -> a message or nullptr; not
// asked of an empty call), the ids' order -- then the set, then the ids against it
template <class Arrays>
const char* stream_call_error(const lz4hip_cstreams* set, const uint32_t* stream_id, uint32_t n_blocks, uint32_t n_chains, Arrays arrays) {
  if (n_chains != 0 || n_blocks != 0) {
    if (!stream_id) return kNullArg;
    if (const char* why = arrays()) return why;
    for (uint32_t c = 1; c < n_chains; c++)
      if (stream_id[c] <= stream_id[c - 1]) return "stream_id must be strictly ascending";
  }
  if (!set) return "null stream set";
  for (uint32_t c = 0; c < n_chains; c++) {
    if (stream_id[c] >= set->n) return "stream_id out of range";
  }
  return nullptr;
}
const char* cstream_arg_error(const lz4hip_cstreams* set, const uint32_t* stream_id, const lz4hip::CChainArgs& h) {
  return stream_call_error(set, stream_id, h.n_blocks, h.n_chains, [&] { return cchain_arg_error(h, true, true); });
}
// ... of lz4hip_compress_fast_stream_ext_batch
const char* cxstream_arg_error(const lz4hip_cstreams* set, const uint32_t* stream_id, const CXStreamHost& h) {
  return stream_call_error(set, stream_id, h.n_blocks, h.n_chains, [&]() -> const char* {
    if (!h.src || !h.src_off || !h.src_len || !h.chain_first || !h.hist_end || !h.hist_len || !h.win_off || !h.win_len || !h.dst || !h.dst_off || !h.dst_cap ||
        !h.out || !h.chain_consumed) return kNullArg;
    return staging::cxstream_shape_error(h.chain_first, h.n_chains, h.n_blocks, h.src_off, h.src_len, h.hist_end, h.hist_len, h.win_off, h.win_len);
  });
}
// One call on a set, for both entry points: whole streams per device, at the boundaries the set was created with -- [c0, c1) of the
// call's chains are part p's -- every share through shard(call, share, ord, c0, c1, err) with the share's state in call.cs_* and what
// the host path needs beside it in share (StreamShare), side by side where there are several.  The set is locked for the call.
// accel: the call's clamped acceleration, which travels in BlockCall::param.
template <class Shard>
int cstreams_call(lz4hip_cstreams* set, const uint32_t* stream_id, uint32_t n_chains, Op op, int accel, Shard shard) {
  std::lock_guard<std::mutex> lk(set->mu);
  struct Share { const lz4hip_cstreams::Part* p; uint32_t c0, c1; int rc = 0; std::string err; bool launched = false; };
  std::vector<Share> shares;
  try {
    for (const auto& p : set->parts) {
      const uint32_t c0 = (uint32_t)(std::lower_bound(stream_id, stream_id + n_chains, p.lo) - stream_id);
      const uint32_t c1 = (uint32_t)(std::lower_bound(stream_id, stream_id + n_chains, p.hi) - stream_id);
      if (c1 > c0) shares.push_back(Share{&p, c0, c1});
    }
  } catch (...) { return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  int prev = -1;
  (void)hipGetDevice(&prev);
  auto run = [&](Share& s) {
    BlockCall call{op, accel};
    call.cs_rec = s.p->rec; call.cs_tables = s.p->tables;
    const StreamShare share{stream_id, s.p->lo, set->poisoned.data(), &s.launched};
    try { s.rc = shard(call, share, s.p->ord, s.c0, s.c1, &s.err); }
    catch (...) { s.rc = LZ4HIP_E_NOMEM; s.err = "out of memory"; }
  };
  if (shares.size() == 1) {
    run(shares[0]);
  } else {
    std::vector<std::thread> th;
    try { for (auto& s : shares) th.emplace_back([&run, &s] { run(s); }); }
    catch (...) { for (auto& t : th) t.join(); if (prev >= 0) (void)hipSetDevice(prev); return fail(LZ4HIP_E_NOMEM, "out of memory or threads"); }
    for (auto& t : th) t.join();
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  // the call failed after a launch: some of the streams it named have gone on and some have not, and the caller has no results to tell
  // which, so EVERY stream the call named is stopped until it is reset (those of the shares that succeeded too)
  bool failed = false, launched = false;
  for (auto& s : shares) { failed |= s.rc != 0; launched |= s.launched; }
  if (failed && launched)
    for (uint32_t c = 0; c < n_chains; c++) set->poisoned[stream_id[c]] = 1;
  for (auto& s : shares)
    if (s.rc) return fail(s.rc, s.err.c_str());
  return LZ4HIP_OK;
}
}  // namespace

// ---- streaming xxhash (StreamingXXHash32JNI / StreamingXXHash64JNI: XXHashJNI.c:89-145, :199-255) ------------------------
struct lz4hip_xxh_stream {
  bool is64;
  int ord;                 // HIP ordinal the record lives on (the engine's first device, or the device of update_dev)
  void* rec = nullptr;     // device record (kernels.h)
  void* stage = nullptr;   // device staging for host-pointer updates
  size_t stage_cap = 0;
  uint64_t seed;
  bool pending_reset = true;   // the record is (re)initialised by the next launch
  // ordering of launches on different streams: every launch records `ev`; the next launch's stream waits for it on the device, the
  // digest and the reuse of the staging buffer wait for it on the host.  (`launched` and not "last stream != NULL": the null stream
  // is a stream too -- a host update() followed by update_dev() on a non-blocking stream raced on the record in round 1.)
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  bool launched = false;
  std::mutex mu;               // the reference's methods are `synchronized`
};
namespace {
constexpr size_t XXH_STAGE_MAX = 64u << 20;
int xxh_stream_create(bool is64, uint64_t seed, lz4hip_xxh_stream** out) {
  if (const int rc = need_device()) return rc;
  if (!out) return fail(LZ4HIP_E_ARG, kNullArg);
  int ord;
  if (ordinal(0, &ord)) return fail(LZ4HIP_E_NO_DEVICE, "no device");
  DeviceGuard g(ord);
  auto* st = new (std::nothrow) lz4hip_xxh_stream();
  if (!st) return fail(LZ4HIP_E_NOMEM, "out of memory");
  st->is64 = is64;
  st->ord = ord;
  st->seed = seed;
  if (hipMalloc(&st->rec, lz4hip::xxh_stream_rec_bytes(is64)) != hipSuccess) {
    delete st;
    return fail(LZ4HIP_E_NOMEM, "hipMalloc failed");
  }
  *out = st;
  return LZ4HIP_OK;
}
// absorbs a DEVICE buffer (len may be 0: only applies a pending reset)
int xxh_stream_launch(lz4hip_xxh_stream* st, const uint8_t* dbuf, uint32_t len, hipStream_t stream) {
  if (!st->ev) HIPCHK(hipEventCreateWithFlags(&st->ev, hipEventDisableTiming));
  if (st->launched && st->last != stream) HIPCHK(hipStreamWaitEvent(stream, st->ev, 0));   // updates of one hash are ordered
  const int reset = st->pending_reset ? 1 : 0;
  int e = st->is64 ? lz4hip::launch_xxh64_stream(st->rec, dbuf, len, reset, st->seed, stream)
                   : lz4hip::launch_xxh32_stream(st->rec, dbuf, len, reset, (uint32_t)st->seed, stream);
  if (e) return fail(LZ4HIP_E_HIP, "kernel launch", (hipError_t)e);
  st->pending_reset = false;
  st->last = stream;
  st->launched = true;
  HIPCHK(hipEventRecord(st->ev, stream));
  return LZ4HIP_OK;
}
template <class T>
int xxh_stream_digest(lz4hip_xxh_stream* st, bool is64, T* out) {
  if (!st || !out || st->is64 != is64) return fail(LZ4HIP_E_ARG, "bad stream handle");
  std::lock_guard<std::mutex> lk(st->mu);
  DeviceGuard g(st->ord);
  if (st->pending_reset) {  // nothing absorbed since create/reset: the digest of the empty stream
    int rc = xxh_stream_launch(st, (const uint8_t*)st->rec, 0, nullptr);
    if (rc) return rc;
  }
  if (st->launched) HIPCHK(hipEventSynchronize(st->ev));
  HIPCHK(hipMemcpy(out, (const uint8_t*)st->rec + lz4hip::xxh_stream_digest_offset(is64), sizeof(T), hipMemcpyDeviceToHost));
  return LZ4HIP_OK;
}
}  // namespace

extern "C" {

int lz4hip_version(void) { return LZ4HIP_VERSION; }
const char* lz4hip_last_error(void) { return g_err.c_str(); }

int lz4hip_init(const int* device_ids, int n_devices) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_inited) return g_devs.empty() ? LZ4HIP_E_NO_DEVICE : LZ4HIP_OK;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_inited = true;  // remember: there is nothing to run on (and nothing else to fall back to)
    g_devs.clear();
    return fail(LZ4HIP_E_NO_DEVICE, "hipGetDeviceCount found no device", e);
  }
  std::vector<int> devs;
  if (device_ids && n_devices > 0) {
    for (int i = 0; i < n_devices; i++) {
      if (device_ids[i] < 0 || device_ids[i] >= count) return fail(LZ4HIP_E_ARG, "device id out of range");
      devs.push_back(device_ids[i]);
    }
  } else {
    for (int i = 0; i < count; i++) devs.push_back(i);
  }
  g_devs = devs;
  g_inited = true;
  return LZ4HIP_OK;
}

void lz4hip_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (int ord : g_devs) {
    if (ord < 0 || ord >= 64) continue;
    if (hipSetDevice(ord) == hipSuccess) { g_ctx[ord].release(); route_release(ord); scratch_free_all(ord); }
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  g_devs.clear();
  g_inited = false;
}

int lz4hip_device_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return (int)g_devs.size();
}

#ifdef LZ4HIP_RING_DBG
}  // extern "C"
namespace lz4hip { int ring_stats_fetch(unsigned long long* out8); }
extern "C" {
__attribute__((visibility("default"))) int lz4hip_dbg_ring_stats(unsigned long long* out8) { return lz4hip::ring_stats_fetch(out8); }
#endif
int lz4hip_last_decode_route(int device, uint32_t* out8) {
  return on_device(device, false, out8 ? nullptr : kNullArg, [&] {
    const int e = lz4hip::last_decode_route(out8);
    return e ? fail(LZ4HIP_E_HIP, "hipMemcpyFromSymbol", (hipError_t)e) : 0;
  });
}
int lz4hip_set_option(const char* name, int value) {
  if (name && strcmp(name, "decode_stage") == 0) {
    if (value < -1 || value > 1) return fail(LZ4HIP_E_ARG, "decode_stage must be -1, 0 or 1");
    g_decode_stage = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "decode_pipe") == 0) {
    if (value < -1 || value > 8 || value == 6) return fail(LZ4HIP_E_ARG, "decode_pipe must be -1 .. 5, 7 or 8");
    g_decode_pipe = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "decode_route_short") == 0) {   // average output bytes per sampled sequence up to which a batch of more than 16 blocks per CU goes to the wave kernel; 0: never
    if (value < 0 || value > 255) return fail(LZ4HIP_E_ARG, "decode_route_short must be 0 .. 255");
    lz4hip::set_route_short(value);
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "decode_route_slots") == 0) {   // how many of the route ring's slots are handed out; every value gives the same bytes
    if (value < 1 || value > (int)kRouteWords) return fail(LZ4HIP_E_ARG, "decode_route_slots must be 1 .. 256");
    g_route_slots = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "decode_ring") == 0) {
    if (value != 0 && value != 256 && value != 512 && value != 1024 && value != 2048 && value != 4096 && value != 8192 && value != 16384 && value != 32768 && value != 65536)
      return fail(LZ4HIP_E_ARG, "decode_ring must be 0, 256 .. 4096 (ring loop) or 8192 .. 65536 (wave loop)");
    g_decode_ring = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "dstream_inorder") == 0) {   // (the twin alone: lz4hip_decompress_safe_stream_batch never looks at it)
    if (value != 0 && value != 1) return fail(LZ4HIP_E_ARG, "dstream_inorder must be 0 or 1");
    g_dstream_inorder = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "decode_lanes") == 0) {
    if (value != 0 && value != 1 && value != 4 && value != 8 && value != 16 && value != 32 && value != 64) return fail(LZ4HIP_E_ARG, "decode_lanes must be 0,1 (ring loop only),4,8,16,32,64");
    g_decode_lanes = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "compress_core") == 0) {
    if (value != 1 && value != 3 && value != 5) return fail(LZ4HIP_E_ARG, "compress_core must be 1, 3 or 5");
    g_compress_core = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "compress_pack") == 0) {
    if (value != 0 && value != 1) return fail(LZ4HIP_E_ARG, "compress_pack must be 0 or 1");
    lz4hip::set_compress_pack(value);
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "hc_chain_segment") == 0) {   // positions per build item of the HC chain compressor: every value gives the same bytes
    if (value < 4096 || value > (1 << 30)) return fail(LZ4HIP_E_ARG, "hc_chain_segment must be 4096 .. 1073741824");
    g_hc_chain_segment = value;
    return LZ4HIP_OK;
  }
  if (name && strcmp(name, "compress_switch") == 0) {
    if (value < 0 || value > 1024) return fail(LZ4HIP_E_ARG, "compress_switch must be 0..1024");
    g_compress_switch = value;
    return LZ4HIP_OK;
  }
  return fail(LZ4HIP_E_ARG, "unknown option");
}

int lz4hip_compress_bound(int n) {
  if (n < 0 || (uint32_t)n > 0x7E000000u) return 0;
  return n + n / 255 + 16;
}

// ---- host-pointer batch API ----
int lz4hip_compress_fast_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                               const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n) {
  return host_batch({OP_COMPRESS_FAST}, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_compress_fast_accel_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                     const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int acceleration) {
  const int a = accel_clamp(acceleration);
  if (a == 1) return lz4hip_compress_fast_batch(src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
  return host_batch({OP_COMPRESS_ACCEL, a}, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_compress_dest_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                    const uint64_t* dst_off, const int32_t* target_size, int32_t* out_len, int32_t* src_consumed, uint32_t n) {
  return host_batch({OP_COMPRESS_DEST, 0, nullptr, src_consumed}, src, src_off, src_len, dst, dst_off, target_size, out_len, n);
}
int lz4hip_decompress_safe_partial_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                         const uint64_t* dst_off, const int32_t* target_len, const int32_t* dst_cap, int32_t* out_len,
                                         uint32_t n) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!target_len || !dst_cap) return fail(LZ4HIP_E_ARG, kNullArg);
  std::vector<int32_t> room;
  try { room.resize(n); } catch (...) { return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  for (uint32_t i = 0; i < n; i++) room[i] = partial_room(target_len[i], dst_cap[i]);
  return host_batch({OP_DECODE_PARTIAL}, src, src_off, src_len, dst, dst_off, room.data(), out_len, n);
}
int lz4hip_dict_create(const uint8_t* dict, int dict_len, lz4hip_dict** out) {
  if (!dict || !out || dict_len < 0) return fail(LZ4HIP_E_ARG, !dict || !out ? kNullArg : "negative dictionary length");
  lz4hip_dict* d = new (std::nothrow) lz4hip_dict();
  if (!d) return fail(LZ4HIP_E_NOMEM, "out of memory");
  d->len = dict_len;
  const size_t keep = std::min<size_t>((size_t)dict_len, 65536u);
  try { d->tail.assign(dict + ((size_t)dict_len - keep), dict + dict_len); }
  catch (...) { delete d; return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  // resident on every initialised device.  Creating a handle initialises nothing (lz4hip_init's device list stays the caller's to
  // choose): where the engine is not up yet, or has no device, the handle only answers lz4hip_dict_size until a decode brings its
  // device's copy (dict_resident) -- or fails with LZ4HIP_E_NO_DEVICE like every other compute entry point
  std::vector<int> devs;
  { std::lock_guard<std::mutex> lk(g_mu); if (g_inited) devs = g_devs; }
  for (int ord : devs) {
    if (ord < 0 || ord >= 64) continue;
    DeviceGuard g(ord);
    const int rc = g.ok ? dict_upload(d, ord) : fail(LZ4HIP_E_HIP, "hipSetDevice failed");
    if (rc) { lz4hip_dict_free(d); return rc; }
  }
  *out = d;
  return LZ4HIP_OK;
}
int lz4hip_dict_size(const lz4hip_dict* dict) { return dict ? dict->len : fail(LZ4HIP_E_ARG, kNullArg); }
void lz4hip_dict_free(lz4hip_dict* dict) {
  if (!dict) return;
  for (int ord = 0; ord < 64; ord++) {
    if (!dict->dev[ord] && !dict->image[ord] && !dict->hc_image[ord]) continue;
    DeviceGuard g(ord);
    if (g.ok && dict->dev[ord]) (void)hipFree(dict->dev[ord]);
    if (g.ok && dict->image[ord]) (void)hipFree(dict->image[ord]);
    if (g.ok && dict->hc_image[ord]) (void)hipFree(dict->hc_image[ord]);
  }
  delete dict;
}
int lz4hip_decompress_safe_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                      const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!dict) return fail(LZ4HIP_E_ARG, kNullArg);
  BlockCall c{OP_DECODE_DICT};
  c.dict = dict;
  return host_batch(c, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_decompress_safe_chain_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const uint8_t* stored,
                                       const int32_t* dst_cap, const uint32_t* chain_first, uint8_t* dst, const uint64_t* chain_dst_off,
                                       const uint64_t* chain_dst_cap, const int32_t* chain_prefix_len, int32_t* out_len, uint64_t* chain_out_len,
                                       uint32_t n_blocks, uint32_t n_chains) {
  const lz4hip::ChainArgs h{src, src_off, src_len, stored, dst_cap, chain_first, dst, chain_dst_off, chain_dst_cap, chain_prefix_len, out_len, chain_out_len,
                            n_blocks, n_chains};
  // whole chains per device: a chain never leaves its lane group, let alone its device
  return chain_entry(chain_arg_error(h, true), n_chains, [&] { return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return chain_host_shard(h, ord, c0, c1, err); }); });
}
int lz4hip_decompress_safe_stream_batch(lz4hip_dstream_state* state, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                        const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                        const uint64_t* chain_win_off, const uint64_t* chain_win_len, int32_t* out_len, uint32_t n_blocks,
                                        uint32_t n_chains) {
  const DStreamHost h{state, src, src_off, src_len, chain_first, dst, dst_off, dst_cap, chain_win_off, chain_win_len, out_len, n_blocks, n_chains};
  // whole streams per device: a stream never leaves its lane group, let alone its device
  return chain_entry(dstream_arg_error(h), n_chains, [&] { return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return dstream_host_shard(h, ord, c0, c1, err); }); });
}
int lz4hip_decompress_safe_stream_inorder_batch(lz4hip_dstream_state* state, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                                const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                                const uint64_t* chain_win_off, const uint64_t* chain_win_len, int32_t* out_len, uint32_t n_blocks,
                                                uint32_t n_chains) {
  const DStreamHost h{state, src, src_off, src_len, chain_first, dst, dst_off, dst_cap, chain_win_off, chain_win_len, out_len, n_blocks, n_chains,
                      OP_DECOMPRESS_STREAM_INORDER, g_dstream_inorder.load()};
  return chain_entry(dstream_arg_error(h), n_chains, [&] { return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return dstream_host_shard(h, ord, c0, c1, err); }); });
}
// LZ4_decoderRingBufferSize (liblz4 1.9.3): 0 for a negative maxBlockSize or one above LZ4_MAX_INPUT_SIZE, else 65536 + 14 + max(maxBlockSize, 16)
int lz4hip_decoder_ring_buffer_size(int max_block) {
  if (max_block < 0 || max_block > 0x7E000000) return 0;
  if (max_block < 16) max_block = 16;
  return 65536 + 14 + max_block;
}
int lz4hip_compress_fast_chain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                                     const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len,
                                     uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains) {
  return lz4hip_compress_fast_chain_accel_batch(src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len, chain_consumed,
                                                n_blocks, n_chains, 1);
}
int lz4hip_compress_fast_chain_accel_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                                           const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len,
                                           uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, int acceleration) {
  const int accel = accel_clamp(acceleration);   // (1: the acceleration-1 kernel, launch_block)
  const lz4hip::CChainArgs h{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len, chain_consumed, n_blocks, n_chains};
  // whole chains per device: a chain never leaves its wavefront, let alone its device
  return chain_entry(cchain_arg_error(h, true, op_chain_stops(OP_COMPRESS_CHAIN)), n_chains, [&] {
    return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return cchain_host_shard({OP_COMPRESS_CHAIN, accel}, {}, h, ord, c0, c1, err); });
  });
}
int lz4hip_cstreams_create(uint32_t n_streams, lz4hip_cstreams** out) {
  if (!out || n_streams == 0 || n_streams > 0x7FFFFFFFu) return fail(LZ4HIP_E_ARG, !out ? kNullArg : "n_streams must be 1 .. 2^31 - 1");
  *out = nullptr;
  if (const int rc = need_device()) return rc;
  std::vector<int> devs;
  { std::lock_guard<std::mutex> lk(g_mu); devs = g_devs; }
  auto* set = new (std::nothrow) lz4hip_cstreams();
  if (!set) return fail(LZ4HIP_E_NOMEM, "out of memory");
  try {
    set->n = n_streams;
    set->poisoned.assign(n_streams, 0);
    const uint32_t D = (uint32_t)std::min<size_t>(devs.size(), n_streams);
    set->parts.resize(D);
    for (uint32_t d = 0; d < D; d++) {
      lz4hip_cstreams::Part& p = set->parts[d];
      p.ord = devs[d];
      p.lo = (uint32_t)((uint64_t)n_streams * d / D); p.hi = (uint32_t)((uint64_t)n_streams * (d + 1) / D);
    }
  } catch (...) { delete set; return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  for (auto& p : set->parts) {
    DeviceGuard g(p.ord);
    const size_t k = p.hi - p.lo;
    hipError_t e = g.ok ? hipMalloc((void**)&p.rec, k * kStreamRecBytes) : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipMalloc((void**)&p.tables, k * kStreamTableBytes);
    if (e == hipSuccess) e = hipMemset(p.rec, 0, k * kStreamRecBytes);
    // (the launches run on non-blocking streams, which are not ordered behind the null stream: the zeros are there before anyone is told)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      cstreams_release(set);
      return fail(e == hipErrorOutOfMemory ? LZ4HIP_E_NOMEM : LZ4HIP_E_HIP, "allocation of the streams' state", e);
    }
  }
  *out = set;
  return LZ4HIP_OK;
}
int lz4hip_cstreams_count(const lz4hip_cstreams* set) { return set ? (int)set->n : fail(LZ4HIP_E_ARG, kNullArg); }
void lz4hip_cstreams_free(lz4hip_cstreams* set) {
  if (!set) return;
  // (as lz4hip_xxh_stream_free: a call in flight on another thread ends first, but free must not RACE with a call -- one that arrives
  // while or after the set is freed uses freed memory; the header says so)
  { std::lock_guard<std::mutex> lk(set->mu); }
  cstreams_release(set);
}
int lz4hip_cstreams_reset(lz4hip_cstreams* set, const uint32_t* stream_id, uint32_t n) {
  if (!set) return fail(LZ4HIP_E_ARG, kNullArg);
  if (stream_id)
    for (uint32_t i = 0; i < n; i++)
      if (stream_id[i] >= set->n) return fail(LZ4HIP_E_ARG, "stream_id out of range");
  std::lock_guard<std::mutex> lk(set->mu);
  for (auto& p : set->parts) {
    DeviceGuard g(p.ord);
    if (!g.ok) return fail(LZ4HIP_E_HIP, "hipSetDevice failed");
    if (!stream_id) { HIPCHK(hipMemset(p.rec, 0, (size_t)(p.hi - p.lo) * kStreamRecBytes)); continue; }
    // (runs of consecutive ids are one memset)
    for (uint32_t i = 0; i < n;) {
      uint32_t j = i + 1;
      while (j < n && stream_id[j] == stream_id[j - 1] + 1u) j++;
      const uint32_t a = std::max(stream_id[i], p.lo), b = std::min(stream_id[j - 1] + 1u, p.hi);
      if (a < b) HIPCHK(hipMemset((uint8_t*)p.rec + (size_t)(a - p.lo) * kStreamRecBytes, 0, (size_t)(b - a) * kStreamRecBytes));
      i = j;
    }
  }
  // (the next launch runs on a non-blocking stream, which is not ordered behind the null stream's memsets: wait for them here)
  for (auto& p : set->parts) {
    DeviceGuard g(p.ord);
    if (!g.ok) return fail(LZ4HIP_E_HIP, "hipSetDevice failed");
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  if (!stream_id) std::fill(set->poisoned.begin(), set->poisoned.end(), 0);
  else for (uint32_t i = 0; i < n; i++) set->poisoned[stream_id[i]] = 0;
  return LZ4HIP_OK;
}
int lz4hip_cstreams_consumed(lz4hip_cstreams* set, uint32_t first, uint32_t n, uint64_t* consumed, uint8_t* stopped) {
  if (!set || (n && !consumed && !stopped)) return fail(LZ4HIP_E_ARG, kNullArg);
  if ((uint64_t)first + n > set->n) return fail(LZ4HIP_E_ARG, "stream range out of bounds");
  std::lock_guard<std::mutex> lk(set->mu);
  std::vector<uint32_t> words;
  try { words.resize((size_t)n * lz4hip::kStreamRecWords); } catch (...) { return fail(LZ4HIP_E_NOMEM, "out of memory"); }
  for (auto& p : set->parts) {
    const uint32_t a = std::max(first, p.lo), b = std::min(first + n, p.hi);
    if (a >= b) continue;
    DeviceGuard g(p.ord);
    if (!g.ok) return fail(LZ4HIP_E_HIP, "hipSetDevice failed");
    HIPCHK(hipMemcpy(words.data() + (size_t)(a - first) * lz4hip::kStreamRecWords, (const uint8_t*)p.rec + (size_t)(a - p.lo) * kStreamRecBytes,
                     (size_t)(b - a) * kStreamRecBytes, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* w = words.data() + (size_t)i * lz4hip::kStreamRecWords;
    if (consumed) consumed[i] = ((uint64_t)w[5] << 32) | w[4];
    if (stopped) stopped[i] = ((w[2] & lz4hip::kStreamStopped) || set->poisoned[first + i]) ? 1 : 0;
  }
  return LZ4HIP_OK;
}
int lz4hip_compress_fast_stream_batch(lz4hip_cstreams* set, const uint32_t* stream_id, const uint8_t* src, const uint64_t* chain_src_off,
                                      const int32_t* chain_prefix_len, const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst,
                                      const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks,
                                      uint32_t n_chains) {
  return lz4hip_compress_fast_stream_accel_batch(set, stream_id, src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len,
                                                 chain_consumed, n_blocks, n_chains, 1);
}
int lz4hip_compress_fast_stream_accel_batch(lz4hip_cstreams* set, const uint32_t* stream_id, const uint8_t* src, const uint64_t* chain_src_off,
                                            const int32_t* chain_prefix_len, const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst,
                                            const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint64_t* chain_consumed,
                                            uint32_t n_blocks, uint32_t n_chains, int acceleration) {
  const int accel = accel_clamp(acceleration);
  const lz4hip::CChainArgs h{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len, chain_consumed, n_blocks, n_chains};
  return chain_entry(cstream_arg_error(set, stream_id, h), n_chains, [&] {
    return cstreams_call(set, stream_id, n_chains, OP_COMPRESS_STREAM, accel, [&](const BlockCall& call, const StreamShare& share, int ord, uint32_t c0, uint32_t c1, std::string* err) {
      return cchain_host_shard(call, share, h, ord, c0, c1, err);
    });
  });
}
int lz4hip_compress_fast_stream_ext_batch(lz4hip_cstreams* set, const uint32_t* stream_id, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                          const uint32_t* chain_first, const uint64_t* chain_hist_end, const int32_t* chain_hist_len,
                                          const uint64_t* chain_win_off, const uint64_t* chain_win_len, uint8_t* dst, const uint64_t* dst_off,
                                          const int32_t* dst_cap, int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains) {
  return lz4hip_compress_fast_stream_ext_accel_batch(set, stream_id, src, src_off, src_len, chain_first, chain_hist_end, chain_hist_len, chain_win_off,
                                                     chain_win_len, dst, dst_off, dst_cap, out_len, chain_consumed, n_blocks, n_chains, 1);
}
int lz4hip_compress_fast_stream_ext_accel_batch(lz4hip_cstreams* set, const uint32_t* stream_id, const uint8_t* src, const uint64_t* src_off,
                                                const int32_t* src_len, const uint32_t* chain_first, const uint64_t* chain_hist_end,
                                                const int32_t* chain_hist_len, const uint64_t* chain_win_off, const uint64_t* chain_win_len, uint8_t* dst,
                                                const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint64_t* chain_consumed,
                                                uint32_t n_blocks, uint32_t n_chains, int acceleration) {
  const int accel = accel_clamp(acceleration);
  const CXStreamHost h{src, src_off, src_len, chain_first, chain_hist_end, chain_hist_len, chain_win_off, chain_win_len, dst, dst_off, dst_cap, out_len,
                       chain_consumed, n_blocks, n_chains};
  return chain_entry(cxstream_arg_error(set, stream_id, h), n_chains, [&] {
    return cstreams_call(set, stream_id, n_chains, OP_COMPRESS_XSTREAM, accel, [&](const BlockCall& call, const StreamShare& share, int ord, uint32_t c0, uint32_t c1, std::string* err) {
      return cxstream_host_shard(call, share, h, ord, c0, c1, err);
    });
  });
}
int lz4hip_compress_hc_chain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                                   const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len,
                                   uint32_t n_blocks, uint32_t n_chains, int level) {
  const lz4hip::CChainArgs h{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len, nullptr, n_blocks, n_chains};
  // whole chains per device: a device's workspace and staging hold a chain's buffer in one piece
  return chain_entry(cchain_arg_error(h, true, op_chain_stops(OP_COMPRESS_HC_CHAIN)), n_chains, [&]() -> int {
    int lv;
    if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
    return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return cchain_host_shard({OP_COMPRESS_HC_CHAIN, lv}, {}, h, ord, c0, c1, err); });
  });
}
int lz4hip_compress_hc_stream_batch(lz4hip_hcstream_state* state, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                    const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len,
                                    uint32_t n_blocks, uint32_t n_chains, int level) {
  const HcStreamHost h{state, src, src_off, src_len, chain_first, dst, dst_off, dst_cap, out_len, n_blocks, n_chains};
  // whole streams per device: a device's workspace and staging hold a stream's linear buffer in one piece
  return chain_entry(hcstream_arg_error(h), n_chains, [&]() -> int {
    int lv;
    if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
    return whole_chains(n_chains, [&](int ord, uint32_t c0, uint32_t c1, std::string* err) { return hcstream_host_shard(lv, h, ord, c0, c1, err); });
  });
}
int lz4hip_hcstream_load_dict(lz4hip_hcstream_state* st, uint64_t dict_end, uint64_t dict_len) {
  if (!st) return fail(LZ4HIP_E_ARG, kNullArg);
  if (dict_len > dict_end) return fail(LZ4HIP_E_ARG, "dict_len reaches in front of src");
  const staging::HcsState v = staging::hcs_load_dict(dict_end, dict_len);
  memcpy(st, &v, sizeof v);
  return LZ4HIP_OK;
}
int lz4hip_hcstream_save_dict(lz4hip_hcstream_state* st, uint64_t buf_off, int k) {
  if (!st) return fail(LZ4HIP_E_ARG, kNullArg);
  staging::HcsState v;
  memcpy(&v, st, sizeof v);
  const int kept = staging::hcs_save_dict(v, buf_off, k);
  memcpy(st, &v, sizeof v);
  return kept;
}
int lz4hip_compress_fast_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                    const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!dict) return fail(LZ4HIP_E_ARG, kNullArg);
  BlockCall c{OP_COMPRESS_DICT};
  c.dict = dict;
  return host_batch(c, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_compress_hc_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                  const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return rc;
  if (n == 0) return LZ4HIP_OK;
  if (!dict) return fail(LZ4HIP_E_ARG, kNullArg);
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  BlockCall c{OP_COMPRESS_HC_DICT, lv};
  c.dict = dict;
  return host_batch(c, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_decompressed_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const int32_t* dst_cap,
                                   int32_t* out_len, uint32_t n) {
  return host_batch({OP_DECODED_SIZE}, src, src_off, src_len, nullptr, nullptr, dst_cap, out_len, n);
}
int lz4hip_decompress_safe_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                 const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n) {
  return host_batch({OP_DECODE_SAFE}, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_decompress_fast_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_cap, uint8_t* dst,
                                 const uint64_t* dst_off, const int32_t* dst_len, int32_t* out_consumed, uint32_t n) {
  return host_batch({OP_DECODE_FAST}, src, src_off, src_cap, dst, dst_off, dst_len, out_consumed, n);
}
int lz4hip_compress_hc_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                             const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return host_batch({OP_COMPRESS_HC, lv}, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n);
}
int lz4hip_compress_hc_dest_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                       const uint64_t* dst_off, const int32_t* target_size, int32_t* out_len, int32_t* src_consumed,
                                       uint32_t n, int level) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return host_batch({OP_COMPRESS_HC_DEST, lv, nullptr, src_consumed}, src, src_off, src_len, dst, dst_off, target_size, out_len, n);
}
int lz4hip_xxh32_batch(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed, uint32_t* out, uint32_t n) {
  return host_xxh<uint32_t>(false, buf, off, len, seed, out, n);
}
int lz4hip_xxh64_batch(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, uint64_t* out, uint32_t n) {
  return host_xxh<uint64_t>(true, buf, off, len, seed, out, n);
}

// ---- device-pointer batch API ----
int lz4hip_compress_fast_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                   const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int device, void* stream) {
  return dev_batch({OP_COMPRESS_FAST}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream);
}
int lz4hip_compress_fast_accel_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                         const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int acceleration,
                                         int device, void* stream) {
  const int a = accel_clamp(acceleration);
  if (a == 1) return lz4hip_compress_fast_batch_dev(src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, device, stream);
  return dev_batch({OP_COMPRESS_ACCEL, a}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream);
}
int lz4hip_compress_dest_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                        const uint64_t* dst_off, const int32_t* target_size, int32_t* out_len, int32_t* src_consumed,
                                        uint32_t n, int device, void* stream) {
  return dev_batch({OP_COMPRESS_DEST, 0, nullptr, src_consumed}, {src, src_off, src_len, dst, dst_off, target_size, out_len, n}, device, stream);
}
int lz4hip_decompress_safe_partial_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                             const uint64_t* dst_off, const int32_t* target_len, const int32_t* dst_cap, int32_t* out_len,
                                             uint32_t n, int device, void* stream) {
  return dev_batch({OP_DECODE_PARTIAL, 0, target_len}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream,
                   target_len ? nullptr : kNullArg);
}
int lz4hip_decompress_safe_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                          const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n,
                                          const uint8_t* dict_dev, int dict_len, int device, void* stream) {
  BlockCall c{OP_DECODE_DICT};
  c.dict_dev = dict_dev;
  c.dict_len = dict_len;
  return dev_batch(c, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream,
                   dict_len < 0 ? "negative dictionary length" : (dict_len > 0 && !dict_dev) ? kNullArg : nullptr);
}
int lz4hip_decompress_safe_chain_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const uint8_t* stored,
                                           const int32_t* dst_cap, const uint32_t* chain_first, uint8_t* dst, const uint64_t* chain_dst_off,
                                           const uint64_t* chain_dst_cap, const int32_t* chain_prefix_len, int32_t* out_len, uint64_t* chain_out_len,
                                           uint32_t n_blocks, uint32_t n_chains, int device, void* stream) {
  const lz4hip::ChainArgs a{src, src_off, src_len, stored, dst_cap, chain_first, dst, chain_dst_off, chain_dst_cap, chain_prefix_len, out_len, chain_out_len,
                            n_blocks, n_chains};
  if (const char* why = chain_arg_error(a, false)) return fail(LZ4HIP_E_ARG, why);
  BlockCall c{OP_DECOMPRESS_CHAIN};
  c.chain = &a;
  return on_device(device, n_chains == 0, nullptr, [&] { return launch_block(c, lz4hip::BatchArgs{}, (hipStream_t)stream); });
}
int lz4hip_compress_fast_chain_batch_dev(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len, const int32_t* src_len,
                                         const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len,
                                         uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains, int device, void* stream) {
  const lz4hip::CChainArgs a{src, chain_src_off, chain_prefix_len, src_len, chain_first, dst, dst_off, dst_cap, out_len, chain_consumed, n_blocks, n_chains};
  if (const char* why = cchain_arg_error(a, false, op_chain_stops(OP_COMPRESS_CHAIN))) return fail(LZ4HIP_E_ARG, why);
  BlockCall c{OP_COMPRESS_CHAIN};
  c.cchain = &a;
  return on_device(device, n_chains == 0, nullptr, [&] { return launch_block(c, lz4hip::BatchArgs{}, (hipStream_t)stream); });
}
int lz4hip_compress_fast_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                        const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n,
                                        const lz4hip_dict* dict, int device, void* stream) {
  BlockCall c{OP_COMPRESS_DICT};
  c.dict = dict;
  return dev_batch(c, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream, dict ? nullptr : kNullArg);
}
int lz4hip_decompressed_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const int32_t* dst_cap,
                                       int32_t* out_len, uint32_t n, int device, void* stream) {
  return dev_batch({OP_DECODED_SIZE}, {src, src_off, src_len, nullptr, nullptr, dst_cap, out_len, n}, device, stream);
}
int lz4hip_decompress_safe_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                     const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int device, void* stream) {
  return dev_batch({OP_DECODE_SAFE}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream);
}
int lz4hip_decompress_fast_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_cap, uint8_t* dst,
                                     const uint64_t* dst_off, const int32_t* dst_len, int32_t* out_consumed, uint32_t n, int device, void* stream) {
  return dev_batch({OP_DECODE_FAST}, {src, src_off, src_cap, dst, dst_off, dst_len, out_consumed, n}, device, stream);
}
size_t lz4hip_hc_workspace_bytes(uint64_t src_span, uint32_t n_blocks, int level) {
  int lv;
  if (hc_level(level, &lv)) return 0;
  return lz4hip::hc_ws_bytes(src_span, n_blocks, lv);
}
int lz4hip_compress_hc_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                    const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level, int device, void* stream,
                                    uint64_t src_span, void* ws, size_t ws_bytes) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return dev_batch({OP_COMPRESS_HC, lv, nullptr, nullptr, ws, src_span}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream,
                   !ws ? kNullArg : ws_bytes < lz4hip::hc_ws_bytes(src_span, n, lv) ? "HC workspace too small for the source span" : nullptr);
}
int lz4hip_compress_hc_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                 const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level, int device, void* stream) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return dev_batch({OP_COMPRESS_HC, lv}, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream);
}
int lz4hip_compress_hc_dict_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                         const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level, const lz4hip_dict* dict, int device,
                                         void* stream, uint64_t src_span, void* ws, size_t ws_bytes) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  BlockCall c{OP_COMPRESS_HC_DICT, lv, nullptr, nullptr, ws, src_span};
  c.dict = dict;
  return dev_batch(c, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream,
                   !dict || !ws ? kNullArg : ws_bytes < lz4hip::hc_ws_bytes(src_span, n, lv) ? "HC workspace too small for the source span" : nullptr);
}
int lz4hip_compress_hc_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                      const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, int level,
                                      const lz4hip_dict* dict, int device, void* stream) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  BlockCall c{OP_COMPRESS_HC_DICT, lv};
  c.dict = dict;
  return dev_batch(c, {src, src_off, src_len, dst, dst_off, dst_cap, out_len, n}, device, stream, dict ? nullptr : kNullArg);
}
int lz4hip_compress_hc_dest_size_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                              const uint64_t* dst_off, const int32_t* target_size, int32_t* out_len, int32_t* src_consumed,
                                              uint32_t n, int level, int device, void* stream, uint64_t src_span, void* ws, size_t ws_bytes) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return dev_batch({OP_COMPRESS_HC_DEST, lv, nullptr, src_consumed, ws, src_span}, {src, src_off, src_len, dst, dst_off, target_size, out_len, n},
                   device, stream, !ws ? kNullArg : ws_bytes < lz4hip::hc_ws_bytes(src_span, n, lv) ? "HC workspace too small for the source span" : nullptr);
}
int lz4hip_compress_hc_dest_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                           const uint64_t* dst_off, const int32_t* target_size, int32_t* out_len, int32_t* src_consumed,
                                           uint32_t n, int level, int device, void* stream) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_E_UNSUPPORTED;
  return dev_batch({OP_COMPRESS_HC_DEST, lv, nullptr, src_consumed}, {src, src_off, src_len, dst, dst_off, target_size, out_len, n}, device, stream);
}
int lz4hip_xxh32_batch_dev(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed, uint32_t* out, uint32_t n, int device, void* stream) {
  return on_device(device, n == 0, !buf || !off || !len || !out ? kNullArg : nullptr,
                   [&] { return lz4hip::launch_xxh32(buf, off, len, seed, out, n, stream); });
}
int lz4hip_xxh64_batch_dev(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed, uint64_t* out, uint32_t n, int device, void* stream) {
  return on_device(device, n == 0, !buf || !off || !len || !out ? kNullArg : nullptr,
                   [&] { return lz4hip::launch_xxh64(buf, off, len, seed, out, n, stream); });
}

#ifdef LZ4HIP_DEV_TOOLS
// developer diagnostics (see include/lz4hip.h)
int lz4hip_dbg_compress_fast_profile_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint8_t* dst,
                                         const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out_len, uint32_t n, uint64_t* prof,
                                         int device, void* stream) {
  const lz4hip::BatchArgs a{src, src_off, src_len, dst, dst_off, dst_cap, out_len, n};
  return on_device(device, n == 0, !src || !src_off || !src_len || !dst || !dst_off || !dst_cap || !out_len || !prof ? kNullArg : nullptr,
                   [&] { return lz4hip::launch_compress_fast_prof(a, prof, g_compress_core.load() == 1 ? 1 : 3, stream); });
}
#endif  // LZ4HIP_DEV_TOOLS

// ---- single-block convenience ----
int lz4hip_compress_fast(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap) { return single({OP_COMPRESS_FAST}, src, src_len, dst, dst_cap); }
int lz4hip_compress_fast_accel(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int acceleration) {
  const int a = accel_clamp(acceleration);
  if (a == 1) return lz4hip_compress_fast(src, src_len, dst, dst_cap);
  return single({OP_COMPRESS_ACCEL, a}, src, src_len, dst, dst_cap);
}
int lz4hip_compress_dest_size(const uint8_t* src, int* src_size, uint8_t* dst, int target_size) {
  if (!src_size) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, "null src_size"));
  int32_t c = 0;
  const int r = single({OP_COMPRESS_DEST, 0, nullptr, &c}, src, *src_size, dst, target_size);
  if (!LZ4HIP_IS_LIB_ERROR(r)) *src_size = c;
  return r;
}
int lz4hip_compress_hc(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int level) {
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_LIB_ERROR(LZ4HIP_E_UNSUPPORTED);
  return single({OP_COMPRESS_HC, lv}, src, src_len, dst, dst_cap);
}
int lz4hip_compress_hc_dest_size(const uint8_t* src, int* src_size, uint8_t* dst, int target_size, int level) {
  if (!src_size) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, "null src_size"));
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_LIB_ERROR(LZ4HIP_E_UNSUPPORTED);
  int32_t c = 0;
  const int r = single({OP_COMPRESS_HC_DEST, lv, nullptr, &c}, src, *src_size, dst, target_size);
  if (!LZ4HIP_IS_LIB_ERROR(r)) *src_size = c;
  return r;
}
int lz4hip_decompress_safe(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap) { return single({OP_DECODE_SAFE}, src, src_len, dst, dst_cap); }
int lz4hip_decompress_fast(const uint8_t* src, int src_cap, uint8_t* dst, int dst_len) { return single({OP_DECODE_FAST}, src, src_cap, dst, dst_len); }
int lz4hip_decompressed_size(const uint8_t* src, int src_len, int dst_cap) { return single({OP_DECODED_SIZE}, src, src_len, nullptr, dst_cap); }
int lz4hip_decompress_safe_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return LZ4HIP_LIB_ERROR(rc);
  if (!dict) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, kNullArg));
  BlockCall c{OP_DECODE_DICT};
  c.dict = dict;
  return single(c, src, src_len, dst, dst_cap);
}
int lz4hip_compress_fast_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return LZ4HIP_LIB_ERROR(rc);
  if (!dict) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, kNullArg));
  BlockCall c{OP_COMPRESS_DICT};
  c.dict = dict;
  return single(c, src, src_len, dst, dst_cap);
}
int lz4hip_compress_hc_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int level, const lz4hip_dict* dict) {
  if (const int rc = need_device()) return LZ4HIP_LIB_ERROR(rc);
  if (!dict) return LZ4HIP_LIB_ERROR(fail(LZ4HIP_E_ARG, kNullArg));
  int lv;
  if (hc_level(level, &lv)) return LZ4HIP_LIB_ERROR(LZ4HIP_E_UNSUPPORTED);
  BlockCall c{OP_COMPRESS_HC_DICT, lv};
  c.dict = dict;
  return single(c, src, src_len, dst, dst_cap);
}
int lz4hip_decompress_safe_partial(const uint8_t* src, int src_len, uint8_t* dst, int target_size, int dst_cap) {
  return single({OP_DECODE_PARTIAL}, src, src_len, dst, partial_room(target_size, dst_cap));
}
int lz4hip_xxh32(const uint8_t* buf, int len, uint32_t seed, uint32_t* out) {
  const uint64_t zero = 0;
  int32_t l = len;
  uint8_t dummy = 0;
  return lz4hip_xxh32_batch(buf ? buf : &dummy, &zero, &l, seed, out, 1);
}
int lz4hip_xxh64(const uint8_t* buf, int len, uint64_t seed, uint64_t* out) {
  const uint64_t zero = 0;
  int32_t l = len;
  uint8_t dummy = 0;
  return lz4hip_xxh64_batch(buf ? buf : &dummy, &zero, &l, seed, out, 1);
}

// ---- streaming xxhash: thin wrappers over the helpers above the extern "C" block ----
int lz4hip_xxh32_stream_create(uint32_t seed, lz4hip_xxh_stream** out) { return xxh_stream_create(false, seed, out); }
int lz4hip_xxh64_stream_create(uint64_t seed, lz4hip_xxh_stream** out) { return xxh_stream_create(true, seed, out); }
int lz4hip_xxh_stream_reset(lz4hip_xxh_stream* st, uint64_t seed) {
  if (!st) return fail(LZ4HIP_E_ARG, "bad stream handle");
  std::lock_guard<std::mutex> lk(st->mu);
  st->seed = st->is64 ? seed : (uint64_t)(uint32_t)seed;
  st->pending_reset = true;
  return LZ4HIP_OK;
}
int lz4hip_xxh_stream_update(lz4hip_xxh_stream* st, const uint8_t* buf, int len) {
  if (!st || len < 0 || (!buf && len)) return fail(LZ4HIP_E_ARG, "bad argument");
  if (len == 0) return LZ4HIP_OK;
  std::lock_guard<std::mutex> lk(st->mu);
  DeviceGuard g(st->ord);
  size_t done = 0;
  while (done < (size_t)len) {
    const size_t part = std::min((size_t)len - done, XXH_STAGE_MAX);
    if (st->stage_cap < part) {
      if (st->launched) HIPCHK(hipEventSynchronize(st->ev));
      if (st->stage) (void)hipFree(st->stage);
      st->stage = nullptr;
      st->stage_cap = 0;
      size_t cap = 1u << 16;
      while (cap < part) cap <<= 1;
      if (hipMalloc(&st->stage, cap) != hipSuccess) return fail(LZ4HIP_E_NOMEM, "hipMalloc failed");
      st->stage_cap = cap;
    }
    if (st->launched) HIPCHK(hipEventSynchronize(st->ev));  // the staging buffer is reused
    HIPCHK(hipMemcpy(st->stage, buf + done, part, hipMemcpyHostToDevice));
    int rc = xxh_stream_launch(st, (const uint8_t*)st->stage, (uint32_t)part, nullptr);
    if (rc) return rc;
    done += part;
  }
  return LZ4HIP_OK;
}
int lz4hip_xxh_stream_update_dev(lz4hip_xxh_stream* st, const uint8_t* dbuf, int len, void* stream) {
  if (!st || len < 0 || (!dbuf && len)) return fail(LZ4HIP_E_ARG, "bad argument");
  if (len == 0) return LZ4HIP_OK;
  std::lock_guard<std::mutex> lk(st->mu);
  DeviceGuard g(st->ord);
  return xxh_stream_launch(st, dbuf, (uint32_t)len, (hipStream_t)stream);
}
int lz4hip_xxh32_stream_digest(lz4hip_xxh_stream* st, uint32_t* out) { return xxh_stream_digest<uint32_t>(st, false, out); }
int lz4hip_xxh64_stream_digest(lz4hip_xxh_stream* st, uint64_t* out) { return xxh_stream_digest<uint64_t>(st, true, out); }
void lz4hip_xxh_stream_free(lz4hip_xxh_stream* st) {
  if (!st) return;
  {
    std::lock_guard<std::mutex> lk(st->mu);
    DeviceGuard g(st->ord);
    if (st->launched) (void)hipEventSynchronize(st->ev);
    if (st->ev) (void)hipEventDestroy(st->ev);
    if (st->rec) (void)hipFree(st->rec);
    if (st->stage) (void)hipFree(st->stage);
  }
  delete st;
}

int lz4hip_gen_blocks_dev(uint8_t* dst, uint64_t stride, int32_t block_len, uint64_t seed, uint64_t first_idx, uint32_t litmax,
                          uint32_t win, uint32_t n_blocks, int device, void* stream) {
  return on_device(device, false, !dst || block_len < 0 || litmax == 0 || win == 0 ? "bad argument" : nullptr,
                   [&] { return lz4hip::launch_gen_blocks(dst, stride, block_len, seed, first_idx, litmax, win, n_blocks, stream); });
}

}  // extern "C"
