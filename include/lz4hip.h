/*
 * lz4hip.h -- C ABI of liblz4hip.so, the MI355X (gfx950) LZ4 block engine that sits behind
 * lz4-java's LZ4Factory as the fourth ("HIP") implementation family.
 *
 * Every entry point replaces one native call of the reference's JNI shim, but processes a BATCH
 * of independent blocks per HIP launch (the reference makes one liblz4 call per block):
 *
 *   lz4hip_compress_fast*     <- Java_net_jpountz_lz4_LZ4JNI_LZ4_1compress_1limitedOutput
 *                                -> LZ4_compress_default   (src/jni/net_jpountz_lz4_LZ4JNI.c:46-86, call :75)
 *   lz4hip_decompress_safe*   <- ..._LZ4_1decompress_1safe -> LZ4_decompress_safe (LZ4JNI.c:187-227, call :216)
 *   lz4hip_decompress_fast*   <- ..._LZ4_1decompress_1fast -> LZ4_decompress_fast (LZ4JNI.c:140-180, call :169)
 *   lz4hip_compress_hc*       <- ..._LZ4_1compressHC       -> LZ4_compress_HC     (LZ4JNI.c:93-133,  call :122)
 *   lz4hip_compress_bound     <- ..._LZ4_1compressBound    -> LZ4_compressBound   (LZ4JNI.c:234-239)
 *   lz4hip_compress_fast_accel*  = LZ4_compress_fast(src, dst, n, cap, acceleration) of liblz4's main API (exported by the
 *                                reference's liblz4-java.so; no JNI entry of the reference reaches it)
 *   lz4hip_compress_dest_size*   = LZ4_compress_destSize(src, dst, &srcSize, targetDstSize) of liblz4's main API (exported by
 *                                the reference's liblz4-java.so; no JNI entry of the reference reaches it)
 *   lz4hip_compress_hc_dest_size* = LZ4_compress_HC_destSize(state, src, dst, &srcSize, targetDstSize, level) of liblz4's HC API
 *                                (exported by the reference's liblz4-java.so; no JNI entry of the reference reaches it)
 *   lz4hip_decompress_safe_partial* = LZ4_decompress_safe_partial(src, dst, srcSize, targetOutputSize, dstCapacity) of liblz4's
 *                                main API (exported by the reference's liblz4-java.so; no JNI entry of the reference reaches it)
 *   lz4hip_decompress_safe_dict* = LZ4_decompress_safe_usingDict(src, dst, srcSize, dstCapacity, dictStart, dictSize) of liblz4's
 *                                main API, for a dictionary that is not contiguous with dst (exported by the reference's
 *                                liblz4-java.so; no JNI entry of the reference reaches it)
 *   lz4hip_xxh32* / xxh64*    <- Java_net_jpountz_xxhash_XXHashJNI_XXH32 / XXH64
 *                                (src/jni/net_jpountz_xxhash_XXHashJNI.c:42-59 / :152-169, calls :54 / :164)
 *
 * Return conventions deliberately equal liblz4's so the Java error mapping of the JNI family
 * (LZ4JNICompressor.java:39-41, LZ4JNISafeDecompressor.java:39-41, LZ4JNIFastDecompressor.java:40-42)
 * carries over unchanged:
 *   compress   : out_len[i] > 0 compressed size, 0 = dst_cap[i] too small
 *   decompress_safe : out_len[i] >= 0 decoded size, < 0 = -(input position) - 1
 *   decompress_fast : out_len[i] > 0 bytes consumed from src, < 0 = -(input position) - 1
 * Results are bit-exact against liblz4 1.9.3 (what LZ4Factory.nativeInstance() loads on linux/amd64).
 *
 * All functions return LZ4HIP_OK (0) or a negative lz4hip_status describing a LIBRARY failure
 * (no device, HIP error, bad argument); per-block codec results go to the out arrays.  There is
 * NO CPU fallback: without a usable gfx950 device every compute entry point fails with
 * LZ4HIP_E_NO_DEVICE.  All entry points are re-entrant and thread-safe; the library never keeps a
 * caller pointer past the call.
 */
#ifndef LZ4HIP_H
#define LZ4HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library itself is built with -fvisibility=hidden */
#endif

#define LZ4HIP_VERSION 100 /* 0.1.0 */

typedef enum lz4hip_status {
  LZ4HIP_OK = 0,
  LZ4HIP_E_NO_DEVICE = -1,  /* no HIP device / not initialised and auto-init failed */
  LZ4HIP_E_HIP = -2,        /* a HIP runtime call failed (see lz4hip_last_error) */
  LZ4HIP_E_ARG = -3,        /* null pointer, negative length, bad device index, ... */
  LZ4HIP_E_NOMEM = -4,      /* device or pinned-host allocation failed */
  LZ4HIP_E_UNSUPPORTED = -5, /* e.g. HC level outside what this build implements */
  LZ4HIP_E_CHAIN_STOPPED = -6 /* never a call's status: a block behind its chain's first failed block (LZ4HIP_CHAIN_STOPPED) */
} lz4hip_status;

/* ---- lifecycle ----------------------------------------------------------------------------- */
/* device_ids == NULL or n_devices <= 0: use every visible device.  Idempotent, thread-safe.      */
int lz4hip_init(const int* device_ids, int n_devices);
void lz4hip_shutdown(void);
int lz4hip_device_count(void);            /* devices the engine is initialised on (0 if none)   */
const char* lz4hip_last_error(void);      /* thread-local description of the last failure       */
int lz4hip_version(void);
/* tuning knobs (not part of the reference API; process-wide atomics read once per launch; every setting produces the same bytes).
 * Which decoder a launch of n blocks gets with every knob at its default (CU = compute units of the device, 256 on an MI355X):
 *   n <= 5 CU    the trio loop (lz4_decode_trio.h): THREE wavefronts per block -- scanner, planner, copier
 *   n <= 16 CU   the parallel wave loop (lz4_decode_wave.h): a wavefront per block, several sequences of it per trip
 *   more         chosen ON THE DEVICE from a sample of the batch (decode_route_kernel): 16384 .. 40959 blocks averaging >= 512 KiB compressed ->
 *                the ring loop (lz4_decode_ring.h); sequences of "decode_route_short" or fewer output bytes on average with near match
 *                sources (text) -> the wave loop; n <= 32 CU and streams that are not mostly literals -> the wave loop; otherwise the deep
 *                loop (lz4_decode_deep.h) below 40960 blocks and, from there on, for near match sources, else the 4-lane staged loop
 * "decode_pipe" = -1 (the table above) or one loop for every launch: 8 = trio loop, 7 = pair loop (two wavefronts per block: a parser and a
 *   copier), 5 = parallel wave loop, 4 = wave loop with one
 *   sequence per trip, 3 = ring loop, 2 = deep loop, 1 = two-trip pipelined loop, 0 = plain loop;
 * "decode_ring" = bytes of the output ring in LDS: 0 (by batch size) / 8192 / 16384 / 32768 / 65536 with decode_pipe 4 / 5,
 *   and 8, 0 / 16384 / 32768 / 65536 with 7, 0 / 256 / 512 / 1024 / 2048 / 4096 with 3 (which ones: by "decode_lanes");
 * "decode_lanes" = lanes of a wavefront sharing one block in the lane-group loops (0 = by batch size, 4 / 8 / 16 / 32 / 64; 1 with the ring
 *   loop: a lane per block); a combination no kernel exists for makes the next decode call fail with LZ4HIP_E_ARG and a message that names it;
 * "decode_stage" = 1 / 0 / -1 (by batch size): the plain loop writes through an LDS staging buffer so that output reaches memory as
 *   whole 128-byte lines (faster when the batch is bandwidth-bound);
 * "decode_route_short" = 0 .. 255 (default 8): average output bytes per sequence up to which the device-side route sends a batch (of near match
 *   sources) to the wave loop; 0 = never;
 * "decode_route_slots" = 1 .. 256 (default 256): how many of the device's route words (below) are handed out, round robin; every value gives
 *   the same bytes (1: every routed launch reuses the word of the one before it -- what the suite sets to exercise that);
 * "compress_core" = 5 (default: adaptive two-pass -- blocks of long sequences are finished by the lean core (lz4_fast_v2_core.h), whose
 *   parked hits a partner wavefront writes out, blocks of short sequences by the window-parallel core), 3 (lean core only) or 1
 *   (window-parallel core only); "compress_switch" = routing threshold of the adaptive scheme in bytes per sequence (default 16);
 * "compress_pack" = 1 (default) / 0: blocks of 65547 bytes .. 4 MiB are compressed with 32-bit table entries on ten match-finder chains
 *   per CU instead of five (0: every block on the five-chain kernel);
 * "hc_chain_segment" = 4096 .. 1073741824 (default 1048576): positions per build item of lz4hip_compress_hc_chain_batch*; every value
 *   gives the same bytes (a segment warms its table up over the 65535 positions in front of it: at most 6.25 % more build work on a
 *   long chain at the default, none on chains of up to 1 MiB);
 * "dstream_inorder" = 0 (default) / 1: lz4hip_decompress_safe_stream_inorder_batch decodes in order the blocks whose slots overlap the
 *   history they can reach / every block; where no slot overlaps both give the same bytes (that call's section, below).
 * Routed launches on any number of streams of a device are independent: the word a launch's route kernel writes and its candidate kernels
 * read is one of a per-device ring, and a word's next use is ordered -- on the device, by an event; the host never waits -- behind the
 * last candidate kernel of the launch that used it before, on whatever stream either runs.
 * The decode_* knobs and the device-side route do not apply to the partial decoder (lz4hip_decompress_safe_partial*): it always runs the
 * 4-lane staged loop from 40960 blocks on and the 8-lane deep loop below.  Nor do they apply to the dictionary decoder
 * (lz4hip_decompress_safe_dict*), which picks its two loops the same way.                                                       */
int lz4hip_set_option(const char* name, int value);
/* diagnostic: what the device-side route of a device's last routed decode launch decided (device = index as in the _dev calls) -- out8
 * (8 words) = { route (0 lane-group default of the batch size, 1 ring loop, 2 wave loop, 3 deep loop instead of the staged one), hops
 * counted by the sampler, stream bytes it walked, average compressed size of 64 blocks, sampled match offsets within 6 KB, sampled
 * sequences, their output bytes, 0 }; synchronises the device.  It describes the device's last routed launch on WHICHEVER stream it ran:
 * a single-stream diagnostic -- with routed launches in flight on several streams it answers for whichever route kernel ran last       */
int lz4hip_last_decode_route(int device, uint32_t* out8);

/* == LZ4_compressBound (LZ4JNI.c:237): n + n/255 + 16, 0 if n < 0 or n > 0x7E000000            */
int lz4hip_compress_bound(int n);

/* ---- host-pointer batch API ----------------------------------------------------------------
 * Block i occupies src[src_off[i] .. +src_len[i]) and owns the slot dst[dst_off[i] .. +dst_cap[i]).
 * The library stages H2D/D2H itself and shards contiguous block ranges over the initialised
 * devices; slots must not overlap.                                        */
int lz4hip_compress_fast_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                               uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                               int32_t* out_len, uint32_t n_blocks);
/* ACCELERATED FAST COMPRESS: the bytes and return value of LZ4_compress_fast(src, dst, n, cap, acceleration), liblz4 1.9.3.
 * A higher acceleration probes fewer positions (each miss-run starts with step counter acceleration << 6 instead of 1 << 6):
 * faster parsing, a lower ratio.  acceleration is clamped as liblz4 does: < 1 -> 1, > 65537 (LZ4_ACCELERATION_MAX) -> 65537.
 *   - after clamping, acceleration 1 IS lz4hip_compress_fast_batch / _batch_dev / lz4hip_compress_fast: same call, same kernels;
 *   - 2 .. 65537 run their own kernel (compress_fast_accel_cu_kernel: one sequence per wavefront step, five wavefronts per CU,
 *     byU16 tables below 65547 bytes, byU32 above, blocks up to 0x7E000000 bytes);
 *   - results as for lz4hip_compress_fast*: out_len[i] > 0 compressed size, 0 = dst_cap[i] too small (also: src_len[i] < 0 or
 *     > 0x7E000000, dst_cap[i] < 0); library failures as the status / LZ4HIP_LIB_ERROR of the call;
 *   - the host batch shards over the initialised devices and returns only the useful bytes of every slot, as the fast path does;
 *   - single calls (lz4hip_compress_fast_accel) are coalesced with concurrent calls of the SAME clamped acceleration only: every
 *     value has a combiner of its own, so one launch never mixes accelerations.                                                  */
int lz4hip_compress_fast_accel_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                     uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                     int32_t* out_len, uint32_t n_blocks, int acceleration);
/* COMPRESS TO A TARGET SIZE: the bytes, return value and consumed size of LZ4_compress_destSize(src, dst, &srcSize, targetDstSize),
 * liblz4 1.9.3: as much of block i as fits in exactly target_size[i] bytes.  Acceleration 1; the table type follows the whole
 * src_len[i] (byU16 below 65547 bytes, byU32 from there on, blocks up to 0x7E000000 bytes).
 *   - out_len[i] is liblz4's return value: the bytes written (<= target_size[i]), 0 for target_size[i] <= 0 and for src_len[i] < 0
 *     or > 0x7E000000; an empty block gives the single token 0x00 (1 byte) for any target >= 1;
 *   - src_consumed[i] is what liblz4 leaves in *srcSizePtr: the input bytes the output covers (decoding out_len[i] bytes gives back
 *     exactly src[0 .. src_consumed[i])), and src_len[i] itself where it returns 0 up front;
 *   - target_size[i] >= compressBound(src_len[i]): the bytes of lz4hip_compress_fast, all of the input consumed;
 *   - block i's slot is dst[dst_off[i] .. + target_size[i]): nothing is written past it;
 *   - one kernel (compress_fast_dest_cu_kernel: the one-sequence-per-step core in fill mode, five wavefronts per CU); a block stops
 *     once its target is full, so its time follows the input consumed, not src_len[i];
 *   - the host batch shards over the initialised devices, returns only the useful bytes of every slot as the fast path does and
 *     brings src_consumed back with the sizes; library failures as the status of the call;
 *   - single calls (lz4hip_compress_dest_size) are coalesced with concurrent destSize calls only, through a combiner of their own. */
int lz4hip_compress_dest_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                    uint8_t* dst, const uint64_t* dst_off, const int32_t* target_size,
                                    int32_t* out_len, int32_t* src_consumed, uint32_t n_blocks);
/* DECODE A PREFIX: the return value and bytes of LZ4_decompress_safe_partial(src, dst, src_len, target_len, dst_cap), liblz4 1.9.3:
 * the first min(target_len[i], dst_cap[i]) bytes of block i, or fewer where the stream ends first -- a cut stream (a prefix of the
 * compressed bytes) decodes to what its bytes hold.
 *   - out_len[i] is liblz4's return value: the bytes decoded (<= min(target_len[i], dst_cap[i])), or -(input position) - 1;
 *     target 0 gives 0 whatever the source holds, an empty source with a target > 0 gives -1;
 *   - block i's slot is dst[dst_off[i] .. + dst_cap[i]): nothing is written at or past dst_off[i] + min(target_len[i], dst_cap[i]);
 *   - a negative src_len[i], target_len[i] or dst_cap[i] gives -1 (the engine's rule: liblz4's behaviour there is undefined);
 *   - a match of offset 0 (invalid: no compressor emits one) that the cut falls in is zero-filled, as offset-0 matches are
 *     everywhere in this engine; liblz4 leaves those bytes as its buffer held them;
 *   - two kernels: >= 40960 blocks decode_partial_kernel (4 lanes per block, output staged in LDS), fewer decode_partial_deep_kernel
 *     (8 lanes, the deep loop) -- the safe decoder's unrouted lane-group loops with the core's PARTIAL switch; a block stops at its
 *     target, so its time follows the bytes decoded;
 *   - the host batch shards over the initialised devices and returns only the decoded bytes of every slot; library failures as
 *     the status of the call;
 *   - single calls (lz4hip_decompress_safe_partial) are coalesced with concurrent partial calls only, through a combiner of their own. */
int lz4hip_decompress_safe_partial_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                         uint8_t* dst, const uint64_t* dst_off, const int32_t* target_len,
                                         const int32_t* dst_cap, int32_t* out_len, uint32_t n_blocks);
/* DECODE AGAINST A DICTIONARY: the return value and bytes of LZ4_decompress_safe_usingDict(src, dst, src_len, dst_cap, dict,
 * dict_len), liblz4 1.9.3, for a dictionary that is NOT contiguous with dst (liblz4's external-dictionary mode) -- records that
 * were each compressed alone against one shared dictionary (LZ4_loadDict + LZ4_compress_fast_continue, LZ4_loadDictHC +
 * LZ4_compress_HC_continue), every one of them readable on its own.  The writers of such records are
 * lz4hip_compress_fast_dict* and lz4hip_compress_hc_dict* below; there is no dictionary form of the fast decoder, of the partial
 * decoder or of the size query; linked blocks (liblz4's prefix mode) are lz4hip_decompress_safe_chain_batch*'s.
 *   - out_len[i] is liblz4's return value on valid AND malformed streams: the decoded size, or -(input position) - 1;
 *   - offsets: with dict_len < 65536 an offset is valid iff offset <= output position + dict_len; with dict_len >= 65536 no
 *     offset is rejected and only the dictionary's last 64 KB can be reached (liblz4's rule, checked where the safe decoder
 *     checks offset > output position: in front of a match length's extension bytes in the fast tier, behind them elsewhere);
 *   - a match that starts before the block takes (offset - output position) bytes from the dictionary's end, or fewer if it is
 *     shorter, and the rest from the block's own start, byte by byte (the rest may overlap what it writes); it is an error if it
 *     ends within the last 5 bytes of dst_cap[i], and no other end-of-block rule applies to it;
 *   - dict_len == 0 is lz4hip_decompress_safe* exactly; a negative src_len[i] or dst_cap[i] gives -1;
 *   - nothing outside [dict, dict + dict_len) is read and nothing outside block i's slot dst[dst_off[i] .. + dst_cap[i]) is written;
 *   - a handle (lz4hip_dict_create) keeps the true length and the last 64 KB, resident on every initialised device (a device
 *     initialised later gets its copy on first use; creating a handle does not initialise the engine); it is immutable: any number
 *     of threads may decode against it, and it must outlive every call that uses it.  dict == NULL, out == NULL or a negative length
 *     is LZ4HIP_E_ARG.  Creating a handle needs no device (lz4hip_dict_size then still answers); decoding against it without one is
 *     LZ4HIP_E_NO_DEVICE;
 *   - two kernels: >= 40960 blocks decode_dict_kernel (4 lanes per block, output staged in LDS), fewer decode_dict_deep_kernel
 *     (8 lanes, the deep loop, the pipelined loop for streams under 2 KB) -- the safe decoder's unrouted lane-group loops with the
 *     core's DICT switch: their interior loops also take the matches that lie wholly inside the dictionary; the decode_* knobs
 *     and the device-side route do not apply;
 *   - the host batch shards over the initialised devices as the safe decoder's does; library failures as the status of the call;
 *   - single calls (lz4hip_decompress_safe_dict) are coalesced only with concurrent calls on the SAME handle.                   */
typedef struct lz4hip_dict lz4hip_dict;
int lz4hip_dict_create(const uint8_t* dict, int dict_len, lz4hip_dict** out);
int lz4hip_dict_size(const lz4hip_dict* dict);   /* the true length given to lz4hip_dict_create (NULL: LZ4HIP_E_ARG) */
void lz4hip_dict_free(lz4hip_dict* dict);        /* NULL is fine; no call on the handle may be in flight */
int lz4hip_decompress_safe_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                      uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                      int32_t* out_len, uint32_t n_blocks, const lz4hip_dict* dict);
/* DECODE CHAINS OF LINKED BLOCKS: the return values and bytes of liblz4 1.9.3's streaming decoder in its rolling-prefix mode.  A CHAIN
 * is a run of blocks whose decoded forms lie back to back in one destination region; a match of block k may reach back into what the
 * blocks before it decoded, and into history that was there before the chain's first block -- what LZ4_compress_fast_continue writes
 * for a stream of messages and the `lz4` command line for a frame without block independence.  None of those blocks decodes on its
 * own.  Chains are independent of each other; one launch decodes many of them.  For block k of chain c the result is
 *     LZ4_setStreamDecode(sd, chain_dst - prefix_len, prefix_len);             (prefix_len may be 0)
 *     r_k = LZ4_decompress_safe_continue(sd, src_k, chain_dst + sum(r_j, j < k), src_len_k, cap_k);
 * with chain_dst = dst + chain_dst_off[c]: every destination is where the previous one ended (withSmallPrefix / withPrefix64k, never
 * liblz4's external-dictionary or double-dictionary mode).
 *   - chain c is the blocks [chain_first[c], chain_first[c + 1]) (n_chains + 1 entries, ascending from 0 to n_blocks); its region is
 *     dst[chain_dst_off[c] .. + chain_dst_cap[c]), and chain_prefix_len[c] bytes of history lie in front of it in dst
 *     (chain_prefix_len == NULL: no chain has any);
 *   - out_len[i] is liblz4's r_k, on valid AND malformed streams: the decoded size, or -(input position) - 1.  The capacity liblz4
 *     gets is cap_k = min(dst_cap[i], what is left of chain_dst_cap[c]) (and at most INT32_MAX - 65535: more than any block the
 *     format allows can decode to); a negative src_len[i] or dst_cap[i] gives -1;
 *   - offsets: with P = prefix_len + the bytes the chain has decoded so far, an offset is valid at output position p of the block iff
 *     offset <= p + P; once P >= 65535 no offset is rejected (checked where the safe decoder checks offset > p, same error codes);
 *   - a match that starts in the history obeys the ordinary end-of-block rules (unlike lz4hip_decompress_safe_dict*'s single rule),
 *     and one that straddles the block's start is one contiguous, possibly overlapping copy;
 *   - stored (NULL, or one byte per block): stored[i] != 0 marks a raw block, copied verbatim: out_len[i] = src_len[i], or -1 if it
 *     does not fit in cap_k.  Later blocks may match into it;
 *   - a block that decodes to 0 bytes changes nothing and the chain goes on; a first block without history is
 *     lz4hip_decompress_safe exactly (which is also why there is no single-call form: a chain of one block IS that call);
 *   - a block whose result is negative ENDS ITS CHAIN (liblz4 leaves the stream state untouched there, nothing meaningful can follow):
 *     every block behind it gets LZ4HIP_CHAIN_STOPPED, a value no liblz4 result can equal.  chain_out_len[c] = the bytes the chain
 *     decoded before it stopped;
 *   - for the region [chain_dst_off[c] - min(prefix_len, 65535), chain_dst_off[c] + chain_dst_cap[c]): nothing outside it is read,
 *     and nothing in front of chain_dst_off[c] is written.  Regions of different chains must not overlap one another's writes;
 *   - LZ4HIP_E_ARG: a required pointer that is NULL (everything but stored and chain_prefix_len), a chain_first that is not ascending
 *     from 0 to n_blocks, a negative chain_prefix_len[c] or one longer than chain_dst_off[c].  These are said before a device is looked
 *     for; without a device a well-formed call is LZ4HIP_E_NO_DEVICE;
 *   - one kernel, decode_chain_kernel: lane groups of 8 draw chains from a queue (chains differ in length) and walk their blocks in
 *     order with the core's PREFIX switch -- the deep loop for streams of 2 KB and more, the pipelined loop and the exact tiers below;
 *     the LDS-staged loops cannot see the history.  ONE CHAIN IS SERIAL BY CONSTRUCTION and runs on 8 lanes; the kernel waits for
 *     no other wavefront or workgroup anywhere, and parallelism comes from the number of chains alone: thousands of chains fill the
 *     device, a single chain is slower than one host thread (profiles/chain_decode_sweep.txt).  The decode_* knobs do not apply;
 *   - the host form uploads the streams and, per chain, the last min(prefix_len, 65536) bytes of history from the caller's dst, and
 *     brings back only the bytes decoded (runs less than 4 KB apart as one copy); it shards over the initialised devices at chain
 *     boundaries;
 *   - out of scope: LZ4_saveDict, chains that start from a non-contiguous dictionary
 *     (LZ4_decompress_safe_doubleDict), ring-buffer destinations that wrap, fast and partial decoders in chain form.  (No longer
 *     out of scope: dictionaries elsewhere, destinations that wrap or alternate and save areas are
 *     lz4hip_decompress_safe_stream_batch, below.)                                                                                */
int lz4hip_decompress_safe_chain_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                       const uint8_t* stored, const int32_t* dst_cap, const uint32_t* chain_first,
                                       uint8_t* dst, const uint64_t* chain_dst_off, const uint64_t* chain_dst_cap,
                                       const int32_t* chain_prefix_len, int32_t* out_len, uint64_t* chain_out_len,
                                       uint32_t n_blocks, uint32_t n_chains);

/* DECODE STREAMS WHOSE BLOCKS LAND ANYWHERE: LZ4_decompress_safe_continue of liblz4 1.9.3 in every mode of its LZ4_streamDecode_t, so
 * that a consumer of a long stream needs no destination as long as the stream: a ring buffer, two alternating block buffers, a 64 KB
 * save area in front of a block buffer, a stream that starts from a dictionary lying somewhere else.  The chain call above is the
 * rolling-prefix mode alone; this one adds LZ4_decompress_safe_forceExtDict (after a jump) and LZ4_decompress_safe_doubleDict (while a
 * short prefix grows behind an external dictionary).
 *
 * A stream's state is liblz4's four fields, written as offsets into dst: the prefix [prefix_end - prefix_len, prefix_end) is what was
 * decoded contiguously last, the external dictionary [ext_end - ext_len, ext_end) is what the prefix was before the last jump.  All
 * zero is a fresh stream; LZ4_setStreamDecode(sd, dst + p, n) is {p + n, n, 0, 0}.  The state is plain host data, read and written
 * by the call: there is no handle and nothing stays on a device between calls.  For a block decoded to d = dst_off[i], capacity cap:
 *     if prefix_len == 0:                 r = LZ4_decompress_safe;                 r > 0: prefix_len = r, prefix_end = d + r
 *     else if prefix_end == d:
 *         if   prefix_len >= 65535:       r = ..._withPrefix64k                    (the external dictionary is ignored)
 *         elif ext_len == 0:              r = ..._withSmallPrefix(prefix_len)
 *         else:                           r = ..._doubleDict(prefix_len, ext)
 *                                                                                  r > 0: prefix_len += r, prefix_end += r
 *     else (a jump):                      ext_len = prefix_len, ext_end = prefix_end     BEFORE decoding, whatever r turns out to be
 *                                         r = ..._forceExtDict(ext);               r > 0: prefix_len = r, prefix_end = d + r
 * r <= 0 leaves the prefix as it was -- so a 0-byte block at a new place drops the old external dictionary and leaves the prefix
 * standing as its own external dictionary: liblz4's behaviour, reproduced.  The history a doubleDict block sees is the last 64 KB of
 * ext ++ prefix: a match that starts in the external dictionary and runs past its end continues at the start of the prefix.
 *   - stream c is the blocks [chain_first[c], chain_first[c + 1]) of this call (n_chains + 1 entries, ascending from 0 to n_blocks),
 *     decoded in order, each to its own dst_off[i] with the capacity min(dst_cap[i], INT32_MAX - 65535); state[c] is read in front
 *     of the first and written back behind the last.  A later call carries on from the state the earlier one left;
 *   - out_len[i] is liblz4's r, on valid AND malformed streams.  A negative src_len[i] or dst_cap[i] counts as a block liblz4 answered
 *     with -1 (a jump's ext = prefix is applied first, as it would be).  A negative result ENDS THE STREAM'S PART OF THE CALL: every
 *     block behind it gets LZ4HIP_CHAIN_STOPPED, and the state written back is the one in front of the failed block (with the jump's
 *     ext = prefix if it was a jump).  A result of 0 goes on;
 *   - THE WINDOW: every slot [dst_off[i], dst_off[i] + dst_cap[i]) of stream c lies inside [chain_win_off[c], + chain_win_len[c]): the
 *     ring, the pair of buffers, the save area plus block area.  It is what the call mirrors on the device.  A history PIECE is the
 *     last min(len, 65535) bytes in front of prefix_end or ext_end -- nothing in front of it is ever read.  A piece lies wholly inside
 *     the window, or wholly outside it (it ends at or before chain_win_off[c], or starts at or behind the window's end).  An outside
 *     piece is only read, may be shared by any number of streams (one dictionary for all) and is uploaded once per staged chunk; an
 *     outside prefix that ends exactly at chain_win_off[c] stays contiguous with the window (once blocks have been decoded behind
 *     it the prefix reaches across that edge: the later calls name a window that begins where the dictionary does).  Windows of
 *     different streams must not overlap;
 *   - WHAT IS GUARANTEED: out_len and the state written back are liblz4's on every input -- the decoder's control flow never depends
 *     on copied bytes.  The BYTES are liblz4's whenever a block's slot does not overlap the history the block can reach: the last
 *     min(prefix_len, 65535) bytes of the prefix and the last 65535 - min(prefix_len, 65535) bytes (at most ext_len) of the external
 *     dictionary.  Where they overlap, the bytes of matches that read the overlapped part are unspecified (the lanes of a group copy
 *     in wider steps than liblz4's); still nothing outside the slot is written and nothing outside window and history pieces is read.
 *     THE RING RULE that follows: a ring that wraps to 0 when the next block no longer fits is safe from 65535 + 2 x maxBlock bytes
 *     on.  liblz4's minimal ring (65536 + 14 + maxBlock, LZ4_DECODER_RING_BUFFER_SIZE) and small rings kept in step with the
 *     encoder's are out of scope: they need a store-exact, strictly in-order copy path -- the follow-up to this call;
 *   - LZ4HIP_E_ARG: a required pointer that is NULL (all are required), a chain_first that is not ascending from 0 to n_blocks, a slot
 *     outside its stream's window, a history piece that straddles a window edge, a history longer than its end offset.  These are
 *     said before a device is looked for; without a device a well-formed call is LZ4HIP_E_NO_DEVICE;
 *   - one kernel, decode_stream_kernel, of decode_chain_kernel's shape: lane groups of 8 draw streams from a queue and walk their
 *     blocks of the call in order; per block the state picks the core's PREFIX instance or its PREFIX && DICT instance, with the deep
 *     loop for streams of 2 KB and more, the pipelined loop and the exact tiers below.  ONE STREAM IS SERIAL BY CONSTRUCTION; nothing
 *     waits for another wavefront or workgroup, and parallelism comes from the number of streams alone.  A stream that never jumps
 *     runs the chain kernel's code.  The decode_* knobs do not apply;
 *   - the host form uploads the compressed blocks and each stream's history pieces (the external dictionary's only while the prefix
 *     is shorter than 65535 bytes), and brings back each block's r decoded bytes (runs less than 4 KB apart as one copy) -- nothing
 *     else of dst is written; it shards over the initialised devices at stream boundaries;
 *   - out of scope: a device-pointer form (as for lz4hip_compress_hc_chain_batch: left to a change that can also extend the far-offset
 *     and stream-contract tables of the device entry points), stored blocks, fast and partial decoders in stream form,
 *     LZ4_decoderRingBufferSize.                                                                                                 */
typedef struct lz4hip_dstream_state { uint64_t prefix_end, prefix_len, ext_end, ext_len; } lz4hip_dstream_state;   /* all zero: a fresh stream */
int lz4hip_decompress_safe_stream_batch(lz4hip_dstream_state* state, const uint8_t* src, const uint64_t* src_off,
                                        const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst,
                                        const uint64_t* dst_off, const int32_t* dst_cap, const uint64_t* chain_win_off,
                                        const uint64_t* chain_win_len, int32_t* out_len, uint32_t n_blocks, uint32_t n_chains);

/* DECODE STREAMS WHOSE SLOTS OVERLAP THEIR HISTORY (MINIMAL RINGS): the twin of lz4hip_decompress_safe_stream_batch that lifts its one
 * exclusion.  Same 13 arguments in the same order, same state record, same state machine, argument errors, window rules, sharding and
 * staging; what differs is what the BYTES are where a block's slot overlaps the history the block can reach -- the layouts liblz4
 * tells its users to use: the ring of LZ4_decoderRingBufferSize() / LZ4_DECODER_RING_BUFFER_SIZE (65536 + 14 + maxBlock), and small
 * rings kept in step with the encoder's (liblz4's ring-buffer streaming example).
 *   - THE CONTRACT is the plain definition: a block is decoded sequence by sequence; within a sequence the literals come first, then the
 *     match, byte by byte, forward; each byte is read at the moment it is due; nothing is stored past the last byte of a sequence.
 *     A match's source follows the state exactly as above: the prefix directly in front of the block, else offset - position bytes back
 *     from ext_end, and a match that runs past the dictionary's end continues at the prefix's start, or at the block's own start when
 *     there is no prefix.  out_len and the state written back are liblz4's on every input, as for the call above;
 *   - THE BYTES ARE LIBLZ4'S wherever liblz4 does not itself overwrite a source before reading it: on every block of every stream an
 *     encoder wrote that the tests decode in such rings (LZ4_compress_fast_continue on rings of 65536 + 14 + maxBlock that wrap when
 *     the block, or maxBlock, no longer fits, with the exact and with the full capacity; rings of 1024 .. 70000 bytes kept in step
 *     with the writer's), and on every hand-built stream whose match source lies 31 bytes or more ahead of its destination;
 *   - THE EXCEPTION: a match whose source lies less than 31 bytes AHEAD of its own destination.  liblz4 1.9.3's fast loop copies literals
 *     in 32-byte steps and its safe loop in 8-byte steps, past the run's end, so it overwrites such a source before the match reads
 *     it: measured on the tests' grid of hand-built two-block streams, liblz4 leaves the plain definition in 1017 of the
 *     3861 cases with a source 1 .. 30 bytes ahead and in none of the 4290 cases from 31 bytes on (with a short
 *     literal tail, where only its safe loop runs, and where the match runs past the dictionary's end into the block's own first
 *     bytes: 1 .. 8 bytes ahead alone).  There the engine's bytes are the plain definition's, not liblz4's.  Neither are they where a
 *     hand-built match has its source BEHIND its destination inside the overlapped dictionary and is longer than that distance:
 *     the plain definition reads what the match has just written (no encoder emits such a match).  The same arithmetic says where a real ring can come near it: in a minimal ring a source can lie as little as 16
 *     bytes ahead of the block's first byte, so a match at the largest offsets, decoded directly behind a literal run of 15 or more
 *     bytes, is where liblz4's own result depends on its copy widths -- no stream the tests' encoder wrote contains one, and this
 *     consequence is stated, not measured;
 *   - THE PER-BLOCK CHOICE: per block the walk tests, from the state it holds, whether [d, d + cap) intersects the piece of the external
 *     dictionary the block can reach -- the last min(ext_len, 65535 - min(prefix_len if the block grows the prefix else 0, 65535))
 *     bytes in front of ext_end, after a jump's ext = prefix (a growing prefix ends where the slot begins: it never overlaps).  Such
 *     a block is decoded by the in-order tier (exact-extent forward copies, every match source loaded behind a wait for every store
 *     of the sequences in front of it); every other block by exactly the code lz4hip_decompress_safe_stream_batch runs.
 *     lz4hip_set_option("dstream_inorder", 1) sends EVERY block of this call through the in-order tier (0, the default: the
 *     per-block test; any other value is LZ4HIP_E_ARG); where no slot overlaps, both settings give the same bytes, and the knob
 *     never touches lz4hip_decompress_safe_stream_batch;
 *   - THE RING RULE that now holds: any ring liblz4's own decoder accepts -- LZ4_DECODER_RING_BUFFER_SIZE(maxBlock) bytes
 *     (lz4hip_decoder_ring_buffer_size, below) and rings in step with the writer's -- with the exception above;
 *   - the two entry points may alternate on one stream from call to call: the state is plain host data and both read and write it alike;
 *   - one kernel, decode_stream_inorder_kernel, of decode_stream_kernel's shape.  Host pointers only, as the call above.             */
int lz4hip_decompress_safe_stream_inorder_batch(lz4hip_dstream_state* state, const uint8_t* src, const uint64_t* src_off,
                                                const int32_t* src_len, const uint32_t* chain_first, uint8_t* dst,
                                                const uint64_t* dst_off, const int32_t* dst_cap, const uint64_t* chain_win_off,
                                                const uint64_t* chain_win_len, int32_t* out_len, uint32_t n_blocks, uint32_t n_chains);
/* LZ4_decoderRingBufferSize(max_block) of liblz4 1.9.3: the smallest ring LZ4_decompress_safe_continue decodes blocks of up to max_block
 * bytes into -- 65536 + 14 + max(max_block, 16); 0 for a negative max_block or one above 0x7E000000.  Needs no device.              */
int lz4hip_decoder_ring_buffer_size(int max_block);

/* COMPRESS CHAINS OF LINKED BLOCKS: the return values and bytes of liblz4 1.9.3's streaming compressor in its prefix mode, acceleration 1
 * -- what lz4hip_decompress_safe_chain_batch* reads and what the lz4 command line writes by default.  A CHAIN is a run of blocks whose
 * SOURCES lie back to back in src; a match of block k may reach into the blocks before it and into history that lies directly in front
 * of the chain.  Chains are independent of each other; one launch compresses many of them.  With chain_src = src + chain_src_off[c]
 * and P = chain_prefix_len[c], the result for block k of chain c is
 *     s = LZ4_createStream();  if (P > 0) LZ4_loadDict(s, chain_src - P, P);
 *     r_k = LZ4_compress_fast_continue(s, chain_src + sum(src_len_j, j < k), dst_k, src_len_k, dst_cap_k, 1);
 * every source follows the previous one and the first follows the loaded history (never the external-dictionary mode):
 *   - chain c is the blocks [chain_first[c], chain_first[c + 1]) (n_chains + 1 entries, ascending from 0 to n_blocks); block i starts
 *     where block i - 1 of its chain ended and owns the slot dst[dst_off[i] .. + dst_cap[i]) -- the outputs are separate messages and
 *     need not be contiguous; chain_prefix_len == NULL: no chain has history.  Of a prefix only the last 65536 bytes count, and one
 *     under 8 bytes is unreachable (LZ4_loadDict loads nothing) although it still moves the stream's indexes;
 *   - out_len[i] > 0: the compressed size.  out_len[i] == 0: what liblz4 returns when the output does not fit (LZ4_compress_default's
 *     capacity rule), and also the result for src_len[i] < 0, dst_cap[i] < 0, and a block with which the chain's kept history, its
 *     consumed bytes and src_len[i] together would exceed 0x7E000000 (a chain never reaches liblz4's index renormalisation);
 *   - a block whose result is 0 ENDS ITS CHAIN (liblz4 goes on from there with a polluted table in another mode; nothing downstream
 *     of that is worth reproducing): every block behind it gets LZ4HIP_CHAIN_STOPPED.  chain_consumed[c] = the source bytes of the
 *     blocks that succeeded.  With dst_cap[i] >= lz4hip_compress_bound(src_len[i]) no block fails;
 *   - a block of 0 bytes is the single token 0x00 and the chain goes on; a block under 13 bytes is one literal run;
 *   - there is no single-call form: chains are the unit;
 *   - nothing outside [chain_src_off[c] - min(P, 65536), chain_src_off[c] + sum src_len) is read, nothing outside a block's slot is
 *     written.  Slots must not overlap;
 *   - LZ4HIP_E_ARG: a required pointer that is NULL (everything but chain_prefix_len), a chain_first that is not ascending from 0 to
 *     n_blocks, a negative chain_prefix_len[c] or one longer than chain_src_off[c].  These are said before a device is looked for;
 *   - one kernel, compress_fast_chain_cu_kernel: five wavefronts per CU with a 32 KB table each draw chains from a queue; a chain's
 *     table is cleared, or built from its prefix, once, and stays in LDS from one block to the next.  ONE CHAIN IS SERIAL BY
 *     CONSTRUCTION and runs on one wavefront; the kernel waits for no other wavefront anywhere, and parallelism comes from the
 *     number of chains alone.  The compress_* knobs do not apply;
 *   - the host form uploads each chain's source with the last min(P, 65536) bytes of its history, brings back only the bytes
 *     produced, and shards over the initialised devices at chain boundaries;
 *   - out of scope: LZ4_saveDict and resuming a stream's exact state across calls (the prefix is LZ4_loadDict's
 *     table, which is not the table a running stream would hold: continuing a stream in a second call gives valid, decodable, but
 *     other bytes than one long chain); sources that are not contiguous; LZ4_attach_dictionary.  (No longer out of scope: an HC form
 *     is lz4hip_compress_hc_chain_batch, below.)  (No longer out of scope: resuming a stream's exact state across calls, LZ4_saveDict
 *     included, is lz4hip_compress_fast_stream_batch, below.)  (No longer out of scope: sources that are not contiguous, on a
 *     resident stream, is lz4hip_compress_fast_stream_ext_batch, below.)  (No longer out of scope: acceleration above 1 is
 *     lz4hip_compress_fast_chain_accel_batch, below.)                                                                               */
int lz4hip_compress_fast_chain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                     const int32_t* src_len, const uint32_t* chain_first,
                                     uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                     int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains);
/* LINKED BLOCKS WITH AN ACCELERATION: the three linked-block fast compressors -- chains (above), resident streams and resident streams
 * whose sources land anywhere (lz4hip_compress_fast_stream_batch and lz4hip_compress_fast_stream_ext_batch, below) -- with the last
 * argument of LZ4_compress_fast_continue(stream, src, dst, srcSize, dstCapacity, acceleration), liblz4 1.9.3.  Each has the argument
 * list of its acceleration-1 twin plus a trailing `int acceleration`, and the twin's contract word for word; these are the blocks that
 * `lz4 --fast=N` writes (the lz4 command line links blocks by default and hands N to that call).
 *   - ONE acceleration per call, for every block of every chain or stream in it.  It is clamped as liblz4 does: < 1 -> 1, > 65537
 *     (LZ4_ACCELERATION_MAX) -> 65537;
 *   - after clamping, acceleration 1 IS the twin: same call, same kernels, same bytes (as lz4hip_compress_fast_accel_batch is
 *     lz4hip_compress_fast_batch at 1);
 *   - acceleration changes where a miss run probes and nothing else: every run starts with liblz4's searchMatchNb = acceleration << 6
 *     instead of 1 << 6, and the table's contents follow from that.  Return values' meaning, the stop rule (a result of 0 ends the
 *     chain or stops the stream), the 0x7E000000 limit, blocks under 13 bytes, the prefix and history rules, argument errors, sharding
 *     and staging are the twins';
 *   - a stream's record and 32 KB table image keep their format: one stream may be driven by any mix of the six entry points, at a
 *     different acceleration in every call.  The table a call leaves depends on its acceleration, and a later call sees that, at any
 *     acceleration, as liblz4's does: the bytes are those of ONE LZ4_stream_t given the same sequence of accelerations;
 *   - kernels: compress_fast_chain_accel_cu_kernel, compress_fast_stream_accel_cu_kernel, compress_fast_xstream_accel_cu_kernel --
 *     their twins' shape (one wavefront per chain or stream, the table in LDS) over the one-sequence core's acceleration switch.  The
 *     acceleration-1 kernels are instruction for instruction what they were (profiles/caccel_kernel_diff.txt);
 *   - bit-exactness was shown against the reference library's own LZ4_compress_fast_continue on one LZ4_stream_t per chain or stream:
 *     in the CPU lane simulator with its bounds checks on (tests/test_caccel_hostsim.py) and on the MI355X (tests/test_gpu_caccel.py);
 *   - NO device-pointer (`*_dev`) forms: as for the stream families, they are left to a change that can also extend the far-offset and
 *     stream-contract tables of the device entry points;
 *   - out of scope: a per-block acceleration array; acceleration in the dictionary-handle form (lz4hip_compress_fast_dict*), which
 *     remains the only fast form without it; device-pointer forms; LZ4_attach_dictionary; acceleration in the lean and
 *     window-parallel block cores (acceleration 1 alone runs on them); byte equality with whole FRAMES written by the lz4 command
 *     line -- header flags and block sizes are its own; the blocks are what is matched.                                             */
int lz4hip_compress_fast_chain_accel_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                           const int32_t* src_len, const uint32_t* chain_first,
                                           uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                           int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                                           int acceleration);
/* COMPRESS CHAINS OF LINKED BLOCKS AT AN HC LEVEL: the arrays of lz4hip_compress_fast_chain_batch without chain_consumed, and a level.
 * With chain_src = src + chain_src_off[c] and P = chain_prefix_len[c], block k of chain c is, byte for byte and in its return value,
 *     s = LZ4_createStreamHC();  LZ4_resetStreamHC_fast(s, level);  if (P > 0) LZ4_loadDictHC(s, chain_src - P, P);
 *     r_k = LZ4_compress_HC_continue(s, chain_src + sum(src_len_j, j < k), dst_k, src_len_k, dst_cap_k);
 * of liblz4 1.9.3: always its prefix mode, never the external-dictionary mode.  These are the linked blocks the lz4 command line
 * writes at -3 and above; lz4hip_decompress_safe_chain_batch* reads them.
 *   - levels are clamped as everywhere (< 1 -> 9, > 12 -> 12); levels 10..12 are functional only, as for lz4hip_compress_hc*;
 *   - of the history only its last 65536 bytes count, and it has no minimum length (LZ4_loadDictHC has none);
 *   - out_len[i] > 0: the compressed size.  out_len[i] == 0: liblz4 returns 0 -- dst_cap[i] is below the bound and the output does
 *     not fit, or src_len[i] > 0x7E000000 -- and also the result for dst_cap[i] < 0 and src_len[i] < 0 (such a block counts as 0
 *     bytes for the positions of the blocks behind it);
 *   - A BLOCK WHOSE RESULT IS 0 DOES NOT END ITS CHAIN, unlike the fast chain's: liblz4 has taken its source into the stream's
 *     history by then, so the blocks behind it are exactly what they would have been, and that is what they are here.  No
 *     LZ4HIP_CHAIN_STOPPED exists in this call;
 *   - a block of 0 bytes is the single token 0x00; a block under 13 bytes is one literal run;
 *   - there is no single-call form: chains are the unit;
 *   - nothing outside [chain_src_off[c] - min(P, 65536), chain_src_off[c] + sum max(src_len, 0)) is read, nothing outside a block's
 *     slot is written (every store is exact).  Slots must not overlap;
 *   - LZ4HIP_E_ARG: a required pointer that is NULL (everything but chain_prefix_len), a chain_first that is not ascending from 0 to
 *     n_blocks, a negative chain_prefix_len[c] or one longer than chain_src_off[c].  These are said before a device is looked for;
 *   - NOT SERIAL: HC's chain table is a function of the data alone, and block k's bytes depend only on the 64 KB in front of it, the
 *     block, the level and the capacity.  Every block of every chain is parsed at the same time, one wavefront per block
 *     (hc_parse_chain_kernel), behind a chain table built over each chain's buffer in segments ("hc_chain_segment" of
 *     lz4hip_set_option: 4096 .. 2^30 positions, default 1 MiB; every value gives the same bytes) that workgroups draw from a queue
 *     (hc_build_chain_kernel): a single long chain fills the device;
 *   - the call takes host pointers: it uploads each chain's source with the last min(P, 65536) bytes of its history, brings back only
 *     the bytes produced, and shards over the initialised devices at chain boundaries.  A stream that is cut in several places is
 *     best passed as ONE chain (it is parallel anyway);
 *   - out of scope: device-pointer forms (the chain workspace is indexed by source offset and the layout needs scratch of its
 *     own; they are left to a change that can also extend the far-offset table of the device entry points);
 *     LZ4_attach_HC_dictionary; a destSize form; favorDecSpeed; byte equality with the FRAMES the lz4 command line writes (its
 *     frame layer moves its dictionary).  (No longer out of scope: LZ4_saveDictHC and sources that are not contiguous are
 *     lz4hip_compress_hc_stream_batch, below.)                                                                                    */
int lz4hip_compress_hc_chain_batch(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                   const int32_t* src_len, const uint32_t* chain_first,
                                   uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                   int32_t* out_len, uint32_t n_blocks, uint32_t n_chains, int level);
/* COMPRESS HC STREAMS WHOSE SOURCES LAND ANYWHERE -- a ring that wraps, two alternating buffers, a save area (LZ4_saveDictHC), a
 * dictionary elsewhere -- and that are continued by any number of calls.  Stream c of a call is the blocks [chain_first[c],
 * chain_first[c + 1]); every block has ITS OWN src_off[i].
 * THE CONTRACT: for every stream, the results are byte for byte and return value for return value what ONE LZ4_streamHC_t of liblz4
 * 1.9.3 gives over all calls -- s = LZ4_createStreamHC(); LZ4_resetStreamHC_fast(s, level); then
 * LZ4_compress_HC_continue(s, src + src_off[i], dst_i, src_len[i], dst_cap[i]) per block -- however the blocks are cut into calls, with
 * the exceptions stated below.
 *   - THE STATE is plain host data, as lz4hip_dstream_state is: state[c] is read in front of stream c's first block of the call and
 *     written back behind its last.  There is no handle and no device memory between calls.  All zero is a fresh stream.  The prefix is
 *     [prefix_end - prefix_len, prefix_end), the external dictionary [ext_end - ext_len, ext_end), both as offsets into this call's src
 *     (liblz4's end, dictLimit, lowLimit and dictBase + dictLimit); index counts the bytes loaded plus consumed and exists for the life
 *     limit only.  These are functions of addresses and lengths alone, never of compressed results;
 *   - the state machine per block [s, s + n), s = src_off[i], n = src_len[i]:
 *       1. s != prefix_end (a jump): the prefix becomes the external dictionary (the old one is dropped), prefix_len = 0,
 *          prefix_end = s.  On an all-zero state this changes nothing;
 *       2. ext_len > 0 and s + n > ext_end - ext_len and s < ext_end (the source overlaps the external dictionary):
 *          ext_len = ext_end - min(s + n, ext_end), and under 4 bytes it becomes 0;
 *       3. the block is compressed; the capacity rule is LZ4_compress_HC_continue's (limited output below the bound);
 *       4. prefix_len += n, prefix_end = s + n, index += n;
 *   - what follows: the history in reach is the last 65535 bytes of external dictionary ++ prefix; a match that runs to the external
 *     dictionary's end goes on at the prefix's start; the backward extension of a match stops at the start of the piece the match lies
 *     in; the last three positions of every contiguous run that a jump ended are never match candidates (liblz4 never inserts them);
 *   - out_len[i] == 0: it does not fit, or dst_cap[i] < 0.  A RESULT OF 0 DOES NOT END THE STREAM, as in lz4hip_compress_hc_chain_batch:
 *     the block's source is history for the blocks behind it;
 *   - the engine's rule for src_len[i] < 0 or > 0x7E000000: the result is 0, step 1 alone is applied, nothing is consumed;
 *   - lz4hip_hcstream_load_dict is LZ4_loadDictHC as a state edit: {dict_end, min(dict_len, 65536), 0, 0, min(dict_len, 65536)}.  A
 *     first block that follows the dictionary runs in prefix mode, one elsewhere in external-dictionary mode: a fresh stream with a
 *     dictionary elsewhere and one block is lz4hip_compress_hc_dict*'s block;
 *   - lz4hip_hcstream_save_dict(st, buf_off, k) is LZ4_saveDictHC as a state edit, for the caller who has copied the prefix's last
 *     bytes to src + buf_off: kept = min(k, 65536), below 4 it is 0, then min(kept, prefix_len); the history is those bytes, ending at
 *     buf_off + kept, and the external dictionary is dropped.  Returns kept (LZ4HIP_E_ARG for a NULL state);
 *   - A CALL IS A SNAPSHOT: all blocks of a call are read from src as it is during the call.  A producer that writes over its ring
 *     ends the call in front of the first block whose bytes land on anything an earlier block of the same call reads -- its source,
 *     or the history it can reach -- as a caller of liblz4 compresses a block before it writes the next over old data;
 *   - levels are clamped as everywhere (< 1 -> 9, > 12 -> 12).  LEVELS 1..9 HAVE NO EXCEPTION to byte equality but one that liblz4
 *     itself leaves to the memory layout: its 2-byte pre-test of a prefix candidate may read up to look-back bytes in front of the
 *     prefix's first byte, whatever lies there in the caller's memory; the engine reads the external dictionary's last bytes there.
 *     LEVELS 10..12: where the optimal parser's chain swap reads the chain entry of a position liblz4 never inserted (the three in
 *     front of a jump), liblz4 reads a stale entry of its 64 K ring; here such a position has the entry 0 and never matches (the rule
 *     of lz4hip_compress_hc_dict*).  On a stream younger than 64 KB the stale entry is 0 and the bytes are liblz4's; on an older
 *     one a block may differ (both outputs are valid LZ4);
 *   - NOT SERIAL, like the chain call: the host walks the state machine and lays every stream out as one buffer in liblz4's own index
 *     space -- the kept external piece (only while the prefix is shorter than 65535 bytes), the kept prefix piece (at most 65536
 *     bytes), the call's blocks -- in which a jump is contiguous; every block of every stream is parsed at once, one wavefront per block
 *     (hc_parse_stream_kernel), behind a chain table built over the buffers in segments ("hc_chain_segment") that skips the never
 *     inserted positions (hc_build_stream_kernel).  Only the bytes produced come back; the call shards over the initialised devices at
 *     stream boundaries;
 *   - nothing outside the call's sources and the kept pieces of the two histories is read, nothing outside a block's slot is written.
 *     Slots must not overlap;
 *   - LZ4HIP_E_ARG, said before a device is looked for: a NULL pointer (all are required), a chain_first that is not ascending from 0 to
 *     n_blocks, a prefix_len longer than prefix_end or an ext_len longer than ext_end, a stream whose 65536 + index would pass 2^31
 *     during the call (liblz4 reloads its dictionary there; that reload is out of scope).  Without a device a well-formed call is
 *     LZ4HIP_E_NO_DEVICE;
 *   - out of scope: device-pointer forms; LZ4_attach_HC_dictionary; LZ4_compress_HC_continue_destSize; favorDecSpeed; the 2 GiB
 *     reload.                                                                                                                      */
typedef struct lz4hip_hcstream_state { uint64_t prefix_end, prefix_len, ext_end, ext_len, index; } lz4hip_hcstream_state;   /* all zero: a fresh stream */
int lz4hip_compress_hc_stream_batch(lz4hip_hcstream_state* state, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                    const uint32_t* chain_first, uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                    int32_t* out_len, uint32_t n_blocks, uint32_t n_chains, int level);
int lz4hip_hcstream_load_dict(lz4hip_hcstream_state* st, uint64_t dict_end, uint64_t dict_len);
int lz4hip_hcstream_save_dict(lz4hip_hcstream_state* st, uint64_t buf_off, int k);
/* COMPRESS STREAMS THAT ARE CONTINUED BY ANY NUMBER OF CALLS: a set of n_streams compress streams whose state -- the hash table and the
 * index position, what an LZ4_stream_t carries beside its history -- is RESIDENT ON THE DEVICE between calls.  The arrays of
 * lz4hip_compress_fast_stream_batch are lz4hip_compress_fast_chain_batch's, with one addition: chain c of a call is the next run of
 * blocks of stream stream_id[c].  stream_id is STRICTLY ASCENDING: a stream appears at most once per call.
 * THE CONTRACT: for every stream, the results are byte for byte and return value for return value what ONE LZ4_stream_t of liblz4
 * 1.9.3 gives over all the calls that ever named the stream since its creation or last reset, however the blocks were cut into calls.
 *   - a fresh stream (created, or reset) is exactly lz4hip_compress_fast_chain_batch's chain: LZ4_loadDict of chain_prefix_len[c] bytes
 *     when that is above 0, then LZ4_compress_fast_continue block by block, with all its rules (the 8-byte minimum of a prefix, the
 *     indexes starting at 65536 behind a prefix, blocks under 13 bytes);
 *   - a stream that has run before continues in liblz4's prefix mode: the source follows directly behind chain_prefix_len[c] bytes in
 *     src, and those bytes must be the last bytes the stream consumed (or loaded).  That is the caller who left the data in place, and
 *     the caller who called LZ4_saveDict(s, buf, k) and put the next block behind buf + k.  The history that counts is
 *     min(chain_prefix_len[c], 65536, what the stream holds); a shorter one than the stream holds is LZ4_saveDict with a smaller size
 *     (candidates below it are refused, liblz4's dictSmall rule) and is what the stream holds from then on.  There is no 8-byte
 *     minimum here.  chain_prefix_len[c] == 0 (or chain_prefix_len == NULL) on a stream that has run is legal and is NOT a reset;
 *   - out_len, chain_consumed (this call's bytes) and LZ4HIP_CHAIN_STOPPED behave as for the chain call.  A block whose result is 0
 *     stops its STREAM: the rest of the call's blocks and every block of later calls get LZ4HIP_CHAIN_STOPPED, and nothing is
 *     consumed, until the stream is reset;
 *   - the index limit applies to the stream's life: a block with which loaded history + everything consumed since the reset +
 *     src_len[i] would pass 0x7E000000 gives 0 and stops the stream.  A STREAM CARRIES JUST UNDER 2 GiB BETWEEN RESETS;
 *   - a call that fails with a library status after its launch leaves EVERY stream it named stopped (on several devices too, where part
 *     of the call may have succeeded); streams a call does not name are untouched;
 *   - lz4hip_cstreams_reset makes the n listed streams (NULL: all of them) fresh; lz4hip_cstreams_consumed reports, for the streams
 *     [first, first + n), the bytes consumed since the reset and whether the stream is stopped (either array may be NULL);
 *   - calls on one set are serialised (as the streaming-xxhash handles are); different sets are independent.  lz4hip_cstreams_free
 *     waits for a call in flight but must not race with one: no call may arrive while or after the set is freed.  Sets are freed before
 *     lz4hip_shutdown();
 *   - LZ4HIP_E_ARG, said before a device is looked for: a NULL set or required pointer, ids that are not strictly ascending or are
 *     >= n_streams, a chain_first that is not ascending from 0 to n_blocks, a negative chain_prefix_len[c] or one longer than
 *     chain_src_off[c].  Without a device lz4hip_cstreams_create and the compress call are LZ4HIP_E_NO_DEVICE;
 *   - DEVICE MEMORY: a 32 KB table image plus a 32-byte record per stream (65536 streams are about 2 GiB); lz4hip_cstreams_create
 *     answers LZ4HIP_E_NOMEM.  The streams are divided into contiguous id ranges over the devices initialised at create, and a
 *     call is sharded at those boundaries;
 *   - one kernel, compress_fast_stream_cu_kernel: compress_fast_chain_cu_kernel's shape; a wavefront that draws a stream loads its
 *     table image into LDS (or builds the fresh table), walks the call's blocks and stores table and record back: 64 KB of state
 *     traffic per stream and call, whatever its blocks' sizes;
 *   - the host form uploads each chain's source with the last min(chain_prefix_len[c], 65536) bytes in front of it and brings back
 *     only the bytes produced;
 *   - out of scope: a device-pointer form (as for lz4hip_compress_hc_chain_batch: left to a change that can also extend the far-offset
 *     table of the device entry points); the external-dictionary mode (a source that does not follow its
 *     history); LZ4_attach_dictionary; an HC form; streams longer than the index limit.  (No longer out of scope: the
 *     external-dictionary mode is lz4hip_compress_fast_stream_ext_batch, below.)  (No longer out of scope: acceleration above 1 is
 *     lz4hip_compress_fast_stream_accel_batch -- LINKED BLOCKS WITH AN ACCELERATION, above; it has no device-pointer form either.) */
typedef struct lz4hip_cstreams lz4hip_cstreams;
int lz4hip_cstreams_create(uint32_t n_streams, lz4hip_cstreams** out);
int lz4hip_cstreams_count(const lz4hip_cstreams* set);
int lz4hip_cstreams_reset(lz4hip_cstreams* set, const uint32_t* stream_id, uint32_t n);
int lz4hip_cstreams_consumed(lz4hip_cstreams* set, uint32_t first, uint32_t n, uint64_t* consumed, uint8_t* stopped);
void lz4hip_cstreams_free(lz4hip_cstreams* set);
int lz4hip_compress_fast_stream_batch(lz4hip_cstreams* set, const uint32_t* stream_id,
                                      const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                      const int32_t* src_len, const uint32_t* chain_first,
                                      uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                      int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains);
int lz4hip_compress_fast_stream_accel_batch(lz4hip_cstreams* set, const uint32_t* stream_id,
                                            const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                            const int32_t* src_len, const uint32_t* chain_first,
                                            uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                            int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                                            int acceleration);
/* COMPRESS STREAMS WHOSE SOURCES LAND ANYWHERE -- a ring that wraps, two alternating buffers, a save area, a dictionary elsewhere: the
 * same sets, the same streams and THE SAME CONTRACT as lz4hip_compress_fast_stream_batch: for every stream, byte for byte and return
 * value for return value what ONE LZ4_stream_t of liblz4 1.9.3 gives over all the calls that named the stream since its creation or
 * last reset -- through both entry points, in any interleaving, however the blocks are cut into calls.  What is new: every block has
 * ITS OWN src_off[i], and a block whose source does not follow the stream's history runs in liblz4's external-dictionary mode.
 *   - where the history lies: per call and stream, it ends at chain_hist_end[c] in this call's src, with chain_hist_len[c] bytes of it
 *     present.  What counts is min(chain_hist_len[c], 65536, what the stream holds); a shorter value than the stream holds is
 *     LZ4_saveDict with a smaller size, as for the call above.  After the call the history ends where the stream's last block of
 *     one byte and more ended, and the caller says so in the next call (or where it has moved the bytes to);
 *   - a fresh stream loads those bytes as LZ4_loadDict does (the 8-byte minimum, indexes from 65536).  A fresh stream whose first
 *     block does not follow that history is lz4hip_compress_fast_dict*'s block, byte for byte;
 *   - the state machine per block, LZ4_compress_fast_continue's.  D = [D_end - D_len, D_end) is the history, the block is
 *     [s, s + n), s = src_off[i]:
 *       1. D_len < 4 and D_end != s: the history is dropped;
 *       2. s + n > D_end - D_len and s + n < D_end (the source overlaps its own history): D_len = D_end - (s + n), at most 64 KB, and
 *          under 4 bytes it becomes 0;
 *       3. D_end == s: prefix mode, the block of the call above; candidates below idx - D_len are refused while D_len < 64 KB and
 *          D_len < idx; afterwards D_len += n, D_end = s + n;
 *       4. otherwise external-dictionary mode: the indexes [idx - D_len, idx) name the bytes of D, those from idx on the block; the same
 *          lower bound; a match that reaches D_end goes on at the block's start; the backward catch-up stops at the start of the
 *          buffer the match lies in.  Afterwards D is the block alone: D_end = s + n, D_len = n (a block of 0 bytes at a jump drops the
 *          history entirely);
 *       5. idx += n.
 *   - A CALL IS A SNAPSHOT: all blocks of a call are read from src as it is during the call.  A producer that writes over its ring
 *     ends the call in front of the first block whose bytes land on anything an earlier block of the same call reads -- its source,
 *     or the history it can reach -- as a caller of liblz4 compresses a block before it writes the next over old data;
 *   - a source that runs over the END of its history (rule 2 catches only one that ends inside it) sees the history as it is now,
 *     as liblz4 does.  ONE EXCEPTION to byte equality: such a source that begins EXACTLY at its history's first byte (one reused
 *     buffer, a longer block than the one before).  liblz4 then takes matches inside the block for dictionary matches and cuts them
 *     short; the engine finds the ordinary, longer ones.  Return values may differ by a few bytes; both outputs are valid LZ4.  The
 *     input is misuse either way: the history was overwritten, and liblz4's own output does not decode there;
 *   - the table is byU32, acceleration 1 (any acceleration: lz4hip_compress_fast_stream_ext_accel_batch); a block under 13 bytes is
 *     one literal run that still moves the index space; the 0x7E000000 life limit, a result of 0 stopping the stream,
 *     LZ4HIP_CHAIN_STOPPED, chain_consumed, lz4hip_cstreams_reset and lz4hip_cstreams_consumed, and what a library failure after the
 *     launch leaves behind are the call above's;
 *   - the window: every source [src_off[i], + src_len[i]) of stream c lies inside [chain_win_off[c], + chain_win_len[c]) -- the ring,
 *     the pair of buffers, the save area plus the block area.  The history PIECE, the last min(chain_hist_len[c], 65536) bytes in front
 *     of chain_hist_end[c], lies wholly inside the window or wholly outside it; one that ends exactly at the window's start stays
 *     contiguous with it (a caller whose dictionary leads into the window widens the window once the history has grown out of the
 *     dictionary).  Outside pieces may be shared by streams.  Sources are only read: windows of different streams may overlap.
 *     Destination slots may not overlap;
 *   - nothing outside the call's sources and history pieces is read, nothing outside a block's slot is written;
 *   - LZ4HIP_E_ARG, said before a device is looked for: a NULL set or pointer (ALL pointers are required), ids that are not strictly
 *     ascending or are >= n_streams, a chain_first that is not ascending from 0 to n_blocks, a source outside its window, a history
 *     piece that straddles a window edge, a chain_hist_len[c] longer than chain_hist_end[c], a negative chain_hist_len[c].  Without
 *     a device a well-formed call is LZ4HIP_E_NO_DEVICE;
 *   - one kernel, compress_fast_xstream_cu_kernel: compress_fast_stream_cu_kernel's shape and state traffic; per block the walk
 *     chooses, on wave-uniform values, between the linked-block core and the core that is linked-block and dictionary at once;
 *   - the host form mirrors the USED part of every window on the device (the call's sources and the history piece), uploads each
 *     outside piece once per staged chunk, brings back only the bytes produced, and shards at the set's device ranges;
 *   - out of scope: device-pointer forms (as above: left to a change that can also extend the far-offset and stream-contract tables
 *     of the device entry points); LZ4_attach_dictionary; an HC form; streams past the index limit.  (No longer out of scope:
 *     acceleration above 1 is lz4hip_compress_fast_stream_ext_accel_batch -- LINKED BLOCKS WITH AN ACCELERATION, above; no
 *     device-pointer form either.)                                                                                                 */
int lz4hip_compress_fast_stream_ext_batch(lz4hip_cstreams* set, const uint32_t* stream_id,
                                          const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const uint32_t* chain_first,
                                          const uint64_t* chain_hist_end, const int32_t* chain_hist_len,
                                          const uint64_t* chain_win_off, const uint64_t* chain_win_len,
                                          uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                          int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains);
int lz4hip_compress_fast_stream_ext_accel_batch(lz4hip_cstreams* set, const uint32_t* stream_id,
                                                const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, const uint32_t* chain_first,
                                                const uint64_t* chain_hist_end, const int32_t* chain_hist_len,
                                                const uint64_t* chain_win_off, const uint64_t* chain_win_len,
                                                uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                                int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                                                int acceleration);
/* COMPRESS AGAINST A DICTIONARY: for every block i, on a fresh stream,
 *     LZ4_loadDict(s, dict, dict_len);  LZ4_compress_fast_continue(s, src_i, dst_i, src_len[i], dst_cap[i], 1)
 * of liblz4 1.9.3 with a dictionary that is NOT contiguous with the source (its external-dictionary mode): the return value and the
 * bytes, byte for byte.  Blocks are independent, nothing carries over from one to the next; lz4hip_decompress_safe_dict* reads them.
 *   - out_len[i] > 0 is the compressed size; 0: dst_cap[i] is too small (LZ4_compress_default's capacity rule), or src_len[i] < 0,
 *     src_len[i] > 0x7E000000 or dst_cap[i] < 0;
 *   - every block is parsed with liblz4's byU32 table whatever its size, so an empty dictionary does NOT give
 *     lz4hip_compress_fast's bytes for blocks under 65547 bytes (from there on it does);
 *   - only the dictionary's last 64 KB count, and a dictionary of fewer than 8 bytes is none (LZ4_loadDict returns 0);
 *   - a match may start in the dictionary (its offset then exceeds its position in the block) and, where it runs to the dictionary's
 *     end, goes on against the block's own start; the dictionary's last 7 positions are never match candidates;
 *   - nothing outside the dictionary's kept bytes and block i's source is read, nothing outside block i's slot is written;
 *   - the handle is the decoder's (lz4hip_dict_create).  The compressor also needs the table LZ4_loadDict leaves: 32 KB of device
 *     memory per device, built by a kernel at the handle's first compress on that device (that one call waits for its stream once;
 *     a handle that only decodes never has one) and freed by lz4hip_dict_free;
 *   - one kernel, compress_fast_dict_cu_kernel: the one-sequence core with its DICT switch, five wavefronts per CU, each loading its
 *     table from the image per block; acceleration is 1 (the only fast form without the knob), there is no attach-dictionary or
 *     prefix form and no LZ4_saveDict (the HC form is lz4hip_compress_hc_dict* below);
 *   - dict == NULL is LZ4HIP_E_ARG, no device LZ4HIP_E_NO_DEVICE; the host batch shards over the initialised devices and brings
 *     back only the bytes each block produced, as lz4hip_compress_fast_batch does;
 *   - single calls (lz4hip_compress_fast_dict) are coalesced only with concurrent compress calls on the SAME handle.            */
int lz4hip_compress_fast_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                    uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                    int32_t* out_len, uint32_t n_blocks, const lz4hip_dict* dict);
/* HC COMPRESS AGAINST A DICTIONARY: for every block i, on a fresh stream,
 *     LZ4_resetStreamHC_fast(s, level);  LZ4_loadDictHC(s, dict, dict_len);
 *     LZ4_compress_HC_continue(s, src_i, dst_i, src_len[i], dst_cap[i])
 * of liblz4 1.9.3 with a dictionary that is NOT contiguous with the source (its external-dictionary mode): the return value and the
 * bytes, byte for byte.  Blocks are independent, nothing carries over from one to the next; lz4hip_decompress_safe_dict* reads them.
 *   - out_len[i] > 0 is the compressed size; 0 where liblz4 returns 0 (dst_cap[i] below the bound and the output does not fit, or
 *     src_len[i] > 0x7E000000) and for a negative src_len[i] or dst_cap[i], as for lz4hip_compress_hc*;
 *   - levels as for lz4hip_compress_hc*: < 1 -> 9, > 12 -> 12; 1..9 the hash chain with lazy evaluation (9: pattern analysis),
 *     10..12 the optimal parser (functional only);
 *   - only the dictionary's last 64 KB count and there is no minimum length: a dictionary of 4 bytes has one candidate position,
 *     one of 0..3 bytes has none.  The dictionary's last three positions are never match candidates;
 *   - a match may start in the dictionary (its offset then exceeds its position in the block) and, where it runs to the dictionary's
 *     end, goes on against the block's own start;
 *   - nothing outside the dictionary's kept bytes and block i's source is read, nothing outside block i's slot is written.  One
 *     consequence: where the chain swap of levels 10..12 lands on one of the dictionary's last three positions, liblz4 compares
 *     bytes behind the dictionary's end; here such a position never matches;
 *   - the handle is the decoder's (lz4hip_dict_create).  The HC compressor also needs what LZ4_loadDictHC leaves -- the head table
 *     and the dictionary's chain deltas: 128 KB + 2 bytes per kept byte of device memory per device --, built by a kernel
 *     (hc_dict_image_kernel) at the handle's first HC compress on that device: that one call waits for its stream once.  The image
 *     does not depend on the level, exists beside the fast compressor's, and is freed by lz4hip_dict_free;
 *   - kernels: hc_build_dict_kernel (hc_build_kernel's twin; each record's head table starts as the image's, 128 KB read per record
 *     whatever its size) and hc_parse_dict_kernel (hc_parse_kernel's twin); the workspace is lz4hip_hc_workspace_bytes, unchanged;
 *     there is no attach-dictionary, prefix or destSize form and no LZ4_saveDict; no existing entry point changed behaviour;
 *   - dict == NULL is LZ4HIP_E_ARG, no device LZ4HIP_E_NO_DEVICE; the host batch shards over the initialised devices and brings
 *     back only the bytes each block produced;
 *   - single calls (lz4hip_compress_hc_dict) are coalesced only with concurrent calls on the SAME handle at the same clamped level. */
int lz4hip_compress_hc_dict_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                  uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                  int32_t* out_len, uint32_t n_blocks, int level, const lz4hip_dict* dict);
int lz4hip_compress_hc_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                             uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                             int32_t* out_len, uint32_t n_blocks, int level);
/* HC COMPRESS TO A TARGET SIZE: the bytes, return value and consumed size of LZ4_compress_HC_destSize(state, src, dst, &srcSize,
 * targetDstSize, level), liblz4 1.9.3: as much of block i as fits in exactly target_size[i] bytes, parsed at HC level `level`
 * (clamped as for lz4hip_compress_hc*: < 1 -> 9, > 12 -> 12; 1..9 the hash chain with lazy evaluation, 10..12 the optimal parser).
 *   - out_len[i] is liblz4's return value: the bytes written (<= target_size[i]), 0 for target_size[i] < 1 and for src_len[i] < 0
 *     or > 0x7E000000; an empty block gives the single token 0x00 (1 byte) for any target >= 1;
 *   - src_consumed[i] is what liblz4 leaves in *srcSizePtr: the input bytes the output covers (decoding out_len[i] bytes gives back
 *     exactly src[0 .. src_consumed[i])), and src_len[i] itself where it returns 0 up front;
 *   - liblz4 makes its fillOutput checks whatever the target: the sequence that fails one has its match cut (or is dropped) and the
 *     last literals are shortened to fit; a target that no check fails for gives the bytes of lz4hip_compress_hc, all input consumed;
 *   - block i's slot is dst[dst_off[i] .. + target_size[i]): nothing is written at or past its end;
 *   - two kernels: hc_build_kernel as for lz4hip_compress_hc*, then hc_parse_dest_kernel (one wavefront per block, the parser of
 *     lz4_hc_core.h with its FILL switch).  The parse of a block stops once its target is full, so the parse time follows the input
 *     consumed; the chain-delta build still covers the whole block;
 *   - levels 10..12 are functional only, as they are for lz4hip_compress_hc*;
 *   - the host batch shards over the initialised devices, returns only the useful bytes of every slot as the fast destSize path does
 *     and brings src_consumed back with the sizes; library failures as the status of the call;
 *   - single calls (lz4hip_compress_hc_dest_size) are coalesced with concurrent HC destSize calls of the SAME clamped level only,
 *     through combiners of their own.                                                                                              */
int lz4hip_compress_hc_dest_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                       uint8_t* dst, const uint64_t* dst_off, const int32_t* target_size,
                                       int32_t* out_len, int32_t* src_consumed, uint32_t n_blocks, int level);
int lz4hip_decompress_safe_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                 uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                 int32_t* out_len, uint32_t n_blocks);
/* DECODED SIZE, NO OUTPUT BUFFER: out_len[i] is the value LZ4_decompress_safe(src_i, dst, src_len[i], dst_cap[i]) of liblz4 1.9.3
 * returns -- the decoded size, or -(input position) - 1 -- for every input, valid or malformed.  There is no dst: that value never
 * depends on the bytes a destination holds, only on the stream, its length and the capacity, so the kernel moves through the block
 * without copying anything.  For a batch of blocks whose decoded sizes are unknown or untrusted this replaces a decode into
 * worst-case slots (a block can expand 255 times).
 *   - dst_cap[i] is an argument, not a buffer size: liblz4's three tiers are chosen by the distance to the output's end, so which
 *     malformed streams are accepted depends on it.  out_len[i] >= 0 means that lz4hip_decompress_safe* with that capacity succeeds
 *     and returns exactly that number: the query is a validator too;
 *   - to learn the size of a block of unknown size pass an upper bound (at most 255 * src_len[i], or the format's block limit);
 *   - a negative src_len[i] or dst_cap[i] gives -1, as for the decoders;
 *   - one kernel, decode_size_kernel: a wavefront per block, the stream read once through an LDS ring (it reads the compressed
 *     bytes and writes 4 bytes per block); no route, no decode_* knob applies;
 *   - the host batch shards over the initialised devices; it stages the streams only -- no destination is allocated or copied on
 *     either side; library failures as the status of the call;
 *   - single calls (lz4hip_decompressed_size) are coalesced with concurrent size queries only, through a combiner of their own. */
int lz4hip_decompressed_size_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                   const int32_t* dst_cap, int32_t* out_len, uint32_t n_blocks);
/* FAST DECODER CONTRACT.  src_cap[i] bounds how far block i may be read (the Java array/buffer length past srcOff):
 * unlike liblz4's LZ4_decompress_fast (which trusts the stream and reads wherever it points) this implementation never reads
 * beyond src_cap[i] bytes of the source slot and never before the destination slot.
 *   - valid stream whose decoded size is dst_len[i]: out_consumed[i] = the compressed length, dst = the decoded bytes --
 *     identical to LZ4_decompress_fast (LZ4JNI.c:169);
 *   - anything else (truncated / corrupted / random bytes, wrong dst_len): liblz4's own decode loop with ONE change -- a read
 *     that would leave the source slot, or an offset that would reach before the destination, is the error at that point:
 *     out_consumed[i] = -(input position) - 1.  Streams liblz4 happens to accept while reading garbage past the slot are
 *     therefore rejected here; streams liblz4 rejects are rejected with the same code when the rejection does not depend on
 *     bytes outside the slot.
 * The behaviour is pinned by 600 vectors in tests/golden/fast_decode_contract.json (generated from oracle/lz4_oracle.c
 * lz4o_decompress_fast_bounded; its valid cases are cross-checked against the reference library) and tested on the CPU
 * (tests/test_oracle.py; tests/test_fast_contract_hostsim.py: one loop of every decoder family in the lane simulator) and on
 * the GPU (tests/test_gpu_scale.py; tests/test_gpu_fast_contract.py: valid, damaged, cut and padded streams through the fast
 * decoder of EVERY decode kernel and batch-size route, twice, with different bytes around every source and destination slot --
 * the cases and the layout are tests/fast_contract_common.py's).                                                           */
int lz4hip_decompress_fast_batch(const uint8_t* src, const uint64_t* src_off, const int32_t* src_cap,
                                 uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_len,
                                 int32_t* out_consumed, uint32_t n_blocks);
int lz4hip_xxh32_batch(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed,
                       uint32_t* out, uint32_t n);
int lz4hip_xxh64_batch(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed,
                       uint64_t* out, uint32_t n);

/* ---- device-pointer batch API ----------------------------------------------------------------
 * Same contracts, every pointer is a DEVICE pointer on `device` (an index into the initialised
 * device list), work is enqueued on `stream` (a hipStream_t, NULL = the null stream) and the call
 * returns without synchronising: no PCIe traffic, this is what bench.py times.
 * Offsets, strides and byte counts (src_off, dst_off, chain_*_off, off, stride * index, n_bytes, src_span) are full 64-bit values:
 * the buffers may be tens of GiB, and a block may lie at, across or past 2^31 and 2^32 bytes from its buffer's start, at any
 * alignment.  This is tested on the GPU: tests/far_common.py lists every *_dev function declared in this header with the test
 * that runs it at such offsets -- tests/test_gpu_far_offsets.py for the block, dictionary, xxhash, generator and container entry
 * points (the containers with an input, compressed slots, a container and output slots that all pass 2^32), tests/test_gpu_cchain.py
 * for the two chain entry points -- and tests/test_far_table.py fails when a *_dev function is declared here without an entry.
 * Not covered there: lz4hip_xxh_stream_update_dev (a pointer and a 32-bit length, no offset) and the developer profile entry.
 * The stream contract -- enqueued on `stream`, no wait for it but where an entry's comment says so, any number of streams at once -- is
 * tested the same way: tests/userstream_common.py lists every *_dev function with what this header says about its synchronisation,
 * tests/test_userstream_table.py keeps that list complete, tests/test_gpu_user_streams.py runs every entry on streams of the caller's. */
int lz4hip_compress_fast_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                   uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                   int32_t* out_len, uint32_t n_blocks, int device, void* stream);
/* accelerated fast compress (see lz4hip_compress_fast_accel_batch), device pointers, asynchronous */
int lz4hip_compress_fast_accel_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                         uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                         int32_t* out_len, uint32_t n_blocks, int acceleration, int device, void* stream);
/* compress to a target size (see lz4hip_compress_dest_size_batch), device pointers, asynchronous */
int lz4hip_compress_dest_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                        uint8_t* dst, const uint64_t* dst_off, const int32_t* target_size,
                                        int32_t* out_len, int32_t* src_consumed, uint32_t n_blocks, int device, void* stream);
/* decode a prefix (see lz4hip_decompress_safe_partial_batch), device pointers, asynchronous */
int lz4hip_decompress_safe_partial_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                             uint8_t* dst, const uint64_t* dst_off, const int32_t* target_len,
                                             const int32_t* dst_cap, int32_t* out_len, uint32_t n_blocks, int device, void* stream);
/* decode against a dictionary (see lz4hip_decompress_safe_dict_batch): device pointers, dict_dev[0 .. dict_len) the caller's device
 * memory on `device` (the whole dictionary or, equally, its last 64 KB with dict_len >= 65536); asynchronous, no synchronisation:
 * the dictionary must stay valid until the work on `stream` is done.  dict_len < 0, or dict_dev == NULL with dict_len > 0, is
 * LZ4HIP_E_ARG */
int lz4hip_decompress_safe_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                          uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                          int32_t* out_len, uint32_t n_blocks, const uint8_t* dict_dev, int dict_len,
                                          int device, void* stream);
/* decode chains of linked blocks (see lz4hip_decompress_safe_chain_batch): device pointers -- every array, per block and per chain --,
 * asynchronous.  The arrays cannot be looked at without waiting for the device, so only the NULL checks are LZ4HIP_E_ARG here; the
 * kernel trusts nothing it reads from them: a chain's block range is cut to [0, n_blocks], a negative chain_prefix_len counts as 0 and
 * one longer than chain_dst_off[c] is cut to it */
int lz4hip_decompress_safe_chain_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                           const uint8_t* stored, const int32_t* dst_cap, const uint32_t* chain_first,
                                           uint8_t* dst, const uint64_t* chain_dst_off, const uint64_t* chain_dst_cap,
                                           const int32_t* chain_prefix_len, int32_t* out_len, uint64_t* chain_out_len,
                                           uint32_t n_blocks, uint32_t n_chains, int device, void* stream);
/* compress chains of linked blocks (see lz4hip_compress_fast_chain_batch): device pointers -- every array, per block and per chain --,
 * asynchronous on `stream`, never synchronises.  Only the pointers can be checked here; the kernel trusts nothing it reads from the
 * arrays: a chain's block range is cut to [0, n_blocks], a negative chain_prefix_len counts as 0 and one longer than chain_src_off[c]
 * is cut to it */
int lz4hip_compress_fast_chain_batch_dev(const uint8_t* src, const uint64_t* chain_src_off, const int32_t* chain_prefix_len,
                                         const int32_t* src_len, const uint32_t* chain_first,
                                         uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                         int32_t* out_len, uint64_t* chain_consumed, uint32_t n_blocks, uint32_t n_chains,
                                         int device, void* stream);
/* compress against a dictionary (see lz4hip_compress_fast_dict_batch): device pointers on `device`, and the HANDLE -- the compressor
 * needs its table image, not only the bytes; asynchronous, except that a handle's first compress on a device builds the image and
 * waits for `stream` once.  dict == NULL is LZ4HIP_E_ARG */
int lz4hip_compress_fast_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                        uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                        int32_t* out_len, uint32_t n_blocks, const lz4hip_dict* dict, int device, void* stream);
/* HC compress against a dictionary (see lz4hip_compress_hc_dict_batch): device pointers on `device`, and the HANDLE.  The plain form
 * sizes the chain workspace itself and synchronises `stream` once, as lz4hip_compress_hc_batch_dev does; the _ws form takes the span
 * (max of src_off + src_len) and a workspace of lz4hip_hc_workspace_bytes(src_span, n_blocks, level) bytes from the caller and is
 * fully asynchronous -- except that the handle's first HC compress on a device builds its image there and waits for `stream` once.  A
 * block whose source reaches past src_span gives 0 and leaves the workspace alone.  dict == NULL (or ws == NULL) is LZ4HIP_E_ARG */
int lz4hip_compress_hc_dict_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                      uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                      int32_t* out_len, uint32_t n_blocks, int level, const lz4hip_dict* dict, int device, void* stream);
int lz4hip_compress_hc_dict_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                         uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                         int32_t* out_len, uint32_t n_blocks, int level, const lz4hip_dict* dict, int device, void* stream,
                                         uint64_t src_span, void* ws, size_t ws_bytes);
/* HC: levels follow liblz4 (< 1 -> 9, > 12 -> 12): 1..9 = hash-chain strategy with lazy evaluation, 10..12 = optimal
 * parser (lz4-java levels 10..17).  Levels 10..12 are FUNCTIONAL ONLY: byte-identical output, but the optimal parser's table
 * walk is wave-uniform scalar work (about 1.0 / 0.7 GB/s per GPU at levels 10 / 12 -- no faster than the reference on the host's
 * cores); levels 1..9 are the ones to use for throughput (level 9: ~12 GB/s per GPU on 1 MiB blocks).  The call sizes an internal
 * u16 workspace (2 bytes per source byte, stream-ordered allocation) and therefore synchronises `stream`
 * once before it enqueues the two kernels.                                                          */
int lz4hip_compress_hc_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                 uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                 int32_t* out_len, uint32_t n_blocks, int level, int device, void* stream);
/* lz4hip_compress_hc_batch_dev sizes its chain workspace from the batch's source span, which it has to read back from the device:
 * it synchronises `stream` ONCE per call (every other *_dev entry never synchronises).  The _ws form is fully asynchronous: the
 * caller states src_span = max over blocks of src_off + src_len (any upper bound, e.g. the size of the source buffer) and passes a
 * device workspace of at least lz4hip_hc_workspace_bytes(src_span, n_blocks, level) bytes that stays valid until the work is done.
 * A block whose range reaches past src_span is not compressed: its out_len is 0 and nothing is written past the workspace.        */
size_t lz4hip_hc_workspace_bytes(uint64_t src_span, uint32_t n_blocks, int level);
int lz4hip_compress_hc_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                    uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                    int32_t* out_len, uint32_t n_blocks, int level, int device, void* stream,
                                    uint64_t src_span, void* ws, size_t ws_bytes);
/* HC compress to a target size (see lz4hip_compress_hc_dest_size_batch), device pointers.  As lz4hip_compress_hc_batch_dev, the
 * plain form sizes the chain workspace itself and synchronises `stream` ONCE; the _ws form is fully asynchronous and takes a
 * workspace of at least lz4hip_hc_workspace_bytes(src_span, n_blocks, level) bytes (the same size as for lz4hip_compress_hc*).     */
int lz4hip_compress_hc_dest_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                           uint8_t* dst, const uint64_t* dst_off, const int32_t* target_size,
                                           int32_t* out_len, int32_t* src_consumed, uint32_t n_blocks, int level, int device, void* stream);
int lz4hip_compress_hc_dest_size_batch_dev_ws(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                              uint8_t* dst, const uint64_t* dst_off, const int32_t* target_size,
                                              int32_t* out_len, int32_t* src_consumed, uint32_t n_blocks, int level, int device, void* stream,
                                              uint64_t src_span, void* ws, size_t ws_bytes);
int lz4hip_decompress_safe_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                     uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                     int32_t* out_len, uint32_t n_blocks, int device, void* stream);
/* decoded sizes without an output buffer (see lz4hip_decompressed_size_batch), device pointers, asynchronous */
int lz4hip_decompressed_size_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                       const int32_t* dst_cap, int32_t* out_len, uint32_t n_blocks, int device, void* stream);
int lz4hip_decompress_fast_batch_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_cap,
                                     uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_len,
                                     int32_t* out_consumed, uint32_t n_blocks, int device, void* stream);
int lz4hip_xxh32_batch_dev(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint32_t seed,
                           uint32_t* out, uint32_t n, int device, void* stream);
int lz4hip_xxh64_batch_dev(const uint8_t* buf, const uint64_t* off, const int32_t* len, uint64_t seed,
                           uint64_t* out, uint32_t n, int device, void* stream);

/* ---- single-block convenience (== batch of 1; what the Java single-call path and the
 * LZ4Factory constructor self-test, LZ4Factory.java:204-220, go through).  The return value is the
 * liblz4 return value of the corresponding function.  A LIBRARY failure (no device, HIP error) is
 * reported as INT32_MIN + (-status), which no codec result can equal: test LZ4HIP_IS_LIB_ERROR().  */
#define LZ4HIP_LIB_ERROR(status) ((int)(INT32_MIN + (-(status))))
#define LZ4HIP_IS_LIB_ERROR(ret) ((ret) < (int)(INT32_MIN + 64))
/* out_len[i] of lz4hip_decompress_safe_chain_batch* and lz4hip_compress_fast_chain_batch*: block i lies behind its chain's first failed
 * block and was not decoded / compressed */
#define LZ4HIP_CHAIN_STOPPED LZ4HIP_LIB_ERROR(LZ4HIP_E_CHAIN_STOPPED)
int lz4hip_compress_fast(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap);
int lz4hip_compress_fast_accel(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int acceleration);  /* LZ4_compress_fast */
/* LZ4_compress_destSize: *src_size in = block size, out = input consumed; returns the bytes written.  A library failure returns
 * LZ4HIP_LIB_ERROR(status) and leaves *src_size untouched; src_size == NULL is LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
int lz4hip_compress_dest_size(const uint8_t* src, int* src_size, uint8_t* dst, int target_size);
int lz4hip_compress_hc(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int level);
/* LZ4_compress_HC_destSize: *src_size in = block size, out = input consumed; returns the bytes written.  A library failure returns
 * LZ4HIP_LIB_ERROR(status) and leaves *src_size untouched; src_size == NULL is LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
int lz4hip_compress_hc_dest_size(const uint8_t* src, int* src_size, uint8_t* dst, int target_size, int level);
int lz4hip_decompress_safe(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap);
int lz4hip_decompress_fast(const uint8_t* src, int src_cap, uint8_t* dst, int dst_len);
int lz4hip_decompress_safe_partial(const uint8_t* src, int src_len, uint8_t* dst, int target_size, int dst_cap);  /* LZ4_decompress_safe_partial */
int lz4hip_decompressed_size(const uint8_t* src, int src_len, int dst_cap);  /* what LZ4_decompress_safe(src, dst, src_len, dst_cap) would return; no dst */
int lz4hip_compress_hc_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, int level, const lz4hip_dict* dict);  /* LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream; dict == NULL: LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
int lz4hip_compress_fast_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, const lz4hip_dict* dict);  /* LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream; dict == NULL: LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
int lz4hip_decompress_safe_dict(const uint8_t* src, int src_len, uint8_t* dst, int dst_cap, const lz4hip_dict* dict);  /* LZ4_decompress_safe_usingDict; dict == NULL: LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
int lz4hip_xxh32(const uint8_t* buf, int len, uint32_t seed, uint32_t* out);
int lz4hip_xxh64(const uint8_t* buf, int len, uint64_t seed, uint64_t* out);

/* ---- streaming xxhash ---------------------------------------------------------------------------
 * What StreamingXXHash32JNI / StreamingXXHash64JNI bind (XXHashJNI.java: XXH32_init / _update / _digest / _free,
 * net_jpountz_xxhash_XXHashJNI.c:89-145; the XXH64 set :199-255).  A stream's state -- accumulators, the bytes of
 * the incomplete stripe, the length so far and the digest of everything so far -- is a small record in DEVICE
 * memory; every update is one kernel launch that continues from it (one wavefront: XXH is a serial chain per
 * stream), so device-resident data (decoded blocks, say) is hashed where it lies.  digest == the one-shot hash
 * of the concatenation of all updates since create / reset.  Calls on one handle are serialised (the
 * reference's methods are `synchronized`).  Handles must be freed before lz4hip_shutdown().                   */
typedef struct lz4hip_xxh_stream lz4hip_xxh_stream;
int lz4hip_xxh32_stream_create(uint32_t seed, lz4hip_xxh_stream** out);  /* XXH32_init, XXHashJNI.c:90-101 */
int lz4hip_xxh64_stream_create(uint64_t seed, lz4hip_xxh_stream** out);  /* XXH64_init, XXHashJNI.c:200-211 */
int lz4hip_xxh_stream_reset(lz4hip_xxh_stream* st, uint64_t seed);       /* StreamingXXHash32JNI.reset()    */
int lz4hip_xxh_stream_update(lz4hip_xxh_stream* st, const uint8_t* buf, int len);   /* host pointer; XXHashJNI.c:108-121 */
/* device pointer (on the engine's first device), enqueued on `stream`, returns without synchronising */
int lz4hip_xxh_stream_update_dev(lz4hip_xxh_stream* st, const uint8_t* dbuf, int len, void* stream);
int lz4hip_xxh32_stream_digest(lz4hip_xxh_stream* st, uint32_t* out);    /* XXH32_digest, XXHashJNI.c:128-133 */
int lz4hip_xxh64_stream_digest(lz4hip_xxh_stream* st, uint64_t* out);    /* XXH64_digest, XXHashJNI.c:238-243 */
void lz4hip_xxh_stream_free(lz4hip_xxh_stream* st);                      /* XXH32_free / XXH64_free          */

/* ---- container blocks assembled on the device ---------------------------
 * The data blocks of an LZ4 Frame (kind 0: what LZ4FrameOutputStream.writeBlock emits per block,
 * /root/reference/src/java/net/jpountz/lz4/LZ4FrameOutputStream.java:199-235 -- 4-byte size word with the "stored uncompressed"
 * bit, payload, and with flags & 1 the XXH32 (seed 0) of the stored payload) or of lz4-java's LZ4Block container (kind 1:
 * LZ4BlockOutputStream.flushBufferedData, LZ4BlockOutputStream.java:203-227 -- 21-byte header {"LZ4Block", method | level,
 * compressed length, original length, XXH32(original, seed 0x9747b28c) & 0x0FFFFFFF}, payload) for src[0, n_bytes) cut into
 * block_size pieces.  Compression, raw-fallback decision, size scan, headers, payload compaction and checksums all run on the
 * device behind one another; frame header, end mark and content checksum stay with the caller (a few bytes, independent of the
 * data).  level 0 = LZ4_compress_default, 1..17 = lz4-java HC levels.  Bytes are identical to the reference writers' for the
 * same input, block size and flags (tests/test_gpu_streams.py: the `lz4` CLI reads and reproduces them).
 *   lz4hip_container_blocks      host pointers (H2D of the data, D2H of the finished blocks only); *out_bytes = bytes written
 *   lz4hip_container_blocks_dev  device pointers, asynchronous on `stream`; *total_dev (device) = bytes written -- if it exceeds
 *                                dst_cap nothing beyond dst_cap was written and the result is unusable; ws = device scratch of
 *                                lz4hip_container_workspace_bytes(n_bytes, block_size, level) bytes                              */
size_t lz4hip_container_workspace_bytes(uint64_t n_bytes, uint32_t block_size, int level);
int lz4hip_container_blocks(int kind, int flags, int level, const uint8_t* src, uint64_t n_bytes, uint32_t block_size,
                            uint8_t* dst, uint64_t dst_cap, uint64_t* out_bytes);
int lz4hip_container_blocks_dev(int kind, int flags, int level, const uint8_t* src, uint64_t n_bytes, uint32_t block_size,
                                uint8_t* dst, uint64_t dst_cap, uint64_t* total_dev, void* ws, size_t ws_bytes, int device, void* stream);

/* Device-side container READ path (round 4; replaces the per-block loops of LZ4FrameInputStream.readBlock,
 * src/java/net/jpountz/lz4/LZ4FrameInputStream.java:258-322, and LZ4BlockInputStream.refill, LZ4BlockInputStream.java:191-264, for a
 * whole run of blocks that lies in DEVICE memory): the size words (kind 0: LZ4 Frame body, starting at the first block's size word;
 * flags & 1 = a block checksum follows every payload; max_block = the frame's block maximum size) or the 21-byte headers (kind 1:
 * lz4-java's "LZ4Block" stream) of body[0, body_bytes) are walked on the device, frame block checksums verified where the payloads
 * lie, compressed blocks decoded (LZ4_decompress_safe into max_block bytes / LZ4_decompress_fast into the header's original length,
 * whose return value must be the header's compressed length), raw blocks copied, LZ4Block checksums verified on the decoded bytes --
 * all asynchronous on `stream`.  Block k decodes to dst + k * slot_bytes (slot_bytes >= max_block for frames; n_max slots);
 * sizes_dev[k] = its decoded size; info_dev[0..4] = { blocks delivered, bytes of body consumed by them (+ the end mark / empty
 * block when it was reached), stop reason, decoded bytes of the delivered blocks, liblz4's code when a decode failed }.
 * Stop reasons follow the readers' own order of checks per block; the first block that fails ends the run:
 *   0 end mark (frame) / empty block (LZ4Block) reached     1 body ended at a block boundary     7 all n_max slots used, more follows
 *   2 body ended inside a block ("Stream ended prematurely")   3 frame: "Block size %s exceeded max"  (or a slot too small;
 *     LZ4Block: an original length above slot_bytes or -- when max_block is not 0 -- above max_block: not a stream error)
 *   4 frame: block checksum mismatch     5 frame: the block does not decode (LZ4Exception)     6 LZ4Block: "Stream is corrupted"
 * ws = device scratch of lz4hip_container_decode_workspace_bytes(n_max) bytes.                                               */
size_t lz4hip_container_decode_workspace_bytes(uint32_t n_max);
int lz4hip_container_decode_dev(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint8_t* dst,
                                uint64_t slot_bytes, uint32_t n_max, int32_t* sizes_dev, uint64_t* info_dev, void* ws, size_t ws_bytes,
                                int device, void* stream);
/* the same with host pointers: H2D of the container bytes, the device path, D2H of the delivered blocks BACK TO BACK into dst
 * (max_block: frame block maximum / an upper bound of the LZ4Block original lengths, e.g. 1 << (10 + level nibble)); sizes[n_max],
 * info[5] as above */
int lz4hip_container_decode(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint32_t n_max,
                            uint8_t* dst, uint64_t dst_cap, int32_t* sizes, uint64_t* info);
/* what a caller of lz4hip_container_decode must provide: a host-side walk of the size words / headers (no device work): *n_blocks =
 * whole blocks of the first n_max that body holds, *dst_bytes = the most their decoded forms can need (frame: max_block per
 * compressed block, the stored size of a raw one; LZ4Block: the headers' original lengths) -- so that a 100-byte frame asks for one
 * block's worth of destination, not n_max x max_block (the readers of LZ4FrameInputStream.java:258-322 / LZ4BlockInputStream.java:
 * 191-264 allocate one block at a time).  The walk stops where the device walk stops, and nothing it stops at sizes anything: an
 * LZ4Block header whose original length exceeds max_block (stop reason 3: the readers take their host path), a payload cut short
 * (2), a header that announces more than 255 x compressedLen + 64 bytes -- more than LZ4 can decode from that many (6, "Stream is
 * corrupted", said by the walk itself).  lz4hip_container_decode sizes its own device slots the same way: a few KB of hostile
 * headers cannot make it allocate gigabytes.                                                                                   */
int lz4hip_container_decode_bound(int kind, int flags, const uint8_t* body, uint64_t body_bytes, uint32_t max_block, uint32_t n_max,
                                  uint32_t* n_blocks, uint64_t* dst_bytes);

/* ---- many containers per call (shuffle blocks, record batches) -----------------------
 * lz4hip_container_decode reads ONE container per call: a stream, a set of device allocations and about ten launches for it.  Callers
 * that hold thousands of small containers -- each an LZ4 Frame or an LZ4Block stream of one to a few blocks -- hand them over together:
 * kind is 0 (LZ4 Frame bodies, starting at the first block's size word) or 1 (LZ4Block streams), one kind per call.  Item c is
 * bodies[body_off[c], + body_len[c]) with its own max_block[c] and flags[c]; bit 0 of flags[c] means the frame has block checksums,
 * and items with and without them may be mixed in one call.  n_max is the most blocks any one item delivers (stop reason 7 beyond it).
 * The contract is the existing call, item by item: info[5c .. 5c + 4], the sizes sizes[item_first[c] .. item_first[c + 1]) and the
 * bytes dst[item_dst_off[c] .. item_dst_off[c + 1]) equal what lz4hip_container_decode(kind, flags[c], bodies + body_off[c],
 * body_len[c], max_block[c], n_max, ...) puts into info, sizes[0 .. info[0]) and dst[0 .. info[3]) -- the stop reason, the bytes
 * consumed, liblz4's code of a failed decode and the readers' order of checks inside a block included.  Delivered blocks lie back to
 * back, item after item; item_dst_off[n_items] is the total written, and nothing at or behind it is written.  An item that stops for
 * any reason changes nothing about any other item.
 *   lz4hip_container_decode_many_bound  needs no device: per item what lz4hip_container_decode_bound returns for it.  A caller sizes
 *                                       dst by the sum of item_dst_bytes and sizes by the sum of item_blocks; hostile headers size
 *                                       nothing, per item.
 *   lz4hip_container_decode_many        host pointers.  item_dst_off and item_first have n_items + 1 entries, info has n_items x 5.
 * LZ4HIP_E_ARG is said before a device is looked for: a bad kind, a NULL required pointer, n_max or a max_block[c] outside
 * 1 .. 2^31 - 1, flag bits other than bit 0, dst_cap or sizes_cap below what the bound call reports, items that hold more than 2^31 - 1 - n_items
 * blocks together (the call's block arrays are indexed with 32 bits: split it).  n_items == 0 is LZ4HIP_OK with
 * item_dst_off[0] = item_first[0] = 0.  Device memory is sized by what the bodies hold and never by n_max x max_block; the items go
 * through the host staging in groups of LZ4HIP_HOST_CHUNK_MB MiB of bodies, and a group costs one stream, one set of allocations
 * and one launch sequence, whatever the number of items.  The call runs on the engine's first device.
 * Every item is walked by one lane: right for many small items.  An item of thousands of blocks walks slowly there -- hand such a
 * container to lz4hip_container_decode, whose parallel walk exists for it.
 * Out of scope: writing many containers per call; device-pointer forms; mixing kinds in one call; sharding items over several
 * devices; linked-block frames inside the many-call; a parallel walk inside one item.                                          */
int lz4hip_container_decode_many_bound(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len,
                                       const uint32_t* max_block, const uint8_t* flags, uint32_t n_items, uint32_t n_max,
                                       uint32_t* item_blocks, uint64_t* item_dst_bytes);
int lz4hip_container_decode_many(int kind, const uint8_t* bodies, const uint64_t* body_off, const uint64_t* body_len,
                                 const uint32_t* max_block, const uint8_t* flags, uint32_t n_items, uint32_t n_max,
                                 uint8_t* dst, uint64_t dst_cap, uint64_t* item_dst_off, uint32_t* item_first, int32_t* sizes,
                                 uint32_t sizes_cap, uint64_t* info);

/* ---- many containers WRITTEN per call (the write side) ---------------------------------
 * lz4hip_container_blocks writes the blocks of ONE container per call: a stream, four device allocations, an upload, six to eight
 * launches, two synchronisations and a copy back.  Callers that write thousands of small containers hand their payloads over together:
 * kind is 0 (LZ4 Frame blocks) or 1 (LZ4Block blocks); a call has one kind and one level (0: LZ4_compress_default, 1..17: lz4-java's
 * HC levels), as the single call.  Item c is src[src_off[c], + src_len[c]), cut into pieces of block_size[c] bytes; items may lie
 * anywhere in src, in any order, and may overlap.  flags[c]: bit 0 a block checksum follows every payload (kind 0 only; items with and
 * without it mix in one call); bit 1 the caller wants content_hash[c], the XXH32 (seed 0) of the item's source -- a frame's content
 * checksum, taken on the device while the source lies there; content_hash[c] is 0 where bit 1 is clear, and content_hash may be NULL
 * when no item sets it.  gap_head[c] and gap_tail[c] reserve that many bytes in front of and behind item c's blocks (either array may
 * be NULL: 0 for every item); they come back as zeros, so that a writer places the frame header, the end mark (its four zero bytes are
 * already there) and the content checksum in place without copying the blocks again.  The frame header, the end mark and the checksum
 * word stay with the caller, as in the single call.
 * The contract is the existing call, item by item: dst[item_dst_off[c] + gap_head[c], item_dst_off[c + 1] - gap_tail[c]) holds exactly
 * the bytes lz4hip_container_blocks(kind, flags[c] & 1, level, src + src_off[c], src_len[c], block_size[c], ...) writes, and the length
 * of that range is its *out_bytes; the LZ4Block token's level nibble follows from block_size[c].  An item of 0 bytes has no blocks and
 * contributes only its gaps.  Items lie back to back in item order; item_dst_off has n_items + 1 entries, and nothing at or behind
 * dst + item_dst_off[n_items] is written.
 *   lz4hip_container_blocks_many_bound  needs no device: item_blocks[c] = ceil(src_len[c] / block_size[c]); item_dst_bytes[c] =
 *                                       gap_head[c] + src_len[c] + item_blocks[c] x (kind 0: 4 + 4 x (flags[c] & 1); kind 1: 21) +
 *                                       gap_tail[c], the single call's own worst case.
 *   lz4hip_container_blocks_many        host pointers; dst_cap must be at least the sum of item_dst_bytes, so the call never fails
 *                                       on capacity after the launch.
 * LZ4HIP_E_ARG is said before a device is looked for: a bad kind, a NULL required pointer, a block_size[c] outside 64 .. 32 MiB, a
 * src_len[c] above 2^31 - 1, flag bits other than 0 and 1, bit 0 with kind 1, bit 1 with content_hash == NULL, dst_cap below the bound,
 * more than 2^31 - 1 items, or more than 2^31 - 1 - n_items blocks in all (split the call).  An unsupported level is LZ4HIP_E_UNSUPPORTED.  n_items == 0 is LZ4HIP_OK
 * with item_dst_off[0] = 0.  The items go through the host staging in groups of LZ4HIP_HOST_CHUNK_MB MiB of sources (one item at
 * least); a group costs one upload, one launch sequence, one copy of the results and one of the finished bytes, whatever the number of
 * items, and compress slots and HC workspace are sized by what the group holds: a block's slot is LZ4_compressBound of the item's
 * largest block, min(block_size[c], src_len[c]), so thousands of payloads far smaller than their block size take device memory by
 * their bytes and not by their block size.  The call runs on the engine's first device.
 * The sizes are scanned by one workgroup, a run of neighbouring items per thread: right for many small items.  An item of millions of
 * blocks belongs to lz4hip_container_blocks.
 * Out of scope: device-pointer forms; mixing kinds in one call; sharding items over several devices; linked-block frames.       */
int lz4hip_container_blocks_many_bound(int kind, const uint64_t* src_len, const uint32_t* block_size, const uint8_t* flags,
                                       const uint32_t* gap_head, const uint32_t* gap_tail, uint32_t n_items, uint32_t* item_blocks,
                                       uint64_t* item_dst_bytes);
int lz4hip_container_blocks_many(int kind, int level, const uint8_t* src, const uint64_t* src_off, const uint64_t* src_len,
                                 const uint32_t* block_size, const uint8_t* flags, const uint32_t* gap_head, const uint32_t* gap_tail,
                                 uint32_t n_items, uint8_t* dst, uint64_t dst_cap, uint64_t* item_dst_off, uint32_t* content_hash);

/* ---- workload helper (not part of the reference API) ------------------------------------------
 * Fills n_blocks slots of `block_len` bytes at dst + i*stride with the SURVEY.md App. F synthetic
 * blocks idx = first_idx + i (deterministic, seed-addressed).  Device pointer, async on stream.
 * bench.py uses it so BASELINE.json's 4 GiB batch never crosses PCIe.                           */
int lz4hip_gen_blocks_dev(uint8_t* dst, uint64_t stride, int32_t block_len, uint64_t seed, uint64_t first_idx,
                          uint32_t litmax, uint32_t win, uint32_t n_blocks, int device, void* stream);

#ifdef LZ4HIP_DEV_TOOLS
/* ---- developer diagnostics (not part of the reference API) --------------------------------------
 * lz4hip_compress_fast_batch_dev with per-phase shader-clock accounting: prof[b*12 .. b*12+11] =
 * {steps, collision steps, fingerprint false positives, sequences, cycles of phases 0..7} of block b
 * (phases are documented in csrc/lz4_fast_core.h).  Output bytes are identical to the product kernel.
 * Only in developer builds of the library (tools/build_variant.sh dev -DLZ4HIP_DEV_TOOLS); the release library does not export it. */
int lz4hip_dbg_compress_fast_profile_dev(const uint8_t* src, const uint64_t* src_off, const int32_t* src_len,
                                         uint8_t* dst, const uint64_t* dst_off, const int32_t* dst_cap,
                                         int32_t* out_len, uint32_t n_blocks, uint64_t* prof, int device, void* stream);
#endif

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* LZ4HIP_H */
