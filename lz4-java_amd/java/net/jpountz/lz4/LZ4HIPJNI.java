package net.jpountz.lz4;

/*
 * Adapted from lz4-java (src/java/net/jpountz/lz4/LZ4JNI.java), Copyright 2020 Adrien Grand and the lz4-java contributors,
 * for the "HIP" implementation family: the argument checks, their order and the exceptions are the original's; the native
 * call goes to liblz4hip instead of liblz4.
 *
 * Licensed under the Apache License, Version 2.0 (the "License");
 * you may not use this file except in compliance with the License.
 * You may obtain a copy of the License at
 *
 *     http://www.apache.org/licenses/LICENSE-2.0
 *
 * Unless required by applicable law or agreed to in writing, software
 * distributed under the License is distributed on an "AS IS" BASIS,
 * WITHOUT WARRANTIES OR CONDITIONS OF ANY KIND, either express or implied.
 * See the License for the specific language governing permissions and
 * limitations under the License.
 */

import java.nio.ByteBuffer;

/**
 * JNI bindings to liblz4hip (include/lz4hip.h), the MI355X LZ4 block engine.
 *
 * Same shape as the reference's {@code LZ4JNI} enum (src/java/net/jpountz/lz4/LZ4JNI.java:27-43):
 * a constant-less enum whose static initialiser loads the native library, and static native
 * methods taking {@code (array | direct buffer, offset, length)} pairs.  The single-block methods
 * back the {@link LZ4Compressor}/{@link LZ4FastDecompressor}/{@link LZ4SafeDecompressor}
 * signatures; the {@code *Batch} methods are the new entry point (many independent blocks per
 * HIP launch) used by {@link LZ4HIPBatch}.
 *
 * NOT COMPILED in the build image (no JDK there); see INTEGRATION.md.
 */
enum LZ4HIPJNI {
  ;

  static {
    // mirrors net.jpountz.util.Native.load() (Native.java:98-162): java.library.path first, then the
    // copy bundled under /net/jpountz/util/linux/amd64/liblz4hip-java.so
    NativeHIP.load();
    init();
  }

  static native void init();

  /* single block: return conventions of liblz4 (0 / negative = failure), or <= Integer.MIN_VALUE + 63 for a
   * library failure (no GPU, HIP error), which the callers turn into an LZ4Exception as well */
  static native int LZ4HIP_compress_fast(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                         byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen);
  /* LZ4_compress_fast(..., acceleration): the arguments, NULL / pinning rules and return conventions of LZ4HIP_compress_fast */
  static native int LZ4HIP_compress_fast_accel(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                               byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen, int acceleration);
  /* LZ4_compress_destSize: srcSize[0] = block size in, input consumed out (untouched on a library failure); returns the bytes
   * written (at most targetDestSize) or a library failure as above.  Same NULL / pinning rules as LZ4HIP_compress_fast */
  static native int LZ4HIP_compress_dest_size(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int[] srcSize,
                                              byte[] destArray, ByteBuffer destBuffer, int destOff, int targetDestSize);
  static native int LZ4HIP_compressHC(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                      byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen, int compressionLevel);
  /* LZ4_compress_HC_destSize at compressionLevel: the arguments, NULL / pinning rules and return conventions of
   * LZ4HIP_compress_dest_size */
  static native int LZ4HIP_compressHC_dest_size(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int[] srcSize,
                                                byte[] destArray, ByteBuffer destBuffer, int destOff, int targetDestSize,
                                                int compressionLevel);
  static native int LZ4HIP_decompress_fast(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcCap,
                                           byte[] destArray, ByteBuffer destBuffer, int destOff, int destLen);
  static native int LZ4HIP_decompress_safe(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                           byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen);
  /* LZ4_decompress_safe_partial: the first min(targetLen, maxDestLen) decoded bytes; liblz4's return value or a library failure as
   * above.  Same NULL / pinning rules as LZ4HIP_decompress_safe */
  static native int LZ4HIP_decompress_safe_partial(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                                   byte[] destArray, ByteBuffer destBuffer, int destOff, int targetLen, int maxDestLen);
  /* the decoded-size query: what LZ4HIP_decompress_safe would return for the same source and maxDestLen, without a destination
   * (lz4hip_decompressed_size); liblz4's return value or a library failure as above.  Exactly one of srcArray / srcBuffer is non-null */
  static native int LZ4HIP_decompressed_length(byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen, int maxDestLen);
  static native int LZ4HIP_compressBound(int len);

  /* batches over DIRECT buffers (so the shim never pins the Java heap across a kernel):
   * op 0 = fast compress, 1 = safe decompress, 2 = fast decompress, 3 = HC compress(level),
   * 4 = accelerated fast compress (level = acceleration).
   * Returns 0 or a negative lz4hip_status; per-block results land in outLen. */
  static native int LZ4HIP_batch(int op, int level, ByteBuffer src, long[] srcOff, int[] srcLen,
                                 ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, int nBlocks);
  /* LZ4_compress_destSize per block over DIRECT buffers: block i fills at most dest[destOff[i], + targetSize[i]); outLen = bytes
   * written, srcConsumed = input consumed.  Returns 0 or a negative lz4hip_status (a null argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchDestSize(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetSize,
                                         int[] outLen, int[] srcConsumed, int nBlocks);
  /* LZ4_decompress_safe_partial per block over DIRECT buffers: block i decodes into at most dest[destOff[i], + min(targetLen[i],
   * destCap[i])); outLen = liblz4's return values.  Returns 0 or a negative lz4hip_status (a null argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchSafePartial(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetLen,
                                            int[] destCap, int[] outLen, int nBlocks);
  /* LZ4_decompress_safe_usingDict against a dictionary that is not contiguous with the destination (LZ4HIPDictionary keeps the handle).
   * dictCreate copies the bytes of the array or direct buffer and returns the handle, or 0 (lastError() says why); dictSize is the true
   * length; dictFree takes 0 too. */
  static native long LZ4HIP_dictCreate(byte[] dictArray, ByteBuffer dictBuffer, int off, int len);
  static native int LZ4HIP_dictSize(long dict);
  static native void LZ4HIP_dictFree(long dict);
  /* the decoded size, a negative liblz4 code or a library failure as LZ4HIP_decompress_safe; same NULL / pinning rules */
  static native int LZ4HIP_decompress_safe_dict(long dict, byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                                byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen);
  /* per block over DIRECT buffers against one dictionary: outLen = liblz4's return values.  Returns 0 or a negative lz4hip_status (a
   * null argument or a 0 handle: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchSafeDict(long dict, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff,
                                         int[] destCap, int[] outLen, int nBlocks);
  /* LZ4_decompress_safe_continue over chains of linked blocks, DIRECT buffers: chain c is the blocks chainFirst[c] .. chainFirst[c + 1] - 1,
   * decoded back to back into dest[chainDestOff[c], + chainDestCap[c]) behind chainPrefixLen[c] bytes of history; stored (null, or != 0 per
   * raw block) and chainPrefixLen may be null.  outLen = liblz4's return values (LZ4HIPBatch.CHAIN_STOPPED behind a chain's first negative
   * one), chainOutLen = the bytes each chain decoded.  Returns 0 or a negative lz4hip_status (a null required argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchSafeChain(ByteBuffer src, long[] srcOff, int[] srcLen, int[] stored, int[] destCap, int[] chainFirst,
                                          ByteBuffer dest, long[] chainDestOff, long[] chainDestCap, int[] chainPrefixLen, int[] outLen,
                                          long[] chainOutLen, int nBlocks, int nChains);
  /* LZ4_decompress_safe_continue on streams whose blocks land anywhere, DIRECT buffers: stream c is the blocks chainFirst[c] ..
   * chainFirst[c + 1] - 1 of this call, block i is decoded to dest[destOff[i], + destCap[i]) inside the window dest[chainWinOff[c], +
   * chainWinLen[c]); state holds four longs per stream (prefixEnd, prefixLen, extEnd, extLen: offsets into dest), read and written back.
   * outLen = liblz4's return values (LZ4HIPBatch.CHAIN_STOPPED behind a stream's first negative one of the call).  Returns 0 or a negative
   * lz4hip_status (a null argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchSafeStream(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
                                           long[] destOff, int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen,
                                           int nBlocks, int nChains);
  /* The same call for streams whose slots overlap the history they can reach (liblz4's minimal ring, rings in step with the writer's):
   * LZ4HIP_batchSafeStream's arguments, state and errors; the two may alternate on one stream from call to call. */
  static native int LZ4HIP_batchSafeStreamInOrder(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
                                                  long[] destOff, int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen,
                                                  int nBlocks, int nChains);
  /* LZ4_decoderRingBufferSize(maxBlock): 65536 + 14 + max(maxBlock, 16); 0 for a negative maxBlock or one above 0x7E000000. */
  static native int LZ4HIP_decoderRingBufferSize(int maxBlock);
  /* LZ4_compress_HC_continue on streams whose sources land anywhere, DIRECT buffers: stream c is the blocks chainFirst[c] ..
   * chainFirst[c + 1] - 1 of this call, block i is src[srcOff[i], + srcLen[i]) and owns dest[destOff[i], + destCap[i]); state holds five
   * longs per stream (prefixEnd, prefixLen, extEnd, extLen, index: offsets into src), read and written back.  outLen = liblz4's return
   * values (0: it did not fit, which does not end the stream).  Returns 0 or a negative lz4hip_status (a null argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchHCStream(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
                                         long[] destOff, int[] destCap, int[] outLen, int nBlocks, int nChains, int level);
  /* LZ4_compress_fast_continue over chains of linked blocks, DIRECT buffers: chain c is the blocks chainFirst[c] .. chainFirst[c + 1] - 1,
   * whose sources lie back to back from src[chainSrcOff[c]] on behind chainPrefixLen[c] bytes of history (null: none); block i owns
   * dest[destOff[i], + destCap[i]).  outLen = liblz4's return values (0 ends a chain, LZ4HIPBatch.CHAIN_STOPPED behind it),
   * chainConsumed = the source bytes of each chain's blocks that succeeded.  Returns 0 or a negative lz4hip_status (a null required
   * argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchFastChain(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
                                          ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed,
                                          int nBlocks, int nChains);
  /* Resident compress streams (lz4hip_cstreams_*): cstreamsCreate returns the handle of a set of nStreams streams, or 0 (lastError() says
   * why); cstreamsCount the number of streams; cstreamsFree takes 0 too; cstreamsReset makes the n listed streams fresh (null: all);
   * cstreamsConsumed fills consumed[i] / stopped[i] (!= 0: stopped) for the streams first .. first + n - 1.  Reset and consumed return 0
   * or a negative lz4hip_status (a 0 handle or a null required array: LZ4HIP_E_ARG). */
  static native long LZ4HIP_cstreamsCreate(int nStreams);
  static native int LZ4HIP_cstreamsCount(long set);
  static native void LZ4HIP_cstreamsFree(long set);
  static native int LZ4HIP_cstreamsReset(long set, int[] streamId, int n);
  static native int LZ4HIP_cstreamsConsumed(long set, int first, int n, long[] consumed, int[] stopped);
  /* LZ4_compress_fast_continue on resident streams, DIRECT buffers: the arguments of LZ4HIP_batchFastChain behind the set and streamId,
   * the stream of every chain (strictly ascending).  Every stream gives, over all the calls that name it, what ONE LZ4_stream_t gives; a
   * 0 stops the stream until it is reset.  Returns 0 or a negative lz4hip_status (a 0 handle or a null required argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchFastStream(long set, int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen,
                                           int[] chainFirst, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed,
                                           int nBlocks, int nChains);
  /* The same streams when their sources land anywhere, DIRECT buffers (lz4hip_compress_fast_stream_ext_batch): every block has its own
   * srcOff[i] inside the window src[chainWinOff[c], + chainWinLen[c]) of its stream, whose history ends at chainHistEnd[c] with
   * chainHistLen[c] bytes of it present.  Every array is required.  Returns 0 or a negative lz4hip_status. */
  static native int LZ4HIP_batchFastStreamAt(long set, int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst,
                                             long[] chainHistEnd, int[] chainHistLen, long[] chainWinOff, long[] chainWinLen, ByteBuffer dest,
                                             long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int nBlocks, int nChains);
  /* The three calls above with LZ4_compress_fast_continue's acceleration as a trailing argument, one value for every block of the call
   * (lz4hip_compress_fast_chain_accel_batch, lz4hip_compress_fast_stream_accel_batch, lz4hip_compress_fast_stream_ext_accel_batch):
   * clamped to 1 .. 65537 as liblz4 does, and 1 is the call above.  A stream may be given another acceleration in every call. */
  static native int LZ4HIP_batchFastChainAccel(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
                                               ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed,
                                               int nBlocks, int nChains, int acceleration);
  static native int LZ4HIP_batchFastStreamAccel(long set, int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen,
                                                int[] chainFirst, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed,
                                                int nBlocks, int nChains, int acceleration);
  static native int LZ4HIP_batchFastStreamAtAccel(long set, int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst,
                                                  long[] chainHistEnd, int[] chainHistLen, long[] chainWinOff, long[] chainWinLen, ByteBuffer dest,
                                                  long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int nBlocks, int nChains,
                                                  int acceleration);
  /* LZ4_compress_HC_continue over chains of linked blocks (prefix mode) at HC level `level`, DIRECT buffers: the arrays of
   * LZ4HIP_batchFastChain without chainConsumed.  outLen = liblz4's return values; a 0 does not end a chain.  Returns 0 or a negative
   * lz4hip_status (a null required argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchHCChain(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
                                        ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, int nBlocks, int nChains, int level);
  /* LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream against a dictionary handle: the compressed size, 0 (maxDestLen too
   * small) or a library failure as LZ4HIP_compress_fast; same NULL / pinning rules */
  static native int LZ4HIP_compress_fast_dict(long dict, byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                              byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen);
  /* per block over DIRECT buffers against one dictionary: outLen = the compressed sizes, 0 where destCap[i] is too small.  Returns 0 or
   * a negative lz4hip_status (a null argument or a 0 handle: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchCompressDict(long dict, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff,
                                             int[] destCap, int[] outLen, int nBlocks);
  /* LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream at HC level `level` against a dictionary handle: the conventions of
   * LZ4HIP_compress_fast_dict and LZ4HIP_batchCompressDict */
  static native int LZ4HIP_compress_hc_dict(long dict, int level, byte[] srcArray, ByteBuffer srcBuffer, int srcOff, int srcLen,
                                            byte[] destArray, ByteBuffer destBuffer, int destOff, int maxDestLen);
  static native int LZ4HIP_batchCompressHCDict(long dict, int level, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff,
                                               int[] destCap, int[] outLen, int nBlocks);
  /* LZ4_compress_HC_destSize per block at HC level `level`: the arguments and return conventions of LZ4HIP_batchDestSize */
  static native int LZ4HIP_batchHCDestSize(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetSize,
                                           int[] outLen, int[] srcConsumed, int nBlocks, int level);

  /* the decoded-size query per block over a DIRECT source buffer, no destination: outLen[i] = what LZ4_decompress_safe would return for
   * block i with capacity destCap[i].  Returns 0 or a negative lz4hip_status (a null argument: LZ4HIP_E_ARG). */
  static native int LZ4HIP_batchDecompressedLengths(ByteBuffer src, long[] srcOff, int[] srcLen, int[] destCap, int[] outLen, int nBlocks);

  /** Container blocks assembled on the device (LZ4HIPBatch.containerBlocks); returns bytes written or the negative lz4hip_status. */
  static native long LZ4HIP_containerBlocks(int kind, int flags, int level, ByteBuffer src, long srcOff, long len, int blockSize,
      ByteBuffer dest, long destOff, long destCap);

  /** The read side on the device (LZ4HIPBatch.containerDecode); returns 0 or the negative lz4hip_status. */
  static native int LZ4HIP_containerDecode(int kind, int flags, ByteBuffer src, long srcOff, long len, int maxBlock, int nMax,
      ByteBuffer dest, long destOff, long destCap, int[] sizes, long[] info);

  /** Destination bytes a containerDecode call can need (host-side walk of the headers); blocks[0] = whole blocks present. */
  static native long LZ4HIP_containerDecodeBound(int kind, int flags, ByteBuffer src, long srcOff, long len, int maxBlock, int nMax,
      int[] blocks);

  /** Many containers of one kind in one call (LZ4HIPBatch.containerDecodeMany); returns 0 or the negative lz4hip_status. */
  static native int LZ4HIP_containerDecodeMany(int kind, ByteBuffer bodies, long[] bodyOff, long[] bodyLen, int[] maxBlock, int[] flags,
      int nItems, int nMax, ByteBuffer dest, long destOff, long destCap, long[] itemDstOff, int[] itemFirst, int[] sizes, long[] info);

  /** Per item what LZ4HIP_containerDecodeBound says of it (host-side walk, no device); returns 0 or the negative lz4hip_status. */
  static native int LZ4HIP_containerDecodeManyBound(int kind, ByteBuffer bodies, long[] bodyOff, long[] bodyLen, int[] maxBlock, int[] flags,
      int nItems, int nMax, int[] itemBlocks, long[] itemDstBytes);

  /** Many containers of one kind written in one call (LZ4HIPBatch.containerBlocksMany); returns 0 or the negative lz4hip_status. */
  static native int LZ4HIP_containerBlocksMany(int kind, int level, ByteBuffer src, long[] srcOff, long[] srcLen, int[] blockSize, int[] flags,
      int[] gapHead, int[] gapTail, int nItems, ByteBuffer dest, long destOff, long destCap, long[] itemDstOff, int[] contentHash);

  /** Per item its blocks and its worst case with the gaps (arithmetic, no device); returns 0 or the negative lz4hip_status. */
  static native int LZ4HIP_containerBlocksManyBound(int kind, long[] srcLen, int[] blockSize, int[] flags, int[] gapHead, int[] gapTail,
      int nItems, int[] itemBlocks, long[] itemDstBytes);

  static native String lastError();
}
