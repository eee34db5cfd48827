package net.jpountz.lz4;

/*
 * Adapted from lz4-java (the batch counterpart of src/java/net/jpountz/lz4/LZ4JNI.java), Copyright 2020 Adrien Grand and the lz4-java contributors,
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
 * Many independent blocks per HIP launch -- the entry point the one-block-per-call API of lz4-java
 * lacks (LZ4Compressor.java:59, SURVEY.md fact 9).  All buffers must be DIRECT: block i is
 * {@code src[srcOff[i], srcOff[i]+srcLen[i])} and owns the slot {@code dest[destOff[i], destOff[i]+destCap[i])}.
 * Results follow liblz4's conventions per block (see include/lz4hip.h).
 */
public final class LZ4HIPBatch {
  private LZ4HIPBatch() {}

  private static void check(ByteBuffer src, ByteBuffer dest, long[] srcOff, int[] srcLen, long[] destOff, int[] destCap, int[] outLen) {
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    final int n = srcOff.length;
    if (srcLen.length != n || destOff.length != n || destCap.length != n || outLen.length < n) {
      throw new IllegalArgumentException("per-block arrays must have the same length");
    }
    for (int i = 0; i < n; i++) {
      if (srcLen[i] < 0 || destCap[i] < 0 || srcOff[i] < 0 || destOff[i] < 0
          || srcOff[i] + srcLen[i] > src.capacity() || destOff[i] + destCap[i] > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException(i);
      }
    }
  }

  private static void run(int op, int level, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen) {
    check(src, dest, srcOff, srcLen, destOff, destCap, outLen);
    final int rc = LZ4HIPJNI.LZ4HIP_batch(op, level, src, srcOff, srcLen, dest, destOff, destCap, outLen, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /** outLen[i] &gt; 0: compressed size; 0: destCap[i] too small. */
  public static void compress(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen) {
    run(0, 0, src, srcOff, srcLen, dest, destOff, destCap, outLen);
  }

  /**
   * The bytes of liblz4's {@code LZ4_compress_fast(..., acceleration)} per block (acceleration below 1 acts as 1, above 65537 as
   * 65537; 1 is {@link #compress(ByteBuffer, long[], int[], ByteBuffer, long[], int[], int[])}).  outLen[i] &gt; 0: compressed size;
   * 0: destCap[i] too small.
   */
  public static void compress(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen,
      int acceleration) {
    run(4, acceleration, src, srcOff, srcLen, dest, destOff, destCap, outLen);
  }

  /**
   * liblz4's {@code LZ4_compress_destSize} per block: as much of block i as fits in exactly {@code targetSize[i]} bytes, written to
   * the slot {@code dest[destOff[i], destOff[i]+targetSize[i])}.  outLen[i]: bytes written (0 for an empty target);
   * srcConsumed[i]: the source bytes they cover.
   */
  public static void compressDestSize(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetSize, int[] outLen,
      int[] srcConsumed) {
    check(src, dest, srcOff, srcLen, destOff, targetSize, outLen);
    if (srcConsumed.length < srcOff.length) {
      throw new IllegalArgumentException("per-block arrays must have the same length");
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchDestSize(src, srcOff, srcLen, dest, destOff, targetSize, outLen, srcConsumed, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_loadDict} + {@code LZ4_compress_fast_continue} per block, a fresh stream each, against one shared dictionary
   * (not contiguous with {@code src}): block i is compressed alone against {@code dict} into the slot
   * {@code dest[destOff[i], destOff[i]+destCap[i])}; {@link #decompressSafeDict} reads it.  outLen[i] &gt; 0: the compressed size;
   * 0: the slot is too small.
   */
  public static void compressDict(LZ4HIPDictionary dict, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff,
      int[] destCap, int[] outLen) {
    check(src, dest, srcOff, srcLen, destOff, destCap, outLen);
    final int rc = LZ4HIPJNI.LZ4HIP_batchCompressDict(dict.handle(), src, srcOff, srcLen, dest, destOff, destCap, outLen, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_loadDictHC} + {@code LZ4_compress_HC_continue} per block at HC level {@code level}, a fresh stream each, against
   * one shared dictionary (not contiguous with {@code src}): block i is compressed alone into the slot
   * {@code dest[destOff[i], destOff[i]+destCap[i])}; {@link #decompressSafeDict} reads it.  outLen[i] &gt; 0: the compressed size;
   * 0: liblz4 returns 0 (the slot is too small).
   */
  public static void compressHCDict(LZ4HIPDictionary dict, int level, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest,
      long[] destOff, int[] destCap, int[] outLen) {
    check(src, dest, srcOff, srcLen, destOff, destCap, outLen);
    final int rc = LZ4HIPJNI.LZ4HIP_batchCompressHCDict(dict.handle(), level, src, srcOff, srcLen, dest, destOff, destCap, outLen, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_decompress_safe_usingDict} per block against one shared dictionary (not contiguous with {@code dest}): block i,
   * compressed alone against {@code dict}, decodes into the slot {@code dest[destOff[i], destOff[i]+destCap[i])}.
   * outLen[i] &gt;= 0: the decoded size; &lt; 0: -(input position)-1.
   */
  public static void decompressSafeDict(LZ4HIPDictionary dict, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff,
      int[] destCap, int[] outLen) {
    check(src, dest, srcOff, srcLen, destOff, destCap, outLen);
    final int rc = LZ4HIPJNI.LZ4HIP_batchSafeDict(dict.handle(), src, srcOff, srcLen, dest, destOff, destCap, outLen, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_compress_fast_continue} over chains of linked blocks (its prefix mode, acceleration 1): chain c is the blocks
   * {@code chainFirst[c] .. chainFirst[c + 1] - 1}, whose sources lie back to back from {@code src[chainSrcOff[c]]} on, behind
   * {@code chainPrefixLen[c]} bytes of history that lie in front of it in {@code src} ({@code null}: no history; the stream loads it with
   * {@code LZ4_loadDict}).  Block i owns the slot {@code dest[destOff[i], destOff[i]+destCap[i])}.  outLen[i] &gt; 0: the compressed size;
   * 0: it did not fit, which ends the chain -- the blocks behind it get {@link #CHAIN_STOPPED}.  chainConsumed[c]: the source bytes of
   * chain c's blocks that succeeded.
   */
  public static void compressFastChain(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
      ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed) {
    compressFastChain(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, 1);
  }

  /**
   * {@link #compressFastChain} with {@code LZ4_compress_fast_continue}'s acceleration, one value for every block of the call: clamped
   * to 1 .. 65537 as liblz4 does; 1 is the call without it.  These are the blocks {@code lz4 --fast=N} writes.
   */
  public static void compressFastChain(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
      ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int acceleration) {
    if (chainConsumed.length != chainSrcOff.length) {
      throw new IllegalArgumentException("per-chain arrays differ in length");
    }
    checkChains(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen);
    final int n = srcLen.length, nc = chainSrcOff.length;
    final int rc = acceleration == 1
        ? LZ4HIPJNI.LZ4HIP_batchFastChain(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, n, nc)
        : LZ4HIPJNI.LZ4HIP_batchFastChainAccel(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, n, nc,
            acceleration);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_compress_fast_continue} on streams that go on from call to call: the arrays of {@link #compressFastChain}, and
   * chain c is the next run of blocks of stream {@code streamId[c]} of {@code streams} (strictly ascending: a stream once per call).
   * Every stream gives, over all the calls that name it, the bytes ONE {@code LZ4_stream_t} gives, however its blocks are cut into
   * calls.  For a stream that has run, {@code chainPrefixLen[c]} is how many of the last bytes it consumed lie in front of the source
   * ({@code LZ4_saveDict}'s size; 0 is legal and no reset).  A block whose result is 0 stops its stream -- {@link #CHAIN_STOPPED} from
   * then on -- until {@link CompressStreams#reset}.
   */
  public static void compressFastStream(CompressStreams streams, int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen,
      int[] srcLen, int[] chainFirst, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed) {
    compressFastStream(streams, streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, 1);
  }

  /**
   * {@link #compressFastStream} with {@code LZ4_compress_fast_continue}'s acceleration for every block of THIS call (clamped to
   * 1 .. 65537; 1 is the call without it).  A stream may be given another acceleration in every call.
   */
  public static void compressFastStream(CompressStreams streams, int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen,
      int[] srcLen, int[] chainFirst, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int acceleration) {
    if (chainConsumed.length != chainSrcOff.length || streamId.length != chainSrcOff.length) {
      throw new IllegalArgumentException("per-chain arrays differ in length");
    }
    final int ns = streams.size();
    for (int c = 0; c < streamId.length; c++) {
      if (streamId[c] < 0 || streamId[c] >= ns || (c > 0 && streamId[c] <= streamId[c - 1])) {
        throw new IllegalArgumentException("streamId must be strictly ascending and below the number of streams");
      }
    }
    checkChains(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen);
    final int rc = acceleration == 1
        ? LZ4HIPJNI.LZ4HIP_batchFastStream(streams.handle(), streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff,
            destCap, outLen, chainConsumed, srcLen.length, chainSrcOff.length)
        : LZ4HIPJNI.LZ4HIP_batchFastStreamAccel(streams.handle(), streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff,
            destCap, outLen, chainConsumed, srcLen.length, chainSrcOff.length, acceleration);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * A set of compress streams whose state -- the hash table and index position an {@code LZ4_stream_t} carries beside its history -- is
   * resident on the device between calls (about 32 KB of device memory per stream).  Calls on one set are serialised; close it before
   * the library is shut down.
   */
  public static final class CompressStreams implements java.io.Closeable {
    private long handle;

    public CompressStreams(int nStreams) {
      if (nStreams < 1) {
        throw new IllegalArgumentException("a set has at least one stream");
      }
      handle = LZ4HIPJNI.LZ4HIP_cstreamsCreate(nStreams);
      if (handle == 0) {
        throw new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
      }
    }

    long handle() {
      if (handle == 0) {
        throw new IllegalStateException("Already closed");
      }
      return handle;
    }

    public int size() {
      return LZ4HIPJNI.LZ4HIP_cstreamsCount(handle());
    }

    /** {@link LZ4HIPBatch#compressFastStream} on this set */
    public void compress(int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
        ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed) {
      compressFastStream(this, streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed);
    }

    /** {@link LZ4HIPBatch#compressFastStream} on this set, at an acceleration */
    public void compress(int[] streamId, ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
        ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int acceleration) {
      compressFastStream(this, streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, acceleration);
    }

    /**
     * The same streams when their sources land anywhere -- a ring that wraps, alternating buffers, a dictionary elsewhere
     * ({@code lz4hip_compress_fast_stream_ext_batch}): every block has its own {@code srcOff[i]} inside its stream's window
     * {@code src[chainWinOff[c], + chainWinLen[c])}; the stream's history ends at {@code chainHistEnd[c]} with {@code chainHistLen[c]}
     * bytes of it present.  A block that does not follow its history runs in liblz4's external-dictionary mode.  A call is a snapshot
     * of {@code src}.  Every array is required.
     */
    public void compressAt(int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, long[] chainHistEnd, int[] chainHistLen,
        long[] chainWinOff, long[] chainWinLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed) {
      compressAt(streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dest, destOff, destCap, outLen, chainConsumed, 1);
    }

    /** {@link #compressAt} at an acceleration ({@code lz4hip_compress_fast_stream_ext_accel_batch}): as for {@link #compress} */
    public void compressAt(int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, long[] chainHistEnd, int[] chainHistLen,
        long[] chainWinOff, long[] chainWinLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, long[] chainConsumed, int acceleration) {
      final int n = srcLen.length, nc = streamId.length;
      if (srcOff.length != n || destOff.length != n || destCap.length != n || outLen.length != n) {
        throw new IllegalArgumentException("per-block arrays differ in length");
      }
      if (chainHistEnd.length != nc || chainHistLen.length != nc || chainWinOff.length != nc || chainWinLen.length != nc
          || chainConsumed.length != nc || chainFirst.length != nc + 1) {
        throw new IllegalArgumentException("per-chain arrays differ in length");
      }
      if (!src.isDirect() || !dest.isDirect()) {
        throw new IllegalArgumentException("direct buffers only");
      }
      final int ns = size();
      for (int c = 0; c < nc; c++) {
        if (streamId[c] < 0 || streamId[c] >= ns || (c > 0 && streamId[c] <= streamId[c - 1])) {
          throw new IllegalArgumentException("streamId must be strictly ascending and below the number of streams");
        }
      }
      final int rc = acceleration == 1
          ? LZ4HIPJNI.LZ4HIP_batchFastStreamAt(handle(), streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff,
              chainWinLen, dest, destOff, destCap, outLen, chainConsumed, n, nc)
          : LZ4HIPJNI.LZ4HIP_batchFastStreamAtAccel(handle(), streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff,
              chainWinLen, dest, destOff, destCap, outLen, chainConsumed, n, nc, acceleration);
      if (rc != 0) {
        throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
      }
    }

    /** makes the listed streams ({@code null}: all of them) fresh */
    public void reset(int[] streamId) {
      final int rc = LZ4HIPJNI.LZ4HIP_cstreamsReset(handle(), streamId, streamId == null ? 0 : streamId.length);
      if (rc != 0) {
        throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
      }
    }

    /** the bytes consumed since the reset, and whether the stream is stopped, for the streams first .. first + consumed.length - 1 */
    public void consumed(int first, long[] consumed, boolean[] stopped) {
      if (stopped.length != consumed.length) {
        throw new IllegalArgumentException("arrays differ in length");
      }
      final int[] st = new int[consumed.length];
      final int rc = LZ4HIPJNI.LZ4HIP_cstreamsConsumed(handle(), first, consumed.length, consumed, st);
      if (rc != 0) {
        throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
      }
      for (int i = 0; i < st.length; i++) {
        stopped[i] = st[i] != 0;
      }
    }

    @Override
    public synchronized void close() {
      if (handle != 0) {
        LZ4HIPJNI.LZ4HIP_cstreamsFree(handle);
        handle = 0;
      }
    }
  }

  /**
   * liblz4's {@code LZ4_compress_HC_continue} over chains of linked blocks (its prefix mode) at HC level {@code level} (&lt; 1: 9, &gt; 12: 12):
   * the arrays of {@link #compressFastChain} without {@code chainConsumed}.  outLen[i] &gt; 0: the compressed size; 0: it did not fit --
   * which does NOT end the chain: the block's source is history for the blocks behind it, and no block gets {@link #CHAIN_STOPPED}.  Not
   * serial: every block of every chain is parsed at the same time.
   */
  public static void compressHCChain(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
      ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen, int level) {
    checkChains(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen);
    final int rc = LZ4HIPJNI.LZ4HIP_batchHCChain(src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, srcLen.length,
        chainSrcOff.length, level);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /** the argument checks of the two chain compressors */
  private static void checkChains(ByteBuffer src, long[] chainSrcOff, int[] chainPrefixLen, int[] srcLen, int[] chainFirst,
      ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen) {
    final int n = srcLen.length, nc = chainSrcOff.length;
    if (destOff.length != n || destCap.length != n || outLen.length != n) {
      throw new IllegalArgumentException("per-block arrays differ in length");
    }
    if (chainFirst.length != nc + 1 || (chainPrefixLen != null && chainPrefixLen.length != nc)) {
      throw new IllegalArgumentException("per-chain arrays differ in length");
    }
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("direct buffers required");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    if (chainFirst[0] != 0 || chainFirst[nc] != n) {
      throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
    }
    for (int c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) {
        throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
      }
      long total = 0;
      for (int i = chainFirst[c]; i < chainFirst[c + 1]; i++) {
        if (srcLen[i] < 0) {
          throw new IllegalArgumentException("lengths must be >= 0");
        }
        total += srcLen[i];
      }
      if (chainSrcOff[c] < 0 || chainSrcOff[c] + total > src.capacity()) {
        throw new ArrayIndexOutOfBoundsException("chain " + c);
      }
      if (chainPrefixLen != null) {
        if (chainPrefixLen[c] < 0) {
          throw new IllegalArgumentException("lengths must be >= 0");
        }
        if (chainPrefixLen[c] > chainSrcOff[c]) {
          throw new ArrayIndexOutOfBoundsException("history of chain " + c);
        }
      }
    }
    for (int i = 0; i < n; i++) {
      if (destCap[i] < 0) {
        throw new IllegalArgumentException("lengths must be >= 0");
      }
      if (destOff[i] < 0 || destOff[i] + destCap[i] > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException("slot " + i);
      }
    }
  }

  /** {@code outLen[i]} of {@link #decompressSafeChain} and {@link #compressFastChain}: block i lies behind its chain's first failed block and was not done. */
  public static final int CHAIN_STOPPED = Integer.MIN_VALUE + 6;

  /**
   * liblz4's {@code LZ4_decompress_safe_continue} over chains of linked blocks (its rolling-prefix mode): chain c is the blocks
   * {@code chainFirst[c] .. chainFirst[c + 1] - 1}, decoded back to back into {@code dest[chainDestOff[c], chainDestOff[c]+chainDestCap[c])}
   * behind {@code chainPrefixLen[c]} bytes of history that lie in front of it in {@code dest} ({@code null}: no history).
   * {@code destCap[i]} is the capacity liblz4 would be given for block i; {@code stored} ({@code null}, or != 0 per block) marks raw
   * blocks, which are copied.  outLen[i] &gt;= 0: the decoded size; &lt; 0: -(input position)-1, which ends the chain -- the blocks behind
   * it get {@link #CHAIN_STOPPED}.  chainOutLen[c]: the bytes chain c decoded.
   */
  public static void decompressSafeChain(ByteBuffer src, long[] srcOff, int[] srcLen, int[] stored, int[] destCap, int[] chainFirst,
      ByteBuffer dest, long[] chainDestOff, long[] chainDestCap, int[] chainPrefixLen, int[] outLen, long[] chainOutLen) {
    final int n = srcOff.length, nc = chainDestOff.length;
    if (srcLen.length != n || destCap.length != n || outLen.length != n || (stored != null && stored.length != n)) {
      throw new IllegalArgumentException("per-block arrays differ in length");
    }
    if (chainFirst.length != nc + 1 || chainDestCap.length != nc || chainOutLen.length != nc || (chainPrefixLen != null && chainPrefixLen.length != nc)) {
      throw new IllegalArgumentException("per-chain arrays differ in length");
    }
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("direct buffers required");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    for (int i = 0; i < n; i++) {
      if (srcLen[i] < 0 || destCap[i] < 0) {
        throw new IllegalArgumentException("lengths must be >= 0");
      }
      if (srcOff[i] < 0 || srcOff[i] + srcLen[i] > src.capacity()) {
        throw new ArrayIndexOutOfBoundsException("block " + i);
      }
    }
    if (chainFirst[0] != 0 || chainFirst[nc] != n) {
      throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
    }
    for (int c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) {
        throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
      }
      if (chainDestOff[c] < 0 || chainDestCap[c] < 0 || chainDestOff[c] + chainDestCap[c] > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException("chain " + c);
      }
      if (chainPrefixLen != null && (chainPrefixLen[c] < 0 || chainPrefixLen[c] > chainDestOff[c])) {
        throw new ArrayIndexOutOfBoundsException("history of chain " + c);
      }
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchSafeChain(src, srcOff, srcLen, stored, destCap, chainFirst, dest, chainDestOff, chainDestCap, chainPrefixLen,
        outLen, chainOutLen, n, nc);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_decompress_safe_continue} on streams whose blocks land anywhere -- a ring buffer, two alternating block buffers, a
   * save area in front of a block buffer, a stream that starts from a dictionary elsewhere: every mode of an {@code LZ4_streamDecode_t}.
   * Stream c is the blocks {@code chainFirst[c] .. chainFirst[c+1]-1} of this call; block i is decoded to
   * {@code dest[destOff[i], destOff[i]+destCap[i])}, inside the stream's window {@code dest[chainWinOff[c], +chainWinLen[c])}.
   * {@code state} holds four longs per stream -- prefixEnd, prefixLen, extEnd, extLen, offsets into dest; all zero is a fresh stream,
   * {@code LZ4_setStreamDecode(dest + p, n)} is {p + n, n, 0, 0} -- and is read and written back.  outLen[i] = liblz4's return value,
   * {@link #CHAIN_STOPPED} behind a stream's first negative one of the call.  include/lz4hip.h says when the bytes are liblz4's (the
   * ring rule).  {@link DecodeStreams} keeps the states for its caller.
   */
  public static void decompressSafeStream(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
      long[] destOff, int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen) {
    decompressSafeStream(state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen, outLen, false);
  }

  /**
   * The same call; {@code inOrder}: the twin for streams whose slots overlap the history they can reach -- a ring of
   * {@link #decoderRingBufferSize} bytes, small rings kept in step with the writer's -- where the bytes are the plain byte-forward
   * definition's (include/lz4hip.h says when those are liblz4's).  The two may alternate on one stream from call to call.
   */
  public static void decompressSafeStream(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
      long[] destOff, int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen, boolean inOrder) {
    final int n = srcOff.length, nc = chainWinOff.length;
    if (srcLen.length != n || destOff.length != n || destCap.length != n || outLen.length != n) {
      throw new IllegalArgumentException("per-block arrays differ in length");
    }
    if (chainFirst.length != nc + 1 || chainWinLen.length != nc || state.length != 4 * nc) {
      throw new IllegalArgumentException("per-stream arrays differ in length");
    }
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("direct buffers required");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    for (int i = 0; i < n; i++) {
      if (srcLen[i] < 0 || destCap[i] < 0) {
        throw new IllegalArgumentException("lengths must be >= 0");
      }
      if (srcOff[i] < 0 || srcOff[i] + srcLen[i] > src.capacity()) {
        throw new ArrayIndexOutOfBoundsException("block " + i);
      }
      if (destOff[i] < 0 || destOff[i] + destCap[i] > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException("slot " + i);
      }
    }
    if (chainFirst[0] != 0 || chainFirst[nc] != n) {
      throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
    }
    for (int c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) {
        throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
      }
      if (chainWinOff[c] < 0 || chainWinLen[c] < 0 || chainWinOff[c] + chainWinLen[c] > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException("window of stream " + c);
      }
      final long pe = state[4 * c], pl = state[4 * c + 1], ee = state[4 * c + 2], el = state[4 * c + 3];
      if (pl < 0 || el < 0 || pl > pe || el > ee || (pl > 0 && pe > dest.capacity()) || (el > 0 && ee > dest.capacity())) {
        throw new ArrayIndexOutOfBoundsException("history of stream " + c);
      }
    }
    final int rc = inOrder
        ? LZ4HIPJNI.LZ4HIP_batchSafeStreamInOrder(state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen, outLen, n, nc)
        : LZ4HIPJNI.LZ4HIP_batchSafeStream(state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen, outLen, n, nc);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /** {@code LZ4_decoderRingBufferSize}: the smallest ring a stream of blocks of up to maxBlock bytes is decoded into; 0: no such ring. */
  public static int decoderRingBufferSize(int maxBlock) {
    return LZ4HIPJNI.LZ4HIP_decoderRingBufferSize(maxBlock);
  }

  /**
   * The states of n decode streams: per stream what an {@code LZ4_streamDecode_t} of liblz4 holds, as offsets into the one destination
   * its caller decodes into.  Plain host data: nothing on a device, nothing to close.  Every stream gives, over all the calls that name
   * it, the values ONE {@code LZ4_streamDecode_t} gives, however its blocks are cut into calls.
   */
  public static final class DecodeStreams {
    private final long[] state;
    private final boolean inOrder;

    public DecodeStreams(int n) {
      this(n, false);
    }

    /** inOrder: the set's calls go to the in-order twin ({@link LZ4HIPBatch#decompressSafeStream} with inOrder) unless a call says otherwise. */
    public DecodeStreams(int n, boolean inOrder) {
      if (n < 1) {
        throw new IllegalArgumentException("a set has at least one stream");
      }
      state = new long[4 * n];
      this.inOrder = inOrder;
    }

    public int size() {
      return state.length / 4;
    }

    /** {@code LZ4_setStreamDecode}: the stream starts behind the prefixLen bytes of dictionary that end at dest[prefixEnd]. */
    public void set(int streamId, long prefixEnd, long prefixLen) {
      if (prefixLen < 0 || prefixLen > prefixEnd) {
        throw new ArrayIndexOutOfBoundsException("history of stream " + streamId);
      }
      state[4 * streamId] = prefixEnd;
      state[4 * streamId + 1] = prefixLen;
      state[4 * streamId + 2] = 0;
      state[4 * streamId + 3] = 0;
    }

    /** makes the listed streams (null: all of them) fresh */
    public void reset(int[] streamId) {
      if (streamId == null) {
        java.util.Arrays.fill(state, 0L);
        return;
      }
      for (int c : streamId) {
        java.util.Arrays.fill(state, 4 * c, 4 * c + 4, 0L);
      }
    }

    /** {prefixEnd, prefixLen, extEnd, extLen} of one stream */
    public long[] state(int streamId) {
      return java.util.Arrays.copyOfRange(state, 4 * streamId, 4 * streamId + 4);
    }

    /** {@link LZ4HIPBatch#decompressSafeStream} for the streams streamId (distinct ids, one per chain of the call). */
    public void decompress(int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest, long[] destOff,
        int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen) {
      decompress(streamId, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen, outLen, inOrder);
    }

    /** the same through the entry point this call names: the two may alternate on a stream from call to call */
    public void decompress(int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest, long[] destOff,
        int[] destCap, long[] chainWinOff, long[] chainWinLen, int[] outLen, boolean inOrder) {
      final long[] st = new long[4 * streamId.length];
      final boolean[] seen = new boolean[size()];
      for (int k = 0; k < streamId.length; k++) {
        if (streamId[k] < 0 || streamId[k] >= size() || seen[streamId[k]]) {
          throw new IllegalArgumentException("streamId must be distinct and below the number of streams");
        }
        seen[streamId[k]] = true;
        System.arraycopy(state, 4 * streamId[k], st, 4 * k, 4);
      }
      decompressSafeStream(st, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen, outLen, inOrder);
      for (int k = 0; k < streamId.length; k++) {
        System.arraycopy(st, 4 * k, state, 4 * streamId[k], 4);
      }
    }
  }

  /**
   * liblz4's {@code LZ4_compress_HC_continue} on streams whose sources land anywhere -- a ring that wraps, two alternating block buffers, a
   * save area kept with {@code LZ4_saveDictHC}, a dictionary elsewhere.  Stream c is the blocks {@code chainFirst[c] .. chainFirst[c+1]-1}
   * of this call; block i is {@code src[srcOff[i], srcOff[i]+srcLen[i])} and owns the slot {@code dest[destOff[i], destOff[i]+destCap[i])}.
   * {@code state} holds five longs per stream -- prefixEnd, prefixLen, extEnd, extLen, index, offsets into src; all zero is a fresh
   * stream -- and is read and written back.  outLen[i] = liblz4's return value; 0 (it did not fit) does not end the stream.  A call is a
   * snapshot of src; include/lz4hip.h states the contract and its exceptions.  {@link CompressStreamsHC} keeps the states for its caller.
   */
  public static void compressHCStream(long[] state, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest,
      long[] destOff, int[] destCap, int[] outLen, int level) {
    final int n = srcOff.length, nc = chainFirst.length - 1;
    if (srcLen.length != n || destOff.length != n || destCap.length != n || outLen.length != n) {
      throw new IllegalArgumentException("per-block arrays differ in length");
    }
    if (nc < 0 || state.length != 5 * nc) {
      throw new IllegalArgumentException("per-stream arrays differ in length");
    }
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("direct buffers required");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    for (int i = 0; i < n; i++) {
      final long len = srcLen[i] >= 0 && srcLen[i] <= 0x7E000000 ? srcLen[i] : 0;   // (any other length reads nothing: the engine's rule)
      if (srcOff[i] < 0 || srcOff[i] + len > src.capacity()) {
        throw new ArrayIndexOutOfBoundsException("block " + i);
      }
      if (destOff[i] < 0 || destOff[i] + Math.max(destCap[i], 0) > dest.capacity()) {
        throw new ArrayIndexOutOfBoundsException("slot " + i);
      }
    }
    if (chainFirst[0] != 0 || chainFirst[nc] != n) {
      throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
    }
    for (int c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) {
        throw new IllegalArgumentException("chainFirst must ascend from 0 to the number of blocks");
      }
      final long pe = state[5 * c], pl = state[5 * c + 1], ee = state[5 * c + 2], el = state[5 * c + 3];
      if (pl < 0 || el < 0 || pl > pe || el > ee || (pl > 0 && pe > src.capacity()) || (el > 0 && ee > src.capacity()) || state[5 * c + 4] < 0) {
        throw new ArrayIndexOutOfBoundsException("history of stream " + c);
      }
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchHCStream(state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, outLen, n, nc, level);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * The states of n HC compress streams whose sources land anywhere: per stream what an {@code LZ4_streamHC_t} of liblz4 keeps beside
   * its tables, as offsets into the one source its caller compresses from.  Plain host data: nothing on a device, nothing to close.
   * Every stream gives, over all the calls that name it, the values ONE {@code LZ4_streamHC_t} gives, however its blocks are cut into
   * calls.  {@code loadDict} and {@code saveDict} are the two state edits include/lz4hip.h states ({@code lz4hip_hcstream_load_dict},
   * {@code lz4hip_hcstream_save_dict}).
   */
  public static final class CompressStreamsHC {
    private final long[] state;
    private final int level;

    public CompressStreamsHC(int n, int level) {
      if (n < 1) {
        throw new IllegalArgumentException("a set has at least one stream");
      }
      state = new long[5 * n];
      this.level = level;
    }

    public int size() {
      return state.length / 5;
    }

    public int level() {
      return level;
    }

    /** {@code LZ4_loadDictHC}: the stream is fresh behind the dictLen bytes of dictionary that end at src[dictEnd]. */
    public void loadDict(int streamId, long dictEnd, long dictLen) {
      if (dictLen < 0 || dictLen > dictEnd) {
        throw new ArrayIndexOutOfBoundsException("history of stream " + streamId);
      }
      final long kept = Math.min(dictLen, 65536);
      final int o = 5 * streamId;
      state[o] = dictEnd;
      state[o + 1] = kept;
      state[o + 2] = 0;
      state[o + 3] = 0;
      state[o + 4] = kept;
    }

    /** {@code LZ4_saveDictHC} for the caller who has copied the last k bytes the stream consumed to src[bufOff ..] -> the bytes kept. */
    public int saveDict(int streamId, long bufOff, int k) {
      final int o = 5 * streamId;
      long kept = Math.min(Math.max(k, 0), 65536);
      if (kept < 4) {
        kept = 0;
      }
      kept = Math.min(kept, state[o + 1]);
      state[o] = bufOff + kept;
      state[o + 1] = kept;
      state[o + 3] = 0;
      return (int) kept;
    }

    /** makes the listed streams (null: all of them) fresh */
    public void reset(int[] streamId) {
      if (streamId == null) {
        java.util.Arrays.fill(state, 0L);
        return;
      }
      for (int c : streamId) {
        java.util.Arrays.fill(state, 5 * c, 5 * c + 5, 0L);
      }
    }

    /** {prefixEnd, prefixLen, extEnd, extLen, index} of one stream */
    public long[] state(int streamId) {
      return java.util.Arrays.copyOfRange(state, 5 * streamId, 5 * streamId + 5);
    }

    /** {@link LZ4HIPBatch#compressHCStream} at the set's level for the streams streamId (distinct ids, one per chain of the call). */
    public void compress(int[] streamId, ByteBuffer src, long[] srcOff, int[] srcLen, int[] chainFirst, ByteBuffer dest, long[] destOff,
        int[] destCap, int[] outLen) {
      final long[] st = new long[5 * streamId.length];
      final boolean[] seen = new boolean[size()];
      for (int k = 0; k < streamId.length; k++) {
        if (streamId[k] < 0 || streamId[k] >= size() || seen[streamId[k]]) {
          throw new IllegalArgumentException("streamId must be distinct and below the number of streams");
        }
        seen[streamId[k]] = true;
        System.arraycopy(state, 5 * streamId[k], st, 5 * k, 5);
      }
      compressHCStream(st, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, outLen, level);
      for (int k = 0; k < streamId.length; k++) {
        System.arraycopy(st, 5 * k, state, 5 * streamId[k], 5);
      }
    }
  }

  /**
   * liblz4's {@code LZ4_decompress_safe_partial} per block: the first {@code min(targetLen[i], destCap[i])} bytes of block i (fewer
   * where a cut stream ends first) into the slot {@code dest[destOff[i], destOff[i]+destCap[i])}, nothing past
   * {@code destOff[i] + min(targetLen[i], destCap[i])}.  outLen[i] &gt;= 0: bytes decoded; &lt; 0: -(input position)-1.
   */
  public static void decompressSafePartial(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetLen,
      int[] destCap, int[] outLen) {
    check(src, dest, srcOff, srcLen, destOff, destCap, outLen);
    if (targetLen.length != srcOff.length) {
      throw new IllegalArgumentException("per-block arrays must have the same length");
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchSafePartial(src, srcOff, srcLen, dest, destOff, targetLen, destCap, outLen, srcOff.length);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * liblz4's {@code LZ4_compress_HC_destSize} per block at HC level {@code level}: as much of block i as fits in exactly
   * {@code targetSize[i]} bytes, written to the slot {@code dest[destOff[i], destOff[i]+targetSize[i])}.  outLen[i]: bytes written
   * (0 for an empty target); srcConsumed[i]: the source bytes they cover.
   */
  public static void compressHCDestSize(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] targetSize,
      int[] outLen, int[] srcConsumed, int level) {
    check(src, dest, srcOff, srcLen, destOff, targetSize, outLen);
    if (srcConsumed.length < srcOff.length) {
      throw new IllegalArgumentException("per-block arrays must have the same length");
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchHCDestSize(src, srcOff, srcLen, dest, destOff, targetSize, outLen, srcConsumed, srcOff.length, level);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * The decoded size of every block without a destination buffer: outLen[i] is what {@link #decompressSafe} would report for block i
   * with a slot of {@code destCap[i]} bytes -- the decoded size, or -(input position)-1 -- and nothing is decoded into memory.
   * For blocks whose sizes are unknown or untrusted this replaces a decode into worst-case slots; outLen[i] &gt;= 0 means that
   * decompressSafe with that capacity succeeds and returns that number.
   */
  public static void decompressedLengths(ByteBuffer src, long[] srcOff, int[] srcLen, int[] destCap, int[] outLen) {
    if (!src.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    final int n = srcOff.length;
    if (srcLen.length != n || destCap.length != n || outLen.length != n) {
      throw new IllegalArgumentException("per-block arrays must have the same length");
    }
    for (int i = 0; i < n; i++) {
      if (srcOff[i] < 0 || srcLen[i] < 0 || srcOff[i] + srcLen[i] > src.capacity() || destCap[i] < 0) {
        throw new IndexOutOfBoundsException("block " + i + " lies outside its buffer");
      }
    }
    final int rc = LZ4HIPJNI.LZ4HIP_batchDecompressedLengths(src, srcOff, srcLen, destCap, outLen, n);
    if (rc != 0) {
      throw new LZ4Exception("liblz4hip status " + rc + ": " + LZ4HIPJNI.lastError());
    }
  }

  /** outLen[i] &gt;= 0: decompressed size; &lt; 0: -(input position)-1. */
  public static void decompressSafe(ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen) {
    run(1, 0, src, srcOff, srcLen, dest, destOff, destCap, outLen);
  }

  /** destLen[i] is the exact decompressed size; outConsumed[i] &gt; 0: bytes read from src. */
  public static void decompressFast(ByteBuffer src, long[] srcOff, int[] srcCap, ByteBuffer dest, long[] destOff, int[] destLen, int[] outConsumed) {
    run(2, 0, src, srcOff, srcCap, dest, destOff, destLen, outConsumed);
  }

  public static void compressHC(int level, ByteBuffer src, long[] srcOff, int[] srcLen, ByteBuffer dest, long[] destOff, int[] destCap, int[] outLen) {
    run(3, level, src, srcOff, srcLen, dest, destOff, destCap, outLen);
  }

  /** Container kinds of {@link #containerBlocks}. */
  public static final int FRAME_BLOCKS = 0, LZ4BLOCK_BLOCKS = 1;

  /**
   * The data blocks of an LZ4 Frame ({@link #FRAME_BLOCKS}: what {@code LZ4FrameOutputStream.writeBlock} emits per block;
   * {@code blockChecksum} adds the XXH32 of each stored payload) or of the LZ4Block container ({@link #LZ4BLOCK_BLOCKS}: what
   * {@code LZ4BlockOutputStream.flushBufferedData} emits) for {@code src[srcOff, srcOff+len)} cut into {@code blockSize} pieces,
   * assembled on the device: compression, raw fallback, headers, payload compaction and checksums happen behind one another
   * there, only the finished bytes come back.  {@code level} 0 = fast, 1..17 = HC.  Returns the bytes written at {@code dest[destOff..)}.
   */
  public static long containerBlocks(int kind, boolean blockChecksum, int level, ByteBuffer src, long srcOff, long len, int blockSize,
                                     ByteBuffer dest, long destOff) {
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    if (srcOff < 0 || len < 0 || destOff < 0 || srcOff + len > src.capacity() || destOff > dest.capacity()) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final long r = LZ4HIPJNI.LZ4HIP_containerBlocks(kind, blockChecksum ? 1 : 0, level, src, srcOff, len, blockSize, dest, destOff,
        dest.capacity() - destOff);
    if (r < 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
    return r;
  }

  /** Stop reasons of {@link #containerDecode} ({@code info[2]}; include/lz4hip.h). */
  public static final int CR_END = 0, CR_MORE = 1, CR_TRUNCATED = 2, CR_BLOCK_TOO_BIG = 3, CR_BLOCK_CHECKSUM = 4, CR_DECODE = 5,
      CR_CORRUPT = 6, CR_SLOTS = 7;

  /**
   * Destination bytes a {@link #containerDecode} call over {@code src[srcOff, srcOff+len)} can need: a host-side walk of the size
   * words / headers (frame: {@code maxBlock} per compressed block, the stored size of a raw one; LZ4Block: the headers' original
   * lengths).  {@code blocks[0]} receives the number of whole blocks present (at most {@code nMax}).
   */
  public static long containerDecodeBound(int kind, boolean blockChecksum, ByteBuffer src, long srcOff, long len, int maxBlock, int nMax,
                                          int[] blocks) {
    if (!src.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (blocks == null) {
      throw new NullPointerException("blocks");
    }
    if (srcOff < 0 || len < 0 || srcOff + len > src.capacity() || blocks.length < 1) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final long r = LZ4HIPJNI.LZ4HIP_containerDecodeBound(kind, blockChecksum ? 1 : 0, src, srcOff, len, maxBlock, nMax, blocks);
    if (r < 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
    return r;
  }

  /**
   * The READ side of the container formats on the device: the data blocks of an LZ4 Frame body ({@link #FRAME_BLOCKS}: {@code src}
   * from the first block's size word on; {@code maxBlock} = the frame's block maximum size) or of an LZ4Block stream
   * ({@link #LZ4BLOCK_BLOCKS}; {@code maxBlock} = an upper bound of the original lengths, {@code 1 << (10 + level nibble)}) are
   * walked, verified and decoded there -- what {@code LZ4FrameInputStream.readBlock} / {@code LZ4BlockInputStream.refill} do block
   * by block, for up to {@code nMax} blocks in one call.  The decoded blocks land back to back at {@code dest[destOff..)},
   * {@code sizes[k]} = decoded size of block k, {@code info} = {blocks delivered, bytes of src consumed, stop reason (CR_*), decoded
   * bytes, liblz4's code of a failed decode}.  The reader maps the stop reason to the reference's exception and goes on from
   * {@code srcOff + info[1]}.
   */
  public static void containerDecode(int kind, boolean blockChecksum, ByteBuffer src, long srcOff, long len, int maxBlock, int nMax,
                                     ByteBuffer dest, long destOff, int[] sizes, long[] info) {
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    if (srcOff < 0 || len < 0 || destOff < 0 || srcOff + len > src.capacity() || destOff > dest.capacity() || sizes.length < nMax
        || info.length < 5) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final int r = LZ4HIPJNI.LZ4HIP_containerDecode(kind, blockChecksum ? 1 : 0, src, srcOff, len, maxBlock, nMax, dest, destOff,
        dest.capacity() - destOff, sizes, info);
    if (r != 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * What a {@link #containerDecodeMany} call over the same items can need: {@code itemBlocks[c]} = whole blocks of the first
   * {@code nMax} that item c holds, {@code itemDstBytes[c]} = the most their decoded forms can need -- per item what
   * {@link #containerDecodeBound} says of it.  No device work.  Size {@code dest} by the sum of {@code itemDstBytes} and
   * {@code sizes} by the sum of {@code itemBlocks}.
   */
  public static void containerDecodeManyBound(int kind, ByteBuffer bodies, long[] bodyOff, long[] bodyLen, int[] maxBlock,
                                              boolean[] blockChecksum, int nMax, int[] itemBlocks, long[] itemDstBytes) {
    final int n = bodyOff.length;
    if (!bodies.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (bodyLen.length != n || maxBlock.length != n || blockChecksum.length != n || itemBlocks.length < n || itemDstBytes.length < n) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final int r = LZ4HIPJNI.LZ4HIP_containerDecodeManyBound(kind, bodies, bodyOff, bodyLen, maxBlock, manyFlags(bodies, bodyOff, bodyLen,
        blockChecksum), n, nMax, itemBlocks, itemDstBytes);
    if (r != 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * {@link #containerDecode} for MANY containers of one kind in ONE call: item c is {@code bodies[bodyOff[c], + bodyLen[c])} with its
   * own {@code maxBlock[c]} and {@code blockChecksum[c]}.  Per item the result is what {@link #containerDecode} gives for that body:
   * {@code info[5c .. 5c+4]}, the sizes {@code sizes[itemFirst[c] .. itemFirst[c+1])} and the bytes
   * {@code dest[destOff + itemDstOff[c] .. destOff + itemDstOff[c+1])}; delivered blocks lie back to back, item after item.  A group of
   * items costs one launch sequence, whatever their number; an item that stops changes nothing about another.
   * {@code itemDstOff} and {@code itemFirst} have one entry more than there are items, {@code info} five per item.
   */
  public static void containerDecodeMany(int kind, ByteBuffer bodies, long[] bodyOff, long[] bodyLen, int[] maxBlock, boolean[] blockChecksum,
                                         int nMax, ByteBuffer dest, long destOff, long[] itemDstOff, int[] itemFirst, int[] sizes, long[] info) {
    final int n = bodyOff.length;
    if (!bodies.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    if (bodyLen.length != n || maxBlock.length != n || blockChecksum.length != n || destOff < 0 || destOff > dest.capacity()
        || itemDstOff.length < n + 1 || itemFirst.length < n + 1 || info.length / 5 < n) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final int r = LZ4HIPJNI.LZ4HIP_containerDecodeMany(kind, bodies, bodyOff, bodyLen, maxBlock, manyFlags(bodies, bodyOff, bodyLen,
        blockChecksum), n, nMax, dest, destOff, dest.capacity() - destOff, itemDstOff, itemFirst, sizes, info);
    if (r != 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * What a {@link #containerBlocksMany} call over the same items can need: {@code itemBlocks[c]} = ceil(srcLen[c] / blockSize[c]),
   * {@code itemDstBytes[c]} = gapHead[c] + srcLen[c] + itemBlocks[c] x (frame blocks: 4, 8 with block checksums; LZ4Block blocks: 21)
   * + gapTail[c].  No device work.  Size {@code dest} by the sum of {@code itemDstBytes}.  {@code gapHead} and {@code gapTail} may be
   * null: no gaps.
   */
  public static void containerBlocksManyBound(int kind, long[] srcLen, int[] blockSize, boolean[] blockChecksum, int[] gapHead, int[] gapTail,
                                              int[] itemBlocks, long[] itemDstBytes) {
    final int n = srcLen.length;
    if (blockSize.length != n || blockChecksum.length != n || (gapHead != null && gapHead.length != n) || (gapTail != null && gapTail.length != n)
        || itemBlocks.length < n || itemDstBytes.length < n) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final int[] flags = new int[n];
    for (int c = 0; c < n; c++) {
      flags[c] = blockChecksum[c] ? 1 : 0;
    }
    final int r = LZ4HIPJNI.LZ4HIP_containerBlocksManyBound(kind, srcLen, blockSize, flags, gapHead != null ? gapHead : new int[n],
        gapTail != null ? gapTail : new int[n], n, itemBlocks, itemDstBytes);
    if (r != 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
  }

  /**
   * {@link #containerBlocks} for MANY payloads of one kind in ONE call: item c is {@code src[srcOff[c], + srcLen[c])} cut into pieces of
   * {@code blockSize[c]} bytes, with block checksums where {@code blockChecksum[c]} ({@link #FRAME_BLOCKS} only).  {@code level}: 0 for
   * the fast compressor, else the HC level.  Item c lands at {@code dest[destOff + itemDstOff[c] .. destOff + itemDstOff[c+1])}:
   * {@code gapHead[c]} zero bytes, the bytes {@link #containerBlocks} writes for the item, {@code gapTail[c]} zero bytes -- room for a
   * frame header, the end mark and the content checksum, so that a writer places them without copying the blocks again.  Where
   * {@code contentHash[c]} is asked for ({@code wantContentHash[c]}), it is the XXH32 (seed 0) of the item's source, else 0.  A group of
   * items costs one launch sequence, whatever their number.  {@code itemDstOff} has one entry more than there are items;
   * {@code gapHead}, {@code gapTail} and {@code wantContentHash} may be null (no gaps, no hashes; {@code contentHash} may then be null).
   */
  public static void containerBlocksMany(int kind, int level, ByteBuffer src, long[] srcOff, long[] srcLen, int[] blockSize, boolean[] blockChecksum,
                                         int[] gapHead, int[] gapTail, boolean[] wantContentHash, ByteBuffer dest, long destOff, long[] itemDstOff,
                                         int[] contentHash) {
    final int n = srcOff.length;
    if (!src.isDirect() || !dest.isDirect()) {
      throw new IllegalArgumentException("LZ4HIPBatch needs direct ByteBuffers");
    }
    if (dest.isReadOnly()) {
      throw new java.nio.ReadOnlyBufferException();
    }
    if (srcLen.length != n || blockSize.length != n || blockChecksum.length != n || (gapHead != null && gapHead.length != n)
        || (gapTail != null && gapTail.length != n) || (wantContentHash != null && (wantContentHash.length != n || contentHash == null))
        || (contentHash != null && contentHash.length < n) || destOff < 0 || destOff > dest.capacity() || itemDstOff.length < n + 1) {
      throw new ArrayIndexOutOfBoundsException();
    }
    final int[] flags = manyFlags(src, srcOff, srcLen, blockChecksum);
    for (int c = 0; wantContentHash != null && c < n; c++) {
      flags[c] |= wantContentHash[c] ? 2 : 0;
    }
    final int r = LZ4HIPJNI.LZ4HIP_containerBlocksMany(kind, level, src, srcOff, srcLen, blockSize, flags, gapHead != null ? gapHead : new int[n],
        gapTail != null ? gapTail : new int[n], n, dest, destOff, dest.capacity() - destOff, itemDstOff, contentHash != null ? contentHash : new int[n]);
    if (r != 0) {
      throw new LZ4Exception("liblz4hip status " + r + ": " + LZ4HIPJNI.lastError());
    }
  }

  /** the items' ranges checked against the buffer (SafeUtils.checkRange per item) -> the flag word of every item */
  private static int[] manyFlags(ByteBuffer bodies, long[] bodyOff, long[] bodyLen, boolean[] blockChecksum) {
    final int[] flags = new int[bodyOff.length];
    for (int c = 0; c < bodyOff.length; c++) {
      if (bodyOff[c] < 0 || bodyLen[c] < 0 || bodyOff[c] + bodyLen[c] > bodies.capacity()) {
        throw new ArrayIndexOutOfBoundsException();
      }
      flags[c] = blockChecksum[c] ? 1 : 0;
    }
    return flags;
  }
}
