package net.jpountz.lz4;

/*
 * Adapted from lz4-java (src/java/net/jpountz/lz4/LZ4HCJNICompressor.java), Copyright 2020 Adrien Grand and the lz4-java contributors,
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

import static net.jpountz.lz4.LZ4Constants.DEFAULT_COMPRESSION_LEVEL;
import static net.jpountz.util.ByteBufferUtils.checkNotReadOnly;
import static net.jpountz.util.ByteBufferUtils.checkRange;
import static net.jpountz.util.SafeUtils.checkRange;

import java.nio.ByteBuffer;

/**
 * High-compression {@link LZ4Compressor} of the "HIP" family (twin of LZ4HCJNICompressor.java:30-89).
 * LZ4Factory needs the INSTANCE field and the declared (int) constructor (LZ4Factory.java:193-202).
 *
 * {@code compressDestSize}: liblz4's {@code LZ4_compress_HC_destSize} at this compressor's level -- as much of the source as
 * fits in exactly {@code targetDestSize} bytes.  {@code compressWithDict}: liblz4's {@code LZ4_loadDictHC} +
 * {@code LZ4_compress_HC_continue} on a fresh stream at this compressor's level.
 */
final class LZ4HCHIPCompressor extends LZ4Compressor {

  public static final LZ4HCHIPCompressor INSTANCE = new LZ4HCHIPCompressor();

  private final int compressionLevel;

  LZ4HCHIPCompressor() { this(DEFAULT_COMPRESSION_LEVEL); }
  LZ4HCHIPCompressor(int compressionLevel) {
    this.compressionLevel = compressionLevel;
  }

  @Override
  public int compress(byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int maxDestLen) {
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, maxDestLen);
    final int result = LZ4HIPJNI.LZ4HIP_compressHC(src, null, srcOff, srcLen, dest, null, destOff, maxDestLen, compressionLevel);
    if (result <= 0) {
      throw new LZ4Exception();
    }
    return result;
  }

  @Override
  public int compress(ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int maxDestLen) {
    checkNotReadOnly(dest);
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, maxDestLen);
    if ((src.hasArray() || src.isDirect()) && (dest.hasArray() || dest.isDirect())) {
      final byte[] srcArr = src.hasArray() ? src.array() : null;
      final byte[] destArr = dest.hasArray() ? dest.array() : null;
      final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
      final int dof = destArr != null ? destOff + dest.arrayOffset() : destOff;
      final int result = LZ4HIPJNI.LZ4HIP_compressHC(srcArr, srcArr == null ? src : null, so, srcLen,
                                                     destArr, destArr == null ? dest : null, dof, maxDestLen, compressionLevel);
      if (result <= 0) {
        throw new LZ4Exception();
      }
      return result;
    }
    return LZ4Factory.safeInstance().highCompressor(compressionLevel).compress(src, srcOff, srcLen, dest, destOff, maxDestLen);
  }

  /**
   * liblz4's {@code LZ4_loadDictHC} + {@code LZ4_compress_HC_continue} on a fresh stream at this compressor's level:
   * {@code src[srcOff, srcOff+srcLen)} compressed alone against {@code dict} (which is not contiguous with {@code src}) into
   * {@code dest[destOff, ...)}; returns the compressed size.  {@code LZ4HIPSafeDecompressor.decompressWithDict} reads it.  The argument
   * checks and the exception are compress()'s.
   */
  public int compressWithDict(LZ4HIPDictionary dict, byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int maxDestLen) {
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, maxDestLen);
    final int result = LZ4HIPJNI.LZ4HIP_compress_hc_dict(dict.handle(), compressionLevel, src, null, srcOff, srcLen, dest, null, destOff, maxDestLen);
    if (result <= 0) {
      throw result == 0 ? new LZ4Exception() : new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
    }
    return result;
  }

  /** {@link #compressWithDict(LZ4HIPDictionary, byte[], int, int, byte[], int, int)} over heap or direct buffers (positions untouched). */
  public int compressWithDict(LZ4HIPDictionary dict, ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int maxDestLen) {
    checkNotReadOnly(dest);
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, maxDestLen);
    if (!(src.hasArray() || src.isDirect()) || !(dest.hasArray() || dest.isDirect())) {
      throw new IllegalArgumentException("compressWithDict needs heap-backed or direct ByteBuffers");
    }
    final byte[] srcArr = src.hasArray() ? src.array() : null;
    final byte[] destArr = dest.hasArray() ? dest.array() : null;
    final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
    final int dof = destArr != null ? destOff + dest.arrayOffset() : destOff;
    final int result = LZ4HIPJNI.LZ4HIP_compress_hc_dict(dict.handle(), compressionLevel, srcArr, srcArr == null ? src : null, so, srcLen,
                                                         destArr, destArr == null ? dest : null, dof, maxDestLen);
    if (result <= 0) {
      throw result == 0 ? new LZ4Exception() : new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
    }
    return result;
  }

  private int nativeDestSize(byte[] srcArr, ByteBuffer srcBuf, int srcOff, int srcLen, byte[] destArr, ByteBuffer destBuf, int destOff,
      int targetDestSize, int[] srcConsumed) {
    if (srcConsumed.length < 1) {
      throw new IllegalArgumentException("srcConsumed must hold one element");
    }
    final int[] size = {srcLen};
    final int result = LZ4HIPJNI.LZ4HIP_compressHC_dest_size(srcArr, srcBuf, srcOff, size, destArr, destBuf, destOff, targetDestSize,
                                                             compressionLevel);
    if (result < 0) {
      throw new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
    }
    srcConsumed[0] = size[0];
    return result;
  }

  /**
   * Compresses as much of {@code src[srcOff, srcOff+srcLen)} as fits in exactly {@code targetDestSize} bytes at
   * {@code dest[destOff..)}: returns the bytes written and sets {@code srcConsumed[0]} to the source bytes they cover.
   */
  public int compressDestSize(byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int targetDestSize, int[] srcConsumed) {
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, targetDestSize);
    return nativeDestSize(src, null, srcOff, srcLen, dest, null, destOff, targetDestSize, srcConsumed);
  }

  /** {@link #compressDestSize(byte[], int, int, byte[], int, int, int[])} on buffers (positions and limits are not used). */
  public int compressDestSize(ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int targetDestSize, int[] srcConsumed) {
    checkNotReadOnly(dest);
    checkRange(src, srcOff, srcLen);
    checkRange(dest, destOff, targetDestSize);
    if ((src.hasArray() || src.isDirect()) && (dest.hasArray() || dest.isDirect())) {
      byte[] srcArr = null, destArr = null;
      ByteBuffer srcBuf = null, destBuf = null;
      if (src.hasArray()) {
        srcArr = src.array();
        srcOff += src.arrayOffset();
      } else {
        srcBuf = src;
      }
      if (dest.hasArray()) {
        destArr = dest.array();
        destOff += dest.arrayOffset();
      } else {
        destBuf = dest;
      }
      return nativeDestSize(srcArr, srcBuf, srcOff, srcLen, destArr, destBuf, destOff, targetDestSize, srcConsumed);
    }
    // neither array-backed nor direct: through byte[] copies (no other family has this call to fall back to)
    final byte[] srcArr = new byte[srcLen];
    final byte[] destArr = new byte[targetDestSize];
    final ByteBuffer s = src.duplicate();
    s.clear();
    s.position(srcOff);
    s.get(srcArr, 0, srcLen);
    final int result = compressDestSize(srcArr, 0, srcLen, destArr, 0, targetDestSize, srcConsumed);
    final ByteBuffer d = dest.duplicate();
    d.clear();
    d.position(destOff);
    d.put(destArr, 0, result);
    return result;
  }
}
