package net.jpountz.lz4;

/*
 * Adapted from lz4-java (src/java/net/jpountz/lz4/LZ4JNISafeDecompressor.java), Copyright 2020 Adrien Grand and the lz4-java contributors,
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

import net.jpountz.util.ByteBufferUtils;
import net.jpountz.util.SafeUtils;

/**
 * {@link LZ4SafeDecompressor} of the "HIP" family; return codes and the exception message equal
 * LZ4JNISafeDecompressor.java:34-43 (liblz4 1.9.3 LZ4_decompress_safe), including on malformed input.
 */
final class LZ4HIPSafeDecompressor extends LZ4SafeDecompressor {

  public static final LZ4HIPSafeDecompressor INSTANCE = new LZ4HIPSafeDecompressor();

  @Override
  public final int decompress(byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int maxDestLen) {
    SafeUtils.checkRange(src, srcOff, srcLen);
    SafeUtils.checkRange(dest, destOff, maxDestLen);
    final int result = LZ4HIPJNI.LZ4HIP_decompress_safe(src, null, srcOff, srcLen, dest, null, destOff, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  @Override
  public int decompress(ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int maxDestLen) {
    ByteBufferUtils.checkNotReadOnly(dest);
    ByteBufferUtils.checkRange(src, srcOff, srcLen);
    ByteBufferUtils.checkRange(dest, destOff, maxDestLen);
    if ((src.hasArray() || src.isDirect()) && (dest.hasArray() || dest.isDirect())) {
      final byte[] srcArr = src.hasArray() ? src.array() : null;
      final byte[] destArr = dest.hasArray() ? dest.array() : null;
      final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
      final int dof = destArr != null ? destOff + dest.arrayOffset() : destOff;
      final int result = LZ4HIPJNI.LZ4HIP_decompress_safe(srcArr, srcArr == null ? src : null, so, srcLen,
                                                          destArr, destArr == null ? dest : null, dof, maxDestLen);
      if (result < 0) {
        throw new LZ4Exception("Error decoding offset " + (srcOff - result) + " of input buffer");
      }
      return result;
    }
    return LZ4Factory.safeInstance().safeDecompressor().decompress(src, srcOff, srcLen, dest, destOff, maxDestLen);
  }

  /**
   * liblz4's {@code LZ4_decompress_safe_usingDict}: decodes a block that was compressed against {@code dict} (a dictionary that is not
   * contiguous with {@code dest}) into {@code dest[destOff, ...)} and returns the decoded size.  The argument checks and the exception
   * message are decompress()'s.
   */
  public final int decompressWithDict(LZ4HIPDictionary dict, byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int maxDestLen) {
    SafeUtils.checkRange(src, srcOff, srcLen);
    SafeUtils.checkRange(dest, destOff, maxDestLen);
    final int result = LZ4HIPJNI.LZ4HIP_decompress_safe_dict(dict.handle(), src, null, srcOff, srcLen, dest, null, destOff, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  /** {@link #decompressWithDict(LZ4HIPDictionary, byte[], int, int, byte[], int, int)} over heap or direct buffers (positions untouched). */
  public int decompressWithDict(LZ4HIPDictionary dict, ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int maxDestLen) {
    ByteBufferUtils.checkNotReadOnly(dest);
    ByteBufferUtils.checkRange(src, srcOff, srcLen);
    ByteBufferUtils.checkRange(dest, destOff, maxDestLen);
    if (!(src.hasArray() || src.isDirect()) || !(dest.hasArray() || dest.isDirect())) {
      throw new IllegalArgumentException("decompressWithDict needs heap-backed or direct ByteBuffers");
    }
    final byte[] srcArr = src.hasArray() ? src.array() : null;
    final byte[] destArr = dest.hasArray() ? dest.array() : null;
    final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
    final int dof = destArr != null ? destOff + dest.arrayOffset() : destOff;
    final int result = LZ4HIPJNI.LZ4HIP_decompress_safe_dict(dict.handle(), srcArr, srcArr == null ? src : null, so, srcLen,
                                                             destArr, destArr == null ? dest : null, dof, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  /**
   * liblz4's {@code LZ4_decompress_safe_partial}: decodes the first {@code min(targetLen, maxDestLen)} bytes of the block (fewer
   * where a cut stream ends first) into {@code dest[destOff, ...)} and returns the count; nothing is written past
   * {@code destOff + min(targetLen, maxDestLen)}.  The argument checks and the exception message are decompress()'s.
   */
  public final int decompressPartial(byte[] src, int srcOff, int srcLen, byte[] dest, int destOff, int targetLen, int maxDestLen) {
    SafeUtils.checkRange(src, srcOff, srcLen);
    SafeUtils.checkRange(dest, destOff, maxDestLen);
    final int result = LZ4HIPJNI.LZ4HIP_decompress_safe_partial(src, null, srcOff, srcLen, dest, null, destOff, targetLen, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  /** {@link #decompressPartial(byte[], int, int, byte[], int, int, int)} over heap or direct buffers (positions untouched). */
  public int decompressPartial(ByteBuffer src, int srcOff, int srcLen, ByteBuffer dest, int destOff, int targetLen, int maxDestLen) {
    ByteBufferUtils.checkNotReadOnly(dest);
    ByteBufferUtils.checkRange(src, srcOff, srcLen);
    ByteBufferUtils.checkRange(dest, destOff, maxDestLen);
    if (!(src.hasArray() || src.isDirect()) || !(dest.hasArray() || dest.isDirect())) {
      throw new IllegalArgumentException("decompressPartial needs heap-backed or direct ByteBuffers");
    }
    final byte[] srcArr = src.hasArray() ? src.array() : null;
    final byte[] destArr = dest.hasArray() ? dest.array() : null;
    final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
    final int dof = destArr != null ? destOff + dest.arrayOffset() : destOff;
    final int result = LZ4HIPJNI.LZ4HIP_decompress_safe_partial(srcArr, srcArr == null ? src : null, so, srcLen,
                                                                destArr, destArr == null ? dest : null, dof, targetLen, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  /**
   * What {@code decompress(src, srcOff, srcLen, dest, destOff, maxDestLen)} would return -- the decoded size of the block for a
   * destination of {@code maxDestLen} bytes -- without a destination: nothing is decoded into memory.  The argument checks and the
   * exception message are decompress()'s; the dispatch is decompress()'s too (heap arrays are staged, direct buffers used in place).
   */
  public final int decompressedLength(byte[] src, int srcOff, int srcLen, int maxDestLen) {
    SafeUtils.checkRange(src, srcOff, srcLen);
    if (maxDestLen < 0) {
      throw new IllegalArgumentException("maxDestLen must be >= 0");
    }
    final int result = LZ4HIPJNI.LZ4HIP_decompressed_length(src, null, srcOff, srcLen, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }

  /** {@link #decompressedLength(byte[], int, int, int)} over a heap or direct buffer (its position is untouched). */
  public int decompressedLength(ByteBuffer src, int srcOff, int srcLen, int maxDestLen) {
    ByteBufferUtils.checkRange(src, srcOff, srcLen);
    if (maxDestLen < 0) {
      throw new IllegalArgumentException("maxDestLen must be >= 0");
    }
    if (!(src.hasArray() || src.isDirect())) {
      throw new IllegalArgumentException("decompressedLength needs a heap-backed or direct ByteBuffer");
    }
    final byte[] srcArr = src.hasArray() ? src.array() : null;
    final int so = srcArr != null ? srcOff + src.arrayOffset() : srcOff;
    final int result = LZ4HIPJNI.LZ4HIP_decompressed_length(srcArr, srcArr == null ? src : null, so, srcLen, maxDestLen);
    if (result < 0) {
      throw new LZ4Exception(result <= Integer.MIN_VALUE + 63 ? "liblz4hip: " + LZ4HIPJNI.lastError()
                                                               : "Error decoding offset " + (srcOff - result) + " of input buffer");
    }
    return result;
  }
}
