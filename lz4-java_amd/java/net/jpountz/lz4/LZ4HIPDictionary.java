package net.jpountz.lz4;

import java.io.Closeable;
import java.nio.ByteBuffer;

import net.jpountz.util.ByteBufferUtils;
import net.jpountz.util.SafeUtils;

/**
 * A shared dictionary of the "HIP" family for liblz4's {@code LZ4_decompress_safe_usingDict}: records that were each compressed alone
 * against one dictionary ({@code LZ4_loadDict} + {@code LZ4_compress_fast_continue}) are decoded against it, one by one
 * ({@link LZ4HIPSafeDecompressor#decompressWithDict}) or many per launch ({@link LZ4HIPBatch#decompressSafeDict}).  Not in the
 * reference.  The native handle keeps the dictionary's true length and its last 64 KB -- all a decoder can reach -- resident on
 * every initialised device; the bytes given to the constructor are copied.  The dictionary is immutable: any number of threads may
 * decode against it.  {@link #close()} frees it; no call that uses it may be in flight then.  Methods that touch the handle are
 * synchronized because finalize() may free it concurrently, as in the streaming hashes.
 */
public final class LZ4HIPDictionary implements Closeable {

  private long handle;

  public LZ4HIPDictionary(byte[] dict, int off, int len) {
    SafeUtils.checkRange(dict, off, len);
    handle = LZ4HIPJNI.LZ4HIP_dictCreate(dict, null, off, len);
    if (handle == 0) {
      throw new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
    }
  }

  public LZ4HIPDictionary(byte[] dict) {
    this(dict, 0, dict.length);
  }

  /** The dictionary in {@code dict[off, off+len)} of a heap-backed or direct buffer (position untouched). */
  public LZ4HIPDictionary(ByteBuffer dict, int off, int len) {
    ByteBufferUtils.checkRange(dict, off, len);
    if (!(dict.hasArray() || dict.isDirect())) {
      throw new IllegalArgumentException("LZ4HIPDictionary needs a heap-backed or direct ByteBuffer");
    }
    final byte[] arr = dict.hasArray() ? dict.array() : null;
    handle = LZ4HIPJNI.LZ4HIP_dictCreate(arr, arr == null ? dict : null, arr != null ? off + dict.arrayOffset() : off, len);
    if (handle == 0) {
      throw new LZ4Exception("liblz4hip: " + LZ4HIPJNI.lastError());
    }
  }

  synchronized long handle() {
    if (handle == 0) {
      throw new AssertionError("Already closed");
    }
    return handle;
  }

  /** The dictionary's true length (not the at most 64 KB the handle keeps). */
  public synchronized int size() {
    return LZ4HIPJNI.LZ4HIP_dictSize(handle());
  }

  @Override
  public synchronized void close() {
    if (handle != 0) {
      LZ4HIPJNI.LZ4HIP_dictFree(handle);
      handle = 0;
    }
  }

  @Override
  protected void finalize() throws Throwable {
    close();
    super.finalize();
  }

  @Override
  public String toString() {
    return getClass().getSimpleName();
  }

}
