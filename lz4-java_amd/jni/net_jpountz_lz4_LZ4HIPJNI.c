/*
 * JNI shim between net.jpountz.lz4.LZ4HIPJNI / net.jpountz.xxhash.XXHashHIPJNI and liblz4hip
 * (include/lz4hip.h).  Counterpart of the reference's src/jni/net_jpountz_lz4_LZ4JNI.c and
 * src/jni/net_jpountz_xxhash_XXHashJNI.c, with two deliberate differences:
 *   * a Java heap array is pinned with GetPrimitiveArrayCritical only long enough to memcpy the
 *     block into / out of a native staging buffer -- the GC lock is never held across a GPU launch
 *     (the reference holds it across the liblz4 call, LZ4JNI.c:54-82);
 *   * `in` is released when `out` cannot be pinned (the reference leaks it, LZ4JNI.c:59-73).
 * Build (needs a JDK, which the build image lacks -- see INTEGRATION.md):
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *       lz4-java_amd/jni/net_jpountz_lz4_LZ4HIPJNI.c -Llz4-java_amd -llz4hip -o liblz4hip-java.so
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "lz4hip.h"

static jclass OutOfMemoryError;
static jclass RuntimeException;

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv* env, jclass cls) {
  (void)cls;
  jclass local = (*env)->FindClass(env, "java/lang/OutOfMemoryError");
  OutOfMemoryError = (jclass)(*env)->NewGlobalRef(env, local);
  local = (*env)->FindClass(env, "java/lang/RuntimeException");
  RuntimeException = (jclass)(*env)->NewGlobalRef(env, local);
  (void)lz4hip_init(NULL, 0); /* a failure surfaces on the first codec call as a library error */
}

static void throw_OOM(JNIEnv* env) { (*env)->ThrowNew(env, OutOfMemoryError, "Out of memory"); }
/* a liblz4hip failure (no device, HIP error, bad handle) in an entry point whose Java signature has no error channel: the
 * reference's XXHashJNI cannot fail there; returning hash 0 or a stale digest silently would let a checksum comparison pass or
 * fail wrongly, so the caller gets an unchecked exception carrying lz4hip_last_error() */
static void throw_lib(JNIEnv* env) { (*env)->ThrowNew(env, RuntimeException, lz4hip_last_error()); }

/* A (array | direct buffer, offset, length) argument made addressable for the native call. */
typedef struct {
  uint8_t* p;     /* address of byte 0 of the region */
  uint8_t* heap;  /* staging copy to free, or NULL for a direct buffer */
} region_t;

static int region_in(JNIEnv* env, jbyteArray arr, jobject buf, jint off, jint len, int copy_in, region_t* r) {
  r->heap = NULL;
  if (arr == NULL) {
    uint8_t* base = (uint8_t*)(*env)->GetDirectBufferAddress(env, buf);
    if (base == NULL) return -1;
    r->p = base + off;
    return 0;
  }
  r->heap = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);
  if (r->heap == NULL) return -1;
  r->p = r->heap;
  if (copy_in && len > 0) {
    uint8_t* a = (uint8_t*)(*env)->GetPrimitiveArrayCritical(env, arr, 0);
    if (a == NULL) { free(r->heap); r->heap = NULL; return -1; }
    memcpy(r->heap, a + off, (size_t)len);
    (*env)->ReleasePrimitiveArrayCritical(env, arr, a, JNI_ABORT);
  }
  return 0;
}

/* copies `n` produced bytes back into the Java array (if staged) and frees the staging copy */
static int region_out(JNIEnv* env, jbyteArray arr, jint off, jint n, region_t* r) {
  int rc = 0;
  if (r->heap != NULL) {
    if (arr != NULL && n > 0) {
      uint8_t* a = (uint8_t*)(*env)->GetPrimitiveArrayCritical(env, arr, 0);
      if (a == NULL) rc = -1;
      else { memcpy(a + off, r->heap, (size_t)n); (*env)->ReleasePrimitiveArrayCritical(env, arr, a, 0); }
    }
    free(r->heap);
    r->heap = NULL;
  }
  return rc;
}

typedef int (*codec_fn)(const uint8_t*, int, uint8_t*, int);

static jint run_single(JNIEnv* env, int op, int level, jbyteArray srcArray, jobject srcBuffer, jint srcOff, jint srcLen,
                       jbyteArray destArray, jobject destBuffer, jint destOff, jint destLen) {
  region_t in, out;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) { throw_OOM(env); return 0; }
  if (region_in(env, destArray, destBuffer, destOff, destLen, 0, &out) != 0) {
    region_out(env, NULL, 0, 0, &in); /* release `in` too */
    throw_OOM(env);
    return 0;
  }
  int result;
  switch (op) {
    case 0: result = lz4hip_compress_fast(in.p, srcLen, out.p, destLen); break;
    case 1: result = lz4hip_decompress_safe(in.p, srcLen, out.p, destLen); break;
    case 2: result = lz4hip_decompress_fast(in.p, srcLen /* readable capacity */, out.p, destLen); break;
    case 4: result = lz4hip_compress_fast_accel(in.p, srcLen, out.p, destLen, level /* acceleration */); break;
    case 5: result = lz4hip_decompress_safe_partial(in.p, srcLen, out.p, level /* target */, destLen); break;
    default: result = lz4hip_compress_hc(in.p, srcLen, out.p, destLen, level); break;
  }
  region_out(env, NULL, 0, 0, &in);
  jint produced = 0;
  if (!LZ4HIP_IS_LIB_ERROR(result)) {
    if (op == 2) produced = result > 0 ? destLen : 0;      /* fast decompress fills destLen bytes */
    else produced = result > 0 ? result : 0;
  }
  if (region_out(env, destArray, destOff, produced, &out) != 0) { throw_OOM(env); return 0; }
  return result;
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen) {
  (void)cls;
  return run_single(env, 0, 0, srcArray, srcBuffer, srcOff, srcLen, destArray, destBuffer, destOff, maxDestLen);
}

/* LZ4_compress_fast(..., acceleration): same arguments, staging and return convention as LZ4HIP_compress_fast */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast_1accel(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen, jint acceleration) {
  (void)cls;
  return run_single(env, 4, acceleration, srcArray, srcBuffer, srcOff, srcLen, destArray, destBuffer, destOff, maxDestLen);
}

/* LZ4_compress_destSize (hc == 0) / LZ4_compress_HC_destSize at `level` (hc != 0): srcSize[0] = the block size in, the input
 * consumed out; returns the bytes written (<= targetDestSize) or a library error (srcSize[0] untouched).  Same staging as
 * LZ4HIP_compress_fast; a NULL or empty srcSize is LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) */
static jint dest_size_single(JNIEnv* env, int hc, int level, jbyteArray srcArray, jobject srcBuffer, jint srcOff, jintArray srcSize,
    jbyteArray destArray, jobject destBuffer, jint destOff, jint targetDestSize) {
  if (srcSize == NULL || (*env)->GetArrayLength(env, srcSize) < 1)
    return hc ? lz4hip_compress_hc_dest_size(NULL, NULL, NULL, 0, level) : lz4hip_compress_dest_size(NULL, NULL, NULL, 0);
  jint* sz = (*env)->GetIntArrayElements(env, srcSize, NULL);
  if (sz == NULL) { throw_OOM(env); return 0; }
  const jint srcLen = sz[0];
  region_t in, out;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) {
    (*env)->ReleaseIntArrayElements(env, srcSize, sz, JNI_ABORT);
    throw_OOM(env);
    return 0;
  }
  if (region_in(env, destArray, destBuffer, destOff, targetDestSize, 0, &out) != 0) {
    region_out(env, NULL, 0, 0, &in);
    (*env)->ReleaseIntArrayElements(env, srcSize, sz, JNI_ABORT);
    throw_OOM(env);
    return 0;
  }
  int consumed = srcLen;
  const int result = hc ? lz4hip_compress_hc_dest_size(in.p, &consumed, out.p, targetDestSize, level)
                        : lz4hip_compress_dest_size(in.p, &consumed, out.p, targetDestSize);
  region_out(env, NULL, 0, 0, &in);
  sz[0] = consumed;   /* (untouched on a library error) */
  (*env)->ReleaseIntArrayElements(env, srcSize, sz, 0);
  const jint produced = !LZ4HIP_IS_LIB_ERROR(result) && result > 0 ? result : 0;
  if (region_out(env, destArray, destOff, produced, &out) != 0) { throw_OOM(env); return 0; }
  return result;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1dest_1size(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jintArray srcSize, jbyteArray destArray, jobject destBuffer, jint destOff, jint targetDestSize) {
  (void)cls;
  return dest_size_single(env, 0, 0, srcArray, srcBuffer, srcOff, srcSize, destArray, destBuffer, destOff, targetDestSize);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compressHC_1dest_1size(JNIEnv* env, jclass cls, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jintArray srcSize, jbyteArray destArray, jobject destBuffer, jint destOff, jint targetDestSize, jint level) {
  (void)cls;
  return dest_size_single(env, 1, level, srcArray, srcBuffer, srcOff, srcSize, destArray, destBuffer, destOff, targetDestSize);
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compressHC(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen, jint level) {
  (void)cls;
  return run_single(env, 3, level, srcArray, srcBuffer, srcOff, srcLen, destArray, destBuffer, destOff, maxDestLen);
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen) {
  (void)cls;
  return run_single(env, 1, 0, srcArray, srcBuffer, srcOff, srcLen, destArray, destBuffer, destOff, maxDestLen);
}

/* LZ4_decompress_safe_partial: the first min(targetLen, maxDestLen) decoded bytes; same arguments, staging and return convention as
 * LZ4HIP_decompress_safe, and only the decoded bytes go back to a heap array */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe_1partial(JNIEnv* env, jclass cls, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint targetLen, jint maxDestLen) {
  (void)cls;
  return run_single(env, 5, targetLen, srcArray, srcBuffer, srcOff, srcLen, destArray, destBuffer, destOff, maxDestLen);
}

/* The decoded-size query (lz4hip_decompressed_size): what LZ4HIP_decompress_safe would return for the same source and maxDestLen,
 * without a destination -- only the source is made addressable (a heap array is staged, a direct buffer is used in place).  Returns
 * liblz4's value or a library failure as above */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompressed_1length(JNIEnv* env, jclass cls, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jint srcLen, jint maxDestLen) {
  (void)cls;
  region_t in;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) { throw_OOM(env); return 0; }
  const int result = lz4hip_decompressed_size(in.p, srcLen, maxDestLen);
  region_out(env, NULL, 0, 0, &in);
  return result;
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1fast(JNIEnv* env, jclass cls, jbyteArray srcArray, jobject srcBuffer,
    jint srcOff, jint srcCap, jbyteArray destArray, jobject destBuffer, jint destOff, jint destLen) {
  (void)cls;
  return run_single(env, 2, 0, srcArray, srcBuffer, srcOff, srcCap, destArray, destBuffer, destOff, destLen);
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compressBound(JNIEnv* env, jclass cls, jint len) {
  (void)env; (void)cls;
  return lz4hip_compress_bound(len);
}

JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv* env, jclass cls) {
  (void)cls;
  return (*env)->NewStringUTF(env, lz4hip_last_error());
}

/* ---- the batch natives: many blocks, direct buffers: nothing is copied on the host side, liblz4hip stages H2D/D2H itself ---- */
/* A long[] / int[] descriptor array of a batch native. */
enum { INTS = 0, LONGS = 1 };
typedef struct {
  jarray arr;
  int is_long;  /* LONGS (offsets) or INTS */
  jint mode;    /* how it is released: JNI_ABORT for an input, 0 for an output (copied back) */
  void* p;      /* its elements while pinned */
} batch_array_t;
/* The arguments of a batch native made addressable: the two direct buffers and up to twelve descriptor arrays. */
typedef struct {
  const uint8_t* src;
  uint8_t* dst;
  int n_arrays;
  batch_array_t a[12];
} batch_args_t;

static void batch_release(JNIEnv* env, batch_args_t* b) {
  for (int i = 0; i < b->n_arrays; i++) {
    batch_array_t* a = &b->a[i];
    if (a->p == NULL) continue;
    if (a->is_long) (*env)->ReleaseLongArrayElements(env, (jlongArray)a->arr, (jlong*)a->p, a->mode);
    else (*env)->ReleaseIntArrayElements(env, (jintArray)a->arr, (jint*)a->p, a->mode);
    a->p = NULL;
  }
}

/* 0: everything is addressable (batch_release when done).  LZ4HIP_E_ARG: a NULL array or buffer, or a buffer that is not direct --
 * decided before the env is asked for anything (Get*ArrayElements of a null reference is undefined in a JVM).  LZ4HIP_E_NOMEM: an
 * array cannot be pinned.  Nothing stays pinned after an error. */
static jint batch_pin(JNIEnv* env, jobject src, jobject dest, batch_args_t* b) {
  if (src == NULL || dest == NULL) return LZ4HIP_E_ARG;
  for (int i = 0; i < b->n_arrays; i++)
    if (b->a[i].arr == NULL) return LZ4HIP_E_ARG;
  b->src = (const uint8_t*)(*env)->GetDirectBufferAddress(env, src);
  b->dst = (uint8_t*)(*env)->GetDirectBufferAddress(env, dest);
  if (b->src == NULL || b->dst == NULL) return LZ4HIP_E_ARG;
  for (int i = 0; i < b->n_arrays; i++) {
    batch_array_t* a = &b->a[i];
    a->p = a->is_long ? (void*)(*env)->GetLongArrayElements(env, (jlongArray)a->arr, NULL) : (void*)(*env)->GetIntArrayElements(env, (jintArray)a->arr, NULL);
    if (a->p == NULL) { batch_release(env, b); return LZ4HIP_E_NOMEM; }
  }
  return 0;
}

JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batch(JNIEnv* env, jclass cls, jint op, jint level, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  batch_args_t b = {NULL, NULL, 5, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  const uint64_t *so = b.a[0].p, *dof = b.a[2].p;
  const int32_t *sl = b.a[1].p, *dc = b.a[3].p;
  int32_t* ol = b.a[4].p;
  switch (op) {
    case 0: rc = lz4hip_compress_fast_batch(b.src, so, sl, b.dst, dof, dc, ol, (uint32_t)n); break;
    case 1: rc = lz4hip_decompress_safe_batch(b.src, so, sl, b.dst, dof, dc, ol, (uint32_t)n); break;
    case 2: rc = lz4hip_decompress_fast_batch(b.src, so, sl, b.dst, dof, dc, ol, (uint32_t)n); break;
    case 4: rc = lz4hip_compress_fast_accel_batch(b.src, so, sl, b.dst, dof, dc, ol, (uint32_t)n, level); break;
    default: rc = lz4hip_compress_hc_batch(b.src, so, sl, b.dst, dof, dc, ol, (uint32_t)n, level); break;
  }
  batch_release(env, &b);
  return rc;
}

/* LZ4_compress_destSize over many blocks, direct buffers (lz4hip_compress_dest_size_batch): outLen[i] = bytes written in block i's
 * slot dest[destOff[i] .. + targetSize[i]), srcConsumed[i] = input consumed.  Returns 0 or a negative lz4hip_status; a NULL array or
 * buffer is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDestSize(JNIEnv* env, jclass cls, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray targetSize, jintArray outLen, jintArray srcConsumed, jint n) {
  (void)cls;
  batch_args_t b = {NULL, NULL, 6, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {targetSize, INTS, JNI_ABORT}, {outLen, INTS, 0},
                                    {srcConsumed, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_dest_size_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, b.a[5].p, (uint32_t)n);
  batch_release(env, &b);
  return rc;
}

/* LZ4_compress_HC_destSize at HC level `level` over many blocks (lz4hip_compress_hc_dest_size_batch): the arguments, results and
 * NULL rule of LZ4HIP_batchDestSize */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCDestSize(JNIEnv* env, jclass cls, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray targetSize, jintArray outLen, jintArray srcConsumed, jint n, jint level) {
  (void)cls;
  batch_args_t b = {NULL, NULL, 6, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {targetSize, INTS, JNI_ABORT}, {outLen, INTS, 0},
                                    {srcConsumed, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_hc_dest_size_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, b.a[5].p, (uint32_t)n, level);
  batch_release(env, &b);
  return rc;
}

/* LZ4_decompress_safe_partial over many blocks, direct buffers (lz4hip_decompress_safe_partial_batch): block i decodes into at most
 * dest[destOff[i] .. + min(targetLen[i], destCap[i])), outLen[i] = liblz4's return value.  Returns 0 or a negative lz4hip_status; a
 * NULL array or buffer is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafePartial(JNIEnv* env, jclass cls, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray targetLen, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  batch_args_t b = {NULL, NULL, 6, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {targetLen, INTS, JNI_ABORT}, {destCap, INTS, JNI_ABORT},
                                    {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_decompress_safe_partial_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, b.a[5].p, (uint32_t)n);
  batch_release(env, &b);
  return rc;
}

/* ---- LZ4_decompress_safe_usingDict against a dictionary handle (lz4hip_dict_create): LZ4HIPDictionary.java keeps the handle as a long ---- */

/* the dictionary bytes of a heap array or a direct buffer -> a handle, or 0 (lz4hip_last_error() says why: a NULL or negative argument
 * is LZ4HIP_E_ARG); the bytes are copied, nothing stays pinned */
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictCreate(JNIEnv* env, jclass cls, jbyteArray dictArray, jobject dictBuffer, jint off, jint len) {
  (void)cls;
  lz4hip_dict* h = NULL;
  if ((dictArray == NULL && dictBuffer == NULL) || off < 0 || len < 0) { (void)lz4hip_dict_create(NULL, len, &h); return 0; }   /* (sets the message) */
  region_t in;
  if (region_in(env, dictArray, dictBuffer, off, len, 1, &in) != 0) { throw_OOM(env); return 0; }
  const int rc = lz4hip_dict_create(in.p, len, &h);
  region_out(env, NULL, 0, 0, &in);
  return rc == 0 ? (jlong)(intptr_t)h : 0;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictSize(JNIEnv* env, jclass cls, jlong dict) {
  (void)env; (void)cls;
  return lz4hip_dict_size((const lz4hip_dict*)(intptr_t)dict);
}
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictFree(JNIEnv* env, jclass cls, jlong dict) {
  (void)env; (void)cls;
  lz4hip_dict_free((lz4hip_dict*)(intptr_t)dict);
}

/* LZ4_decompress_safe_usingDict: the arguments, staging and return convention of LZ4HIP_decompress_safe behind the handle (0: a
 * library error, LZ4HIP_E_ARG) */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe_1dict(JNIEnv* env, jclass cls, jlong dict, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen) {
  (void)cls;
  region_t in, out;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) { throw_OOM(env); return 0; }
  if (region_in(env, destArray, destBuffer, destOff, maxDestLen, 0, &out) != 0) {
    region_out(env, NULL, 0, 0, &in); /* release `in` too */
    throw_OOM(env);
    return 0;
  }
  const int result = lz4hip_decompress_safe_dict(in.p, srcLen, out.p, maxDestLen, (const lz4hip_dict*)(intptr_t)dict);
  region_out(env, NULL, 0, 0, &in);
  const jint produced = (!LZ4HIP_IS_LIB_ERROR(result) && result > 0) ? result : 0;
  if (region_out(env, destArray, destOff, produced, &out) != 0) { throw_OOM(env); return 0; }
  return result;
}

/* LZ4_decompress_safe_usingDict over many blocks against one handle, direct buffers (lz4hip_decompress_safe_dict_batch): outLen[i] =
 * liblz4's return value.  Returns 0 or a negative lz4hip_status; a NULL array or buffer or a 0 handle is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeDict(JNIEnv* env, jclass cls, jlong dict, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  if (dict == 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 5, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_decompress_safe_dict_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, (uint32_t)n, (const lz4hip_dict*)(intptr_t)dict);
  batch_release(env, &b);
  return rc;
}

/* LZ4_decompress_safe_continue over chains of linked blocks, direct buffers (lz4hip_decompress_safe_chain_batch): chain c is the blocks
 * chainFirst[c] .. chainFirst[c + 1] - 1, decoded back to back into dest[chainDestOff[c], + chainDestCap[c]) behind chainPrefixLen[c]
 * bytes of history (chainPrefixLen may be NULL: none); stored may be NULL, else stored[i] != 0 marks a raw block; outLen[i] = liblz4's
 * return value (LZ4HIP_CHAIN_STOPPED behind a chain's first negative one), chainOutLen[c] = the bytes the chain decoded.  Returns 0 or a
 * negative lz4hip_status; a NULL required array or buffer is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeChain(JNIEnv* env, jclass cls, jobject src, jlongArray srcOff, jintArray srcLen,
    jintArray stored, jintArray destCap, jintArray chainFirst, jobject dest, jlongArray chainDestOff, jlongArray chainDestCap, jintArray chainPrefixLen,
    jintArray outLen, jlongArray chainOutLen, jint nBlocks, jint nChains) {
  (void)cls;
  if (nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 8, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT},
                                    {chainDestOff, LONGS, JNI_ABORT}, {chainDestCap, LONGS, JNI_ABORT}, {outLen, INTS, 0}, {chainOutLen, LONGS, 0}}};
  if (stored != NULL) { b.a[b.n_arrays].arr = stored; b.a[b.n_arrays].is_long = INTS; b.a[b.n_arrays].mode = JNI_ABORT; b.a[b.n_arrays].p = NULL; b.n_arrays++; }
  const int i_stored = stored != NULL ? b.n_arrays - 1 : -1;
  if (chainPrefixLen != NULL) { b.a[b.n_arrays].arr = chainPrefixLen; b.a[b.n_arrays].is_long = INTS; b.a[b.n_arrays].mode = JNI_ABORT; b.a[b.n_arrays].p = NULL; b.n_arrays++; }
  const int i_prefix = chainPrefixLen != NULL ? b.n_arrays - 1 : -1;
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  uint8_t* raw = NULL;   /* the C ABI takes one byte per block */
  if (i_stored >= 0 && nBlocks > 0) {
    raw = (uint8_t*)malloc((size_t)nBlocks);
    if (raw == NULL) { batch_release(env, &b); return LZ4HIP_E_NOMEM; }
    for (jint i = 0; i < nBlocks; i++) raw[i] = ((const jint*)b.a[i_stored].p)[i] != 0;
  }
  rc = lz4hip_decompress_safe_chain_batch(b.src, b.a[0].p, b.a[1].p, raw, b.a[2].p, (const uint32_t*)b.a[3].p, b.dst, b.a[4].p, b.a[5].p,
                                          i_prefix >= 0 ? (const int32_t*)b.a[i_prefix].p : NULL, b.a[6].p, b.a[7].p, (uint32_t)nBlocks, (uint32_t)nChains);
  free(raw);
  batch_release(env, &b);
  return rc;
}

/* LZ4_decompress_safe_continue on streams whose blocks land anywhere, direct buffers (lz4hip_decompress_safe_stream_batch): stream c is the
 * blocks chainFirst[c] .. chainFirst[c + 1] - 1 of this call, block i is decoded to dest[destOff[i], + destCap[i]) inside the window
 * dest[chainWinOff[c], + chainWinLen[c]); state holds four longs per stream -- prefixEnd, prefixLen, extEnd, extLen, offsets into dest --,
 * read and written back; outLen[i] = liblz4's return value (LZ4HIP_CHAIN_STOPPED behind a stream's first negative one of the call).
 * Returns 0 or a negative lz4hip_status; a NULL array or buffer is LZ4HIP_E_ARG (LZ4HIPBatch.java checks the arrays' lengths) */
typedef int (*dstream_entry_t)(lz4hip_dstream_state*, const uint8_t*, const uint64_t*, const int32_t*, const uint32_t*, uint8_t*, const uint64_t*,
                               const int32_t*, const uint64_t*, const uint64_t*, int32_t*, uint32_t, uint32_t);
/* the two stream-decode natives: the arrays pinned, `entry` called, everything released */
static jint batch_safe_stream(JNIEnv* env, dstream_entry_t entry, jlongArray state, jobject src, jlongArray srcOff, jintArray srcLen, jintArray chainFirst,
                              jobject dest, jlongArray destOff, jintArray destCap, jlongArray chainWinOff, jlongArray chainWinLen, jintArray outLen,
                              jint nBlocks, jint nChains) {
  if (nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 9, {{state, LONGS, 0}, {srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT},
                                    {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {chainWinOff, LONGS, JNI_ABORT},
                                    {chainWinLen, LONGS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = entry((lz4hip_dstream_state*)b.a[0].p, b.src, b.a[1].p, b.a[2].p, (const uint32_t*)b.a[3].p, b.dst, b.a[4].p, b.a[5].p, b.a[6].p, b.a[7].p, b.a[8].p,
             (uint32_t)nBlocks, (uint32_t)nChains);
  batch_release(env, &b);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStream(JNIEnv* env, jclass cls, jlongArray state, jobject src, jlongArray srcOff,
    jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jlongArray chainWinOff, jlongArray chainWinLen,
    jintArray outLen, jint nBlocks, jint nChains) {
  (void)cls;
  return batch_safe_stream(env, lz4hip_decompress_safe_stream_batch, state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff, chainWinLen,
                           outLen, nBlocks, nChains);
}

/* The same call for streams whose slots overlap the history they can reach -- liblz4's minimal ring, rings in step with the writer's
 * (lz4hip_decompress_safe_stream_inorder_batch): the arguments, the state and the errors of LZ4HIP_batchSafeStream, which it may
 * alternate with on one stream from call to call */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStreamInOrder(JNIEnv* env, jclass cls, jlongArray state, jobject src, jlongArray srcOff,
    jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jlongArray chainWinOff, jlongArray chainWinLen,
    jintArray outLen, jint nBlocks, jint nChains) {
  (void)cls;
  return batch_safe_stream(env, lz4hip_decompress_safe_stream_inorder_batch, state, src, srcOff, srcLen, chainFirst, dest, destOff, destCap, chainWinOff,
                           chainWinLen, outLen, nBlocks, nChains);
}

/* LZ4_decoderRingBufferSize (lz4hip_decoder_ring_buffer_size): needs no device */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decoderRingBufferSize(JNIEnv* env, jclass cls, jint maxBlock) {
  (void)env; (void)cls;
  return lz4hip_decoder_ring_buffer_size(maxBlock);
}

/* LZ4_compress_HC_continue on streams whose sources land anywhere, direct buffers (lz4hip_compress_hc_stream_batch): stream c is the blocks
 * chainFirst[c] .. chainFirst[c + 1] - 1 of this call, block i is src[srcOff[i], + srcLen[i]) and owns dest[destOff[i], + destCap[i]); state
 * holds five longs per stream -- prefixEnd, prefixLen, extEnd, extLen, index, offsets into src --, read and written back; outLen[i] =
 * liblz4's return value.  Returns 0 or a negative lz4hip_status; a NULL array or buffer is LZ4HIP_E_ARG and nothing stays pinned
 * (LZ4HIPBatch.java checks the arrays' lengths) */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCStream(JNIEnv* env, jclass cls, jlongArray state, jobject src, jlongArray srcOff,
    jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jint nBlocks, jint nChains, jint level) {
  (void)cls;
  if (nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 7, {{state, LONGS, 0}, {srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT},
                                    {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_hc_stream_batch((lz4hip_hcstream_state*)b.a[0].p, b.src, b.a[1].p, b.a[2].p, (const uint32_t*)b.a[3].p, b.dst, b.a[4].p, b.a[5].p,
                                       b.a[6].p, (uint32_t)nBlocks, (uint32_t)nChains, level);
  batch_release(env, &b);
  return rc;
}

/* LZ4_compress_fast_continue over chains of linked blocks, DIRECT buffers: chainPrefixLen may be null.  acceleration: the call's last
 * argument; 1 is lz4hip_compress_fast_chain_batch, anything else lz4hip_compress_fast_chain_accel_batch (which clamps it) */
static jint fast_chain(JNIEnv* env, jobject src, jlongArray chainSrcOff, jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest,
    jlongArray destOff, jintArray destCap, jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains, jint acceleration) {
  if (nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 7, {{chainSrcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT},
                                    {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}, {chainConsumed, LONGS, 0}}};
  if (chainPrefixLen != NULL) { b.a[b.n_arrays].arr = chainPrefixLen; b.a[b.n_arrays].is_long = INTS; b.a[b.n_arrays].mode = JNI_ABORT; b.a[b.n_arrays].p = NULL; b.n_arrays++; }
  const int i_prefix = chainPrefixLen != NULL ? b.n_arrays - 1 : -1;
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  const int32_t* prefix = i_prefix >= 0 ? (const int32_t*)b.a[i_prefix].p : NULL;
  if (acceleration == 1)
    rc = lz4hip_compress_fast_chain_batch(b.src, b.a[0].p, prefix, b.a[1].p, (const uint32_t*)b.a[2].p, b.dst, b.a[3].p, b.a[4].p, b.a[5].p, b.a[6].p,
                                          (uint32_t)nBlocks, (uint32_t)nChains);
  else
    rc = lz4hip_compress_fast_chain_accel_batch(b.src, b.a[0].p, prefix, b.a[1].p, (const uint32_t*)b.a[2].p, b.dst, b.a[3].p, b.a[4].p, b.a[5].p, b.a[6].p,
                                                (uint32_t)nBlocks, (uint32_t)nChains, acceleration);
  batch_release(env, &b);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastChain(JNIEnv* env, jclass cls, jobject src, jlongArray chainSrcOff,
    jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen,
    jlongArray chainConsumed, jint nBlocks, jint nChains) {
  (void)cls;
  return fast_chain(env, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, nBlocks, nChains, 1);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastChainAccel(JNIEnv* env, jclass cls, jobject src, jlongArray chainSrcOff,
    jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen,
    jlongArray chainConsumed, jint nBlocks, jint nChains, jint acceleration) {
  (void)cls;
  return fast_chain(env, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, nBlocks, nChains, acceleration);
}

/* Resident compress streams (lz4hip_cstreams_*): a set of nStreams streams whose tables and index positions stay on the device between
 * calls.  cstreamsCreate returns the handle, or 0 (lastError() says why); cstreamsCount is the number of streams; cstreamsFree takes
 * 0 too. */
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate(JNIEnv* env, jclass cls, jint nStreams) {
  (void)env; (void)cls;
  lz4hip_cstreams* h = NULL;
  if (lz4hip_cstreams_create(nStreams < 0 ? 0u : (uint32_t)nStreams, &h) != 0) return 0;   /* (sets the message) */
  return (jlong)(intptr_t)h;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCount(JNIEnv* env, jclass cls, jlong set) {
  (void)env; (void)cls;
  return lz4hip_cstreams_count((const lz4hip_cstreams*)(intptr_t)set);
}
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree(JNIEnv* env, jclass cls, jlong set) {
  (void)env; (void)cls;
  lz4hip_cstreams_free((lz4hip_cstreams*)(intptr_t)set);
}
/* makes the listed streams fresh (streamId == NULL: all of them).  Returns 0 or a negative lz4hip_status; a 0 handle is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsReset(JNIEnv* env, jclass cls, jlong set, jintArray streamId, jint n) {
  (void)cls;
  if (set == 0 || n < 0) return LZ4HIP_E_ARG;
  if (streamId == NULL) return lz4hip_cstreams_reset((lz4hip_cstreams*)(intptr_t)set, NULL, 0);
  jint* ids = (*env)->GetIntArrayElements(env, streamId, NULL);
  if (ids == NULL) return LZ4HIP_E_NOMEM;
  const jint rc = lz4hip_cstreams_reset((lz4hip_cstreams*)(intptr_t)set, (const uint32_t*)ids, (uint32_t)n);
  (*env)->ReleaseIntArrayElements(env, streamId, ids, JNI_ABORT);
  return rc;
}
/* consumed[i] = the bytes stream first + i has consumed since its reset, stopped[i] != 0: it is stopped; n entries each.  Returns 0 or a
 * negative lz4hip_status; a 0 handle or a NULL array is LZ4HIP_E_ARG, nothing stays pinned */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsConsumed(JNIEnv* env, jclass cls, jlong set, jint first, jint n, jlongArray consumed,
    jintArray stopped) {
  (void)cls;
  if (set == 0 || first < 0 || n < 0 || consumed == NULL || stopped == NULL) return LZ4HIP_E_ARG;
  uint8_t* st = (uint8_t*)malloc(n > 0 ? (size_t)n : 1u);   /* the C ABI writes one byte per stream */
  if (st == NULL) return LZ4HIP_E_NOMEM;
  jlong* c = (*env)->GetLongArrayElements(env, consumed, NULL);
  jint* s = c != NULL ? (*env)->GetIntArrayElements(env, stopped, NULL) : NULL;
  jint rc = LZ4HIP_E_NOMEM;
  if (c != NULL && s != NULL) {
    rc = lz4hip_cstreams_consumed((lz4hip_cstreams*)(intptr_t)set, (uint32_t)first, (uint32_t)n, (uint64_t*)c, st);
    if (rc == 0) for (jint i = 0; i < n; i++) s[i] = st[i] != 0;
  }
  if (s != NULL) (*env)->ReleaseIntArrayElements(env, stopped, s, rc == 0 ? 0 : JNI_ABORT);
  if (c != NULL) (*env)->ReleaseLongArrayElements(env, consumed, c, rc == 0 ? 0 : JNI_ABORT);
  free(st);
  return rc;
}
/* LZ4_compress_fast_continue on resident streams, DIRECT buffers: LZ4HIP_batchFastChain's arguments behind the set and the stream of
 * every chain (strictly ascending); chainPrefixLen may be null.  A 0 handle is LZ4HIP_E_ARG.  acceleration: as for fast_chain, for
 * every block of THIS call (lz4hip_compress_fast_stream_accel_batch) */
static jint fast_stream(JNIEnv* env, jlong set, jintArray streamId, jobject src, jlongArray chainSrcOff, jintArray chainPrefixLen, jintArray srcLen,
    jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains,
    jint acceleration) {
  if (set == 0 || nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 8, {{chainSrcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT},
                                    {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}, {chainConsumed, LONGS, 0}, {streamId, INTS, JNI_ABORT}}};
  if (chainPrefixLen != NULL) { b.a[b.n_arrays].arr = chainPrefixLen; b.a[b.n_arrays].is_long = INTS; b.a[b.n_arrays].mode = JNI_ABORT; b.a[b.n_arrays].p = NULL; b.n_arrays++; }
  const int i_prefix = chainPrefixLen != NULL ? b.n_arrays - 1 : -1;
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  const int32_t* prefix = i_prefix >= 0 ? (const int32_t*)b.a[i_prefix].p : NULL;
  if (acceleration == 1)
    rc = lz4hip_compress_fast_stream_batch((lz4hip_cstreams*)(intptr_t)set, (const uint32_t*)b.a[7].p, b.src, b.a[0].p, prefix, b.a[1].p,
                                           (const uint32_t*)b.a[2].p, b.dst, b.a[3].p, b.a[4].p, b.a[5].p, b.a[6].p, (uint32_t)nBlocks, (uint32_t)nChains);
  else
    rc = lz4hip_compress_fast_stream_accel_batch((lz4hip_cstreams*)(intptr_t)set, (const uint32_t*)b.a[7].p, b.src, b.a[0].p, prefix, b.a[1].p,
                                                 (const uint32_t*)b.a[2].p, b.dst, b.a[3].p, b.a[4].p, b.a[5].p, b.a[6].p, (uint32_t)nBlocks,
                                                 (uint32_t)nChains, acceleration);
  batch_release(env, &b);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStream(JNIEnv* env, jclass cls, jlong set, jintArray streamId, jobject src,
    jlongArray chainSrcOff, jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap,
    jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains) {
  (void)cls;
  return fast_stream(env, set, streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, nBlocks, nChains, 1);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAccel(JNIEnv* env, jclass cls, jlong set, jintArray streamId, jobject src,
    jlongArray chainSrcOff, jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap,
    jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains, jint acceleration) {
  (void)cls;
  return fast_stream(env, set, streamId, src, chainSrcOff, chainPrefixLen, srcLen, chainFirst, dest, destOff, destCap, outLen, chainConsumed, nBlocks, nChains,
                     acceleration);
}
/* The same streams when their sources land anywhere, DIRECT buffers (lz4hip_compress_fast_stream_ext_batch): every block has its own
 * srcOff[i] inside the window src[chainWinOff[c], + chainWinLen[c]) of its stream; the stream's history ends at chainHistEnd[c] with
 * chainHistLen[c] bytes of it present.  Every array is required.  A 0 handle is LZ4HIP_E_ARG.  acceleration: as for fast_stream
 * (lz4hip_compress_fast_stream_ext_accel_batch) */
static jint fast_stream_at(JNIEnv* env, jlong set, jintArray streamId, jobject src, jlongArray srcOff, jintArray srcLen, jintArray chainFirst,
    jlongArray chainHistEnd, jintArray chainHistLen, jlongArray chainWinOff, jlongArray chainWinLen, jobject dest, jlongArray destOff, jintArray destCap,
    jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains, jint acceleration) {
  if (set == 0 || nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 12, {{streamId, INTS, JNI_ABORT}, {srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT},
                                     {chainHistEnd, LONGS, JNI_ABORT}, {chainHistLen, INTS, JNI_ABORT}, {chainWinOff, LONGS, JNI_ABORT},
                                     {chainWinLen, LONGS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0},
                                     {chainConsumed, LONGS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  if (acceleration == 1)
    rc = lz4hip_compress_fast_stream_ext_batch((lz4hip_cstreams*)(intptr_t)set, (const uint32_t*)b.a[0].p, b.src, b.a[1].p, b.a[2].p, (const uint32_t*)b.a[3].p,
                                               b.a[4].p, b.a[5].p, b.a[6].p, b.a[7].p, b.dst, b.a[8].p, b.a[9].p, b.a[10].p, b.a[11].p, (uint32_t)nBlocks,
                                               (uint32_t)nChains);
  else
    rc = lz4hip_compress_fast_stream_ext_accel_batch((lz4hip_cstreams*)(intptr_t)set, (const uint32_t*)b.a[0].p, b.src, b.a[1].p, b.a[2].p,
                                                     (const uint32_t*)b.a[3].p, b.a[4].p, b.a[5].p, b.a[6].p, b.a[7].p, b.dst, b.a[8].p, b.a[9].p, b.a[10].p,
                                                     b.a[11].p, (uint32_t)nBlocks, (uint32_t)nChains, acceleration);
  batch_release(env, &b);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAt(JNIEnv* env, jclass cls, jlong set, jintArray streamId, jobject src,
    jlongArray srcOff, jintArray srcLen, jintArray chainFirst, jlongArray chainHistEnd, jintArray chainHistLen, jlongArray chainWinOff,
    jlongArray chainWinLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains) {
  (void)cls;
  return fast_stream_at(env, set, streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dest, destOff, destCap, outLen,
                        chainConsumed, nBlocks, nChains, 1);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAtAccel(JNIEnv* env, jclass cls, jlong set, jintArray streamId, jobject src,
    jlongArray srcOff, jintArray srcLen, jintArray chainFirst, jlongArray chainHistEnd, jintArray chainHistLen, jlongArray chainWinOff,
    jlongArray chainWinLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jlongArray chainConsumed, jint nBlocks, jint nChains,
    jint acceleration) {
  (void)cls;
  return fast_stream_at(env, set, streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dest, destOff, destCap, outLen,
                        chainConsumed, nBlocks, nChains, acceleration);
}

/* LZ4_compress_HC_continue over chains of linked blocks at an HC level, DIRECT buffers: chainPrefixLen may be null */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCChain(JNIEnv* env, jclass cls, jobject src, jlongArray chainSrcOff,
    jintArray chainPrefixLen, jintArray srcLen, jintArray chainFirst, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen,
    jint nBlocks, jint nChains, jint level) {
  (void)cls;
  if (nBlocks < 0 || nChains < 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 6, {{chainSrcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {chainFirst, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT},
                                    {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  if (chainPrefixLen != NULL) { b.a[b.n_arrays].arr = chainPrefixLen; b.a[b.n_arrays].is_long = INTS; b.a[b.n_arrays].mode = JNI_ABORT; b.a[b.n_arrays].p = NULL; b.n_arrays++; }
  const int i_prefix = chainPrefixLen != NULL ? b.n_arrays - 1 : -1;
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_hc_chain_batch(b.src, b.a[0].p, i_prefix >= 0 ? (const int32_t*)b.a[i_prefix].p : NULL, b.a[1].p, (const uint32_t*)b.a[2].p, b.dst,
                                      b.a[3].p, b.a[4].p, b.a[5].p, (uint32_t)nBlocks, (uint32_t)nChains, (int)level);
  batch_release(env, &b);
  return rc;
}

/* LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream, against a dictionary handle: the arguments, staging and return
 * convention of LZ4HIP_compress_fast behind the handle (0 handle: a library error, LZ4HIP_E_ARG) */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast_1dict(JNIEnv* env, jclass cls, jlong dict, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen) {
  (void)cls;
  region_t in, out;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) { throw_OOM(env); return 0; }
  if (region_in(env, destArray, destBuffer, destOff, maxDestLen, 0, &out) != 0) {
    region_out(env, NULL, 0, 0, &in); /* release `in` too */
    throw_OOM(env);
    return 0;
  }
  const int result = lz4hip_compress_fast_dict(in.p, srcLen, out.p, maxDestLen, (const lz4hip_dict*)(intptr_t)dict);
  region_out(env, NULL, 0, 0, &in);
  const jint produced = (!LZ4HIP_IS_LIB_ERROR(result) && result > 0) ? result : 0;
  if (region_out(env, destArray, destOff, produced, &out) != 0) { throw_OOM(env); return 0; }
  return result;
}

/* the same over many blocks against one handle, direct buffers (lz4hip_compress_fast_dict_batch): outLen[i] = the compressed size, 0
 * where destCap[i] is too small.  Returns 0 or a negative lz4hip_status; a NULL array or buffer or a 0 handle is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchCompressDict(JNIEnv* env, jclass cls, jlong dict, jobject src, jlongArray srcOff,
    jintArray srcLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  if (dict == 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 5, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_fast_dict_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, (uint32_t)n, (const lz4hip_dict*)(intptr_t)dict);
  batch_release(env, &b);
  return rc;
}

/* LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream at HC level `level` against a dictionary handle (lz4hip_compress_hc_dict):
 * the conventions of LZ4HIP_compress_fast_dict */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1hc_1dict(JNIEnv* env, jclass cls, jlong dict, jint level, jbyteArray srcArray,
    jobject srcBuffer, jint srcOff, jint srcLen, jbyteArray destArray, jobject destBuffer, jint destOff, jint maxDestLen) {
  (void)cls;
  region_t in, out;
  if (region_in(env, srcArray, srcBuffer, srcOff, srcLen, 1, &in) != 0) { throw_OOM(env); return 0; }
  if (region_in(env, destArray, destBuffer, destOff, maxDestLen, 0, &out) != 0) {
    region_out(env, NULL, 0, 0, &in); /* release `in` too */
    throw_OOM(env);
    return 0;
  }
  const int result = lz4hip_compress_hc_dict(in.p, srcLen, out.p, maxDestLen, level, (const lz4hip_dict*)(intptr_t)dict);
  region_out(env, NULL, 0, 0, &in);
  const jint produced = (!LZ4HIP_IS_LIB_ERROR(result) && result > 0) ? result : 0;
  if (region_out(env, destArray, destOff, produced, &out) != 0) { throw_OOM(env); return 0; }
  return result;
}

/* the same over many blocks against one handle, direct buffers (lz4hip_compress_hc_dict_batch): the conventions of
 * LZ4HIP_batchCompressDict */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchCompressHCDict(JNIEnv* env, jclass cls, jlong dict, jint level, jobject src,
    jlongArray srcOff, jintArray srcLen, jobject dest, jlongArray destOff, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  if (dict == 0) return LZ4HIP_E_ARG;
  batch_args_t b = {NULL, NULL, 5, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destOff, LONGS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, dest, &b);
  if (rc != 0) return rc;
  rc = lz4hip_compress_hc_dict_batch(b.src, b.a[0].p, b.a[1].p, b.dst, b.a[2].p, b.a[3].p, b.a[4].p, (uint32_t)n, level, (const lz4hip_dict*)(intptr_t)dict);
  batch_release(env, &b);
  return rc;
}

/* The decoded-size query over many blocks, a direct source buffer (lz4hip_decompressed_size_batch): outLen[i] = what
 * LZ4_decompress_safe would return for block i with capacity destCap[i].  There is no destination buffer (batch_pin gets the source in
 * its place: its address is not used).  Returns 0 or a negative lz4hip_status; a NULL array or buffer is LZ4HIP_E_ARG */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDecompressedLengths(JNIEnv* env, jclass cls, jobject src, jlongArray srcOff,
    jintArray srcLen, jintArray destCap, jintArray outLen, jint n) {
  (void)cls;
  batch_args_t b = {NULL, NULL, 4, {{srcOff, LONGS, JNI_ABORT}, {srcLen, INTS, JNI_ABORT}, {destCap, INTS, JNI_ABORT}, {outLen, INTS, 0}}};
  jint rc = batch_pin(env, src, src, &b);
  if (rc != 0) return rc;
  rc = lz4hip_decompressed_size_batch(b.src, b.a[0].p, b.a[1].p, b.a[2].p, b.a[3].p, (uint32_t)n);
  batch_release(env, &b);
  return rc;
}

/* the data blocks of an LZ4 Frame (kind 0) / of lz4-java's LZ4Block container (kind 1) for src[srcOff, srcOff + len) cut into
 * blockSize pieces, assembled on the device (include/lz4hip.h lz4hip_container_blocks): what LZ4FrameOutputStream.writeBlock /
 * LZ4BlockOutputStream.flushBufferedData emit block by block, in one call.  Direct buffers; returns the bytes written at
 * dest[destOff ..), or the (negative) lz4hip_status */
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocks(JNIEnv* env, jclass cls, jint kind, jint flags, jint level, jobject src,
    jlong srcOff, jlong len, jint blockSize, jobject dest, jlong destOff, jlong destCap) {
  (void)cls;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, src);
  uint8_t* d = (uint8_t*)(*env)->GetDirectBufferAddress(env, dest);
  if (s == NULL || d == NULL || srcOff < 0 || len < 0 || destOff < 0 || destCap < 0 || blockSize <= 0) return (jlong)LZ4HIP_E_ARG;
  uint64_t out = 0;
  const int rc = lz4hip_container_blocks(kind, flags, level, s + srcOff, (uint64_t)len, (uint32_t)blockSize, d + destOff, (uint64_t)destCap, &out);
  return rc == 0 ? (jlong)out : (jlong)rc;   /* (status codes are negative) */
}

/* the READ side (include/lz4hip.h lz4hip_container_decode): the data blocks of an LZ4 Frame body (kind 0: from the first block's size
 * word on; flags & 1 = block checksums; maxBlock = the frame's block maximum) / of an LZ4Block stream (kind 1) in
 * src[srcOff, srcOff + len) are walked, verified and decoded on the device -- LZ4FrameInputStream.readBlock (LZ4FrameInputStream.java:
 * 258-322) / LZ4BlockInputStream.refill (LZ4BlockInputStream.java:191-264) for a run of up to nMax blocks in one call.  The decoded
 * blocks land back to back at dest[destOff ..); sizes[k] = decoded size of block k; info[0..4] = { blocks delivered, bytes of src
 * consumed, stop reason, decoded bytes, liblz4's code of a failed decode }.  Direct buffers; returns 0 or the (negative)
 * lz4hip_status.  LZ4HIPBatch.containerDecodeBound tells how much of dest a call can need. */
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecode(JNIEnv* env, jclass cls, jint kind, jint flags, jobject src, jlong srcOff,
    jlong len, jint maxBlock, jint nMax, jobject dest, jlong destOff, jlong destCap, jintArray sizes, jlongArray info) {
  (void)cls;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, src);
  uint8_t* d = (uint8_t*)(*env)->GetDirectBufferAddress(env, dest);
  if (s == NULL || d == NULL || srcOff < 0 || len < 0 || destOff < 0 || destCap < 0 || maxBlock <= 0 || nMax <= 0) return LZ4HIP_E_ARG;
  if (sizes == NULL || info == NULL) return LZ4HIP_E_ARG;   /* (GetArrayLength of a null reference crashes a real JVM: round-5 advisor) */
  if ((*env)->GetArrayLength(env, sizes) < nMax || (*env)->GetArrayLength(env, info) < 5) return LZ4HIP_E_ARG;
  jint* sz = (*env)->GetIntArrayElements(env, sizes, NULL);
  jlong* inf = (*env)->GetLongArrayElements(env, info, NULL);
  jint rc = LZ4HIP_E_NOMEM;
  if (sz && inf) rc = lz4hip_container_decode(kind, flags, s + srcOff, (uint64_t)len, (uint32_t)maxBlock, (uint32_t)nMax, d + destOff, (uint64_t)destCap,
                                              (int32_t*)sz, (uint64_t*)inf);
  if (sz) (*env)->ReleaseIntArrayElements(env, sizes, sz, 0);
  if (inf) (*env)->ReleaseLongArrayElements(env, info, inf, 0);
  return rc;
}
/* what a containerDecode call can need of dest (a host-side walk of the headers, no device work): returns the bytes, or the (negative)
 * lz4hip_status; blocks[0] = whole blocks of the first nMax that src holds */
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeBound(JNIEnv* env, jclass cls, jint kind, jint flags, jobject src, jlong srcOff,
    jlong len, jint maxBlock, jint nMax, jintArray blocks) {
  (void)cls;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, src);
  if (s == NULL || srcOff < 0 || len < 0 || blocks == NULL || (*env)->GetArrayLength(env, blocks) < 1) return (jlong)LZ4HIP_E_ARG;
  uint32_t nb = 0;
  uint64_t need = 0;
  const int rc = lz4hip_container_decode_bound(kind, flags, s + srcOff, (uint64_t)len, (uint32_t)maxBlock, (uint32_t)nMax, &nb, &need);
  if (rc != 0) return (jlong)rc;
  jint* b = (*env)->GetIntArrayElements(env, blocks, NULL);
  if (b == NULL) return (jlong)LZ4HIP_E_NOMEM;
  b[0] = (jint)nb;
  (*env)->ReleaseIntArrayElements(env, blocks, b, 0);
  return (jlong)need;
}

/* MANY containers of one kind in one call (include/lz4hip.h lz4hip_container_decode_many{,_bound}): item c is
 * bodies[bodyOff[c], + bodyLen[c]) with its own maxBlock[c] and flags[c] (bit 0: block checksums).  bound != 0: the host-side walk alone
 * -- outA = itemBlocks[nItems], outB = itemDstBytes[nItems], nothing else is looked at.  Otherwise the read: the delivered blocks land
 * back to back at dest[destOff ..), outA = itemFirst[nItems + 1], outB = itemDstOff[nItems + 1], sizes[sum of itemBlocks],
 * info[5 x nItems].  Direct buffers; NULL arrays and arrays that are too short are argument errors; returns 0 or the (negative)
 * lz4hip_status. */
static jint container_many(JNIEnv* env, int bound, jint kind, jobject bodies, jlongArray bodyOff, jlongArray bodyLen, jintArray maxBlock, jintArray flags,
                           jint nItems, jint nMax, jobject dest, jlong destOff, jlong destCap, jintArray outA, jlongArray outB, jintArray sizes, jlongArray info) {
  if (bodies == NULL || (!bound && dest == NULL)) return LZ4HIP_E_ARG;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, bodies);
  uint8_t* d = bound ? NULL : (uint8_t*)(*env)->GetDirectBufferAddress(env, dest);
  if (s == NULL || nItems < 0 || nMax <= 0 || (!bound && (d == NULL || destOff < 0 || destCap < 0))) return LZ4HIP_E_ARG;
  if (bodyOff == NULL || bodyLen == NULL || maxBlock == NULL || flags == NULL || outA == NULL || outB == NULL || (!bound && (sizes == NULL || info == NULL)))
    return LZ4HIP_E_ARG;   /* (GetArrayLength of a null reference crashes a real JVM) */
  const jint nOut = bound ? nItems : nItems + 1;
  if ((*env)->GetArrayLength(env, bodyOff) < nItems || (*env)->GetArrayLength(env, bodyLen) < nItems || (*env)->GetArrayLength(env, maxBlock) < nItems ||
      (*env)->GetArrayLength(env, flags) < nItems || (*env)->GetArrayLength(env, outA) < nOut || (*env)->GetArrayLength(env, outB) < nOut ||
      (!bound && (*env)->GetArrayLength(env, info) / 5 < nItems))
    return LZ4HIP_E_ARG;
  uint8_t* fl = (uint8_t*)malloc((size_t)nItems + 1u);
  jlong* bo = (*env)->GetLongArrayElements(env, bodyOff, NULL);
  jlong* bl = (*env)->GetLongArrayElements(env, bodyLen, NULL);
  jint* mb = (*env)->GetIntArrayElements(env, maxBlock, NULL);
  jint* fi = (*env)->GetIntArrayElements(env, flags, NULL);
  jint* oa = (*env)->GetIntArrayElements(env, outA, NULL);
  jlong* ob = (*env)->GetLongArrayElements(env, outB, NULL);
  jint* sz = bound ? NULL : (*env)->GetIntArrayElements(env, sizes, NULL);
  jlong* inf = bound ? NULL : (*env)->GetLongArrayElements(env, info, NULL);
  jint rc = LZ4HIP_E_NOMEM;
  if (fl && bo && bl && mb && fi && oa && ob && (bound || (sz && inf))) {
    rc = 0;
    for (jint c = 0; c < nItems; c++) {
      if (bo[c] < 0 || bl[c] < 0 || fi[c] < 0 || fi[c] > 255) rc = LZ4HIP_E_ARG;
      fl[c] = (uint8_t)fi[c];
    }
    if (rc == 0 && bound)
      rc = lz4hip_container_decode_many_bound(kind, s, (const uint64_t*)bo, (const uint64_t*)bl, (const uint32_t*)mb, fl, (uint32_t)nItems, (uint32_t)nMax,
                                              (uint32_t*)oa, (uint64_t*)ob);
    else if (rc == 0)
      rc = lz4hip_container_decode_many(kind, s, (const uint64_t*)bo, (const uint64_t*)bl, (const uint32_t*)mb, fl, (uint32_t)nItems, (uint32_t)nMax, d + destOff,
                                        (uint64_t)destCap, (uint64_t*)ob, (uint32_t*)oa, (int32_t*)sz, (uint32_t)(*env)->GetArrayLength(env, sizes), (uint64_t*)inf);
  }
  if (bo) (*env)->ReleaseLongArrayElements(env, bodyOff, bo, 0);
  if (bl) (*env)->ReleaseLongArrayElements(env, bodyLen, bl, 0);
  if (mb) (*env)->ReleaseIntArrayElements(env, maxBlock, mb, 0);
  if (fi) (*env)->ReleaseIntArrayElements(env, flags, fi, 0);
  if (oa) (*env)->ReleaseIntArrayElements(env, outA, oa, 0);
  if (ob) (*env)->ReleaseLongArrayElements(env, outB, ob, 0);
  if (sz) (*env)->ReleaseIntArrayElements(env, sizes, sz, 0);
  if (inf) (*env)->ReleaseLongArrayElements(env, info, inf, 0);
  free(fl);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeMany(JNIEnv* env, jclass cls, jint kind, jobject bodies, jlongArray bodyOff,
    jlongArray bodyLen, jintArray maxBlock, jintArray flags, jint nItems, jint nMax, jobject dest, jlong destOff, jlong destCap, jlongArray itemDstOff,
    jintArray itemFirst, jintArray sizes, jlongArray info) {
  (void)cls;
  return container_many(env, 0, kind, bodies, bodyOff, bodyLen, maxBlock, flags, nItems, nMax, dest, destOff, destCap, itemFirst, itemDstOff, sizes, info);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeManyBound(JNIEnv* env, jclass cls, jint kind, jobject bodies, jlongArray bodyOff,
    jlongArray bodyLen, jintArray maxBlock, jintArray flags, jint nItems, jint nMax, jintArray itemBlocks, jlongArray itemDstBytes) {
  (void)cls;
  return container_many(env, 1, kind, bodies, bodyOff, bodyLen, maxBlock, flags, nItems, nMax, NULL, 0, 0, itemBlocks, itemDstBytes, NULL, NULL);
}

/* MANY containers WRITTEN in one call (include/lz4hip.h lz4hip_container_blocks_many{,_bound}): item c is src[srcOff[c], + srcLen[c]) cut
 * into blockSize[c] pieces, with flags[c] (bit 0: block checksums, kind 0; bit 1: its content hash is wanted) and gapHead[c] / gapTail[c]
 * zero bytes around its blocks.  bound != 0: the arithmetic alone -- outA = itemBlocks[nItems], outB = itemDstBytes[nItems], no buffer is
 * looked at.  Otherwise the write: the items land back to back at dest[destOff ..), outB = itemDstOff[nItems + 1], outA =
 * contentHash[nItems].  Direct buffers; NULL arrays (gapHead and gapTail too: Java passes arrays of zeros) and arrays that are too short
 * are argument errors; returns 0 or the (negative) lz4hip_status. */
static jint container_write_many(JNIEnv* env, int bound, jint kind, jint level, jobject src, jlongArray srcOff, jlongArray srcLen, jintArray blockSize,
                                 jintArray flags, jintArray gapHead, jintArray gapTail, jint nItems, jobject dest, jlong destOff, jlong destCap, jintArray outA,
                                 jlongArray outB) {
  if (!bound && (src == NULL || dest == NULL)) return LZ4HIP_E_ARG;
  const uint8_t* s = bound ? NULL : (const uint8_t*)(*env)->GetDirectBufferAddress(env, src);
  uint8_t* d = bound ? NULL : (uint8_t*)(*env)->GetDirectBufferAddress(env, dest);
  if (nItems < 0 || (!bound && (s == NULL || d == NULL || destOff < 0 || destCap < 0))) return LZ4HIP_E_ARG;
  if ((!bound && srcOff == NULL) || srcLen == NULL || blockSize == NULL || flags == NULL || gapHead == NULL || gapTail == NULL || outA == NULL || outB == NULL)
    return LZ4HIP_E_ARG;   /* (GetArrayLength of a null reference crashes a real JVM) */
  const jint nOut = bound ? nItems : nItems + 1;
  if ((!bound && (*env)->GetArrayLength(env, srcOff) < nItems) || (*env)->GetArrayLength(env, srcLen) < nItems ||
      (*env)->GetArrayLength(env, blockSize) < nItems || (*env)->GetArrayLength(env, flags) < nItems || (*env)->GetArrayLength(env, gapHead) < nItems ||
      (*env)->GetArrayLength(env, gapTail) < nItems || (*env)->GetArrayLength(env, outA) < nItems || (*env)->GetArrayLength(env, outB) < nOut)
    return LZ4HIP_E_ARG;
  uint8_t* fl = (uint8_t*)malloc((size_t)nItems + 1u);
  jlong* so = bound ? NULL : (*env)->GetLongArrayElements(env, srcOff, NULL);
  jlong* sl = (*env)->GetLongArrayElements(env, srcLen, NULL);
  jint* bs = (*env)->GetIntArrayElements(env, blockSize, NULL);
  jint* fi = (*env)->GetIntArrayElements(env, flags, NULL);
  jint* gh = (*env)->GetIntArrayElements(env, gapHead, NULL);
  jint* gt = (*env)->GetIntArrayElements(env, gapTail, NULL);
  jint* oa = (*env)->GetIntArrayElements(env, outA, NULL);
  jlong* ob = (*env)->GetLongArrayElements(env, outB, NULL);
  jint rc = LZ4HIP_E_NOMEM;
  if (fl && (bound || so) && sl && bs && fi && gh && gt && oa && ob) {
    rc = 0;
    for (jint c = 0; c < nItems; c++) {
      if ((!bound && so[c] < 0) || sl[c] < 0 || fi[c] < 0 || fi[c] > 255 || gh[c] < 0 || gt[c] < 0) rc = LZ4HIP_E_ARG;
      fl[c] = (uint8_t)fi[c];
    }
    if (rc == 0 && bound)
      rc = lz4hip_container_blocks_many_bound(kind, (const uint64_t*)sl, (const uint32_t*)bs, fl, (const uint32_t*)gh, (const uint32_t*)gt, (uint32_t)nItems,
                                              (uint32_t*)oa, (uint64_t*)ob);
    else if (rc == 0)
      rc = lz4hip_container_blocks_many(kind, level, s, (const uint64_t*)so, (const uint64_t*)sl, (const uint32_t*)bs, fl, (const uint32_t*)gh,
                                        (const uint32_t*)gt, (uint32_t)nItems, d + destOff, (uint64_t)destCap, (uint64_t*)ob, (uint32_t*)oa);
  }
  if (so) (*env)->ReleaseLongArrayElements(env, srcOff, so, 0);
  if (sl) (*env)->ReleaseLongArrayElements(env, srcLen, sl, 0);
  if (bs) (*env)->ReleaseIntArrayElements(env, blockSize, bs, 0);
  if (fi) (*env)->ReleaseIntArrayElements(env, flags, fi, 0);
  if (gh) (*env)->ReleaseIntArrayElements(env, gapHead, gh, 0);
  if (gt) (*env)->ReleaseIntArrayElements(env, gapTail, gt, 0);
  if (oa) (*env)->ReleaseIntArrayElements(env, outA, oa, 0);
  if (ob) (*env)->ReleaseLongArrayElements(env, outB, ob, 0);
  free(fl);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksMany(JNIEnv* env, jclass cls, jint kind, jint level, jobject src, jlongArray srcOff,
    jlongArray srcLen, jintArray blockSize, jintArray flags, jintArray gapHead, jintArray gapTail, jint nItems, jobject dest, jlong destOff, jlong destCap,
    jlongArray itemDstOff, jintArray contentHash) {
  (void)cls;
  return container_write_many(env, 0, kind, level, src, srcOff, srcLen, blockSize, flags, gapHead, gapTail, nItems, dest, destOff, destCap, contentHash, itemDstOff);
}
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksManyBound(JNIEnv* env, jclass cls, jint kind, jlongArray srcLen, jintArray blockSize,
    jintArray flags, jintArray gapHead, jintArray gapTail, jint nItems, jintArray itemBlocks, jlongArray itemDstBytes) {
  (void)cls;
  return container_write_many(env, 1, kind, 0, NULL, NULL, srcLen, blockSize, flags, gapHead, gapTail, nItems, NULL, 0, 0, itemBlocks, itemDstBytes);
}

/* ---- xxhash (XXHashJNI.c:42-82, :152-192 counterparts) ---- */
static int hash_region(JNIEnv* env, jbyteArray arr, jobject buf, jint off, jint len, int is64, uint64_t seed, uint64_t* out) {
  region_t in;
  if (region_in(env, arr, buf, off, len, 1, &in) != 0) { throw_OOM(env); return -1; }
  int rc;
  if (is64) rc = lz4hip_xxh64(in.p, len, seed, out);
  else { uint32_t h = 0; rc = lz4hip_xxh32(in.p, len, (uint32_t)seed, &h); *out = h; }
  region_out(env, NULL, 0, 0, &in);
  if (rc != 0) throw_lib(env);
  return rc;
}

JNIEXPORT jint JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32(JNIEnv* env, jclass cls, jbyteArray buf, jint off, jint len, jint seed) {
  (void)cls; uint64_t h = 0; hash_region(env, buf, NULL, off, len, 0, (uint32_t)seed, &h); return (jint)(uint32_t)h;
}
JNIEXPORT jint JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32BB(JNIEnv* env, jclass cls, jobject buf, jint off, jint len, jint seed) {
  (void)cls; uint64_t h = 0; hash_region(env, NULL, buf, off, len, 0, (uint32_t)seed, &h); return (jint)(uint32_t)h;
}
JNIEXPORT jlong JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64(JNIEnv* env, jclass cls, jbyteArray buf, jint off, jint len, jlong seed) {
  (void)cls; uint64_t h = 0; hash_region(env, buf, NULL, off, len, 1, (uint64_t)seed, &h); return (jlong)h;
}
JNIEXPORT jlong JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64BB(JNIEnv* env, jclass cls, jobject buf, jint off, jint len, jlong seed) {
  (void)cls; uint64_t h = 0; hash_region(env, NULL, buf, off, len, 1, (uint64_t)seed, &h); return (jlong)h;
}
JNIEXPORT jint JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32Batch(JNIEnv* env, jclass cls, jobject input, jlongArray off, jintArray len, jint seed,
    jintArray out32, jint n) {
  (void)cls;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, input);
  if (s == NULL) return LZ4HIP_E_ARG;
  jlong* o = (*env)->GetLongArrayElements(env, off, NULL);
  jint* l = (*env)->GetIntArrayElements(env, len, NULL);
  jint* h = (*env)->GetIntArrayElements(env, out32, NULL);
  jint rc = (o && l && h) ? lz4hip_xxh32_batch(s, (const uint64_t*)o, (const int32_t*)l, (uint32_t)seed, (uint32_t*)h, (uint32_t)n) : LZ4HIP_E_NOMEM;
  if (o) (*env)->ReleaseLongArrayElements(env, off, o, JNI_ABORT);
  if (l) (*env)->ReleaseIntArrayElements(env, len, l, JNI_ABORT);
  if (h) (*env)->ReleaseIntArrayElements(env, out32, h, 0);
  return rc;
}
JNIEXPORT jint JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64Batch(JNIEnv* env, jclass cls, jobject input, jlongArray off, jintArray len, jlong seed,
    jlongArray out64, jint n) {
  (void)cls;
  const uint8_t* s = (const uint8_t*)(*env)->GetDirectBufferAddress(env, input);
  if (s == NULL) return LZ4HIP_E_ARG;
  jlong* o = (*env)->GetLongArrayElements(env, off, NULL);
  jint* l = (*env)->GetIntArrayElements(env, len, NULL);
  jlong* h = (*env)->GetLongArrayElements(env, out64, NULL);
  jint rc = (o && l && h) ? lz4hip_xxh64_batch(s, (const uint64_t*)o, (const int32_t*)l, (uint64_t)seed, (uint64_t*)h, (uint32_t)n) : LZ4HIP_E_NOMEM;
  if (o) (*env)->ReleaseLongArrayElements(env, off, o, JNI_ABORT);
  if (l) (*env)->ReleaseIntArrayElements(env, len, l, JNI_ABORT);
  if (h) (*env)->ReleaseLongArrayElements(env, out64, h, 0);
  return rc;
}

/* ---- streaming xxhash (XXHashJNI.c:89-145, :199-255 counterparts): the jlong is a lz4hip_xxh_stream* ---- */
static jlong stream_init(JNIEnv* env, int is64, uint64_t seed) {
  lz4hip_xxh_stream* st = NULL;
  const int rc = is64 ? lz4hip_xxh64_stream_create(seed, &st) : lz4hip_xxh32_stream_create((uint32_t)seed, &st);
  if (rc != 0) { throw_OOM(env); return 0; }   /* same surface as the reference: XXHashJNI.c:94-98 */
  return (jlong)(intptr_t)st;
}
static void stream_update(JNIEnv* env, jlong state, jbyteArray src, jint off, jint len) {
  region_t in;   /* staged copy: the GC lock is not held across the launch */
  if (region_in(env, src, NULL, off, len, 1, &in) != 0) { throw_OOM(env); return; }
  const int rc = lz4hip_xxh_stream_update((lz4hip_xxh_stream*)(intptr_t)state, in.p, len);
  region_out(env, NULL, 0, 0, &in);
  if (rc != 0) throw_lib(env);
}
JNIEXPORT jlong JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32_1init(JNIEnv* env, jclass cls, jint seed) { (void)cls; return stream_init(env, 0, (uint32_t)seed); }
JNIEXPORT jlong JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64_1init(JNIEnv* env, jclass cls, jlong seed) { (void)cls; return stream_init(env, 1, (uint64_t)seed); }
JNIEXPORT void JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32_1reset(JNIEnv* env, jclass cls, jlong state, jint seed) {
  (void)cls; if (lz4hip_xxh_stream_reset((lz4hip_xxh_stream*)(intptr_t)state, (uint32_t)seed) != 0) throw_lib(env);
}
JNIEXPORT void JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64_1reset(JNIEnv* env, jclass cls, jlong state, jlong seed) {
  (void)cls; if (lz4hip_xxh_stream_reset((lz4hip_xxh_stream*)(intptr_t)state, (uint64_t)seed) != 0) throw_lib(env);
}
JNIEXPORT void JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32_1update(JNIEnv* env, jclass cls, jlong state, jbyteArray src, jint off, jint len) {
  (void)cls; stream_update(env, state, src, off, len);
}
JNIEXPORT void JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64_1update(JNIEnv* env, jclass cls, jlong state, jbyteArray src, jint off, jint len) {
  (void)cls; stream_update(env, state, src, off, len);
}
JNIEXPORT jint JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH32_1digest(JNIEnv* env, jclass cls, jlong state) {
  (void)cls; uint32_t h = 0; if (lz4hip_xxh32_stream_digest((lz4hip_xxh_stream*)(intptr_t)state, &h) != 0) throw_lib(env); return (jint)h;
}
JNIEXPORT jlong JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH64_1digest(JNIEnv* env, jclass cls, jlong state) {
  (void)cls; uint64_t h = 0; if (lz4hip_xxh64_stream_digest((lz4hip_xxh_stream*)(intptr_t)state, &h) != 0) throw_lib(env); return (jlong)h;
}
JNIEXPORT void JNICALL Java_net_jpountz_xxhash_XXHashHIPJNI_XXH_1free(JNIEnv* env, jclass cls, jlong state) {
  (void)env; (void)cls; lz4hip_xxh_stream_free((lz4hip_xxh_stream*)(intptr_t)state);
}
