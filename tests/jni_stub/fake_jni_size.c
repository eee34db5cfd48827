/* tests/jni_stub/fake_jni_size.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The decoded-size natives of the JNI shim (LZ4HIPJNI.LZ4HIP_decompressed_length and LZ4HIP_batchDecompressedLengths) executed without
 * a JVM, with the fake JNIEnv of fake_env.h (a byte[] / int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer
 * is a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by tests/test_size_abi.py / tests/test_gpu_size.py.
 *
 *   fake_jni_size --no-gpu                  anywhere: NULL arrays are argument errors, every compute call fails LOUDLY without a
 *                                           device (library error code, nothing leaked or left pinned)
 *   fake_jni_size <stream> <cap> <out-dir>  on a GPU box: the decoded size of the LZ4 block <stream> for capacity <cap> through the
 *                                           byte-array path, the direct-buffer path and the batch native; writes the value to
 *                                           <out-dir>/size.txt (the test compares it with the reference's LZ4_decompress_safe);
 *                                           prints "fake_jni_size: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_size"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompressed_1length(JNIEnv*, jclass, jbyteArray, jobject, jint, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDecompressedLengths(JNIEnv*, jclass, jobject, jlongArray, jintArray, jintArray, jintArray, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define SIZE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompressed_1length
#define BATCH Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDecompressedLengths

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  const int no_gpu = arg_no_gpu(argc, argv);
  fobj* src = mk(1, 64); fobj* dsrc = mk(4, 64);
  /* NULL arrays / buffers of the batch native: LZ4HIP_E_ARG, nothing pinned */
  { fobj* so = mk(3, 8); fobj* sl = int1(20); fobj* dc = int1(100); fobj* ol = int1(-7);
    fobj* a[4] = {so, sl, dc, ol};
    for (int k = 0; k < 5; k++) {
      jint rc = BATCH(env, NULL, k == 4 ? NULL : (jobject)dsrc, k == 0 ? NULL : (jlongArray)so, k == 1 ? NULL : (jintArray)sl, k == 2 ? NULL : (jintArray)dc,
                      k == 3 ? NULL : (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(ol) == -7);
      for (int t = 0; t < 4; t++) CHECK(a[t]->pins == 0);
    }
    /* a heap ByteBuffer where a direct one is required */
    fobj* hb = mk(5, 64);
    CHECK(BATCH(env, NULL, (jobject)hb, (jlongArray)so, (jintArray)sl, (jintArray)dc, (jintArray)ol, 1) == LZ4HIP_E_ARG);
    if (no_gpu) {
      const jint rc = BATCH(env, NULL, (jobject)dsrc, (jlongArray)so, (jintArray)sl, (jintArray)dc, (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc() && get1(ol) == -7);
      for (int t = 0; t < 4; t++) CHECK(a[t]->pins == 0);
    } }
  if (no_gpu) {
    jint r = SIZE(env, NULL, (jbyteArray)src, NULL, 7, 20, 100);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0 && src->pins == 0);
    r = SIZE(env, NULL, NULL, (jobject)dsrc, 0, 20, 0);   /* (capacity 0 included: no answer without a device) */
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strlen(msg) > 0);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 4) { fprintf(stderr, "usage: fake_jni_size --no-gpu | <stream> <cap> <out-dir>\n"); return 2; }
  const size_t SO = 5;
  long n = 0;
  fobj* asrc = slurp(argv[1], 1, SO, &n); fobj* dsrc2 = copy_as(asrc, 4);
  CHECK(n > 0);
  const int cap = atoi(argv[2]);
  CHECK(cap >= 0);
  /* byte[] */
  const jint r = SIZE(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, cap);
  CHECK(no_exc() && !LZ4HIP_IS_LIB_ERROR(r) && r <= cap && g_alloc == 0 && asrc->pins == 0);
  /* direct buffer: the same value, nothing staged */
  const jint r2 = SIZE(env, NULL, NULL, (jobject)dsrc2, (jint)SO, (jint)n, cap);
  CHECK(no_exc() && r2 == r && g_alloc == 0);
  write_text(argv[3], "size.txt", "%d\n", (int)r);
  /* a source array that cannot be pinned: OutOfMemoryError, nothing leaked */
  { fobj* nopin = mk(1, (size_t)n + 16); nopin->refuse_pin = 1;
    (void)SIZE(env, NULL, (jbyteArray)nopin, NULL, (jint)SO, (jint)n, cap);
    CHECK(g_alloc == 0 && nopin->pins == 0 && g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0);
    clear_exc(); }
  /* the batch native: the stream, the stream with capacity 0, and the stream cut by one byte */
  { fobj* bsrc = mk(4, 2 * (size_t)n);
    memcpy(bsrc->data, asrc->data + SO, (size_t)n); memcpy(bsrc->data + n, asrc->data + SO, (size_t)n);
    fobj* so = mk(3, 24); fobj* sl = mk(2, 12); fobj* dc = mk(2, 12); fobj* ol = mk(2, 12);
    ((jlong*)so->data)[0] = 0; ((jlong*)so->data)[1] = n; ((jlong*)so->data)[2] = n;
    ((jint*)sl->data)[0] = ((jint*)sl->data)[1] = (jint)n; ((jint*)sl->data)[2] = (jint)n - 1;
    ((jint*)dc->data)[0] = cap; ((jint*)dc->data)[1] = 0; ((jint*)dc->data)[2] = cap;
    const jint rc = BATCH(env, NULL, (jobject)bsrc, (jlongArray)so, (jintArray)sl, (jintArray)dc, (jintArray)ol, 3);
    const jint* out = (const jint*)ol->data;
    CHECK(rc == 0 && no_exc() && out[0] == r && so->pins == 0 && sl->pins == 0 && dc->pins == 0 && ol->pins == 0 && g_alloc == 0);
    CHECK(out[1] == SIZE(env, NULL, NULL, (jobject)dsrc2, (jint)SO, (jint)n, 0));
    CHECK(out[2] == SIZE(env, NULL, NULL, (jobject)dsrc2, (jint)SO, (jint)n - 1, cap));
    write_text(argv[3], "size_batch.txt", "%d %d %d\n", (int)out[0], (int)out[1], (int)out[2]); }
  return checks_ok(NULL);
}
