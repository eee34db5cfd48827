/* tests/jni_stub/fake_jni_partial.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The partial-decode natives of the JNI shim (LZ4HIPJNI.LZ4HIP_decompress_safe_partial and LZ4HIP_batchSafePartial) executed without a
 * JVM, with the fake JNIEnv of fake_env.h (a byte[] / int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer
 * is a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by tests/test_partial_abi.py / tests/test_gpu_partial.py.
 *
 *   fake_jni_partial --no-gpu                          anywhere: NULL arrays are argument errors, every compute call fails LOUDLY
 *                                                      without a device (library error code, nothing leaked or left pinned)
 *   fake_jni_partial <stream> <target> <cap> <out-dir> on a GPU box: decodes the LZ4 block <stream> into min(<target>, <cap>) bytes
 *                                                      through every argument shape and the batch native, writes the bytes and the
 *                                                      return value to <out-dir>/partial.bin / partial.txt (the test compares them
 *                                                      with the reference's LZ4_decompress_safe_partial); prints
 *                                                      "fake_jni_partial: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_partial"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe_1partial(JNIEnv*, jclass, jbyteArray, jobject, jint, jint, jbyteArray, jobject, jint, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafePartial(JNIEnv*, jclass, jobject, jlongArray, jintArray, jobject, jlongArray, jintArray, jintArray, jintArray, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define PART Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decompress_1safe_1partial
#define BATCH Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafePartial

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  fobj* src = mk(1, 64); fobj* dst = mk(1, 128); fobj* dsrc = mk(4, 64); fobj* ddst = mk(4, 128);
  /* NULL arrays / buffers of the batch native: LZ4HIP_E_ARG, nothing pinned */
  { fobj* so = mk(3, 8); fobj* sl = int1(20); fobj* dof = mk(3, 8); fobj* tl = int1(50); fobj* dc = int1(100); fobj* ol = int1(-7);
    fobj* a[6] = {so, sl, dof, tl, dc, ol};
    for (int k = 0; k < 8; k++) {
      jint rc = BATCH(env, NULL, k == 6 ? NULL : (jobject)dsrc, k == 0 ? NULL : (jlongArray)so, k == 1 ? NULL : (jintArray)sl, k == 7 ? NULL : (jobject)ddst,
                      k == 2 ? NULL : (jlongArray)dof, k == 3 ? NULL : (jintArray)tl, k == 4 ? NULL : (jintArray)dc, k == 5 ? NULL : (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(ol) == -7);
      for (int t = 0; t < 6; t++) CHECK(a[t]->pins == 0);
    }
    /* heap ByteBuffers where direct ones are required */
    fobj* hb = mk(5, 64);
    CHECK(BATCH(env, NULL, (jobject)hb, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)tl, (jintArray)dc, (jintArray)ol, 1) == LZ4HIP_E_ARG);
    if (arg_no_gpu(argc, argv)) {
      const jint rc = BATCH(env, NULL, (jobject)dsrc, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)tl, (jintArray)dc, (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc());
      for (int t = 0; t < 6; t++) CHECK(a[t]->pins == 0);
    } }
  if (arg_no_gpu(argc, argv)) {
    memset(dst->data, 0xEE, dst->bytes);
    jint r = PART(env, NULL, (jbyteArray)src, NULL, 7, 20, (jbyteArray)dst, NULL, 3, 50, 100);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0 && src->pins == 0 && dst->pins == 0 && guarded(dst, 0, 0, 0xEE));
    r = PART(env, NULL, NULL, (jobject)dsrc, 0, 20, NULL, (jobject)ddst, 0, 0, 30);   /* (target 0 included: no answer without a device) */
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strlen(msg) > 0);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 5) { fprintf(stderr, "usage: fake_jni_partial --no-gpu | <stream> <target> <cap> <out-dir>\n"); return 2; }
  const size_t SO = 5, DO = 7;
  long n = 0;
  fobj* asrc = slurp(argv[1], 1, SO, &n); fobj* dsrc2 = copy_as(asrc, 4);
  CHECK(n > 0);
  const int t = atoi(argv[2]), cap = atoi(argv[3]);
  CHECK(t >= 0 && cap >= 0);
  const int room = t < cap ? t : cap;
  fobj* adst = mk(1, (size_t)cap + 32); fobj* ddst2 = mk(4, (size_t)cap + 32);
  /* byte[] -> byte[] */
  memset(adst->data, 0xEE, adst->bytes);
  const jint r = PART(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)adst, NULL, (jint)DO, t, cap);
  CHECK(no_exc() && !LZ4HIP_IS_LIB_ERROR(r) && r <= room && g_alloc == 0 && asrc->pins == 0 && adst->pins == 0);
  const size_t got = r > 0 ? (size_t)r : 0;
  CHECK(guarded(adst, DO, got, 0xEE));
  write_bytes(argv[4], "partial.bin", adst->data + DO, got);
  write_text(argv[4], "partial.txt", "%d\n", (int)r);
  /* direct -> direct (NULL arrays), byte[] -> direct, direct -> byte[]: the same result, nothing written past DO + room */
  for (int shape = 0; shape < 3; shape++) {
    fobj* adst2 = mk(1, (size_t)cap + 32);
    memset(ddst2->data, 0xEE, ddst2->bytes); memset(adst2->data, 0xEE, adst2->bytes);
    const int dir_in = shape != 1, dir_out = shape != 2;
    const jint r2 = PART(env, NULL, dir_in ? NULL : (jbyteArray)asrc, dir_in ? (jobject)dsrc2 : NULL, (jint)SO, (jint)n,
                         dir_out ? NULL : (jbyteArray)adst2, dir_out ? (jobject)ddst2 : NULL, (jint)DO, t, cap);
    const fobj* d = dir_out ? ddst2 : adst2;
    CHECK(no_exc() && r2 == r && memcmp(d->data + DO, adst->data + DO, got) == 0 && g_alloc == 0);
    if (dir_out) for (size_t i = DO + (size_t)room; i < d->bytes; i++) CHECK(d->data[i] == 0xEE);
    else CHECK(guarded(d, DO, got, 0xEE));
    free(adst2->data); free(adst2);
  }
  /* `out` cannot be pinned: `in` is released, OutOfMemoryError */
  { fobj* nopin = mk(1, (size_t)cap + 1); nopin->refuse_pin = 1;
    (void)PART(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)nopin, NULL, 0, t, cap);
    CHECK(g_alloc == 0 && asrc->pins == 0 && nopin->pins == 0);
    if (r > 0) CHECK(g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0);
    clear_exc(); }
  /* the batch native: two copies of the stream, the second with target 0 -> the single call's result, then 0; slots untouched past
   * min(target, cap) */
  { fobj* bsrc = mk(4, 2 * (size_t)n); fobj* bdst = mk(4, 2 * (size_t)cap + 64);
    memset(bdst->data, 0xEE, bdst->bytes);
    memcpy(bsrc->data, asrc->data + SO, (size_t)n); memcpy(bsrc->data + n, asrc->data + SO, (size_t)n);
    fobj* so = mk(3, 16); fobj* sl = mk(2, 8); fobj* dof = mk(3, 16); fobj* tl = mk(2, 8); fobj* dc = mk(2, 8); fobj* ol = mk(2, 8);
    ((jlong*)so->data)[0] = 0; ((jlong*)so->data)[1] = n; ((jint*)sl->data)[0] = ((jint*)sl->data)[1] = (jint)n;
    ((jlong*)dof->data)[0] = 0; ((jlong*)dof->data)[1] = cap + 32; ((jint*)tl->data)[0] = t; ((jint*)tl->data)[1] = 0;
    ((jint*)dc->data)[0] = ((jint*)dc->data)[1] = cap;
    const jint rc = BATCH(env, NULL, (jobject)bsrc, (jlongArray)so, (jintArray)sl, (jobject)bdst, (jlongArray)dof, (jintArray)tl, (jintArray)dc, (jintArray)ol, 2);
    const jint* out = (const jint*)ol->data;
    CHECK(rc == 0 && out[0] == r && out[1] == 0 && so->pins == 0 && ol->pins == 0 && tl->pins == 0 && dc->pins == 0);
    CHECK(memcmp(bdst->data, adst->data + DO, got) == 0);
    for (size_t i = (size_t)room; i < (size_t)cap + 32; i++) CHECK(bdst->data[i] == 0xEE);
    for (size_t i = (size_t)cap + 32; i < bdst->bytes; i++) CHECK(bdst->data[i] == 0xEE); }
  return checks_ok(NULL);
}
