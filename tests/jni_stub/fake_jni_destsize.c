/* tests/jni_stub/fake_jni_destsize.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The destSize natives of the JNI shim (LZ4HIPJNI.LZ4HIP_compress_dest_size and LZ4HIP_batchDestSize) executed without a JVM, with
 * the fake JNIEnv of fake_env.h (a byte[] / int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is a
 * pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by tests/test_destsize_abi.py / tests/test_gpu_destsize.py.
 *
 *   fake_jni_destsize --no-gpu                   anywhere: NULL arrays are argument errors, every compute call fails LOUDLY without
 *                                                a device (library error code, srcSize untouched, nothing leaked or left pinned)
 *   fake_jni_destsize <input> <target> <out-dir> on a GPU box: compresses <input> into <target> bytes through every argument shape and
 *                                                the batch native, writes the stream and the consumed size to <out-dir>/dest.bin /
 *                                                dest.txt (the test compares them with the reference's LZ4_compress_destSize);
 *                                                prints "fake_jni_destsize: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_destsize"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1dest_1size(JNIEnv*, jclass, jbyteArray, jobject, jint, jintArray, jbyteArray, jobject, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDestSize(JNIEnv*, jclass, jobject, jlongArray, jintArray, jobject, jlongArray, jintArray, jintArray, jintArray, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define DEST Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1dest_1size
#define BATCH Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchDestSize

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  fobj* src = mk(1, 64); fobj* dst = mk(1, 128); fobj* dsrc = mk(4, 64); fobj* ddst = mk(4, 128);
  /* NULL / empty srcSize: an argument error, whatever the device */
  { jint r = DEST(env, NULL, (jbyteArray)src, NULL, 0, NULL, (jbyteArray)dst, NULL, 0, 100);
    CHECK(r == LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) && no_exc() && g_alloc == 0 && src->pins == 0 && dst->pins == 0);
    fobj* empty = mk(2, 0);
    r = DEST(env, NULL, (jbyteArray)src, NULL, 0, (jintArray)empty, (jbyteArray)dst, NULL, 0, 100);
    CHECK(r == LZ4HIP_LIB_ERROR(LZ4HIP_E_ARG) && no_exc() && g_alloc == 0 && empty->pins == 0); }
  /* NULL arrays / buffers of the batch native: LZ4HIP_E_ARG, nothing pinned */
  { fobj* so = mk(3, 8); fobj* sl = int1(20); fobj* dof = mk(3, 8); fobj* ts = int1(100); fobj* ol = int1(-7); fobj* sc = int1(-7);
    fobj* a[6] = {so, sl, dof, ts, ol, sc};
    for (int k = 0; k < 8; k++) {
      jint rc = BATCH(env, NULL, k == 6 ? NULL : (jobject)dsrc, k == 0 ? NULL : (jlongArray)so, k == 1 ? NULL : (jintArray)sl, k == 7 ? NULL : (jobject)ddst,
                      k == 2 ? NULL : (jlongArray)dof, k == 3 ? NULL : (jintArray)ts, k == 4 ? NULL : (jintArray)ol, k == 5 ? NULL : (jintArray)sc, 1);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(ol) == -7 && get1(sc) == -7);
      for (int t = 0; t < 6; t++) CHECK(a[t]->pins == 0);
    }
    /* heap ByteBuffers where direct ones are required */
    fobj* hb = mk(5, 64);
    CHECK(BATCH(env, NULL, (jobject)hb, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)ts, (jintArray)ol, (jintArray)sc, 1) == LZ4HIP_E_ARG);
    if (arg_no_gpu(argc, argv)) {
      const jint rc = BATCH(env, NULL, (jobject)dsrc, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)ts, (jintArray)ol, (jintArray)sc, 1);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc() && get1(sc) == -7);
      for (int t = 0; t < 6; t++) CHECK(a[t]->pins == 0);
    } }
  if (arg_no_gpu(argc, argv)) {
    fobj* sz = int1(40);
    jint r = DEST(env, NULL, (jbyteArray)src, NULL, 7, (jintArray)sz, (jbyteArray)dst, NULL, 3, 100);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && get1(sz) == 40 && g_alloc == 0 && src->pins == 0 && dst->pins == 0 && sz->pins == 0);
    r = DEST(env, NULL, NULL, (jobject)dsrc, 0, (jintArray)sz, NULL, (jobject)ddst, 0, 30);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && get1(sz) == 40 && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strlen(msg) > 0);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 4) { fprintf(stderr, "usage: fake_jni_destsize --no-gpu | <input> <target> <out-dir>\n"); return 2; }
  const size_t SO = 5, DO = 7;
  long n = 0;
  fobj* asrc = slurp(argv[1], 1, SO, &n); fobj* dsrc2 = copy_as(asrc, 4);
  CHECK(n > 1000);
  const int t = atoi(argv[2]);
  CHECK(t > 0 && t < n);
  fobj* adst = mk(1, (size_t)t + 32); fobj* ddst2 = mk(4, (size_t)t + 32);
  /* byte[] -> byte[] */
  memset(adst->data, 0xEE, adst->bytes);
  fobj* sz = int1((jint)n);
  const jint r = DEST(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jintArray)sz, (jbyteArray)adst, NULL, (jint)DO, t);
  const jint consumed = get1(sz);
  CHECK(no_exc() && r > 0 && r <= t && consumed > 0 && consumed < n && g_alloc == 0 && asrc->pins == 0 && adst->pins == 0 && sz->pins == 0);
  CHECK(guarded(adst, DO, (size_t)r, 0xEE));
  write_bytes(argv[3], "dest.bin", adst->data + DO, (size_t)r);
  write_text(argv[3], "dest.txt", "%d %d\n", (int)r, (int)consumed);
  /* direct -> direct (NULL arrays), byte[] -> direct, direct -> byte[]: the same bytes, nothing outside the slot */
  for (int shape = 0; shape < 3; shape++) {
    fobj* adst2 = mk(1, (size_t)t + 32);
    memset(ddst2->data, 0xEE, ddst2->bytes); memset(adst2->data, 0xEE, adst2->bytes);
    ((jint*)sz->data)[0] = (jint)n;
    const int dir_in = shape != 1, dir_out = shape != 2;
    const jint r2 = DEST(env, NULL, dir_in ? NULL : (jbyteArray)asrc, dir_in ? (jobject)dsrc2 : NULL, (jint)SO, (jintArray)sz,
                         dir_out ? NULL : (jbyteArray)adst2, dir_out ? (jobject)ddst2 : NULL, (jint)DO, t);
    const fobj* d = dir_out ? ddst2 : adst2;
    CHECK(no_exc() && r2 == r && get1(sz) == consumed && memcmp(d->data + DO, adst->data + DO, (size_t)r) == 0 && guarded(d, DO, (size_t)r, 0xEE) && g_alloc == 0);
    free(adst2->data); free(adst2);
  }
  /* `out` cannot be pinned: `in` and srcSize are released, OutOfMemoryError */
  { fobj* nopin = mk(1, (size_t)t); nopin->refuse_pin = 1;
    ((jint*)sz->data)[0] = (jint)n;
    (void)DEST(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jintArray)sz, (jbyteArray)nopin, NULL, 0, t);
    CHECK(g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0 && g_alloc == 0 && asrc->pins == 0 && nopin->pins == 0 && sz->pins == 0);
    clear_exc(); }
  /* the batch native: two copies of the input -> the single call's bytes and consumed size twice, slots untouched past t */
  { fobj* bsrc = mk(4, 2 * (size_t)n); fobj* bdst = mk(4, 2 * (size_t)t + 64);
    memset(bdst->data, 0xEE, bdst->bytes);
    memcpy(bsrc->data, asrc->data + SO, (size_t)n); memcpy(bsrc->data + n, asrc->data + SO, (size_t)n);
    fobj* so = mk(3, 16); fobj* sl = mk(2, 8); fobj* dof = mk(3, 16); fobj* ts = mk(2, 8); fobj* ol = mk(2, 8); fobj* sc = mk(2, 8);
    ((jlong*)so->data)[0] = 0; ((jlong*)so->data)[1] = n; ((jint*)sl->data)[0] = ((jint*)sl->data)[1] = (jint)n;
    ((jlong*)dof->data)[0] = 0; ((jlong*)dof->data)[1] = t + 32; ((jint*)ts->data)[0] = ((jint*)ts->data)[1] = t;
    const jint rc = BATCH(env, NULL, (jobject)bsrc, (jlongArray)so, (jintArray)sl, (jobject)bdst, (jlongArray)dof, (jintArray)ts, (jintArray)ol, (jintArray)sc, 2);
    const jint* out = (const jint*)ol->data; const jint* cs = (const jint*)sc->data;
    CHECK(rc == 0 && out[0] == r && out[1] == r && cs[0] == consumed && cs[1] == consumed && so->pins == 0 && ol->pins == 0 && sc->pins == 0);
    CHECK(memcmp(bdst->data, adst->data + DO, (size_t)r) == 0 && memcmp(bdst->data + t + 32, adst->data + DO, (size_t)r) == 0);
    for (size_t i = (size_t)t; i < (size_t)t + 32; i++) CHECK(bdst->data[i] == 0xEE);
    for (size_t i = 2 * (size_t)t + 32; i < bdst->bytes; i++) CHECK(bdst->data[i] == 0xEE); }
  return checks_ok(NULL);
}
