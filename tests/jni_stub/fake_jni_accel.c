/* tests/jni_stub/fake_jni_accel.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The accelerated fast-compress native of the JNI shim (LZ4HIPJNI.LZ4HIP_compress_fast_accel and LZ4HIP_batch op 4) executed
 * without a JVM, with the fake JNIEnv of fake_env.h (a byte[] / int[] / long[] is a malloc'd buffer with pin accounting, a
 * direct ByteBuffer is a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by tests/test_gpu_accel.py /
 * tests/test_accel_abi.py.
 *
 *   fake_jni_accel --no-gpu            anywhere: the new native fails LOUDLY without a device (library error code, nothing leaked)
 *   fake_jni_accel <input> <out-dir>   on a GPU box: compresses <input> through every argument shape at accelerations 1 and 8 and
 *                                      writes the streams to <out-dir>/accel_<a>.bin (the test compares them with the reference
 *                                      library's LZ4_compress_fast); prints "fake_jni_accel: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_accel"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast(JNIEnv*, jclass, jbyteArray, jobject, jint, jint, jbyteArray, jobject, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast_1accel(JNIEnv*, jclass, jbyteArray, jobject, jint, jint, jbyteArray, jobject, jint, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batch(JNIEnv*, jclass, jint, jint, jobject, jlongArray, jintArray, jobject, jlongArray, jintArray, jintArray, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define ACCEL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast_1accel

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  if (arg_no_gpu(argc, argv)) {
    fobj* src = mk(1, 64); fobj* dst = mk(1, 128);
    for (int a = -3; a <= 9; a += 4) {   /* (acceleration 1 and below go through the plain fast path: loud as well) */
      jint r = ACCEL(env, NULL, (jbyteArray)src, NULL, 7, 20, (jbyteArray)dst, NULL, 3, 100, a);
      CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0 && src->pins == 0 && dst->pins == 0);
    }
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strlen(msg) > 0);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_accel --no-gpu | <input> <out-dir>\n"); return 2; }
  const size_t SO = 5, DO = 7;   /* offsets of the regions inside their arrays / buffers */
  long n = 0;
  fobj* asrc = slurp(argv[1], 1, SO, &n); fobj* dsrc = copy_as(asrc, 4);
  CHECK(n > 1000);
  const int bound = (int)n + (int)n / 255 + 16;
  fobj* adst = mk(1, (size_t)bound + 32); fobj* ddst = mk(4, (size_t)bound + 32);
  const int accels[2] = {1, 8};
  jint sizes[2] = {0, 0};
  for (int t = 0; t < 2; t++) {
    const int a = accels[t];
    /* byte[] -> byte[] */
    memset(adst->data, 0xEE, adst->bytes);
    jint r = ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)adst, NULL, (jint)DO, bound, a);
    CHECK(no_exc() && r > 0 && g_alloc == 0 && asrc->pins == 0 && adst->pins == 0);
    CHECK(guarded(adst, DO, (size_t)r, 0xEE));
    sizes[t] = r;
    char name[32];
    snprintf(name, sizeof name, "accel_%d.bin", a);
    write_bytes(argv[2], name, adst->data + DO, (size_t)r);
    /* direct -> direct (NULL arrays): the same bytes */
    memset(ddst->data, 0xEE, ddst->bytes);
    jint r2 = ACCEL(env, NULL, NULL, (jobject)dsrc, (jint)SO, (jint)n, NULL, (jobject)ddst, (jint)DO, bound, a);
    CHECK(no_exc() && r2 == r && memcmp(ddst->data + DO, adst->data + DO, (size_t)r) == 0 && guarded(ddst, DO, (size_t)r, 0xEE) && g_alloc == 0);
    /* byte[] -> direct and direct -> byte[] */
    memset(ddst->data, 0xEE, ddst->bytes);
    r2 = ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, NULL, (jobject)ddst, (jint)DO, bound, a);
    CHECK(no_exc() && r2 == r && memcmp(ddst->data + DO, adst->data + DO, (size_t)r) == 0 && g_alloc == 0 && asrc->pins == 0);
    fobj* adst2 = mk(1, (size_t)bound + 32);
    memset(adst2->data, 0xEE, adst2->bytes);
    r2 = ACCEL(env, NULL, NULL, (jobject)dsrc, (jint)SO, (jint)n, (jbyteArray)adst2, NULL, (jint)DO, bound, a);
    CHECK(no_exc() && r2 == r && memcmp(adst2->data + DO, adst->data + DO, (size_t)r) == 0 && guarded(adst2, DO, (size_t)r, 0xEE) && g_alloc == 0);
    /* too small by one byte: 0, and the staged byte[] destination is not touched at all */
    memset(adst2->data, 0xEE, adst2->bytes);
    r2 = ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)adst2, NULL, (jint)DO, r - 1, a);
    CHECK(no_exc() && r2 == 0 && guarded(adst2, 0, 0, 0xEE) && g_alloc == 0 && adst2->pins == 0);
    /* ... a direct destination: nothing outside the slot */
    memset(ddst->data, 0xEE, ddst->bytes);
    r2 = ACCEL(env, NULL, NULL, (jobject)dsrc, (jint)SO, (jint)n, NULL, (jobject)ddst, (jint)DO, r - 1, a);
    CHECK(no_exc() && r2 == 0 && guarded(ddst, DO, (size_t)r - 1, 0xEE));
    free(adst2->data); free(adst2);
  }
  /* acceleration 1 through the new native IS the plain native */
  { fobj* p = mk(1, (size_t)bound + 32);
    jint r = Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1fast(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)p, NULL, (jint)DO, bound);
    fobj* q = mk(1, (size_t)bound + 32);
    jint r2 = ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)q, NULL, (jint)DO, bound, -4);   /* clamps to 1 */
    CHECK(no_exc() && r == sizes[0] && r2 == r && memcmp(p->data, q->data, p->bytes) == 0); }
  /* a heap ByteBuffer where a direct one is required: no address, OutOfMemoryError as for the plain native */
  { fobj* hb = mk(5, 64);
    (void)ACCEL(env, NULL, NULL, (jobject)hb, 0, 20, (jbyteArray)adst, NULL, 0, 100, 8);
    CHECK(g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0 && g_alloc == 0);
    clear_exc(); }
  /* `out` cannot be pinned: `in` is released, OutOfMemoryError */
  { fobj* nopin = mk(1, (size_t)bound); nopin->refuse_pin = 1;
    (void)ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)nopin, NULL, 0, bound, 8);
    CHECK(g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0 && g_alloc == 0 && asrc->pins == 0 && nopin->pins == 0);
    clear_exc(); }
  /* the batch entry, op 4: two copies of the input at acceleration 8 -> the single call's bytes twice */
  { fobj* bsrc = mk(4, 2 * (size_t)n); fobj* bdst = mk(4, 2 * (size_t)bound);
    memcpy(bsrc->data, asrc->data + SO, (size_t)n); memcpy(bsrc->data + n, asrc->data + SO, (size_t)n);
    fobj* so = mk(3, 16); fobj* sl = mk(2, 8); fobj* dof = mk(3, 16); fobj* dc = mk(2, 8); fobj* ol = mk(2, 8);
    ((jlong*)so->data)[0] = 0; ((jlong*)so->data)[1] = n; ((jint*)sl->data)[0] = ((jint*)sl->data)[1] = (jint)n;
    ((jlong*)dof->data)[0] = 0; ((jlong*)dof->data)[1] = bound; ((jint*)dc->data)[0] = ((jint*)dc->data)[1] = bound;
    jint rc = Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batch(env, NULL, 4, 8, (jobject)bsrc, (jlongArray)so, (jintArray)sl, (jobject)bdst,
                                                           (jlongArray)dof, (jintArray)dc, (jintArray)ol, 2);
    const jint* out = (const jint*)ol->data;
    CHECK(rc == 0 && out[0] == sizes[1] && out[1] == sizes[1] && so->pins == 0 && ol->pins == 0);
    fobj* ref8 = mk(1, (size_t)bound + 32);
    (void)ACCEL(env, NULL, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)ref8, NULL, 0, bound, 8);
    CHECK(memcmp(bdst->data, ref8->data, (size_t)sizes[1]) == 0 && memcmp(bdst->data + bound, ref8->data, (size_t)sizes[1]) == 0); }
  CHECK(sizes[1] > sizes[0]);   /* acceleration 8 trades ratio for speed: a bigger stream on this input */
  return checks_ok(NULL);
}
