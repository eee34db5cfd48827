/* tests/jni_stub/fake_jni_hcdict.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The dictionary HC compress natives of the JNI shim (LZ4HIPJNI.LZ4HIP_compress_hc_dict and LZ4HIP_batchCompressHCDict, over the handles of
 * LZ4HIP_dictCreate) executed without a JVM, with the fake JNIEnv of fake_env.h (a byte[] / int[] / long[] is a malloc'd buffer with pin
 * accounting, a direct ByteBuffer is a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by
 * tests/test_hcdict_abi.py / tests/test_gpu_hcdict.py.
 *
 *   fake_jni_hcdict --no-gpu                     anywhere: NULL arguments and a 0 handle are argument errors, every compress fails LOUDLY
 *                                               without a device (library error code, nothing leaked or left pinned)
 *   fake_jni_hcdict <dict> <record> <out-dir> <level>   on a GPU box: compresses <record> against the dictionary <dict> through every argument
 *                                               shape and the batch native, writes the bytes to <out-dir>/hcdict.bin (the test compares
 *                                               them with the reference's LZ4_loadDictHC + LZ4_compress_HC_continue); a capacity one
 *                                               byte short gives 0; prints "fake_jni_hcdict: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_hcdict"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictCreate(JNIEnv*, jclass, jbyteArray, jobject, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictSize(JNIEnv*, jclass, jlong);
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictFree(JNIEnv*, jclass, jlong);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1hc_1dict(JNIEnv*, jclass, jlong, jint, jbyteArray, jobject, jint, jint, jbyteArray, jobject, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchCompressHCDict(JNIEnv*, jclass, jlong, jint, jobject, jlongArray, jintArray, jobject, jlongArray, jintArray, jintArray, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define CREATE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictCreate
#define SIZE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictSize
#define FREE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1dictFree
#define CMP(e, c, h, ...) Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1compress_1hc_1dict(e, c, h, g_level, __VA_ARGS__)
#define BATCH(e, c, h, ...) Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchCompressHCDict(e, c, h, g_level, __VA_ARGS__)
static jint g_level = 9;

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  const int no_gpu = arg_no_gpu(argc, argv);
  fobj* src = mk(1, 64); fobj* dst = mk(1, 128); fobj* dsrc = mk(4, 64); fobj* ddst = mk(4, 128);
  fobj* dbytes = mk(1, 100);
  for (size_t i = 0; i < dbytes->bytes; i++) dbytes->data[i] = (uint8_t)(i * 7u);
  const jlong h1 = CREATE(env, NULL, (jbyteArray)dbytes, NULL, 10, 90);
  CHECK(h1 != 0 && no_exc() && dbytes->pins == 0 && g_alloc == 0 && SIZE(env, NULL, h1) == 90);
  /* NULL arrays / buffers and a 0 handle of the batch native: LZ4HIP_E_ARG, nothing pinned */
  { fobj* so = mk(3, 8); fobj* sl = int1(20); fobj* dof = mk(3, 8); fobj* dc = int1(100); fobj* ol = int1(-7);
    fobj* a[5] = {so, sl, dof, dc, ol};
    for (int k = 0; k < 8; k++) {
      jint rc = BATCH(env, NULL, k == 7 ? 0 : h1, k == 5 ? NULL : (jobject)dsrc, k == 0 ? NULL : (jlongArray)so, k == 1 ? NULL : (jintArray)sl,
                      k == 6 ? NULL : (jobject)ddst, k == 2 ? NULL : (jlongArray)dof, k == 3 ? NULL : (jintArray)dc, k == 4 ? NULL : (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(ol) == -7);
      for (int t = 0; t < 5; t++) CHECK(a[t]->pins == 0);
    }
    fobj* hb = mk(5, 64);   /* a heap ByteBuffer where a direct one is required */
    CHECK(BATCH(env, NULL, h1, (jobject)hb, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)dc, (jintArray)ol, 1) == LZ4HIP_E_ARG);
    if (no_gpu) {
      const jint rc = BATCH(env, NULL, h1, (jobject)dsrc, (jlongArray)so, (jintArray)sl, (jobject)ddst, (jlongArray)dof, (jintArray)dc, (jintArray)ol, 1);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc());
      for (int t = 0; t < 5; t++) CHECK(a[t]->pins == 0);
    } }
  if (no_gpu) {
    memset(dst->data, 0xEE, dst->bytes);
    jint r = CMP(env, NULL, h1, (jbyteArray)src, NULL, 7, 20, (jbyteArray)dst, NULL, 3, 100);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0 && src->pins == 0 && dst->pins == 0 && guarded(dst, 0, 0, 0xEE));
    r = CMP(env, NULL, h1, NULL, (jobject)dsrc, 0, 20, NULL, (jobject)ddst, 0, 60);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0);
    r = CMP(env, NULL, 0, NULL, (jobject)dsrc, 0, 20, NULL, (jobject)ddst, 0, 60);
    CHECK(LZ4HIP_IS_LIB_ERROR(r) && no_exc() && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strlen(msg) > 0);
    FREE(env, NULL, h1);
    return checks_ok("every compress failed loudly");
  }
  FREE(env, NULL, h1);
  if (argc < 5) { fprintf(stderr, "usage: fake_jni_hcdict --no-gpu | <dict> <record> <out-dir> <level>\n"); return 2; }
  g_level = atoi(argv[4]);
  long dn = 0, n = 0;
  const size_t SO = 5, DO = 7;
  fobj* adict = slurp(argv[1], 1, 3, &dn);
  fobj* asrc = slurp(argv[2], 1, SO, &n);
  fobj* dsrc2 = copy_as(asrc, 4);
  const int cap = (int)(n + n / 255 + 16);
  const jlong h = CREATE(env, NULL, (jbyteArray)adict, NULL, 3, (jint)dn);
  CHECK(h != 0 && no_exc() && SIZE(env, NULL, h) == (jint)dn && adict->pins == 0 && g_alloc == 0);
  memset(adict->data, 0, adict->bytes);   /* the handle holds a copy */
  fobj* adst = mk(1, (size_t)cap + 32); fobj* ddst2 = mk(4, (size_t)cap + 32);
  /* byte[] -> byte[] */
  memset(adst->data, 0xEE, adst->bytes);
  const jint r = CMP(env, NULL, h, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)adst, NULL, (jint)DO, cap);
  CHECK(no_exc() && !LZ4HIP_IS_LIB_ERROR(r) && r > 0 && r <= cap && g_alloc == 0 && asrc->pins == 0 && adst->pins == 0);
  const size_t got = (size_t)r;
  CHECK(guarded(adst, DO, got, 0xEE));
  write_bytes(argv[3], "hcdict.bin", adst->data + DO, got);
  /* direct -> direct (NULL arrays), byte[] -> direct, direct -> byte[]: the same result, nothing written outside the slot */
  for (int shape = 0; shape < 3; shape++) {
    fobj* adst2 = mk(1, (size_t)cap + 32);
    memset(ddst2->data, 0xEE, ddst2->bytes); memset(adst2->data, 0xEE, adst2->bytes);
    const int dir_in = shape != 1, dir_out = shape != 2;
    const jint r2 = CMP(env, NULL, h, dir_in ? NULL : (jbyteArray)asrc, dir_in ? (jobject)dsrc2 : NULL, (jint)SO, (jint)n,
                        dir_out ? NULL : (jbyteArray)adst2, dir_out ? (jobject)ddst2 : NULL, (jint)DO, cap);
    const fobj* d = dir_out ? ddst2 : adst2;
    CHECK(no_exc() && r2 == r && memcmp(d->data + DO, adst->data + DO, got) == 0 && g_alloc == 0);
    if (dir_out) CHECK(guarded(d, DO, (size_t)cap, 0xEE));
    else CHECK(guarded(d, DO, got, 0xEE));
    free(adst2->data); free(adst2);
  }
  /* one byte short: 0, and nothing outside the slot */
  { memset(ddst2->data, 0xEE, ddst2->bytes);
    const jint r0 = CMP(env, NULL, h, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, NULL, (jobject)ddst2, (jint)DO, r - 1);
    CHECK(no_exc() && r0 == 0 && g_alloc == 0 && guarded(ddst2, DO, (size_t)(r - 1), 0xEE)); }
  /* `out` cannot be pinned: `in` is released, OutOfMemoryError */
  { fobj* nopin = mk(1, (size_t)cap + 1); nopin->refuse_pin = 1;
    (void)CMP(env, NULL, h, (jbyteArray)asrc, NULL, (jint)SO, (jint)n, (jbyteArray)nopin, NULL, 0, cap);
    CHECK(g_alloc == 0 && asrc->pins == 0 && nopin->pins == 0);
    CHECK(g_exc_class && strcmp(g_exc_class, "java/lang/OutOfMemoryError") == 0);
    clear_exc(); }
  /* the batch native: the record twice, the second slot one byte short -> the single call's result, then 0; nothing written outside
   * the two slots */
  { fobj* bsrc = mk(4, 2 * (size_t)n + 1); fobj* bdst = mk(4, 2 * (size_t)cap + 64);
    memset(bdst->data, 0xEE, bdst->bytes);
    memcpy(bsrc->data, asrc->data + SO, (size_t)n); memcpy(bsrc->data + n, asrc->data + SO, (size_t)n);
    fobj* so = mk(3, 16); fobj* sl = mk(2, 8); fobj* dof = mk(3, 16); fobj* dc = mk(2, 8); fobj* ol = mk(2, 8);
    ((jlong*)so->data)[0] = 0; ((jlong*)so->data)[1] = n; ((jint*)sl->data)[0] = ((jint*)sl->data)[1] = (jint)n;
    ((jlong*)dof->data)[0] = 0; ((jlong*)dof->data)[1] = cap + 32;
    ((jint*)dc->data)[0] = cap; ((jint*)dc->data)[1] = r - 1;
    const jint rc = BATCH(env, NULL, h, (jobject)bsrc, (jlongArray)so, (jintArray)sl, (jobject)bdst, (jlongArray)dof, (jintArray)dc, (jintArray)ol, 2);
    const jint* out = (const jint*)ol->data;
    CHECK(rc == 0 && out[0] == r && out[1] == 0 && so->pins == 0 && ol->pins == 0 && dc->pins == 0);
    CHECK(memcmp(bdst->data, adst->data + DO, got) == 0);
    for (size_t i = (size_t)cap; i < (size_t)cap + 32; i++) CHECK(bdst->data[i] == 0xEE);
    for (size_t i = (size_t)cap + 32 + (size_t)(r - 1); i < bdst->bytes; i++) CHECK(bdst->data[i] == 0xEE); }
  FREE(env, NULL, h);
  return checks_ok(NULL);
}
