/* tests/jni_stub/fake_jni_container_many.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The many-container natives of the JNI shim (LZ4HIPJNI.LZ4HIP_containerDecodeMany and LZ4HIP_containerDecodeManyBound) executed
 * without a JVM, with the fake JNIEnv of fake_env.h (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is
 * a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of tests/support.py) by
 * tests/test_container_many_abi.py / tests/test_gpu_container_many.py.
 *
 *   fake_jni_container_many --no-gpu             anywhere: NULL arrays and short arrays are argument errors, the bound native needs no
 *                                                device, the read fails LOUDLY without one (nothing leaked or left pinned)
 *   fake_jni_container_many <cases> <out-dir>    on a GPU box: the items of the case file (tests/cpp/container_rules_test.cpp says the
 *                                                format; one kind and one n_max for all) in ONE call; writes per item
 *                                                "I <blocks> <consumed> <why> <code> <decoded bytes> <sizes...>" to <out-dir>/results.txt
 *                                                and the decoded bytes, item after item, to <out-dir>/decoded.bin; checks the guard bytes
 *                                                behind the delivered bytes; prints "fake_jni_container_many: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_container_many"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeMany(JNIEnv*, jclass, jint, jobject, jlongArray, jlongArray, jintArray, jintArray, jint, jint,
                                                                                  jobject, jlong, jlong, jlongArray, jintArray, jintArray, jlongArray);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeManyBound(JNIEnv*, jclass, jint, jobject, jlongArray, jlongArray, jintArray, jintArray, jint,
                                                                                       jint, jintArray, jlongArray);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define MANY Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeMany
#define BOUND Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerDecodeManyBound

static int unpinned(fobj** a, int n) { for (int t = 0; t < n; t++) if (a[t]->pins != 0) return 0; return 1; }

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  const int no_gpu = arg_no_gpu(argc, argv);
  /* two frame bodies of one raw block each (5 bytes "hello", 3 bytes "abc") with the end mark, 17 and 15 bytes */
  { static const uint8_t two[] = {5, 0, 0, 0x80, 'h', 'e', 'l', 'l', 'o', 0, 0, 0, 0, 3, 0, 0, 0x80, 'a', 'b', 'c', 0, 0, 0, 0};
    fobj* bodies = mk(4, sizeof two); memcpy(bodies->data, two, sizeof two);
    fobj* off = mk(3, 16); fobj* len = mk(3, 16); fobj* mb = mk(2, 8); fobj* fl = mk(2, 8);
    ((jlong*)off->data)[1] = 13; ((jlong*)len->data)[0] = 13; ((jlong*)len->data)[1] = 11;
    ((jint*)mb->data)[0] = ((jint*)mb->data)[1] = 65536;
    fobj* nb = mk(2, 8); fobj* need = mk(3, 16);
    fobj* dest = mk(4, 64); fobj* doff = mk(3, 24); fobj* first = mk(2, 12); fobj* sizes = mk(2, 8); fobj* info = mk(3, 80);
    fobj* all[11] = {off, len, mb, fl, nb, need, doff, first, sizes, info, dest};
    /* the bound native: no device needed */
    CHECK(BOUND(env, NULL, 0, (jobject)bodies, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 2, 4, (jintArray)nb, (jlongArray)need) == 0);
    CHECK(((jint*)nb->data)[0] == 1 && ((jint*)nb->data)[1] == 1 && ((jlong*)need->data)[0] == 5 && ((jlong*)need->data)[1] == 3 && unpinned(all, 11) && g_alloc == 0);
    /* NULL arrays / buffers: LZ4HIP_E_ARG, nothing pinned, nothing allocated */
    for (int k = 0; k < 7; k++) {
      const jint rc = BOUND(env, NULL, 0, k == 0 ? NULL : (jobject)bodies, k == 1 ? NULL : (jlongArray)off, k == 2 ? NULL : (jlongArray)len, k == 3 ? NULL : (jintArray)mb,
                            k == 4 ? NULL : (jintArray)fl, 2, 4, k == 5 ? NULL : (jintArray)nb, k == 6 ? NULL : (jlongArray)need);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && unpinned(all, 11) && g_alloc == 0);
    }
    for (int k = 0; k < 10; k++) {
      const jint rc = MANY(env, NULL, 0, k == 0 ? NULL : (jobject)bodies, k == 1 ? NULL : (jlongArray)off, k == 2 ? NULL : (jlongArray)len, k == 3 ? NULL : (jintArray)mb,
                           k == 4 ? NULL : (jintArray)fl, 2, 4, k == 5 ? NULL : (jobject)dest, 0, 64, k == 6 ? NULL : (jlongArray)doff, k == 7 ? NULL : (jintArray)first,
                           k == 8 ? NULL : (jintArray)sizes, k == 9 ? NULL : (jlongArray)info);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && unpinned(all, 11) && g_alloc == 0);
    }
    /* arrays that are too short for the items, a heap ByteBuffer where a direct one is required, a flag word that is no flag */
    CHECK(MANY(env, NULL, 0, (jobject)bodies, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 3, 4, (jobject)dest, 0, 64, (jlongArray)doff, (jintArray)first,
               (jintArray)sizes, (jlongArray)info) == LZ4HIP_E_ARG);
    { fobj* short_first = mk(2, 8);
      CHECK(MANY(env, NULL, 0, (jobject)bodies, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 2, 4, (jobject)dest, 0, 64, (jlongArray)doff,
                 (jintArray)short_first, (jintArray)sizes, (jlongArray)info) == LZ4HIP_E_ARG); }
    { fobj* hb = mk(5, 64);
      CHECK(MANY(env, NULL, 0, (jobject)hb, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 2, 4, (jobject)dest, 0, 64, (jlongArray)doff, (jintArray)first,
                 (jintArray)sizes, (jlongArray)info) == LZ4HIP_E_ARG); }
    ((jint*)fl->data)[1] = 2;
    CHECK(MANY(env, NULL, 0, (jobject)bodies, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 2, 4, (jobject)dest, 0, 64, (jlongArray)doff, (jintArray)first,
               (jintArray)sizes, (jlongArray)info) == LZ4HIP_E_ARG && unpinned(all, 11) && g_alloc == 0);
    ((jint*)fl->data)[1] = 0;
    memset(dest->data, 0xEE, 64);
    const jint rc = MANY(env, NULL, 0, (jobject)bodies, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, 2, 4, (jobject)dest, 7, 64 - 7, (jlongArray)doff,
                         (jintArray)first, (jintArray)sizes, (jlongArray)info);
    CHECK(no_exc() && unpinned(all, 11) && g_alloc == 0);
    if (no_gpu) {
      CHECK(rc == LZ4HIP_E_NO_DEVICE && guarded(dest, 0, 0, 0xEE));
      const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
      CHECK(msg && strlen(msg) > 0);
      return checks_ok("the read failed loudly");
    }
    CHECK(rc == 0 && memcmp(dest->data + 7, "helloabc", 8) == 0 && guarded(dest, 7, 8, 0xEE));
    CHECK(((jlong*)doff->data)[1] == 5 && ((jlong*)doff->data)[2] == 8 && ((jint*)first->data)[1] == 1 && ((jint*)first->data)[2] == 2);
    CHECK(((jint*)sizes->data)[0] == 5 && ((jint*)sizes->data)[1] == 3 && ((jlong*)info->data)[1] == 13 && ((jlong*)info->data)[5 + 2] == 0); }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_container_many --no-gpu | <cases> <out-dir>\n"); return 2; }
  long n = 0;
  fobj* file = slurp(argv[1], 4, 0, &n);
  CHECK(n >= 4);
  uint32_t count;
  memcpy(&count, file->data, 4);
  fobj* off = mk(3, 8u * count + 8); fobj* len = mk(3, 8u * count + 8); fobj* mb = mk(2, 4u * count + 4); fobj* fl = mk(2, 4u * count + 4);
  jint kind = 0, n_max = 1;
  size_t p = 4;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t h[4]; uint64_t l;
    CHECK(p + 32 <= (size_t)n);
    memcpy(h, file->data + p, 16); memcpy(&l, file->data + p + 24, 8); p += 32;
    CHECK(p + l <= (size_t)n);
    kind = (jint)h[0]; n_max = (jint)h[3];
    ((jint*)fl->data)[i] = (jint)h[1]; ((jint*)mb->data)[i] = (jint)h[2]; ((jlong*)off->data)[i] = (jlong)p; ((jlong*)len->data)[i] = (jlong)l;
    p += l;
  }
  fobj* nb = mk(2, 4u * count + 4); fobj* need = mk(3, 8u * count + 8);
  CHECK(BOUND(env, NULL, kind, (jobject)file, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, (jint)count, n_max, (jintArray)nb, (jlongArray)need) == 0);
  uint64_t cap = 0, scap = 0;
  for (uint32_t i = 0; i < count; i++) { cap += (uint64_t)((jlong*)need->data)[i]; scap += (uint64_t)((jint*)nb->data)[i]; }
  const size_t G = 64;
  fobj* dest = mk(4, cap + 2 * G); memset(dest->data, 0xEE, cap + 2 * G);
  fobj* doff = mk(3, 8u * count + 8); fobj* first = mk(2, 4u * count + 4); fobj* sizes = mk(2, 4u * scap); fobj* info = mk(3, 40u * count);
  const jint rc = MANY(env, NULL, kind, (jobject)file, (jlongArray)off, (jlongArray)len, (jintArray)mb, (jintArray)fl, (jint)count, n_max, (jobject)dest, (jlong)G,
                       (jlong)cap, (jlongArray)doff, (jintArray)first, (jintArray)sizes, (jlongArray)info);
  CHECK(rc == 0 && no_exc() && g_alloc == 0);
  { fobj* all[10] = {off, len, mb, fl, nb, need, doff, first, sizes, info}; CHECK(unpinned(all, 10)); }
  const uint64_t total = (uint64_t)((jlong*)doff->data)[count];
  CHECK(total <= cap && guarded(dest, G, (size_t)total, 0xEE));
  FILE* o = out_file(argv[2], "results.txt", "w");
  for (uint32_t i = 0; i < count; i++) {
    const jlong* inf = (const jlong*)info->data + 5u * i;
    const jint f0 = ((jint*)first->data)[i], f1 = ((jint*)first->data)[i + 1];
    CHECK(f1 - f0 == (jint)inf[0] && ((jlong*)doff->data)[i + 1] - ((jlong*)doff->data)[i] == inf[3]);
    fprintf(o, "I %d %lld %d %lld %lld", (int)inf[0], (long long)inf[1], (int)inf[2], (long long)inf[4], (long long)inf[3]);
    for (jint k = f0; k < f1; k++) fprintf(o, " %d", (int)((jint*)sizes->data)[k]);
    fprintf(o, "\n");
  }
  fclose(o);
  write_bytes(argv[2], "decoded.bin", dest->data + G, (size_t)total);
  return checks_ok(NULL);
}
