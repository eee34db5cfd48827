/* tests/jni_stub/fake_jni_container_write_many.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The many-container write natives of the JNI shim (LZ4HIPJNI.LZ4HIP_containerBlocksMany and LZ4HIP_containerBlocksManyBound) executed
 * without a JVM, with the fake JNIEnv of fake_env.h (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is
 * a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of tests/support.py) by
 * tests/test_container_write_many_mirrors.py / tests/test_gpu_container_write_many.py.
 *
 *   fake_jni_container_write_many --no-gpu            anywhere: NULL arrays and short arrays are argument errors, the bound native needs
 *                                                     no device, the write fails LOUDLY without one (nothing leaked or left pinned)
 *   fake_jni_container_write_many <cases> <out-dir>   on a GPU box: the items of the case file (u32 kind, u32 level, u32 count, then per
 *                                                     item {u32 block_size, u32 flags, u32 gap_head, u32 gap_tail, u64 len, bytes}) in
 *                                                     ONE call; writes per item "I <item bytes> <content hash>" to <out-dir>/results.txt
 *                                                     and the items' bytes (gaps included), item after item, to <out-dir>/written.bin;
 *                                                     checks the guard bytes around them; prints "...: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_container_write_many"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksMany(JNIEnv*, jclass, jint, jint, jobject, jlongArray, jlongArray, jintArray, jintArray,
                                                                                  jintArray, jintArray, jint, jobject, jlong, jlong, jlongArray, jintArray);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksManyBound(JNIEnv*, jclass, jint, jlongArray, jintArray, jintArray, jintArray, jintArray, jint,
                                                                                       jintArray, jlongArray);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define MANY Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksMany
#define BOUND Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksManyBound

static int unpinned(fobj** a, int n) { for (int t = 0; t < n; t++) if (a[t]->pins != 0) return 0; return 1; }

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  const int no_gpu = arg_no_gpu(argc, argv);
  /* two items of noise-like bytes that stay raw: 5 bytes "hello" (block size 64, gaps 3 / 2, content hash) and 3 bytes "abc" (no gaps) */
  { fobj* src = mk(4, 16); memcpy(src->data, "helloabc", 8);
    fobj* off = mk(3, 16); fobj* len = mk(3, 16); fobj* bs = mk(2, 8); fobj* fl = mk(2, 8); fobj* gh = mk(2, 8); fobj* gt = mk(2, 8);
    ((jlong*)off->data)[1] = 5; ((jlong*)len->data)[0] = 5; ((jlong*)len->data)[1] = 3;
    ((jint*)bs->data)[0] = ((jint*)bs->data)[1] = 64; ((jint*)fl->data)[0] = 2; ((jint*)gh->data)[0] = 3; ((jint*)gt->data)[0] = 2;
    fobj* nb = mk(2, 8); fobj* need = mk(3, 16);
    fobj* dest = mk(4, 64); fobj* doff = mk(3, 24); fobj* hash = mk(2, 8);
    fobj* all[11] = {off, len, bs, fl, gh, gt, nb, need, doff, hash, dest};
    /* the bound native: no device needed */
    CHECK(BOUND(env, NULL, 0, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jintArray)nb, (jlongArray)need) == 0);
    CHECK(((jint*)nb->data)[0] == 1 && ((jint*)nb->data)[1] == 1 && ((jlong*)need->data)[0] == 3 + 5 + 4 + 2 && ((jlong*)need->data)[1] == 3 + 4 && unpinned(all, 11) &&
          g_alloc == 0);
    /* NULL arrays / buffers: LZ4HIP_E_ARG, nothing pinned, nothing allocated */
    for (int k = 0; k < 7; k++) {
      const jint rc = BOUND(env, NULL, 0, k == 0 ? NULL : (jlongArray)len, k == 1 ? NULL : (jintArray)bs, k == 2 ? NULL : (jintArray)fl, k == 3 ? NULL : (jintArray)gh,
                            k == 4 ? NULL : (jintArray)gt, 2, k == 5 ? NULL : (jintArray)nb, k == 6 ? NULL : (jlongArray)need);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && unpinned(all, 11) && g_alloc == 0);
    }
    for (int k = 0; k < 10; k++) {
      const jint rc = MANY(env, NULL, 0, 0, k == 0 ? NULL : (jobject)src, k == 1 ? NULL : (jlongArray)off, k == 2 ? NULL : (jlongArray)len, k == 3 ? NULL : (jintArray)bs,
                           k == 4 ? NULL : (jintArray)fl, k == 5 ? NULL : (jintArray)gh, k == 6 ? NULL : (jintArray)gt, 2, k == 7 ? NULL : (jobject)dest, 0, 64,
                           k == 8 ? NULL : (jlongArray)doff, k == 9 ? NULL : (jintArray)hash);
      CHECK(rc == LZ4HIP_E_ARG && no_exc() && unpinned(all, 11) && g_alloc == 0);
    }
    /* arrays that are too short for the items, a heap ByteBuffer where a direct one is required, a flag word that is no flag, a bad
     * block size, block checksums with LZ4Block blocks, a destination below the bound */
    CHECK(MANY(env, NULL, 0, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 3, (jobject)dest, 0, 64,
               (jlongArray)doff, (jintArray)hash) == LZ4HIP_E_ARG);
    { fobj* short_off = mk(3, 16);
      CHECK(MANY(env, NULL, 0, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 0, 64,
                 (jlongArray)short_off, (jintArray)hash) == LZ4HIP_E_ARG); }
    { fobj* hb = mk(5, 64);
      CHECK(MANY(env, NULL, 0, 0, (jobject)hb, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 0, 64,
                 (jlongArray)doff, (jintArray)hash) == LZ4HIP_E_ARG); }
    ((jint*)fl->data)[1] = 4;
    CHECK(MANY(env, NULL, 0, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 0, 64,
               (jlongArray)doff, (jintArray)hash) == LZ4HIP_E_ARG && unpinned(all, 11) && g_alloc == 0);
    ((jint*)fl->data)[1] = 1;
    CHECK(MANY(env, NULL, 1, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 0, 64,
               (jlongArray)doff, (jintArray)hash) == LZ4HIP_E_ARG);
    ((jint*)fl->data)[1] = 0;
    ((jint*)bs->data)[1] = 63;
    CHECK(BOUND(env, NULL, 0, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jintArray)nb, (jlongArray)need) == LZ4HIP_E_ARG);
    ((jint*)bs->data)[1] = 64;
    CHECK(MANY(env, NULL, 0, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 0, 20,
               (jlongArray)doff, (jintArray)hash) == LZ4HIP_E_ARG && unpinned(all, 11) && g_alloc == 0);
    memset(dest->data, 0xEE, 64);
    const jint rc = MANY(env, NULL, 0, 0, (jobject)src, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, 2, (jobject)dest, 7,
                         64 - 7, (jlongArray)doff, (jintArray)hash);
    CHECK(no_exc() && unpinned(all, 11) && g_alloc == 0);
    if (no_gpu) {
      CHECK(rc == LZ4HIP_E_NO_DEVICE && guarded(dest, 0, 0, 0xEE));
      const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
      CHECK(msg && strlen(msg) > 0);
      return checks_ok("the write failed loudly");
    }
    static const uint8_t want[21] = {0, 0, 0, 5, 0, 0, 0x80, 'h', 'e', 'l', 'l', 'o', 0, 0, 3, 0, 0, 0x80, 'a', 'b', 'c'};
    CHECK(rc == 0 && memcmp(dest->data + 7, want, 21) == 0 && guarded(dest, 7, 21, 0xEE));
    CHECK(((jlong*)doff->data)[0] == 0 && ((jlong*)doff->data)[1] == 14 && ((jlong*)doff->data)[2] == 21);
    CHECK((uint32_t)((jint*)hash->data)[0] == 0xFB0077F9u && ((jint*)hash->data)[1] == 0); }   /* XXH32("hello", 0) */
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_container_write_many --no-gpu | <cases> <out-dir>\n"); return 2; }
  long n = 0;
  fobj* file = slurp(argv[1], 4, 0, &n);
  CHECK(n >= 12);
  uint32_t head[3];
  memcpy(head, file->data, 12);
  const uint32_t count = head[2];
  fobj* off = mk(3, 8u * count + 8); fobj* len = mk(3, 8u * count + 8); fobj* bs = mk(2, 4u * count + 4); fobj* fl = mk(2, 4u * count + 4);
  fobj* gh = mk(2, 4u * count + 4); fobj* gt = mk(2, 4u * count + 4);
  size_t p = 12;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t h[4]; uint64_t l;
    CHECK(p + 24 <= (size_t)n);
    memcpy(h, file->data + p, 16); memcpy(&l, file->data + p + 16, 8); p += 24;
    CHECK(p + l <= (size_t)n);
    ((jint*)bs->data)[i] = (jint)h[0]; ((jint*)fl->data)[i] = (jint)h[1]; ((jint*)gh->data)[i] = (jint)h[2]; ((jint*)gt->data)[i] = (jint)h[3];
    ((jlong*)off->data)[i] = (jlong)p; ((jlong*)len->data)[i] = (jlong)l;
    p += l;
  }
  fobj* nb = mk(2, 4u * count + 4); fobj* need = mk(3, 8u * count + 8);
  CHECK(BOUND(env, NULL, (jint)head[0], (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt, (jint)count, (jintArray)nb, (jlongArray)need) == 0);
  uint64_t cap = 0;
  for (uint32_t i = 0; i < count; i++) cap += (uint64_t)((jlong*)need->data)[i];
  const size_t G = 64;
  fobj* dest = mk(4, cap + 2 * G); memset(dest->data, 0xEE, cap + 2 * G);
  fobj* doff = mk(3, 8u * count + 8); fobj* hash = mk(2, 4u * count + 4);
  const jint rc = MANY(env, NULL, (jint)head[0], (jint)head[1], (jobject)file, (jlongArray)off, (jlongArray)len, (jintArray)bs, (jintArray)fl, (jintArray)gh, (jintArray)gt,
                       (jint)count, (jobject)dest, (jlong)G, (jlong)cap, (jlongArray)doff, (jintArray)hash);
  CHECK(rc == 0 && no_exc() && g_alloc == 0);
  { fobj* all[10] = {off, len, bs, fl, gh, gt, nb, need, doff, hash}; CHECK(unpinned(all, 10)); }
  const uint64_t total = (uint64_t)((jlong*)doff->data)[count];
  CHECK(total <= cap && guarded(dest, G, (size_t)total, 0xEE));
  FILE* o = out_file(argv[2], "results.txt", "w");
  for (uint32_t i = 0; i < count; i++)
    fprintf(o, "I %lld %u\n", (long long)(((jlong*)doff->data)[i + 1] - ((jlong*)doff->data)[i]), (unsigned)((jint*)hash->data)[i]);
  fclose(o);
  write_bytes(argv[2], "written.bin", dest->data + G, (size_t)total);
  return checks_ok(NULL);
}
