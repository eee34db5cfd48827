/* tests/jni_stub/fake_jni_chain.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The linked-block native of the JNI shim (LZ4HIPJNI.LZ4HIP_batchSafeChain) executed without a JVM, with the fake JNIEnv of fake_env.h
 * (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is a pointer; the shim's malloc / free are counted
 * through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py; the shared file reading, output files and closing line are fake_env.h's) by tests/test_chain_abi.py / tests/test_gpu_chain.py.
 *
 *   fake_jni_chain --no-gpu           anywhere: NULL arrays and a bad chainFirst are argument errors, a well-formed call fails LOUDLY
 *                                     without a device (library status, nothing leaked or left pinned, nothing written)
 *   fake_jni_chain <chain> <out-dir>  on a GPU box: one chain through the native, with and without the optional arrays where the chain
 *                                     allows it.  <chain>: u32 n_blocks, u32 prefix_len, u64 chain capacity, then per block {u32 stream
 *                                     length, u32 stored, i32 capacity}, the history bytes, the streams back to back.  Writes
 *                                     "<out_len ...> | <chain_out_len>" to <out-dir>/chain.txt and the decoded bytes to <out-dir>/chain.out
 *                                     (the test compares both with the reference's LZ4_decompress_safe_continue); prints
 *                                     "fake_jni_chain: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_chain"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeChain(JNIEnv*, jclass, jobject, jlongArray, jintArray, jintArray, jintArray, jintArray,
    jobject, jlongArray, jlongArray, jintArray, jintArray, jlongArray, jint, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define CHAIN Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeChain

static int no_gpu_checks(JNIEnv* env) {
  fobj* src = mk(4, 64); fobj* dst = mk(4, 64);
  src->data[0] = 0x10; src->data[1] = 'a';
  memset(dst->data, 7, 64);
  fobj* so = mk(3, 8); fobj* sl = int1(2); fobj* st = int1(0); fobj* dc = int1(8); fobj* first = mk(2, 8);
  fobj* cdo = mk(3, 8); fobj* ccap = mk(3, 8); fobj* pre = int1(4); fobj* ol = int1(-7); fobj* col = mk(3, 8);
  ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = 1;
  ((jlong*)cdo->data)[0] = 16; ((jlong*)ccap->data)[0] = 8; ((jlong*)col->data)[0] = 99;
  fobj* all[10] = {so, sl, st, dc, first, cdo, ccap, pre, ol, col};
  /* every required argument NULL in turn: LZ4HIP_E_ARG, nothing pinned (k = 2 and 7 are the optional arrays: tested below) */
  for (int k = 0; k < 12; k++) {
    if (k == 2 || k == 7) continue;
    const jint rc = CHAIN(env, NULL, k == 10 ? NULL : (jobject)src, k == 0 ? NULL : (jlongArray)so, k == 1 ? NULL : (jintArray)sl, (jintArray)st,
                          k == 3 ? NULL : (jintArray)dc, k == 4 ? NULL : (jintArray)first, k == 11 ? NULL : (jobject)dst, k == 5 ? NULL : (jlongArray)cdo,
                          k == 6 ? NULL : (jlongArray)ccap, (jintArray)pre, k == 8 ? NULL : (jintArray)ol, k == 9 ? NULL : (jlongArray)col, 1, 1);
    CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(ol) == -7 && g_alloc == 0);
    for (int t = 0; t < 10; t++) CHECK(all[t]->pins == 0);
  }
  fobj* hb = mk(5, 64);   /* a heap ByteBuffer where a direct one is required */
  CHECK(CHAIN(env, NULL, (jobject)hb, (jlongArray)so, (jintArray)sl, (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst, (jlongArray)cdo,
              (jlongArray)ccap, (jintArray)pre, (jintArray)ol, (jlongArray)col, 1, 1) == LZ4HIP_E_ARG);
  CHECK(CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst, (jlongArray)cdo,
              (jlongArray)ccap, (jintArray)pre, (jintArray)ol, (jlongArray)col, -1, 1) == LZ4HIP_E_ARG);
  /* chainFirst that does not end at the number of blocks; a history longer than the chain's offset: the library's own LZ4HIP_E_ARG */
  ((jint*)first->data)[1] = 2;
  CHECK(CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst, (jlongArray)cdo,
              (jlongArray)ccap, (jintArray)pre, (jintArray)ol, (jlongArray)col, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)first->data)[1] = 1;
  ((jint*)pre->data)[0] = 17;
  CHECK(CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst, (jlongArray)cdo,
              (jlongArray)ccap, (jintArray)pre, (jintArray)ol, (jlongArray)col, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)pre->data)[0] = 4;
  for (int t = 0; t < 10; t++) CHECK(all[t]->pins == 0);
  CHECK(g_alloc == 0 && get1(ol) == -7 && ((jlong*)col->data)[0] == 99);
  return 0;
}

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  (void)no_gpu_checks(env);
  if (arg_no_gpu(argc, argv)) {
    fobj* src = mk(4, 64); fobj* dst = mk(4, 64);
    src->data[0] = 0x10; src->data[1] = 'a';
    memset(dst->data, 7, 64);
    fobj* so = mk(3, 8); fobj* sl = int1(2); fobj* st = int1(0); fobj* dc = int1(8); fobj* first = mk(2, 8);
    fobj* cdo = mk(3, 8); fobj* ccap = mk(3, 8); fobj* pre = int1(4); fobj* ol = int1(-7); fobj* col = mk(3, 8);
    ((jint*)first->data)[1] = 1;
    ((jlong*)cdo->data)[0] = 16; ((jlong*)ccap->data)[0] = 8; ((jlong*)col->data)[0] = 99;
    for (int opt = 0; opt < 2; opt++) {   /* with and without the optional arrays */
      const jint rc = CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, opt ? NULL : (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst,
                            (jlongArray)cdo, (jlongArray)ccap, opt ? NULL : (jintArray)pre, (jintArray)ol, (jlongArray)col, 1, 1);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc() && get1(ol) == -7 && ((jlong*)col->data)[0] == 99 && g_alloc == 0);
      CHECK(so->pins == 0 && sl->pins == 0 && st->pins == 0 && dc->pins == 0 && first->pins == 0 && cdo->pins == 0 && ccap->pins == 0 && pre->pins == 0 &&
            ol->pins == 0 && col->pins == 0);
    }
    for (int i = 0; i < 64; i++) CHECK(dst->data[i] == 7);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_chain --no-gpu | <chain> <out-dir>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != NULL);
  fseek(f, 0, SEEK_END);
  const long total = ftell(f);
  fseek(f, 0, SEEK_SET);
  CHECK(total >= 16 && total < (1 << 26));
  uint8_t* in = (uint8_t*)malloc((size_t)total);
  CHECK(in != NULL && fread(in, 1, (size_t)total, f) == (size_t)total);
  fclose(f);
  uint32_t n, prefix; uint64_t cap64;
  memcpy(&n, in, 4); memcpy(&prefix, in + 4, 4); memcpy(&cap64, in + 8, 8);
  CHECK(n > 0 && n < 100000 && 16 + 12 * (size_t)n + prefix <= (size_t)total);
  const size_t GUARD = 32;
  fobj* so = mk(3, 8 * (size_t)n); fobj* sl = mk(2, 4 * (size_t)n); fobj* st = mk(2, 4 * (size_t)n); fobj* dc = mk(2, 4 * (size_t)n);
  fobj* ol = mk(2, 4 * (size_t)n); fobj* first = mk(2, 8); fobj* cdo = mk(3, 8); fobj* ccap = mk(3, 8); fobj* pre = int1((jint)prefix); fobj* col = mk(3, 8);
  size_t o = 0;
  int any_stored = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t len, raw; int32_t c;
    memcpy(&len, in + 16 + 12 * (size_t)i, 4); memcpy(&raw, in + 20 + 12 * (size_t)i, 4); memcpy(&c, in + 24 + 12 * (size_t)i, 4);
    ((jlong*)so->data)[i] = (jlong)o; ((jint*)sl->data)[i] = (jint)len; ((jint*)st->data)[i] = (jint)raw; ((jint*)dc->data)[i] = c; ((jint*)ol->data)[i] = -7;
    any_stored |= raw != 0;
    o += len;
  }
  const uint8_t* hist = in + 16 + 12 * (size_t)n;
  const uint8_t* streams = hist + prefix;
  CHECK((size_t)(streams - in) + o == (size_t)total);
  fobj* src = mk(4, o + 1); memcpy(src->data, streams, o);
  fobj* dst = mk(4, GUARD + prefix + (size_t)cap64 + GUARD);
  memset(dst->data, 0xEE, dst->bytes);
  memcpy(dst->data + GUARD, hist, prefix);
  ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = (jint)n;
  ((jlong*)cdo->data)[0] = (jlong)(GUARD + prefix); ((jlong*)ccap->data)[0] = (jlong)cap64; ((jlong*)col->data)[0] = -1;
  jint rc = CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)st, (jintArray)dc, (jintArray)first, (jobject)dst, (jlongArray)cdo,
                  (jlongArray)ccap, (jintArray)pre, (jintArray)ol, (jlongArray)col, (jint)n, 1);
  CHECK(rc == 0 && no_exc() && g_alloc == 0);
  CHECK(so->pins == 0 && sl->pins == 0 && st->pins == 0 && dc->pins == 0 && first->pins == 0 && cdo->pins == 0 && ccap->pins == 0 && pre->pins == 0 &&
        ol->pins == 0 && col->pins == 0);
  const uint64_t done = (uint64_t)((jlong*)col->data)[0];
  CHECK(done <= cap64);
  for (size_t i = 0; i < GUARD; i++) CHECK(dst->data[i] == 0xEE && dst->data[GUARD + prefix + (size_t)cap64 + i] == 0xEE);
  CHECK(memcmp(dst->data + GUARD, hist, prefix) == 0);
  for (size_t i = (size_t)done; i < (size_t)cap64; i++) CHECK(dst->data[GUARD + prefix + i] == 0xEE);
  FILE* t = out_file(argv[2], "chain.txt", "w");
  for (uint32_t i = 0; i < n; i++) fprintf(t, "%d ", (int)((jint*)ol->data)[i]);
  fprintf(t, "| %llu\n", (unsigned long long)done);
  fclose(t);
  write_bytes(argv[2], "chain.out", dst->data + GUARD + prefix, (size_t)done);
  if (!any_stored) {   /* stored == NULL: the same values and bytes */
    fobj* ol2 = mk(2, 4 * (size_t)n); fobj* dst2 = mk(4, dst->bytes);
    memset(dst2->data, 0xEE, dst2->bytes);
    memcpy(dst2->data + GUARD, hist, prefix);
    ((jlong*)col->data)[0] = -1;
    rc = CHAIN(env, NULL, (jobject)src, (jlongArray)so, (jintArray)sl, NULL, (jintArray)dc, (jintArray)first, (jobject)dst2, (jlongArray)cdo, (jlongArray)ccap,
               (jintArray)pre, (jintArray)ol2, (jlongArray)col, (jint)n, 1);
    CHECK(rc == 0 && no_exc() && g_alloc == 0 && (uint64_t)((jlong*)col->data)[0] == done);
    CHECK(memcmp(ol2->data, ol->data, 4 * (size_t)n) == 0 && memcmp(dst2->data, dst->data, dst->bytes) == 0);
  }
  free(in);
  return checks_ok(NULL);
}
