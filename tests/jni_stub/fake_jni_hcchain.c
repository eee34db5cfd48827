/* tests/jni_stub/fake_jni_hcchain.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The HC linked-block compress native of the JNI shim (LZ4HIPJNI.LZ4HIP_batchHCChain) executed without a JVM, with the fake JNIEnv of
 * fake_env.h (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is a pointer; the shim's malloc / free are
 * counted through shim_alloc.h).  Built (build_fake_jni of tests/support.py; the shared file reading, output files and closing line are
 * fake_env.h's) by tests/test_hcchain_abi.py / tests/test_gpu_hcchain.py.
 *
 *   fake_jni_hcchain --no-gpu          anywhere: NULL arrays and a bad chainFirst are argument errors, a well-formed call fails LOUDLY
 *                                      without a device (library status, nothing leaked or left pinned, nothing written)
 *   fake_jni_hcchain <chain> <out-dir> <level>
 *                                      on a GPU box: one chain through the native, with the prefix array and -- where the chain has no
 *                                      history -- without it.  <chain>: u32 n_blocks, u32 prefix_len, then per block {i32 src_len, i32
 *                                      dst_cap}, the history bytes, the source.  Writes "<out_len ...>" to <out-dir>/hcchain.txt and the
 *                                      bytes of the blocks that succeeded, back to back, to <out-dir>/hcchain.out (the test compares
 *                                      both with the reference's LZ4_compress_HC_continue); prints "fake_jni_hcchain: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_hcchain"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCChain(JNIEnv*, jclass, jobject, jlongArray, jintArray, jintArray, jintArray, jobject,
    jlongArray, jintArray, jintArray, jint, jint, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define HCCHAIN Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCChain

/* one well-formed call: one chain of one block of 4 bytes behind 4 bytes of history */
typedef struct { fobj *src, *dst, *cso, *pre, *sl, *first, *doff, *dc, *ol; } call_t;
static call_t one_call(void) {
  call_t c;
  c.src = mk(4, 64); c.dst = mk(4, 64);
  memcpy(c.src->data, "0123abcd", 8);
  memset(c.dst->data, 7, 64);
  c.cso = mk(3, 8); c.pre = int1(4); c.sl = int1(4); c.first = mk(2, 8); c.doff = mk(3, 8); c.dc = int1(20); c.ol = int1(-7);
  ((jlong*)c.cso->data)[0] = 4; ((jint*)c.first->data)[1] = 1; ((jlong*)c.doff->data)[0] = 8;
  return c;
}
static int unpinned(const call_t* c) {
  return c->cso->pins == 0 && c->pre->pins == 0 && c->sl->pins == 0 && c->first->pins == 0 && c->doff->pins == 0 && c->dc->pins == 0 && c->ol->pins == 0;
}

static int no_gpu_checks(JNIEnv* env) {
  call_t c = one_call();
  /* every required argument NULL in turn: LZ4HIP_E_ARG, nothing pinned (the prefix array is optional: tested below) */
  for (int k = 0; k < 8; k++) {
    const jint rc = HCCHAIN(env, NULL, k == 0 ? NULL : (jobject)c.src, k == 1 ? NULL : (jlongArray)c.cso, (jintArray)c.pre, k == 2 ? NULL : (jintArray)c.sl,
                           k == 3 ? NULL : (jintArray)c.first, k == 4 ? NULL : (jobject)c.dst, k == 5 ? NULL : (jlongArray)c.doff, k == 6 ? NULL : (jintArray)c.dc,
                           k == 7 ? NULL : (jintArray)c.ol, 1, 1, 9);
    CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(c.ol) == -7 && g_alloc == 0);
    CHECK(unpinned(&c));
  }
  fobj* hb = mk(5, 64);   /* a heap ByteBuffer where a direct one is required */
  CHECK(HCCHAIN(env, NULL, (jobject)hb, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst, (jlongArray)c.doff,
               (jintArray)c.dc, (jintArray)c.ol, 1, 1, 9) == LZ4HIP_E_ARG);
  CHECK(HCCHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst, (jlongArray)c.doff,
               (jintArray)c.dc, (jintArray)c.ol, -1, 1, 9) == LZ4HIP_E_ARG);
  /* chainFirst that does not end at the number of blocks; a history longer than the chain's offset: the library's own LZ4HIP_E_ARG */
  ((jint*)c.first->data)[1] = 2;
  CHECK(HCCHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst, (jlongArray)c.doff,
               (jintArray)c.dc, (jintArray)c.ol, 1, 1, 9) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 1;
  ((jint*)c.pre->data)[0] = 5;
  CHECK(HCCHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst, (jlongArray)c.doff,
               (jintArray)c.dc, (jintArray)c.ol, 1, 1, 9) == LZ4HIP_E_ARG);
  CHECK(unpinned(&c));
  CHECK(g_alloc == 0 && get1(c.ol) == -7);
  return 0;
}

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  (void)no_gpu_checks(env);
  if (arg_no_gpu(argc, argv)) {
    call_t c = one_call();
    for (int opt = 0; opt < 2; opt++) {   /* with and without the optional array */
      if (opt) ((jlong*)c.cso->data)[0] = 0;
      const jint rc = HCCHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, opt ? NULL : (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst,
                             (jlongArray)c.doff, (jintArray)c.dc, (jintArray)c.ol, 1, 1, opt ? 13 : 0);   /* (levels are clamped, never refused) */
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc() && get1(c.ol) == -7 && g_alloc == 0);
      CHECK(unpinned(&c));
    }
    for (int i = 0; i < 64; i++) CHECK(c.dst->data[i] == 7);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 4) { fprintf(stderr, "usage: fake_jni_hcchain --no-gpu | <chain> <out-dir> <level>\n"); return 2; }
  const jint level = (jint)atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != NULL);
  fseek(f, 0, SEEK_END);
  const long total = ftell(f);
  fseek(f, 0, SEEK_SET);
  CHECK(total >= 8 && total < (1 << 26));
  uint8_t* in = (uint8_t*)malloc((size_t)total);
  CHECK(in != NULL && fread(in, 1, (size_t)total, f) == (size_t)total);
  fclose(f);
  uint32_t n, prefix;
  memcpy(&n, in, 4); memcpy(&prefix, in + 4, 4);
  CHECK(n > 0 && n < 100000 && 8 + 8 * (size_t)n + prefix <= (size_t)total);
  const size_t GUARD = 32;
  fobj* sl = mk(2, 4 * (size_t)n); fobj* dc = mk(2, 4 * (size_t)n); fobj* doff = mk(3, 8 * (size_t)n); fobj* ol = mk(2, 4 * (size_t)n);
  fobj* first = mk(2, 8); fobj* cso = mk(3, 8); fobj* pre = int1((jint)prefix);
  size_t bytes = 0, room = GUARD;
  for (uint32_t i = 0; i < n; i++) {
    int32_t len, c;
    memcpy(&len, in + 8 + 8 * (size_t)i, 4); memcpy(&c, in + 12 + 8 * (size_t)i, 4);
    CHECK(len >= 0 && c >= 0);
    ((jint*)sl->data)[i] = len; ((jint*)dc->data)[i] = c; ((jlong*)doff->data)[i] = (jlong)room; ((jint*)ol->data)[i] = -7;
    bytes += (size_t)len; room += (size_t)c + GUARD;
  }
  const uint8_t* hist = in + 8 + 8 * (size_t)n;
  CHECK((size_t)(hist - in) + prefix + bytes == (size_t)total);
  fobj* src = mk(4, GUARD + prefix + bytes + GUARD);
  memset(src->data, 0xA5, src->bytes);
  memcpy(src->data + GUARD, hist, prefix + bytes);
  fobj* dst = mk(4, room);
  memset(dst->data, 0xEE, dst->bytes);
  ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = (jint)n;
  ((jlong*)cso->data)[0] = (jlong)(GUARD + prefix);
  jint rc = HCCHAIN(env, NULL, (jobject)src, (jlongArray)cso, (jintArray)pre, (jintArray)sl, (jintArray)first, (jobject)dst, (jlongArray)doff, (jintArray)dc,
                   (jintArray)ol, (jint)n, 1, level);
  CHECK(rc == 0 && no_exc() && g_alloc == 0);
  CHECK(sl->pins == 0 && dc->pins == 0 && doff->pins == 0 && ol->pins == 0 && first->pins == 0 && cso->pins == 0 && pre->pins == 0);
  FILE* t = out_file(argv[2], "hcchain.txt", "w");
  FILE* o = out_file(argv[2], "hcchain.out", "wb");
  size_t at = 0;   /* every byte of dst is a guard, a block's result, or untouched */
  for (uint32_t i = 0; i < n; i++) {
    const jint r = ((jint*)ol->data)[i];
    const size_t off = (size_t)((jlong*)doff->data)[i], cap = (size_t)((jint*)dc->data)[i], got = r > 0 ? (size_t)r : 0;
    CHECK(got <= cap);
    for (; at < off; at++) CHECK(dst->data[at] == 0xEE);
    for (size_t k = got; k < cap; k++) CHECK(dst->data[off + k] == 0xEE);
    at = off + cap;
    fprintf(t, "%d ", (int)r);
    CHECK(fwrite(dst->data + off, 1, got, o) == got);
  }
  for (; at < dst->bytes; at++) CHECK(dst->data[at] == 0xEE);
  fprintf(t, "\n");
  fclose(t);
  fclose(o);
  if (prefix == 0) {   /* chainPrefixLen == NULL: the same values and bytes */
    fobj* ol2 = mk(2, 4 * (size_t)n); fobj* dst2 = mk(4, dst->bytes);
    memset(dst2->data, 0xEE, dst2->bytes);
    rc = HCCHAIN(env, NULL, (jobject)src, (jlongArray)cso, NULL, (jintArray)sl, (jintArray)first, (jobject)dst2, (jlongArray)doff, (jintArray)dc, (jintArray)ol2,
                (jint)n, 1, level);
    CHECK(rc == 0 && no_exc() && g_alloc == 0);
    CHECK(memcmp(ol2->data, ol->data, 4 * (size_t)n) == 0 && memcmp(dst2->data, dst->data, dst->bytes) == 0);
  }
  free(in);
  return checks_ok(NULL);
}
