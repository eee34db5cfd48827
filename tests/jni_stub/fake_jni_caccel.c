/* tests/jni_stub/fake_jni_caccel.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The accelerated linked-block natives of the JNI shim (LZ4HIPJNI.LZ4HIP_batchFastChainAccel, LZ4HIP_batchFastStreamAccel,
 * LZ4HIP_batchFastStreamAtAccel) executed without a JVM, with the fake JNIEnv of fake_env.h.  Built (build_fake_jni of tests/support.py)
 * by tests/test_caccel_abi.py / tests/test_gpu_caccel.py.
 *
 *   fake_jni_caccel --no-gpu                          anywhere: NULL arrays are argument errors, a 0 handle is one, a well-formed chain
 *                                                     call fails LOUDLY without a device (nothing leaked or left pinned, nothing written)
 *   fake_jni_caccel <chain> <out-dir> <acceleration>  on a GPU box: one chain through the chain native at the acceleration, then the same
 *                                                     blocks through the two stream natives on a set of two streams; all three agree.
 *                                                     <chain>: u32 n_blocks, u32 prefix_len, per block {i32 src_len, i32 dst_cap}, the
 *                                                     history, the source.  Writes "<out_len ...> | <chain_consumed>" to
 *                                                     <out-dir>/caccel.txt and the blocks' bytes to <out-dir>/caccel.out
 */
#define FAKE_JNI_NAME "fake_jni_caccel"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastChainAccel(JNIEnv*, jclass, jobject, jlongArray, jintArray, jintArray, jintArray, jobject,
    jlongArray, jintArray, jintArray, jlongArray, jint, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAccel(JNIEnv*, jclass, jlong, jintArray, jobject, jlongArray, jintArray, jintArray,
    jintArray, jobject, jlongArray, jintArray, jintArray, jlongArray, jint, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAtAccel(JNIEnv*, jclass, jlong, jintArray, jobject, jlongArray, jintArray, jintArray,
    jlongArray, jintArray, jlongArray, jlongArray, jobject, jlongArray, jintArray, jintArray, jlongArray, jint, jint, jint);
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate(JNIEnv*, jclass, jint);
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree(JNIEnv*, jclass, jlong);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define CHAIN Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastChainAccel
#define STREAM Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAccel
#define STREAM_AT Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAtAccel

/* one well-formed call: one chain of one block of 4 bytes behind 4 bytes of history */
typedef struct { fobj *src, *dst, *cso, *pre, *sl, *first, *doff, *dc, *ol, *cons, *ids; } call_t;
static call_t one_call(void) {
  call_t c;
  c.src = mk(4, 64); c.dst = mk(4, 64);
  memcpy(c.src->data, "0123abcd", 8);
  memset(c.dst->data, 7, 64);
  c.cso = mk(3, 8); c.pre = int1(4); c.sl = int1(4); c.first = mk(2, 8); c.doff = mk(3, 8); c.dc = int1(20); c.ol = int1(-7); c.cons = mk(3, 8); c.ids = int1(0);
  ((jlong*)c.cso->data)[0] = 4; ((jint*)c.first->data)[1] = 1; ((jlong*)c.doff->data)[0] = 8; ((jlong*)c.cons->data)[0] = 99;
  return c;
}
static int unpinned(const call_t* c) {
  return c->cso->pins == 0 && c->pre->pins == 0 && c->sl->pins == 0 && c->first->pins == 0 && c->doff->pins == 0 && c->dc->pins == 0 && c->ol->pins == 0 &&
         c->cons->pins == 0 && c->ids->pins == 0;
}

static int no_gpu_checks(JNIEnv* env) {
  call_t c = one_call();
  for (int k = 0; k < 9; k++) {   /* every required argument NULL in turn: LZ4HIP_E_ARG, nothing pinned */
    const jint rc = CHAIN(env, NULL, k == 0 ? NULL : (jobject)c.src, k == 1 ? NULL : (jlongArray)c.cso, (jintArray)c.pre, k == 2 ? NULL : (jintArray)c.sl,
                          k == 3 ? NULL : (jintArray)c.first, k == 4 ? NULL : (jobject)c.dst, k == 5 ? NULL : (jlongArray)c.doff, k == 6 ? NULL : (jintArray)c.dc,
                          k == 7 ? NULL : (jintArray)c.ol, k == 8 ? NULL : (jlongArray)c.cons, 1, 1, 8);
    CHECK(rc == LZ4HIP_E_ARG && no_exc() && get1(c.ol) == -7 && g_alloc == 0);
    CHECK(unpinned(&c));
  }
  CHECK(CHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst, (jlongArray)c.doff,
              (jintArray)c.dc, (jintArray)c.ol, (jlongArray)c.cons, -1, 1, 8) == LZ4HIP_E_ARG);
  /* a 0 handle: LZ4HIP_E_ARG from both stream natives, at any acceleration */
  CHECK(STREAM(env, NULL, 0, (jintArray)c.ids, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst,
               (jlongArray)c.doff, (jintArray)c.dc, (jintArray)c.ol, (jlongArray)c.cons, 1, 1, 8) == LZ4HIP_E_ARG);
  CHECK(STREAM_AT(env, NULL, 0, (jintArray)c.ids, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.sl, (jintArray)c.first, (jlongArray)c.cso, (jintArray)c.pre,
                  (jlongArray)c.doff, (jlongArray)c.cons, (jobject)c.dst, (jlongArray)c.doff, (jintArray)c.dc, (jintArray)c.ol, (jlongArray)c.cons, 1, 1, 8) ==
        LZ4HIP_E_ARG);
  CHECK(unpinned(&c));
  CHECK(g_alloc == 0 && get1(c.ol) == -7 && ((jlong*)c.cons->data)[0] == 99);
  return 0;
}

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  (void)no_gpu_checks(env);
  if (arg_no_gpu(argc, argv)) {
    call_t c = one_call();
    for (int a = 0; a < 3; a++) {   /* clamped to 1, 8, clamped to 65537: the same loud failure */
      const jint rc = CHAIN(env, NULL, (jobject)c.src, (jlongArray)c.cso, (jintArray)c.pre, (jintArray)c.sl, (jintArray)c.first, (jobject)c.dst,
                            (jlongArray)c.doff, (jintArray)c.dc, (jintArray)c.ol, (jlongArray)c.cons, 1, 1, a == 0 ? 0 : a == 1 ? 8 : 70000);
      CHECK(rc == LZ4HIP_E_NO_DEVICE && no_exc() && get1(c.ol) == -7 && ((jlong*)c.cons->data)[0] == 99 && g_alloc == 0);
      CHECK(unpinned(&c));
    }
    for (int i = 0; i < 64; i++) CHECK(c.dst->data[i] == 7);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("every compute call failed loudly");
  }
  if (argc < 4) { fprintf(stderr, "usage: fake_jni_caccel --no-gpu | <chain> <out-dir> <acceleration>\n"); return 2; }
  const jint accel = (jint)atoi(argv[3]);
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
  fobj* sl = mk(2, 4 * (size_t)n); fobj* dc = mk(2, 4 * (size_t)n); fobj* doff = mk(3, 8 * (size_t)n); fobj* soff = mk(3, 8 * (size_t)n);
  fobj* first = mk(2, 8); fobj* cso = mk(3, 8); fobj* pre = int1((jint)prefix); fobj* cons = mk(3, 8); fobj* ids = int1(1);
  fobj* win_off = mk(3, 8); fobj* win_len = mk(3, 8);
  size_t bytes = 0, room = GUARD;
  for (uint32_t i = 0; i < n; i++) {
    int32_t len, c;
    memcpy(&len, in + 8 + 8 * (size_t)i, 4); memcpy(&c, in + 12 + 8 * (size_t)i, 4);
    CHECK(len >= 0 && c >= 0);
    ((jint*)sl->data)[i] = len; ((jint*)dc->data)[i] = c; ((jlong*)doff->data)[i] = (jlong)room;
    ((jlong*)soff->data)[i] = (jlong)(GUARD + prefix + bytes);
    bytes += (size_t)len; room += (size_t)c + GUARD;
  }
  const uint8_t* hist = in + 8 + 8 * (size_t)n;
  CHECK((size_t)(hist - in) + prefix + bytes == (size_t)total);
  fobj* src = mk(4, GUARD + prefix + bytes + GUARD);
  memset(src->data, 0xA5, src->bytes);
  memcpy(src->data + GUARD, hist, prefix + bytes);
  ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = (jint)n;
  ((jlong*)cso->data)[0] = (jlong)(GUARD + prefix);
  ((jlong*)win_off->data)[0] = 0; ((jlong*)win_len->data)[0] = (jlong)src->bytes;
  fobj* dst[3]; fobj* ol[3];
  uint64_t done[3];
  const jlong set = Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate(env, NULL, 2);
  CHECK(set != 0);
  for (int k = 0; k < 3; k++) {
    dst[k] = mk(4, room); ol[k] = mk(2, 4 * (size_t)n);
    memset(dst[k]->data, 0xEE, dst[k]->bytes);
    for (uint32_t i = 0; i < n; i++) ((jint*)ol[k]->data)[i] = -7;
    ((jlong*)cons->data)[0] = -1;
    ((jint*)ids->data)[0] = k == 1 ? 1 : 0;
    jint rc;
    if (k == 0)
      rc = CHAIN(env, NULL, (jobject)src, (jlongArray)cso, (jintArray)pre, (jintArray)sl, (jintArray)first, (jobject)dst[k], (jlongArray)doff, (jintArray)dc,
                 (jintArray)ol[k], (jlongArray)cons, (jint)n, 1, accel);
    else if (k == 1)
      rc = STREAM(env, NULL, set, (jintArray)ids, (jobject)src, (jlongArray)cso, (jintArray)pre, (jintArray)sl, (jintArray)first, (jobject)dst[k],
                  (jlongArray)doff, (jintArray)dc, (jintArray)ol[k], (jlongArray)cons, (jint)n, 1, accel);
    else
      rc = STREAM_AT(env, NULL, set, (jintArray)ids, (jobject)src, (jlongArray)soff, (jintArray)sl, (jintArray)first, (jlongArray)cso, (jintArray)pre,
                     (jlongArray)win_off, (jlongArray)win_len, (jobject)dst[k], (jlongArray)doff, (jintArray)dc, (jintArray)ol[k], (jlongArray)cons, (jint)n, 1,
                     accel);
    CHECK(rc == 0 && no_exc() && g_alloc == 0);
    CHECK(sl->pins == 0 && dc->pins == 0 && doff->pins == 0 && soff->pins == 0 && ol[k]->pins == 0 && first->pins == 0 && cso->pins == 0 && pre->pins == 0 &&
          cons->pins == 0 && ids->pins == 0 && win_off->pins == 0 && win_len->pins == 0);
    done[k] = (uint64_t)((jlong*)cons->data)[0];
    if (k) CHECK(done[k] == done[0] && memcmp(ol[k]->data, ol[0]->data, 4 * (size_t)n) == 0 && memcmp(dst[k]->data, dst[0]->data, room) == 0);
  }
  Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree(env, NULL, set);
  CHECK(done[0] <= bytes);
  FILE* t = out_file(argv[2], "caccel.txt", "w");
  FILE* o = out_file(argv[2], "caccel.out", "wb");
  size_t at = 0;   /* every byte of dst is a guard, a block's result, or untouched */
  for (uint32_t i = 0; i < n; i++) {
    const jint r = ((jint*)ol[0]->data)[i];
    const size_t off = (size_t)((jlong*)doff->data)[i], cap = (size_t)((jint*)dc->data)[i], got = r > 0 ? (size_t)r : 0;
    CHECK(got <= cap);
    for (; at < off; at++) CHECK(dst[0]->data[at] == 0xEE);
    for (size_t k = got; k < cap; k++) CHECK(dst[0]->data[off + k] == 0xEE);
    at = off + cap;
    fprintf(t, "%d ", (int)r);
    CHECK(fwrite(dst[0]->data + off, 1, got, o) == got);
  }
  for (; at < dst[0]->bytes; at++) CHECK(dst[0]->data[at] == 0xEE);
  fprintf(t, "| %llu\n", (unsigned long long)done[0]);
  fclose(t);
  fclose(o);
  free(in);
  return checks_ok(NULL);
}
