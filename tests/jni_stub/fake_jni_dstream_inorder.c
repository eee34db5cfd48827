/* tests/jni_stub/fake_jni_dstream_inorder.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The in-order stream-decode native of the JNI shim (LZ4HIPJNI.LZ4HIP_batchSafeStreamInOrder) and LZ4HIP_decoderRingBufferSize executed
 * without a JVM, with the fake JNIEnv of fake_env.h, as fake_jni_dstream.c executes LZ4HIP_batchSafeStream.  Built (build_fake_jni of
 * tests/support.py) by tests/test_dstream_inorder_abi.py / tests/test_gpu_dstream_inorder.py.
 *
 *   fake_jni_dstream_inorder --no-gpu          anywhere: the ring sizes; NULL arrays, a bad chainFirst, a slot outside its window and a
 *                                              straddling history are argument errors; a well-formed call fails LOUDLY without a device
 *                                              (library status, nothing leaked or left pinned, nothing written, the state as it was)
 *   fake_jni_dstream_inorder <stream> <out>    on a GPU box: one stream through the native, call after call, the calls alternating with
 *                                              LZ4HIP_batchSafeStream where <stream>'s name ends in ".alt" (a stream none of whose
 *                                              slots overlaps).  <stream>: the file tests/cpp/dstream_mirror_test.cpp describes (no
 *                                              dictionary).  Prints the out_len values, then "prefix_end prefix_len ext_end ext_len"
 *                                              behind the last call (ends relative to the window), then "... checks ok"; writes the
 *                                              window to <out>
 */
#define FAKE_JNI_NAME "fake_jni_dstream_inorder"
#include "fake_env.h"

typedef jint (JNICALL *stream_fn)(JNIEnv*, jclass, jlongArray, jobject, jlongArray, jintArray, jintArray, jobject, jlongArray, jintArray, jlongArray, jlongArray,
                                  jintArray, jint, jint);
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStream(JNIEnv*, jclass, jlongArray, jobject, jlongArray, jintArray, jintArray, jobject,
    jlongArray, jintArray, jlongArray, jlongArray, jintArray, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStreamInOrder(JNIEnv*, jclass, jlongArray, jobject, jlongArray, jintArray, jintArray, jobject,
    jlongArray, jintArray, jlongArray, jlongArray, jintArray, jint, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decoderRingBufferSize(JNIEnv*, jclass, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define INORDER Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStreamInOrder
#define PLAIN Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchSafeStream
#define RING Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1decoderRingBufferSize

typedef struct { fobj *state, *src, *so, *sl, *first, *dst, *dof, *dc, *wo, *wl, *ol; } call_t;

/* one stream, one block of two literals to dst[16, 24), window dst[8, 40), behind a prefix of 4 bytes that ends at 16 */
static call_t small_call(void) {
  call_t c = {mk(3, 32), mk(4, 64), mk(3, 8), int1(3), mk(2, 8), mk(4, 64), mk(3, 8), int1(8), mk(3, 8), mk(3, 8), int1(-7)};
  c.src->data[0] = 0x20; c.src->data[1] = 'a'; c.src->data[2] = 'b';
  memset(c.dst->data, 7, 64);
  ((jlong*)c.state->data)[0] = 16; ((jlong*)c.state->data)[1] = 4;
  ((jint*)c.first->data)[1] = 1;
  ((jlong*)c.dof->data)[0] = 16; ((jlong*)c.wo->data)[0] = 8; ((jlong*)c.wl->data)[0] = 32;
  return c;
}
static jint run(JNIEnv* env, const call_t* c, int null_at, jint nb, jint nc) {
  return INORDER(env, NULL, null_at == 0 ? NULL : (jlongArray)c->state, null_at == 1 ? NULL : (jobject)c->src, null_at == 2 ? NULL : (jlongArray)c->so,
                 null_at == 3 ? NULL : (jintArray)c->sl, null_at == 4 ? NULL : (jintArray)c->first, null_at == 5 ? NULL : (jobject)c->dst,
                 null_at == 6 ? NULL : (jlongArray)c->dof, null_at == 7 ? NULL : (jintArray)c->dc, null_at == 8 ? NULL : (jlongArray)c->wo,
                 null_at == 9 ? NULL : (jlongArray)c->wl, null_at == 10 ? NULL : (jintArray)c->ol, nb, nc);
}
static void nothing_pinned_or_written(const call_t* c) {
  const fobj* all[9] = {c->state, c->so, c->sl, c->first, c->dof, c->dc, c->wo, c->wl, c->ol};
  for (int t = 0; t < 9; t++) CHECK(all[t]->pins == 0);
  CHECK(g_alloc == 0 && no_exc() && get1(c->ol) == -7);
  for (int i = 0; i < 64; i++) CHECK(c->dst->data[i] == 7);
}

static void no_gpu_checks(JNIEnv* env) {
  CHECK(RING(env, NULL, -1) == 0 && RING(env, NULL, 0) == 65536 + 14 + 16 && RING(env, NULL, 16) == 65536 + 14 + 16 && RING(env, NULL, 17) == 65536 + 14 + 17);
  CHECK(RING(env, NULL, 4096) == 65536 + 14 + 4096 && RING(env, NULL, 0x7E000000) == 65536 + 14 + 0x7E000000 && RING(env, NULL, 0x7E000001) == 0);
  call_t c = small_call();
  for (int k = 0; k <= 10; k++) {   /* every argument NULL in turn */
    CHECK(run(env, &c, k, 1, 1) == LZ4HIP_E_ARG);
    nothing_pinned_or_written(&c);
  }
  CHECK(run(env, &c, -1, -1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 2;                     /* chainFirst does not end at the number of blocks */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 1;
  ((jlong*)c.dof->data)[0] = 36;                     /* the slot leaves its window */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.dof->data)[0] = 16;
  ((jlong*)c.state->data)[0] = 10;                   /* the prefix [6, 10) straddles the window's start */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.state->data)[0] = 3;                    /* a history longer than its end offset */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.state->data)[0] = 16;
  nothing_pinned_or_written(&c);
}

static int64_t rd(const uint8_t* in, size_t* p) { int64_t v; memcpy(&v, in + *p, 8); *p += 8; return v; }

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  no_gpu_checks(env);
  if (arg_no_gpu(argc, argv)) {
    call_t c = small_call();
    CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_NO_DEVICE);
    nothing_pinned_or_written(&c);
    CHECK(((jlong*)c.state->data)[0] == 16 && ((jlong*)c.state->data)[1] == 4 && ((jlong*)c.state->data)[3] == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("the compute call failed loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_dstream_inorder --no-gpu | <stream> <out>\n"); return 2; }
  const size_t nl = strlen(argv[1]);
  const int alternate = nl > 4 && strcmp(argv[1] + nl - 4, ".alt") == 0;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != NULL);
  fseek(f, 0, SEEK_END);
  const long total = ftell(f);
  fseek(f, 0, SEEK_SET);
  CHECK(total >= 72 && total < (1 << 26));
  uint8_t* in = (uint8_t*)malloc((size_t)total);
  CHECK(in != NULL && fread(in, 1, (size_t)total, f) == (size_t)total);
  fclose(f);
  size_t p = 0;
  const int64_t win_len = rd(in, &p), dict_len = rd(in, &p), lead = rd(in, &p), n = rd(in, &p), calls = rd(in, &p);
  int64_t st[4];
  for (int k = 0; k < 4; k++) st[k] = rd(in, &p);
  CHECK(n >= 0 && n < 100000 && calls > 0 && calls <= n + 1 && win_len >= 0 && dict_len == 0 && lead == 0 && st[1] == 0);
  const size_t cuts_at = p, blocks_at = p + 8 * (size_t)calls, src_at = blocks_at + 24 * (size_t)n;
  CHECK(src_at <= (size_t)total);
  const size_t GUARD = 128, win = GUARD;
  fobj* dst = mk(4, win + (size_t)win_len + GUARD);
  memset(dst->data, 0xEE, dst->bytes);
  fobj* src = mk(4, (size_t)total - src_at + 1);
  memcpy(src->data, in + src_at, (size_t)total - src_at);
  fobj* state = mk(3, 32);
  fobj* wo = mk(3, 8); fobj* wl = mk(3, 8); fobj* first = mk(2, 8);
  int64_t k = 0, so_run = 0;
  for (int64_t ci = 0; ci < calls; ci++) {
    p = cuts_at + 8 * (size_t)ci;
    const int64_t cut = rd(in, &p), nb = cut - k;
    CHECK(nb >= 0 && cut <= n);
    fobj* so = mk(3, 8 * (size_t)nb); fobj* sl = mk(2, 4 * (size_t)nb); fobj* dof = mk(3, 8 * (size_t)nb); fobj* dc = mk(2, 4 * (size_t)nb); fobj* ol = mk(2, 4 * (size_t)nb);
    for (int64_t i = 0; i < nb; i++) {
      p = blocks_at + 24 * (size_t)(k + i);
      const int64_t off = rd(in, &p), cap = rd(in, &p), len = rd(in, &p);
      ((jlong*)so->data)[i] = so_run; ((jint*)sl->data)[i] = (jint)len; ((jlong*)dof->data)[i] = (jlong)win + off; ((jint*)dc->data)[i] = (jint)cap;
      ((jint*)ol->data)[i] = -7;
      so_run += len;
    }
    ((jlong*)wo->data)[0] = (jlong)win; ((jlong*)wl->data)[0] = (jlong)win_len;
    ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = (jint)nb;
    const stream_fn fn = (alternate && (ci & 1)) ? PLAIN : INORDER;
    const jint rc = fn(env, NULL, (jlongArray)state, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)first, (jobject)dst, (jlongArray)dof,
                       (jintArray)dc, (jlongArray)wo, (jlongArray)wl, (jintArray)ol, (jint)nb, 1);
    CHECK(rc == 0 && no_exc() && g_alloc == 0);
    CHECK(state->pins == 0 && so->pins == 0 && sl->pins == 0 && first->pins == 0 && dof->pins == 0 && dc->pins == 0 && wo->pins == 0 && wl->pins == 0 && ol->pins == 0);
    for (int64_t i = 0; i < nb; i++) printf("%d ", (int)((jint*)ol->data)[i]);
    k = cut;
  }
  const jlong* s = (const jlong*)state->data;
  printf("\n%lld %lld %lld %lld\n", (long long)s[0] - (long long)win, (long long)s[1], (long long)s[2] - (long long)win, (long long)s[3]);
  for (size_t i = 0; i < GUARD; i++) CHECK(dst->data[i] == 0xEE && dst->data[win + (size_t)win_len + i] == 0xEE);
  FILE* o = fopen(argv[2], "wb");
  CHECK(o != NULL && fwrite(dst->data + win, 1, (size_t)win_len, o) == (size_t)win_len);
  fclose(o);
  free(in);
  return checks_ok(NULL);
}
