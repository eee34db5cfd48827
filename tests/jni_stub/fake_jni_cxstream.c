/* tests/jni_stub/fake_jni_cxstream.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The native of the JNI shim for resident streams whose sources land anywhere (LZ4HIPJNI.LZ4HIP_batchFastStreamAt) executed without a
 * JVM, with the fake JNIEnv of fake_env.h (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is a pointer;
 * the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of tests/support.py) by tests/test_cxstream_abi.py /
 * tests/test_gpu_cxstream.py.
 *
 *   fake_jni_cxstream --no-gpu            anywhere: a 0 handle and negative counts are argument errors, nothing pinned; without a device
 *                                         no set can be made and the failure is LOUD (handle 0, the library's message), nothing leaked
 *   fake_jni_cxstream <stream> <out-dir>  on a GPU box: one stream through stream 1 of a set of three, call after call, the producer
 *                                         writing each call's blocks into the window first.  <stream>: i64 win_len, n_blocks, n_calls;
 *                                         per call {i64 end block, hist_end (relative to the window), hist_len}; per block {i64 off,
 *                                         len, cap}; the blocks' bytes.  Writes the out_len values to <out-dir>/cxstream.txt and the
 *                                         bytes of the blocks that succeeded, back to back, to <out-dir>/cxstream.out (the test compares
 *                                         both with ONE LZ4_stream_t of the reference); checks the argument errors with a live set;
 *                                         prints "fake_jni_cxstream: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_cxstream"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate(JNIEnv*, jclass, jint);
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree(JNIEnv*, jclass, jlong);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAt(JNIEnv*, jclass, jlong, jintArray, jobject, jlongArray, jintArray, jintArray,
    jlongArray, jintArray, jlongArray, jlongArray, jobject, jlongArray, jintArray, jintArray, jlongArray, jint, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define CREATE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate
#define FREE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree
#define AT Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStreamAt

/* one well-formed call apart from its set: stream 0, one block of 4 bytes at src[20, 24) in the window src[8, 40), behind a history of
 * 4 bytes that ends at 16 */
typedef struct { fobj *id, *src, *so, *sl, *first, *he, *hl, *wo, *wl, *dst, *doff, *dc, *ol, *cons; } call_t;
#define N_ARGS 14
static call_t one_call(void) {
  call_t c;
  c.src = mk(4, 64); c.dst = mk(4, 64);
  memcpy(c.src->data + 12, "0123", 4); memcpy(c.src->data + 20, "abcd", 4);
  memset(c.dst->data, 7, 64);
  c.id = int1(0); c.so = mk(3, 8); c.sl = int1(4); c.first = mk(2, 8); c.he = mk(3, 8); c.hl = int1(4); c.wo = mk(3, 8); c.wl = mk(3, 8);
  c.doff = mk(3, 8); c.dc = int1(20); c.ol = int1(-7); c.cons = mk(3, 8);
  ((jlong*)c.so->data)[0] = 20; ((jint*)c.first->data)[1] = 1; ((jlong*)c.he->data)[0] = 16; ((jlong*)c.wo->data)[0] = 8; ((jlong*)c.wl->data)[0] = 32;
  ((jlong*)c.doff->data)[0] = 8; ((jlong*)c.cons->data)[0] = 99;
  return c;
}
static int unpinned(const call_t* c) {
  const fobj* all[12] = {c->id, c->so, c->sl, c->first, c->he, c->hl, c->wo, c->wl, c->doff, c->dc, c->ol, c->cons};
  for (int t = 0; t < 12; t++) if (all[t] && all[t]->pins != 0) return 0;
  return 1;
}
static jint call(JNIEnv* env, jlong set, const call_t* c, jint nb, jint nc) {
  return AT(env, NULL, set, (jintArray)c->id, (jobject)c->src, (jlongArray)c->so, (jintArray)c->sl, (jintArray)c->first, (jlongArray)c->he, (jintArray)c->hl,
            (jlongArray)c->wo, (jlongArray)c->wl, (jobject)c->dst, (jlongArray)c->doff, (jintArray)c->dc, (jintArray)c->ol, (jlongArray)c->cons, nb, nc);
}
static int untouched(const call_t* c) {
  for (int i = 0; i < 64; i++) if (c->dst->data[i] != 7) return 0;
  return get1(c->ol) == -7 && ((jlong*)c->cons->data)[0] == 99;
}

/* with a live set: every argument error of the native and of the library behind it, nothing pinned, written or consumed */
static void set_checks(JNIEnv* env, jlong set) {
  call_t c = one_call();
  for (int k = 0; k < N_ARGS; k++) {   /* every argument NULL in turn: all are required */
    call_t d = c;
    fobj** f[N_ARGS] = {&d.id, &d.src, &d.so, &d.sl, &d.first, &d.he, &d.hl, &d.wo, &d.wl, &d.dst, &d.doff, &d.dc, &d.ol, &d.cons};
    *f[k] = NULL;
    CHECK(call(env, set, &d, 1, 1) == LZ4HIP_E_ARG && no_exc() && g_alloc == 0);
    CHECK(unpinned(&c) && untouched(&c));
  }
  CHECK(call(env, set, &c, -1, 1) == LZ4HIP_E_ARG && call(env, set, &c, 1, -1) == LZ4HIP_E_ARG);
  ((jint*)c.id->data)[0] = 3;                      /* three streams exist */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.id->data)[0] = 0;
  ((jint*)c.first->data)[1] = 2;                   /* chainFirst does not end at the number of blocks */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 1;
  ((jlong*)c.so->data)[0] = 38;                    /* the source leaves its window */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.so->data)[0] = 20;
  ((jlong*)c.he->data)[0] = 10;                    /* the history [6, 10) straddles the window's start */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.he->data)[0] = 3;                     /* a history longer than its end offset */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jlong*)c.he->data)[0] = 16;
  ((jint*)c.hl->data)[0] = -1;                     /* a negative history length */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  CHECK(unpinned(&c) && untouched(&c) && g_alloc == 0);
}

static int64_t rd(const uint8_t* in, size_t* p) { int64_t v; memcpy(&v, in + *p, 8); *p += 8; return v; }

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  {   /* what needs no set: a 0 handle is an argument error, and nothing is pinned for it */
    call_t c = one_call();
    CHECK(call(env, 0, &c, 1, 1) == LZ4HIP_E_ARG && no_exc() && g_alloc == 0 && unpinned(&c) && untouched(&c));
  }
  if (arg_no_gpu(argc, argv)) {
    CHECK(CREATE(env, NULL, 3) == 0 && no_exc() && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("no set without a device, loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_cxstream --no-gpu | <stream> <out-dir>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != NULL);
  fseek(f, 0, SEEK_END);
  const long total = ftell(f);
  fseek(f, 0, SEEK_SET);
  CHECK(total >= 24 && total < (1 << 26));
  uint8_t* in = (uint8_t*)malloc((size_t)total);
  CHECK(in != NULL && fread(in, 1, (size_t)total, f) == (size_t)total);
  fclose(f);
  size_t p = 0;
  const int64_t win_len = rd(in, &p), n = rd(in, &p), calls = rd(in, &p);
  CHECK(win_len >= 0 && n >= 0 && n < 100000 && calls > 0 && calls <= n + 1);
  const size_t calls_at = p, blocks_at = calls_at + 24 * (size_t)calls, data_at = blocks_at + 24 * (size_t)n;
  CHECK(data_at <= (size_t)total);
  const jlong set = CREATE(env, NULL, 3);
  CHECK(set != 0);
  set_checks(env, set);
  const size_t GUARD = 32, win = GUARD;
  fobj* src = mk(4, GUARD + (size_t)win_len + GUARD);
  memset(src->data, 0xA5, src->bytes);
  size_t room = GUARD;
  for (int64_t i = 0; i < n; i++) { p = blocks_at + 24 * (size_t)i + 16; room += (size_t)rd(in, &p) + GUARD; }
  fobj* dst = mk(4, room);
  memset(dst->data, 0xEE, dst->bytes);
  FILE* t = out_file(argv[2], "cxstream.txt", "w");
  FILE* o = out_file(argv[2], "cxstream.out", "wb");
  fobj* id = int1(1); fobj* first = mk(2, 8); fobj* he = mk(3, 8); fobj* hl = int1(0); fobj* wo = mk(3, 8); fobj* wl = mk(3, 8); fobj* cons = mk(3, 8);
  ((jlong*)wo->data)[0] = (jlong)win; ((jlong*)wl->data)[0] = (jlong)win_len;
  int64_t k = 0;
  size_t data_p = data_at, slot = GUARD;
  for (int64_t ci = 0; ci < calls; ci++) {
    p = calls_at + 24 * (size_t)ci;
    const int64_t cut = rd(in, &p), hist_end = rd(in, &p), hist_len = rd(in, &p), nb = cut - k;
    CHECK(nb >= 0 && cut <= n);
    fobj* so = mk(3, 8 * (size_t)nb); fobj* sl = mk(2, 4 * (size_t)nb); fobj* dof = mk(3, 8 * (size_t)nb); fobj* dc = mk(2, 4 * (size_t)nb); fobj* ol = mk(2, 4 * (size_t)nb);
    for (int64_t i = 0; i < nb; i++) {
      p = blocks_at + 24 * (size_t)(k + i);
      const int64_t off = rd(in, &p), len = rd(in, &p), cap = rd(in, &p);
      CHECK(off >= 0 && len >= 0 && cap >= 0 && off + len <= win_len && data_p + (size_t)len <= (size_t)total);
      memcpy(src->data + win + (size_t)off, in + data_p, (size_t)len);   /* the producer writes the block into its place */
      data_p += (size_t)len;
      ((jlong*)so->data)[i] = (jlong)win + off; ((jint*)sl->data)[i] = (jint)len; ((jlong*)dof->data)[i] = (jlong)slot; ((jint*)dc->data)[i] = (jint)cap;
      ((jint*)ol->data)[i] = -7;
      slot += (size_t)cap + GUARD;
    }
    ((jint*)first->data)[0] = 0; ((jint*)first->data)[1] = (jint)nb;
    ((jlong*)he->data)[0] = hist_len ? (jlong)win + hist_end : 0; ((jint*)hl->data)[0] = (jint)hist_len;
    const jint rc = AT(env, NULL, set, (jintArray)id, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)first, (jlongArray)he, (jintArray)hl, (jlongArray)wo,
                       (jlongArray)wl, (jobject)dst, (jlongArray)dof, (jintArray)dc, (jintArray)ol, (jlongArray)cons, (jint)nb, 1);
    CHECK(rc == 0 && no_exc() && g_alloc == 0);
    CHECK(id->pins == 0 && so->pins == 0 && sl->pins == 0 && first->pins == 0 && he->pins == 0 && hl->pins == 0 && wo->pins == 0 && wl->pins == 0 &&
          dof->pins == 0 && dc->pins == 0 && ol->pins == 0 && cons->pins == 0);
    for (int64_t i = 0; i < nb; i++) {
      const jint r = ((jint*)ol->data)[i];
      const size_t off = (size_t)((jlong*)dof->data)[i], cap = (size_t)((jint*)dc->data)[i], got = r > 0 ? (size_t)r : 0;
      CHECK(got <= cap);
      for (size_t g = 0; g < GUARD; g++) CHECK(dst->data[off - GUARD + g] == 0xEE && dst->data[off + cap + g] == 0xEE);
      if (r != 0) for (size_t g = got; g < cap; g++) CHECK(dst->data[off + g] == 0xEE);
      fprintf(t, "%d ", (int)r);
      CHECK(fwrite(dst->data + off, 1, got, o) == got);
    }
    k = cut;
  }
  fprintf(t, "\n");
  fclose(t);
  fclose(o);
  for (size_t g = 0; g < GUARD; g++) CHECK(src->data[g] == 0xA5 && src->data[win + (size_t)win_len + g] == 0xA5);
  FREE(env, NULL, set);
  free(in);
  return checks_ok(NULL);
}
