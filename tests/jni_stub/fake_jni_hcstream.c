/* tests/jni_stub/fake_jni_hcstream.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The HC stream-compress native of the JNI shim (LZ4HIPJNI.LZ4HIP_batchHCStream) executed without a JVM, with the fake JNIEnv of
 * fake_env.h (an int[] / long[] is a malloc'd buffer with pin accounting, a direct ByteBuffer is a pointer; the shim's malloc / free are
 * counted through shim_alloc.h).  Built (build_fake_jni of tests/support.py) by tests/test_hcstream_abi.py / tests/test_gpu_hcstream.py.
 *
 *   fake_jni_hcstream --no-gpu       anywhere: NULL arrays, a bad chainFirst, a history longer than its end offset and a stream at the
 *                                    index limit are argument errors, a well-formed call fails LOUDLY without a device (library status,
 *                                    nothing leaked or left pinned, nothing written, the state as it was)
 *   fake_jni_hcstream <in> <out>     on a GPU box: one stream through the native, a call per block, LZ4_loadDictHC and LZ4_saveDictHC as
 *                                    the C ABI's state edits.  <in> / <out>: the files tests/cpp/hcstream_mirror_test.cpp describes.
 *                                    Prints "fake_jni_hcstream: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_hcstream"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCStream(JNIEnv*, jclass, jlongArray, jobject, jlongArray, jintArray, jintArray, jobject,
    jlongArray, jintArray, jintArray, jint, jint, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define STREAM Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchHCStream

typedef struct { fobj *state, *src, *so, *sl, *first, *dst, *dof, *dc, *ol; } call_t;

/* one stream behind a prefix of 4 bytes that ends at 16, one block of 8 bytes at src[16, 24) to dst[0, 40) */
static call_t small_call(void) {
  call_t c = {mk(3, 40), mk(4, 64), mk(3, 8), int1(8), mk(2, 8), mk(4, 64), mk(3, 8), int1(40), int1(-7)};
  for (int i = 0; i < 64; i++) c.src->data[i] = (uint8_t)(i * 7);
  memset(c.dst->data, 7, 64);
  ((jlong*)c.state->data)[0] = 16; ((jlong*)c.state->data)[1] = 4; ((jlong*)c.state->data)[4] = 4;
  ((jint*)c.first->data)[1] = 1;
  ((jlong*)c.so->data)[0] = 16;
  return c;
}
static jint run(JNIEnv* env, const call_t* c, int null_at, jint nb, jint nc) {
  return STREAM(env, NULL, null_at == 0 ? NULL : (jlongArray)c->state, null_at == 1 ? NULL : (jobject)c->src, null_at == 2 ? NULL : (jlongArray)c->so,
                null_at == 3 ? NULL : (jintArray)c->sl, null_at == 4 ? NULL : (jintArray)c->first, null_at == 5 ? NULL : (jobject)c->dst,
                null_at == 6 ? NULL : (jlongArray)c->dof, null_at == 7 ? NULL : (jintArray)c->dc, null_at == 8 ? NULL : (jintArray)c->ol, nb, nc, 9);
}
static void nothing_pinned_or_written(const call_t* c) {
  const fobj* all[7] = {c->state, c->so, c->sl, c->first, c->dof, c->dc, c->ol};
  for (int t = 0; t < 7; t++) CHECK(all[t]->pins == 0);
  CHECK(g_alloc == 0 && no_exc() && get1(c->ol) == -7);
  for (int i = 0; i < 64; i++) CHECK(c->dst->data[i] == 7);
}

static void no_gpu_checks(JNIEnv* env) {
  call_t c = small_call();
  jlong* st = (jlong*)c.state->data;
  for (int k = 0; k <= 8; k++) {   /* every argument NULL in turn */
    CHECK(run(env, &c, k, 1, 1) == LZ4HIP_E_ARG);
    nothing_pinned_or_written(&c);
  }
  CHECK(run(env, &c, -1, -1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 2;                     /* chainFirst does not end at the number of blocks */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 1;
  st[0] = 3;                                         /* a prefix longer than its end offset */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  st[0] = 16; st[2] = 2; st[3] = 3;                  /* an external dictionary longer than its end offset */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  st[2] = 0; st[3] = 0; st[4] = (1ll << 31) - 65536 - 7;   /* 65536 + index would pass 2^31 during the call */
  CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_ARG);
  st[4] = 4;
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
    const jlong* st = (const jlong*)c.state->data;
    CHECK(run(env, &c, -1, 1, 1) == LZ4HIP_E_NO_DEVICE);
    nothing_pinned_or_written(&c);
    CHECK(st[0] == 16 && st[1] == 4 && st[2] == 0 && st[3] == 0 && st[4] == 4);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("the compute call failed loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_hcstream --no-gpu | <in> <out>\n"); return 2; }
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
  const int64_t level = rd(in, &p), arena_size = rd(in, &p), n_ops = rd(in, &p);
  CHECK(arena_size > 0 && arena_size < (1 << 26) && n_ops >= 0 && n_ops < 100000 && 24 + 40 * (size_t)n_ops <= (size_t)total);
  const size_t ops_at = 24, data_at = ops_at + 40 * (size_t)n_ops;
  fobj* src = mk(4, (size_t)arena_size);
  memset(src->data, 0xA5, (size_t)arena_size);
  size_t d = data_at;
  for (int64_t i = 0; i < n_ops; i++) {   /* the dictionaries lie in the arena from the start */
    p = ops_at + 40 * (size_t)i;
    const int64_t kind = rd(in, &p), off = rd(in, &p), n = rd(in, &p);
    if (kind == 1) memcpy(src->data + off - n, in + d, (size_t)n);
    if (kind != 2 && n > 0 && n <= 0x7E000000) d += (size_t)n;
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o != NULL);
  int64_t* head = (int64_t*)malloc(48 * (size_t)(n_ops ? n_ops : 1));
  uint8_t* body = (uint8_t*)malloc((size_t)total * 2 + 64 * (size_t)n_ops + 64);
  size_t body_n = 0;
  fobj* state = mk(3, 40);
  fobj* first = mk(2, 8);
  ((jint*)first->data)[1] = 1;
  d = data_at;
  for (int64_t i = 0; i < n_ops; i++) {
    p = ops_at + 40 * (size_t)i;
    const int64_t kind = rd(in, &p), off = rd(in, &p), n = rd(in, &p), cap = rd(in, &p), k = rd(in, &p);
    const size_t held = kind != 2 && n > 0 && n <= 0x7E000000 ? (size_t)n : 0;
    int64_t r = 0;
    if (kind == 1) {
      CHECK(lz4hip_hcstream_load_dict((lz4hip_hcstream_state*)state->data, (uint64_t)off, (uint64_t)n) == 0);
    } else if (kind == 2) {
      const uint64_t end = (uint64_t)((jlong*)state->data)[0];
      r = lz4hip_hcstream_save_dict((lz4hip_hcstream_state*)state->data, (uint64_t)off, (int)k);
      CHECK(r >= 0);
      memmove(src->data + off, src->data + end - r, (size_t)r);   /* (the caller's part of LZ4_saveDictHC: the copy) */
    } else {
      memcpy(src->data + off, in + d, held);
      const size_t room = cap > 0 ? (size_t)cap : 0;
      fobj* dst = mk(4, room + 16);
      memset(dst->data, 0xEE, room + 16);
      fobj* so = mk(3, 8); fobj* sl = int1((jint)n); fobj* dof = mk(3, 8); fobj* dc = int1((jint)cap); fobj* ol = int1(-7);
      ((jlong*)so->data)[0] = (jlong)off;
      const jint rc = STREAM(env, NULL, (jlongArray)state, (jobject)src, (jlongArray)so, (jintArray)sl, (jintArray)first, (jobject)dst, (jlongArray)dof,
                             (jintArray)dc, (jintArray)ol, 1, 1, (jint)level);
      CHECK(rc == 0 && no_exc() && g_alloc == 0);
      CHECK(state->pins == 0 && so->pins == 0 && sl->pins == 0 && first->pins == 0 && dof->pins == 0 && dc->pins == 0 && ol->pins == 0);
      r = get1(ol);
      CHECK(r >= 0 && (size_t)r <= room);
      for (size_t g = r > 0 ? (size_t)r : room; g < room + 16; g++) CHECK(dst->data[g] == 0xEE);   /* nothing past the result, nothing past the slot */
      memcpy(body + body_n, dst->data, (size_t)r);
      body_n += (size_t)r;
    }
    d += held;
    head[6 * i] = r;
    for (int t = 0; t < 5; t++) head[6 * i + 1 + t] = (int64_t)((jlong*)state->data)[t];
  }
  CHECK(fwrite(head, 48, (size_t)n_ops, o) == (size_t)n_ops && fwrite(body, 1, body_n, o) == body_n && fclose(o) == 0);
  free(in);
  return checks_ok(NULL);
}
