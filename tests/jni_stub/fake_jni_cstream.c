/* tests/jni_stub/fake_jni_cstream.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The resident-stream natives of the JNI shim (LZ4HIPJNI.LZ4HIP_cstreamsCreate / Count / Reset / Consumed / Free and
 * LZ4HIP_batchFastStream) executed without a JVM, with the fake JNIEnv of fake_env.h (an int[] / long[] is a malloc'd buffer with pin
 * accounting, a direct ByteBuffer is a pointer; the shim's malloc / free are counted through shim_alloc.h).  Built (build_fake_jni of
 * tests/support.py) by tests/test_cstream_abi.py / tests/test_gpu_cstream.py.
 *
 *   fake_jni_cstream --no-gpu           anywhere: a 0 handle and negative counts are argument errors, nothing pinned; without a device
 *                                       no set can be made and the failure is LOUD (handle 0, the library's message), nothing leaked
 *   fake_jni_cstream <chain> <out-dir>  on a GPU box: one chain through stream 1 of a set of three, cut into TWO calls behind
 *                                       everything the stream holds, the second call without the optional array where nothing is
 *                                       held.  <chain>: the file of fake_jni_cchain (u32 n_blocks >= 2, u32 prefix_len, per block {i32
 *                                       src_len, i32 dst_cap}, the history, the source).  Writes "<out_len ...> | <consumed>" to
 *                                       <out-dir>/cstream.txt and the bytes of the blocks that succeeded, back to back, to
 *                                       <out-dir>/cstream.out (the test compares both with ONE LZ4_stream_t of the reference); checks
 *                                       consumed / stopped, the id errors and reset; prints "fake_jni_cstream: N checks ok"
 */
#define FAKE_JNI_NAME "fake_jni_cstream"
#include "fake_env.h"

JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_init(JNIEnv*, jclass);
JNIEXPORT jlong JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate(JNIEnv*, jclass, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCount(JNIEnv*, jclass, jlong);
JNIEXPORT void JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree(JNIEnv*, jclass, jlong);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsReset(JNIEnv*, jclass, jlong, jintArray, jint);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsConsumed(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jintArray);
JNIEXPORT jint JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStream(JNIEnv*, jclass, jlong, jintArray, jobject, jlongArray, jintArray, jintArray,
    jintArray, jobject, jlongArray, jintArray, jintArray, jlongArray, jint, jint);
JNIEXPORT jstring JNICALL Java_net_jpountz_lz4_LZ4HIPJNI_lastError(JNIEnv*, jclass);

#define CREATE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCreate
#define COUNT Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsCount
#define FREE Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsFree
#define RESET Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsReset
#define CONSUMED Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1cstreamsConsumed
#define CSTREAM Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1batchFastStream

/* one well-formed call apart from its set: one chain of one block of 4 bytes behind 4 bytes of history, for stream 0 */
typedef struct { fobj *id, *src, *dst, *cso, *pre, *sl, *first, *doff, *dc, *ol, *cons; } call_t;
static call_t one_call(void) {
  call_t c;
  c.src = mk(4, 64); c.dst = mk(4, 64);
  memcpy(c.src->data, "0123abcd", 8);
  memset(c.dst->data, 7, 64);
  c.id = int1(0); c.cso = mk(3, 8); c.pre = int1(4); c.sl = int1(4); c.first = mk(2, 8); c.doff = mk(3, 8); c.dc = int1(20); c.ol = int1(-7); c.cons = mk(3, 8);
  ((jlong*)c.cso->data)[0] = 4; ((jint*)c.first->data)[1] = 1; ((jlong*)c.doff->data)[0] = 8; ((jlong*)c.cons->data)[0] = 99;
  return c;
}
static int unpinned(const call_t* c) {
  return c->id->pins == 0 && c->cso->pins == 0 && c->pre->pins == 0 && c->sl->pins == 0 && c->first->pins == 0 && c->doff->pins == 0 && c->dc->pins == 0 &&
         c->ol->pins == 0 && c->cons->pins == 0;
}
static jint call(JNIEnv* env, jlong set, const call_t* c, jint nb, jint nc) {
  return CSTREAM(env, NULL, set, (jintArray)c->id, (jobject)c->src, (jlongArray)c->cso, (jintArray)c->pre, (jintArray)c->sl, (jintArray)c->first, (jobject)c->dst,
                 (jlongArray)c->doff, (jintArray)c->dc, (jintArray)c->ol, (jlongArray)c->cons, nb, nc);
}
static int untouched(const call_t* c) {
  for (int i = 0; i < 64; i++) if (c->dst->data[i] != 7) return 0;
  return get1(c->ol) == -7 && ((jlong*)c->cons->data)[0] == 99;
}

/* what needs no set: a 0 handle is an argument error everywhere, and nothing is pinned for it */
static int no_set_checks(JNIEnv* env) {
  call_t c = one_call();
  fobj* cons = mk(3, 8); fobj* st = int1(-3);
  CHECK(call(env, 0, &c, 1, 1) == LZ4HIP_E_ARG && no_exc() && g_alloc == 0 && unpinned(&c) && untouched(&c));
  CHECK(RESET(env, NULL, 0, NULL, 0) == LZ4HIP_E_ARG && RESET(env, NULL, 0, (jintArray)c.id, 1) == LZ4HIP_E_ARG && c.id->pins == 0);
  CHECK(CONSUMED(env, NULL, 0, 0, 1, (jlongArray)cons, (jintArray)st) == LZ4HIP_E_ARG && cons->pins == 0 && st->pins == 0 && get1(st) == -3 && g_alloc == 0);
  CHECK(COUNT(env, NULL, 0) == LZ4HIP_E_ARG);
  FREE(env, NULL, 0);
  CHECK(CREATE(env, NULL, 0) == 0 && CREATE(env, NULL, -5) == 0 && no_exc());
  return 0;
}

/* with a live set: every argument error of the native and of the library behind it, nothing pinned, written or consumed */
static int set_checks(JNIEnv* env, jlong set) {
  call_t c = one_call();
  for (int k = 0; k < 10; k++) {   /* every required argument NULL in turn (the prefix array is optional) */
    call_t d = c;
    fobj** f[10] = {&d.id, &d.src, &d.cso, &d.sl, &d.first, &d.dst, &d.doff, &d.dc, &d.ol, &d.cons};
    *f[k] = NULL;
    CHECK(call(env, set, &d, 1, 1) == LZ4HIP_E_ARG && no_exc() && g_alloc == 0);
    CHECK(unpinned(&c) && untouched(&c));
  }
  CHECK(call(env, set, &c, -1, 1) == LZ4HIP_E_ARG && call(env, set, &c, 1, -1) == LZ4HIP_E_ARG);
  ((jint*)c.id->data)[0] = 3;      /* three streams exist */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.id->data)[0] = 0;
  ((jint*)c.first->data)[1] = 2;   /* chainFirst does not end at the number of blocks */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.first->data)[1] = 1;
  ((jint*)c.pre->data)[0] = 5;     /* a history longer than the chain's offset */
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  ((jint*)c.pre->data)[0] = -1;
  CHECK(call(env, set, &c, 1, 1) == LZ4HIP_E_ARG);
  CHECK(unpinned(&c) && untouched(&c) && g_alloc == 0);
  fobj* cons = mk(3, 24); fobj* st = mk(2, 12);
  CHECK(CONSUMED(env, NULL, set, 0, 3, NULL, (jintArray)st) == LZ4HIP_E_ARG && CONSUMED(env, NULL, set, 0, 3, (jlongArray)cons, NULL) == LZ4HIP_E_ARG);
  CHECK(CONSUMED(env, NULL, set, 1, 3, (jlongArray)cons, (jintArray)st) == LZ4HIP_E_ARG);   /* streams 1 .. 3 of three */
  CHECK(CONSUMED(env, NULL, set, 0, 3, (jlongArray)cons, (jintArray)st) == 0 && cons->pins == 0 && st->pins == 0 && g_alloc == 0);
  for (int i = 0; i < 3; i++) CHECK(((jlong*)cons->data)[i] == 0 && ((jint*)st->data)[i] == 0);
  fobj* bad = int1(7);
  CHECK(RESET(env, NULL, set, (jintArray)bad, 1) == LZ4HIP_E_ARG && bad->pins == 0);
  return 0;
}

int main(int argc, char** argv) {
  JNIEnv* env = &g_env;
  Java_net_jpountz_lz4_LZ4HIPJNI_init(env, NULL);
  CHECK(no_exc());
  (void)no_set_checks(env);
  if (arg_no_gpu(argc, argv)) {
    CHECK(CREATE(env, NULL, 3) == 0 && no_exc() && g_alloc == 0);
    const char* msg = (const char*)Java_net_jpountz_lz4_LZ4HIPJNI_lastError(env, NULL);
    CHECK(msg && strstr(msg, "no HIP device") != NULL);
    return checks_ok("no set without a device, loudly");
  }
  if (argc < 3) { fprintf(stderr, "usage: fake_jni_cstream --no-gpu | <chain> <out-dir>\n"); return 2; }
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
  CHECK(n >= 2 && n < 100000 && 8 + 8 * (size_t)n + prefix <= (size_t)total);
  const jlong set = CREATE(env, NULL, 3);
  CHECK(set != 0 && COUNT(env, NULL, set) == 3);
  (void)set_checks(env, set);
  const size_t GUARD = 32;
  const uint32_t cut = n / 2;
  fobj* ol = mk(2, 4 * (size_t)n); fobj* dcap = mk(2, 4 * (size_t)n); fobj* lens = mk(2, 4 * (size_t)n); fobj* offs = mk(3, 8 * (size_t)n);
  size_t bytes = 0, room = GUARD, first_bytes = 0;
  for (uint32_t i = 0; i < n; i++) {
    int32_t len, c;
    memcpy(&len, in + 8 + 8 * (size_t)i, 4); memcpy(&c, in + 12 + 8 * (size_t)i, 4);
    CHECK(len >= 0 && c >= 0);
    ((jint*)lens->data)[i] = len; ((jint*)dcap->data)[i] = c; ((jlong*)offs->data)[i] = (jlong)room; ((jint*)ol->data)[i] = -7;
    bytes += (size_t)len; room += (size_t)c + GUARD;
    if (i < cut) first_bytes += (size_t)len;
  }
  const uint8_t* hist = in + 8 + 8 * (size_t)n;
  CHECK((size_t)(hist - in) + prefix + bytes == (size_t)total);
  fobj* src = mk(4, GUARD + prefix + bytes + GUARD);
  memset(src->data, 0xA5, src->bytes);
  memcpy(src->data + GUARD, hist, prefix + bytes);
  fobj* dst = mk(4, room);
  memset(dst->data, 0xEE, dst->bytes);
  uint64_t done = 0;
  for (int k = 0; k < 2; k++) {   /* blocks [0, cut) and [cut, n) of stream 1 */
    const uint32_t b0 = k ? cut : 0, nb = k ? n - cut : cut;
    fobj* sl = mk(2, 4 * (size_t)nb); fobj* dc = mk(2, 4 * (size_t)nb); fobj* doff = mk(3, 8 * (size_t)nb); fobj* o = mk(2, 4 * (size_t)nb);
    memcpy(sl->data, (jint*)lens->data + b0, 4 * (size_t)nb); memcpy(dc->data, (jint*)dcap->data + b0, 4 * (size_t)nb);
    memcpy(doff->data, (jlong*)offs->data + b0, 8 * (size_t)nb); memcpy(o->data, (jint*)ol->data + b0, 4 * (size_t)nb);
    /* everything the stream holds lies in front of the source: the loaded prefix (none under 8 bytes) and what the first call consumed */
    size_t held = k ? (prefix < 8 ? 0 : prefix) + (size_t)done : prefix;
    if (held > 65536) held = 65536;
    fobj* id = int1(1); fobj* first = mk(2, 8); fobj* cso = mk(3, 8); fobj* pre = int1((jint)held); fobj* cons = mk(3, 8);
    ((jint*)first->data)[1] = (jint)nb;
    ((jlong*)cso->data)[0] = (jlong)(GUARD + prefix + (k ? first_bytes : 0)); ((jlong*)cons->data)[0] = -1;
    const jint rc = CSTREAM(env, NULL, set, (jintArray)id, (jobject)src, (jlongArray)cso, (k && held == 0) ? NULL : (jintArray)pre, (jintArray)sl, (jintArray)first,
                            (jobject)dst, (jlongArray)doff, (jintArray)dc, (jintArray)o, (jlongArray)cons, (jint)nb, 1);
    CHECK(rc == 0 && no_exc() && g_alloc == 0);
    CHECK(id->pins == 0 && sl->pins == 0 && dc->pins == 0 && doff->pins == 0 && o->pins == 0 && first->pins == 0 && cso->pins == 0 && pre->pins == 0 && cons->pins == 0);
    memcpy((jint*)ol->data + b0, o->data, 4 * (size_t)nb);
    if (k == 0) CHECK((uint64_t)((jlong*)cons->data)[0] <= first_bytes);
    done += (uint64_t)((jlong*)cons->data)[0];
  }
  CHECK(done <= bytes);
  FILE* t = out_file(argv[2], "cstream.txt", "w");
  FILE* o = out_file(argv[2], "cstream.out", "wb");
  size_t at = 0;   /* every byte of dst is a guard, a block's result, or untouched (a block that failed may have written its own slot) */
  for (uint32_t i = 0; i < n; i++) {
    const jint r = ((jint*)ol->data)[i];
    const size_t off = (size_t)((jlong*)offs->data)[i], cap = (size_t)((jint*)dcap->data)[i], got = r > 0 ? (size_t)r : 0;
    CHECK(got <= cap);
    for (; at < off; at++) CHECK(dst->data[at] == 0xEE);
    if (r != 0) for (size_t k = got; k < cap; k++) CHECK(dst->data[off + k] == 0xEE);
    at = off + cap;
    fprintf(t, "%d ", (int)r);
    CHECK(fwrite(dst->data + off, 1, got, o) == got);
  }
  for (; at < dst->bytes; at++) CHECK(dst->data[at] == 0xEE);
  fprintf(t, "| %llu\n", (unsigned long long)done);
  fclose(t);
  fclose(o);
  /* consumed / stopped as reported; reset of stream 1 alone */
  fobj* cons = mk(3, 24); fobj* st = mk(2, 12); fobj* one = int1(1);
  CHECK(CONSUMED(env, NULL, set, 0, 3, (jlongArray)cons, (jintArray)st) == 0 && g_alloc == 0);
  CHECK(((jlong*)cons->data)[0] == 0 && (uint64_t)((jlong*)cons->data)[1] == done && ((jlong*)cons->data)[2] == 0);
  CHECK(((jint*)st->data)[0] == 0 && ((jint*)st->data)[1] == (done != bytes) && ((jint*)st->data)[2] == 0);
  CHECK(RESET(env, NULL, set, (jintArray)one, 1) == 0 && one->pins == 0);
  CHECK(CONSUMED(env, NULL, set, 1, 1, (jlongArray)cons, (jintArray)st) == 0 && ((jlong*)cons->data)[0] == 0 && ((jint*)st->data)[0] == 0);
  CHECK(RESET(env, NULL, set, NULL, 0) == 0);
  FREE(env, NULL, set);
  free(in);
  return checks_ok(NULL);
}
