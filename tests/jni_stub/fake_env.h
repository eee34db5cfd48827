/* tests/jni_stub/fake_env.h -- TEST INFRASTRUCTURE ONLY.
 *
 * The fake JNIEnv the fake_jni*.c programs run the JNI shim (lz4-java_amd/jni/net_jpountz_lz4_LZ4HIPJNI.c) in, without a JVM: a
 * function table in which a Java byte[] / int[] / long[] is a malloc'd buffer with pin accounting and a direct ByteBuffer is a
 * pointer.  The shim's malloc / free are counted (-Dmalloc=t_malloc -Dfree=t_free on its translation unit, through shim_alloc.h).
 * The including program defines FAKE_JNI_NAME (its name in messages) first; one program per executable includes this.
 */
#ifndef FAKE_ENV_H
#define FAKE_ENV_H
#include <jni.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lz4hip.h"

/* ---- fake objects ---- */
typedef struct {
  int kind;          /* 1 = byte[], 2 = int[], 3 = long[], 4 = direct ByteBuffer, 5 = heap ByteBuffer (no direct address) */
  uint8_t* data;
  size_t bytes;
  int pins;          /* outstanding Get*Critical / Get*ArrayElements */
  int refuse_pin;    /* GetPrimitiveArrayCritical returns NULL (a VM that cannot pin) */
} fobj;

static long g_alloc = 0;       /* outstanding shim allocations */
void* t_malloc(size_t n) { g_alloc++; return malloc(n); }
void t_free(void* p) { if (p) g_alloc--; free(p); }

static const char* g_exc_class = NULL;
static char g_exc_msg[512];
static int g_checks = 0;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, FAKE_JNI_NAME ": CHECK failed at line %d: %s (pending exception: %s \"%s\")\n", __LINE__, #c, \
    g_exc_class ? g_exc_class : "none", g_exc_msg); exit(1); } g_checks++; } while (0)

static jclass f_FindClass(JNIEnv* e, const char* name) { (void)e; return (jclass)strdup(name); }
static jint f_ThrowNew(JNIEnv* e, jclass c, const char* msg) { (void)e; g_exc_class = (const char*)c; snprintf(g_exc_msg, sizeof g_exc_msg, "%s", msg ? msg : ""); return 0; }
static jobject f_NewGlobalRef(JNIEnv* e, jobject o) { (void)e; return o; }
static void* f_GetCritical(JNIEnv* e, jarray a, jboolean* isCopy) {
  (void)e; fobj* o = (fobj*)a;
  if (isCopy) *isCopy = 0;
  if (o->refuse_pin) return NULL;
  o->pins++;
  return o->data;
}
static void f_ReleaseCritical(JNIEnv* e, jarray a, void* p, jint mode) { (void)e; (void)mode; fobj* o = (fobj*)a; if (p != o->data) { fprintf(stderr, "release of a foreign pointer\n"); exit(1); } o->pins--; }
static void* f_GetDirect(JNIEnv* e, jobject b) { (void)e; fobj* o = (fobj*)b; return o->kind == 4 ? o->data : NULL; }
static jstring f_NewStringUTF(JNIEnv* e, const char* s) { (void)e; return (jstring)strdup(s ? s : ""); }
static jlong* f_GetLongs(JNIEnv* e, jlongArray a, jboolean* c) { (void)e; if (c) *c = 0; ((fobj*)a)->pins++; return (jlong*)((fobj*)a)->data; }
static jint* f_GetInts(JNIEnv* e, jintArray a, jboolean* c) { (void)e; if (c) *c = 0; ((fobj*)a)->pins++; return (jint*)((fobj*)a)->data; }
static void f_RelLongs(JNIEnv* e, jlongArray a, jlong* p, jint m) { (void)e; (void)p; (void)m; ((fobj*)a)->pins--; }
static void f_RelInts(JNIEnv* e, jintArray a, jint* p, jint m) { (void)e; (void)p; (void)m; ((fobj*)a)->pins--; }

static jint f_ArrayLength(JNIEnv* e, jarray a) { (void)e; const fobj* o = (const fobj*)a; return (jint)(o->bytes / (o->kind == 3 ? 8u : o->kind == 2 ? 4u : 1u)); }

static const struct JNINativeInterface_ g_table = {f_FindClass, f_ThrowNew, f_NewGlobalRef, f_GetCritical, f_ReleaseCritical, f_GetDirect,
                                                   f_NewStringUTF, f_GetLongs, f_GetInts, f_RelLongs, f_RelInts, f_ArrayLength};
static JNIEnv g_env = &g_table;

static inline fobj* mk(int kind, size_t bytes) { fobj* o = calloc(1, sizeof *o); o->kind = kind; o->bytes = bytes; o->data = calloc(bytes ? bytes : 1, 1); return o; }
static inline int no_exc(void) { return g_exc_class == NULL; }
static inline void clear_exc(void) { g_exc_class = NULL; g_exc_msg[0] = 0; }
/* every byte of o outside [off, off + n) still holds `fill` */
static inline int guarded(const fobj* o, size_t off, size_t n, uint8_t fill) {
  for (size_t i = 0; i < o->bytes; i++)
    if ((i < off || i >= off + n) && o->data[i] != fill) return 0;
  return 1;
}
/* an int[1] and its element */
static inline fobj* int1(jint v) { fobj* o = mk(2, 4); ((jint*)o->data)[0] = v; return o; }
static inline jint get1(const fobj* o) { return ((const jint*)o->data)[0]; }

/* ---- what every fake_jni*.c program does around its scenarios ---- */
#include <stdarg.h>
/* the program was started as "<program> --no-gpu" */
static inline int arg_no_gpu(int argc, char** argv) { return argc > 1 && strcmp(argv[1], "--no-gpu") == 0; }
/* a new object of `kind` with the file's n bytes (fewer than 16 MiB) at offset `lead` and 16 spare bytes behind them */
static inline fobj* slurp(const char* path, int kind, size_t lead, long* n_out) {
  FILE* f = fopen(path, "rb");
  CHECK(f != NULL);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  CHECK(n >= 0 && n < (1 << 24));
  fobj* o = mk(kind, (size_t)n + lead + 16);
  CHECK(fread(o->data + lead, 1, (size_t)n, f) == (size_t)n);
  fclose(f);
  *n_out = n;
  return o;
}
/* the same bytes in a new object of another kind (a heap array's content as a direct buffer) */
static inline fobj* copy_as(const fobj* o, int kind) { fobj* c = mk(kind, o->bytes); memcpy(c->data, o->data, o->bytes); return c; }
/* <dir>/<name>, opened for writing */
static inline FILE* out_file(const char* dir, const char* name, const char* mode) {
  char path[4096];
  snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE* o = fopen(path, mode);
  CHECK(o != NULL);
  return o;
}
static inline void write_bytes(const char* dir, const char* name, const uint8_t* p, size_t n) {
  FILE* o = out_file(dir, name, "wb");
  CHECK(fwrite(p, 1, n, o) == n);
  fclose(o);
}
static inline void write_text(const char* dir, const char* name, const char* fmt, ...) {
  FILE* o = out_file(dir, name, "w");
  va_list ap;
  va_start(ap, fmt);
  vfprintf(o, fmt, ap);
  va_end(ap);
  fclose(o);
}
/* the closing line, and main's return value: "<program>: N checks ok", without a device "... (no device: <what failed loudly>)" */
static inline int checks_ok(const char* no_device) {
  if (no_device) printf(FAKE_JNI_NAME ": %d checks ok (no device: %s)\n", g_checks, no_device);
  else printf(FAKE_JNI_NAME ": %d checks ok\n", g_checks);
  return 0;
}
#endif
