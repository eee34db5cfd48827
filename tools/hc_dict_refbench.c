/* tools/hc_dict_refbench.c -- the host side of tools/hc_dict_sweep.py: the reference library's LZ4_resetStreamHC_fast +
 * LZ4_loadDictHC + LZ4_compress_HC_continue, a fresh stream per record, on T threads.
 *   hc_dict_refbench <liblz4.so> <dictionary file> <records file> <record bytes> <threads> <level>
 * The records file holds records of <record bytes> each, back to back.  Every thread compresses the records k, k + T, k + 2T, ...: it
 * resets its stream to the level, loads the dictionary and compresses the record into its own buffer (dlopen'd library; the dictionary
 * lies in a buffer of its own, so liblz4 runs its external-dictionary mode).  Prints the source bytes, the
 * compressed bytes and the best of three passes as "<source bytes> <compressed bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef void* (*create_fn)(void);
typedef int (*free_fn)(void*);
typedef void (*reset_fn)(void*, int);
typedef int (*load_fn)(void*, const char*, int);
typedef int (*cont_fn)(void*, const char*, char*, int, int);
static create_fn f_create;
static free_fn f_free;
static reset_fn f_reset;
static load_fn f_load;
static cont_fn f_cont;
static const char* data;
static const char* dict;
static long nblk, blk, dict_len, T, level;
static long long produced[256];

static void* work(void* arg) {
  const long k = (long)arg;
  const int cap = (int)(blk + blk / 255 + 16);
  char* out = malloc((size_t)cap);
  void* st = f_create();
  long long c = 0;
  for (long i = k; i < nblk; i += T) {
    f_reset(st, (int)level);
    f_load(st, dict, (int)dict_len);
    const int r = f_cont(st, data + i * blk, out, (int)blk, cap);
    if (r > 0) c += r;
  }
  produced[k] = c;
  f_free(st);
  free(out);
  return NULL;
}

static char* slurp(const char* path, long* bytes) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return NULL;
  fseek(fp, 0, SEEK_END);
  *bytes = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  char* buf = malloc((size_t)*bytes + 64);
  if (!buf || fread(buf, 1, (size_t)*bytes, fp) != (size_t)*bytes) return NULL;
  fclose(fp);
  return buf;
}

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: hc_dict_refbench <lib> <dictionary> <records> <record bytes> <threads> <level>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
  f_create = (create_fn)dlsym(h, "LZ4_createStreamHC");
  f_free = (free_fn)dlsym(h, "LZ4_freeStreamHC");
  f_reset = (reset_fn)dlsym(h, "LZ4_resetStreamHC_fast");
  f_load = (load_fn)dlsym(h, "LZ4_loadDictHC");
  f_cont = (cont_fn)dlsym(h, "LZ4_compress_HC_continue");
  if (!f_create || !f_free || !f_reset || !f_load || !f_cont) { fprintf(stderr, "no streaming HC compressor in %s\n", argv[1]); return 2; }
  long dbytes = 0;
  dict = slurp(argv[2], &dict_len);
  data = slurp(argv[3], &dbytes);
  if (!dict || !data) return 2;
  blk = atol(argv[4]); T = atol(argv[5]); level = atol(argv[6]);
  if (blk <= 0 || T < 1 || T > 256) return 2;
  nblk = dbytes / blk;
  double best = 1e30;
  long long total = 0;
  for (int pass = 0; pass < 3; pass++) {
    pthread_t th[256];
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long k = 0; k < T; k++) pthread_create(&th[k], NULL, work, (void*)k);
    for (long k = 0; k < T; k++) pthread_join(th[k], NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    if (s < best) best = s;
    total = 0;
    for (long k = 0; k < T; k++) total += produced[k];
  }
  printf("%lld %lld %.6f\n", (long long)nblk * blk, total, best);
  return 0;
}
