/* tools/chain_compress_refbench.c -- the host side of tools/chain_compress_sweep.py: the reference library's LZ4_compress_fast_continue on
 * T threads.
 *   chain_compress_refbench <liblz4.so> <data file> <prefix bytes> <blocks per chain> <block bytes> <threads>
 * The data file holds the chains back to back, each as <prefix bytes> of history followed by <blocks per chain> x <block bytes> of
 * source.  The chains are dealt to the threads: thread k compresses the chains k, k + T, k + 2T, ... -- a reset stream, LZ4_loadDict of
 * the history where there is any, then block after block with acceleration 1, every block into the same scratch buffer (dlopen'd
 * library); prints the source bytes, the compressed bytes and the best of three passes as "<source bytes> <compressed bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef void* (*create_fn)(void);
typedef int (*free_fn)(void*);
typedef void (*reset_fn)(void*);
typedef int (*load_fn)(void*, const char*, int);
typedef int (*cont_fn)(void*, const char*, char*, int, int, int);
static create_fn f_create;
static free_fn f_free;
static reset_fn f_reset;
static load_fn f_load;
static cont_fn f_cont;
static const char* data;
static long nchains, prefix, bpc, blk, T;
static long long consumed[256], produced[256];

static void* work(void* arg) {
  const long k = (long)arg, cap = blk + blk / 255 + 16, stride = prefix + bpc * blk;
  char* out = malloc((size_t)cap + 64);
  void* s = f_create();
  long long c = 0, p = 0;
  for (long ch = k; ch < nchains; ch += T) {
    const char* src = data + ch * stride + prefix;
    f_reset(s);
    if (prefix > 0) f_load(s, src - prefix, (int)prefix);
    for (long i = 0; i < bpc; i++) {
      const int r = f_cont(s, src + i * blk, out, (int)blk, (int)cap, 1);
      if (r <= 0) break;
      c += blk; p += r;
    }
  }
  consumed[k] = c; produced[k] = p;
  f_free(s);
  free(out);
  return NULL;
}

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: chain_compress_refbench <lib> <data> <prefix bytes> <blocks per chain> <block bytes> <threads>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
  f_create = (create_fn)dlsym(h, "LZ4_createStream");
  f_free = (free_fn)dlsym(h, "LZ4_freeStream");
  f_reset = (reset_fn)dlsym(h, "LZ4_resetStream");
  f_load = (load_fn)dlsym(h, "LZ4_loadDict");
  f_cont = (cont_fn)dlsym(h, "LZ4_compress_fast_continue");
  if (!f_create || !f_free || !f_reset || !f_load || !f_cont) { fprintf(stderr, "no stream compressor in %s\n", argv[1]); return 2; }
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  fseek(fp, 0, SEEK_END);
  const long bytes = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  char* buf = malloc((size_t)bytes + 64);
  if (!buf || fread(buf, 1, (size_t)bytes, fp) != (size_t)bytes) return 2;
  fclose(fp);
  data = buf;
  prefix = atol(argv[3]); bpc = atol(argv[4]); blk = atol(argv[5]); T = atol(argv[6]);
  if (prefix < 0 || bpc <= 0 || blk <= 0 || T < 1 || T > 256 || bytes % (prefix + bpc * blk)) return 2;
  nchains = bytes / (prefix + bpc * blk);
  double best = 1e30;
  long long in_total = 0, out_total = 0;
  for (int pass = 0; pass < 3; pass++) {
    pthread_t th[256];
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long k = 0; k < T; k++) pthread_create(&th[k], NULL, work, (void*)k);
    for (long k = 0; k < T; k++) pthread_join(th[k], NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    if (s < best) best = s;
    in_total = out_total = 0;
    for (long k = 0; k < T; k++) { in_total += consumed[k]; out_total += produced[k]; }
  }
  printf("%lld %lld %.6f\n", in_total, out_total, best);
  return 0;
}
