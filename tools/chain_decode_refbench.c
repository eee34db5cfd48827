/* tools/chain_decode_refbench.c -- the host side of tools/chain_decode_sweep.py: the reference library's LZ4_decompress_safe_continue on
 * T threads.
 *   chain_decode_refbench <liblz4.so> <streams file> <lengths file> <blocks per chain> <block bytes> <threads>
 * The streams file holds the compressed blocks back to back, the lengths file their sizes (int32 each); every <blocks per chain>
 * consecutive blocks are one chain of linked blocks.  Every thread decodes the chains k, k + T, k + 2T, ... -- LZ4_setStreamDecode(sd,
 * NULL, 0), then block after block, each destination where the previous one ended -- into its own buffer of one chain (dlopen'd
 * library); prints the decoded bytes and the best of three passes as "<decoded bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef void* (*create_fn)(void);
typedef int (*free_fn)(void*);
typedef int (*set_fn)(void*, const char*, int);
typedef int (*cont_fn)(void*, const char*, char*, int, int);
static create_fn f_create;
static free_fn f_free;
static set_fn f_set;
static cont_fn f_cont;
static const char* data;
static const int32_t* lens;
static long* offs;
static long nblk, bpc, blk, T;
static long long decoded[256];

static void* work(void* arg) {
  const long k = (long)arg, nchains = nblk / bpc;
  char* out = malloc((size_t)(bpc * blk) + 64);
  void* sd = f_create();
  long long c = 0;
  for (long ch = k; ch < nchains; ch += T) {
    f_set(sd, NULL, 0);
    long at = 0;
    for (long i = ch * bpc; i < (ch + 1) * bpc; i++) {
      const int r = f_cont(sd, data + offs[i], out + at, lens[i], (int)blk);
      if (r < 0) break;
      at += r;
    }
    c += at;
  }
  decoded[k] = c;
  f_free(sd);
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
  if (argc < 7) { fprintf(stderr, "usage: chain_decode_refbench <lib> <streams> <lengths> <blocks per chain> <block bytes> <threads>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
  f_create = (create_fn)dlsym(h, "LZ4_createStreamDecode");
  f_free = (free_fn)dlsym(h, "LZ4_freeStreamDecode");
  f_set = (set_fn)dlsym(h, "LZ4_setStreamDecode");
  f_cont = (cont_fn)dlsym(h, "LZ4_decompress_safe_continue");
  if (!f_create || !f_free || !f_set || !f_cont) { fprintf(stderr, "no stream decoder in %s\n", argv[1]); return 2; }
  long sbytes = 0, lbytes = 0;
  data = slurp(argv[2], &sbytes);
  lens = (const int32_t*)slurp(argv[3], &lbytes);
  if (!data || !lens) return 2;
  nblk = lbytes / 4;
  offs = malloc(sizeof(long) * (size_t)(nblk + 1));
  offs[0] = 0;
  for (long i = 0; i < nblk; i++) offs[i + 1] = offs[i] + lens[i];
  if (offs[nblk] > sbytes) return 2;
  bpc = atol(argv[4]); blk = atol(argv[5]); T = atol(argv[6]);
  if (bpc <= 0 || blk <= 0 || T < 1 || T > 256 || nblk % bpc) return 2;
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
    for (long k = 0; k < T; k++) total += decoded[k];
  }
  printf("%lld %.6f\n", total, best);
  return 0;
}
