/* tools/hc_destsize_refbench.c -- the host side of tools/hc_destsize_sweep.py: the reference library's LZ4_compress_HC_destSize on T threads.
 *   hc_destsize_refbench <liblz4.so> <blocks file> <block bytes> <target> <threads> <level>
 * Every thread compresses the blocks k, k + T, k + 2T, ... of the file (dlopen'd library, its own output buffer and HC state); prints the consumed
 * bytes and the best of three passes as "<consumed bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef int (*dest_fn)(void*, const char*, char*, int*, int, int);
static dest_fn f;
static const char* data;
static long nblk, blk, target, T, level;
static long long consumed[256];

static void* work(void* arg) {
  const long k = (long)arg;
  char* out = malloc((size_t)target);
  void* state = aligned_alloc(64, 1 << 19);   /* LZ4_sizeofStateHC() is 262200 in 1.9.3 */
  long long c = 0;
  for (long i = k; i < nblk; i += T) {
    int sz = (int)blk;
    f(state, data + i * blk, out, &sz, (int)target, (int)level);
    c += sz;
  }
  consumed[k] = c;
  free(out);
  free(state);
  return NULL;
}

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: hc_destsize_refbench <lib> <file> <block> <target> <threads> <level>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h || !(f = (dest_fn)dlsym(h, "LZ4_compress_HC_destSize"))) { fprintf(stderr, "no LZ4_compress_HC_destSize in %s\n", argv[1]); return 2; }
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  fseek(fp, 0, SEEK_END);
  const long bytes = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  char* buf = malloc((size_t)bytes);
  if (!buf || fread(buf, 1, (size_t)bytes, fp) != (size_t)bytes) return 2;
  fclose(fp);
  data = buf;
  blk = atol(argv[3]); target = atol(argv[4]); T = atol(argv[5]); level = atol(argv[6]);
  if (blk <= 0 || target <= 0 || T < 1 || T > 256) return 2;
  nblk = bytes / blk;
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
    for (long k = 0; k < T; k++) total += consumed[k];
  }
  printf("%lld %.6f\n", total, best);
  return 0;
}
