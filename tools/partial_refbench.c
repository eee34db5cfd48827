/* tools/partial_refbench.c -- the host side of tools/partial_sweep.py: the reference library's LZ4_decompress_safe_partial on T threads.
 *   partial_refbench <liblz4.so> <streams file> <lengths file> <block bytes> <target> <threads>
 * The streams file holds the compressed blocks back to back, the lengths file their sizes (int32 each).  Every thread decodes the
 * blocks k, k + T, k + 2T, ... into min(target, block bytes) bytes of its own buffer (dlopen'd library); prints the decoded bytes and
 * the best of three passes as "<decoded bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef int (*partial_fn)(const char*, char*, int, int, int);
static partial_fn f;
static const char* data;
static const int32_t* lens;
static long* offs;
static long nblk, blk, target, T;
static long long decoded[256];

static void* work(void* arg) {
  const long k = (long)arg;
  char* out = malloc((size_t)blk);
  long long c = 0;
  for (long i = k; i < nblk; i += T) {
    const int r = f(data + offs[i], out, lens[i], (int)target, (int)blk);
    if (r > 0) c += r;
  }
  decoded[k] = c;
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
  if (argc < 7) { fprintf(stderr, "usage: partial_refbench <lib> <streams> <lengths> <block> <target> <threads>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h || !(f = (partial_fn)dlsym(h, "LZ4_decompress_safe_partial"))) { fprintf(stderr, "no LZ4_decompress_safe_partial in %s\n", argv[1]); return 2; }
  long sbytes = 0, lbytes = 0;
  data = slurp(argv[2], &sbytes);
  lens = (const int32_t*)slurp(argv[3], &lbytes);
  if (!data || !lens) return 2;
  nblk = lbytes / 4;
  offs = malloc(sizeof(long) * (size_t)(nblk + 1));
  offs[0] = 0;
  for (long i = 0; i < nblk; i++) offs[i + 1] = offs[i] + lens[i];
  if (offs[nblk] > sbytes) return 2;
  blk = atol(argv[4]); target = atol(argv[5]); T = atol(argv[6]);
  if (blk <= 0 || target < 0 || T < 1 || T > 256) return 2;
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
