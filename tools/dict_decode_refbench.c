/* tools/dict_decode_refbench.c -- the host side of tools/dict_decode_sweep.py: the reference library's LZ4_decompress_safe_usingDict on
 * T threads.
 *   dict_decode_refbench <liblz4.so> <dictionary file> <streams file> <lengths file> <record bytes> <threads>
 * The streams file holds the compressed records back to back, the lengths file their sizes (int32 each).  Every thread decodes the
 * records k, k + T, k + 2T, ... against the one dictionary into its own buffer of <record bytes> (dlopen'd library; the dictionary
 * lies in a buffer of its own, so liblz4 runs its external-dictionary mode); prints the decoded bytes and the best of three passes
 * as "<decoded bytes> <seconds>". */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

typedef int (*dict_fn)(const char*, char*, int, int, const char*, int);
static dict_fn f;
static const char* data;
static const char* dict;
static const int32_t* lens;
static long* offs;
static long nblk, blk, dict_len, T;
static long long decoded[256];

static void* work(void* arg) {
  const long k = (long)arg;
  char* out = malloc((size_t)blk + 64);
  long long c = 0;
  for (long i = k; i < nblk; i += T) {
    const int r = f(data + offs[i], out, lens[i], (int)blk, dict, (int)dict_len);
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
  if (argc < 7) { fprintf(stderr, "usage: dict_decode_refbench <lib> <dictionary> <streams> <lengths> <record bytes> <threads>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h || !(f = (dict_fn)dlsym(h, "LZ4_decompress_safe_usingDict"))) { fprintf(stderr, "no LZ4_decompress_safe_usingDict in %s\n", argv[1]); return 2; }
  long sbytes = 0, lbytes = 0;
  dict = slurp(argv[2], &dict_len);
  data = slurp(argv[3], &sbytes);
  lens = (const int32_t*)slurp(argv[4], &lbytes);
  if (!dict || !data || !lens) return 2;
  nblk = lbytes / 4;
  offs = malloc(sizeof(long) * (size_t)(nblk + 1));
  offs[0] = 0;
  for (long i = 0; i < nblk; i++) offs[i + 1] = offs[i] + lens[i];
  if (offs[nblk] > sbytes) return 2;
  blk = atol(argv[5]); T = atol(argv[6]);
  if (blk <= 0 || T < 1 || T > 256) return 2;
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
