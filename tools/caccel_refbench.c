/* tools/caccel_refbench.c -- the CPU side of tools/caccel_sweep.py: the reference library's LZ4_compress_fast_continue at an acceleration
 * over chains of 16 x 4096 bytes that lie back to back (its prefix mode), ONE LZ4_stream_t per chain, on T host threads.
 *   caccel_refbench <liblz4 .so> <pool file> <n chains> <threads> <acceleration>
 * <pool file>: pool chains of 16 x 4096 bytes back to back; chain c compresses pool chain c % pool, in place.  Prints
 * "<seconds> <source bytes> <compressed bytes>" (the best of three passes).  The library is loaded at run time: nothing of it is linked in. */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

enum { BLOCK = 4096, BLOCKS = 16 };
typedef void* (*create_t)(void);
typedef int (*free_t)(void*);
typedef void (*reset_t)(void*);
typedef int (*cont_t)(void*, const char*, char*, int, int, int);
static create_t f_create; static free_t f_free; static reset_t f_reset; static cont_t f_cont;
static const uint8_t* g_pool; static long g_pool_chains, g_n; static int g_threads, g_accel;
typedef struct { int t; uint64_t out; } job_t;

static void* work(void* arg) {
  job_t* j = (job_t*)arg;
  void* st = f_create();
  char dst[BLOCK + BLOCK / 255 + 32];
  uint64_t out = 0;
  for (long c = j->t; c < g_n; c += g_threads) {
    const char* raw = (const char*)g_pool + (size_t)(c % g_pool_chains) * BLOCK * BLOCKS;
    f_reset(st);
    for (int k = 0; k < BLOCKS; k++) out += (uint64_t)f_cont(st, raw + (size_t)k * BLOCK, dst, BLOCK, (int)sizeof dst, g_accel);
  }
  f_free(st);
  j->out = out;
  return NULL;
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: caccel_refbench <liblz4 .so> <pool file> <n chains> <threads> <acceleration>\n"); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  f_create = (create_t)dlsym(h, "LZ4_createStream"); f_free = (free_t)dlsym(h, "LZ4_freeStream");
  f_reset = (reset_t)dlsym(h, "LZ4_resetStream_fast"); f_cont = (cont_t)dlsym(h, "LZ4_compress_fast_continue");
  if (!f_create || !f_free || !f_reset || !f_cont) { fprintf(stderr, "a symbol is missing\n"); return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* pool = (uint8_t*)malloc((size_t)bytes);
  if (!pool || fread(pool, 1, (size_t)bytes, f) != (size_t)bytes) return 2;
  fclose(f);
  g_pool = pool; g_pool_chains = bytes / (BLOCK * BLOCKS); g_n = atol(argv[3]); g_threads = atoi(argv[4]); g_accel = atoi(argv[5]);
  if (g_pool_chains < 1 || g_n < 1 || g_threads < 1 || g_threads > 256) return 2;
  double best = 1e30;
  uint64_t out = 0;
  for (int pass = 0; pass < 3; pass++) {
    pthread_t th[256]; job_t jobs[256];
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int t = 0; t < g_threads; t++) { jobs[t].t = t; jobs[t].out = 0; pthread_create(&th[t], NULL, work, &jobs[t]); }
    out = 0;
    for (int t = 0; t < g_threads; t++) { pthread_join(th[t], NULL); out += jobs[t].out; }
    clock_gettime(CLOCK_MONOTONIC, &b);
    const double s = (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
    if (s < best) best = s;
  }
  printf("%.6f %llu %llu\n", best, (unsigned long long)g_n * BLOCK * BLOCKS, (unsigned long long)out);
  free(pool);
  return 0;
}
