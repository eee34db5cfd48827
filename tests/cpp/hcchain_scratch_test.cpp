// tests/cpp/hcchain_scratch_test.cpp -- the scratch layout of the HC chain compressor (staging::HcChainScratchLayout of
// lz4-java_amd/csrc/host_staging.h) against restatements written here: the arrays are disjoint, aligned, in order and fill the total;
// max_items is enough for every way of laying chains side by side inside a span, for every segment size the knob allows.  It includes
// nothing else of the project and needs no device; tests/test_hcchain_scratch.py builds it with the address and undefined-behaviour
// sanitizers and runs it.  Exit status 0 and "ok", or the first failed check on stderr.
#include "../../lz4-java_amd/csrc/host_staging.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(cond, ...)                                                                        \
  do {                                                                                          \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
  } while (0)

using staging::HcChainScratchLayout;

// the items the layout kernel lists for a chain whose buffer (kept history + sources) is n bytes long
static uint64_t items_of(uint64_t n, uint32_t seg) { return n >= 4 ? (n - 3 + seg - 1) / seg : 0; }

int main() {
  const uint32_t segs[] = {4096u, 4097u, 65536u, 1u << 20, 1u << 30};
  const uint32_t counts[] = {0u, 1u, 2u, 3u, 16u, 1000u, 1u << 20};
  for (uint32_t seg : segs)
    for (uint32_t nb : counts)
      for (uint32_t nc : counts)
        for (uint64_t span : {(uint64_t)0, (uint64_t)80, (uint64_t)4095, (uint64_t)4096, (uint64_t)1 << 20, ((uint64_t)1 << 32) + 5, (uint64_t)1 << 44}) {
          const HcChainScratchLayout l(span, nb, nc, seg);
          CHECK(l.blk_start == 0 && l.chain_buf == 8u * (size_t)nb && l.chain_len == l.chain_buf + 8u * (size_t)nc, "the 8-byte arrays");
          CHECK(l.items == l.chain_len + 8u * (size_t)nc && l.blk_hist == l.items + 8u * (size_t)l.max_items, "items and blk_hist");
          CHECK(l.words == l.blk_hist + 4u * (size_t)nb && l.total == l.words + 8u, "words and total");
          CHECK(l.chain_buf % 8 == 0 && l.chain_len % 8 == 0 && l.items % 8 == 0 && l.blk_hist % 4 == 0 && l.words % 4 == 0, "alignment");
          const uint64_t want = span / seg + nc + 1u;   // (capped where a uint32_t ends)
          CHECK((uint64_t)l.max_items == (want > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : want), "max_items %u for span %llu, %u chains, seg %u", l.max_items, (unsigned long long)span, nc, seg);
        }
  // the cap where a uint32_t ends
  CHECK(HcChainScratchLayout(~(uint64_t)0, 1, 1, 4096).max_items == 0xFFFFFFF0u, "the cap");
  CHECK(HcChainScratchLayout((uint64_t)0xFFFFFFF0u * 4096u, 0, 0, 4096).max_items == 0xFFFFFFF0u, "at the cap");
  CHECK(HcChainScratchLayout((uint64_t)0xFFFFFFEEu * 4096u, 0, 0, 4096).max_items == 0xFFFFFFEFu, "under the cap");
  // chains laid side by side inside a span never list more items than max_items
  std::mt19937_64 rng(20240907);
  size_t tight = 0;
  for (int round = 0; round < 20000; round++) {
    const uint32_t seg = segs[rng() % 3] + (round % 5 == 0 ? (uint32_t)(rng() % 1000) : 0u);
    const uint32_t nc = 1 + (uint32_t)(rng() % 40);
    uint64_t at = rng() % 100, items = 0;
    for (uint32_t c = 0; c < nc; c++) {
      const uint64_t kind = rng() % 6;
      const uint64_t n = kind == 0 ? rng() % 8 : kind == 1 ? (uint64_t)seg * (1 + rng() % 4) + rng() % 8 : kind == 2 ? seg + 3 : rng() % (5 * (uint64_t)seg);
      items += items_of(n, seg);
      at += n + rng() % 3;   // (regions do not overlap; gaps are allowed)
    }
    const HcChainScratchLayout l(at, 7, nc, seg);
    CHECK(items <= l.max_items, "round %d: %llu items, room for %u", round, (unsigned long long)items, l.max_items);
    tight += items + nc + 1 >= l.max_items;
  }
  CHECK(tight > 100, "the bound was never near: %zu", tight);
  puts("ok");
  return 0;
}
