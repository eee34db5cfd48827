// tests/cpp/host_staging_test.cpp -- the arithmetic of lz4-java_amd/csrc/host_staging.h against naive restatements written here: the
// metadata layouts, the chunk cut, the run plan, the chain-shape check and what a chunk of chains calls its blocks, chains and slots.  It includes nothing else of the project and needs no device;
// tests/test_host_staging.py builds it with the address and undefined-behaviour sanitizers and runs it.  Exit status 0 and "ok", or the
// first failed check on stderr.
#include "../../lz4-java_amd/csrc/host_staging.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#define CHECK(cond, ...)                                                                        \
  do {                                                                                          \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
  } while (0)

using namespace staging;

// ---- layouts ----
struct Span { size_t off, bytes, align; bool result; };
template <class T>
Span span(const Region<T>& r, bool result) { return {r.off, r.bytes(), alignof(T), result}; }

// regions disjoint, aligned and inside the total; the inputs a prefix that [0, upload) covers; the results one contiguous range
// [results, total) that holds nothing else; `zeroed` bytes of results at its start are uploaded too
static void check_layout(const char* what, size_t n, const MetaLayout& l, std::vector<Span> spans, size_t zeroed) {
  std::stable_sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.off < b.off; });   // (empty regions keep their place)
  size_t end = 0, inputs_end = 0, results_begin = l.total;
  bool seen_result = false;
  for (const Span& s : spans) {
    CHECK(s.off % s.align == 0, "%s n=%zu: offset %zu not aligned to %zu", what, n, s.off, s.align);
    CHECK(s.off >= end, "%s n=%zu: region at %zu overlaps the one before (ends %zu)", what, n, s.off, end);
    CHECK(s.off - end < 8, "%s n=%zu: %zu bytes of padding", what, n, s.off - end);
    end = s.off + s.bytes;
    CHECK(end <= l.total, "%s n=%zu: region ends at %zu, total %zu", what, n, end, l.total);
    if (s.result) { if (!seen_result) results_begin = s.off; seen_result = true; }
    else { CHECK(!seen_result, "%s n=%zu: an input behind a result", what, n); inputs_end = end; }
  }
  CHECK(seen_result && end == l.total, "%s n=%zu: total %zu, last region ends %zu", what, n, l.total, end);
  CHECK(l.results == results_begin && l.results_bytes() == l.total - results_begin, "%s n=%zu: results [%zu, +%zu)", what, n, l.results, l.results_bytes());
  CHECK(inputs_end <= l.results, "%s n=%zu: inputs end %zu, results begin %zu", what, n, inputs_end, l.results);
  // one H2D: all inputs, the zeroed results, nothing behind them (alignment padding in front of the results may ride along)
  CHECK(l.upload >= inputs_end && l.upload <= l.results + zeroed && (zeroed == 0 || l.upload == l.results + zeroed), "%s n=%zu: upload %zu, inputs end %zu, results %zu + %zu zeroed",
        what, n, l.upload, inputs_end, l.results, zeroed);
  // zero_results clears exactly [results, upload)
  if (l.total <= (1u << 16)) {
    std::vector<uint8_t> buf(l.total + 1, 0xAB);
    l.zero_results(buf.data());
    for (size_t i = 0; i <= l.total; i++)
      CHECK(buf[i] == ((i >= l.results && i < l.upload) ? 0 : 0xAB), "%s n=%zu: zero_results at byte %zu", what, n, i);
  }
}

static void test_layouts() {
  const size_t counts[] = {0, 1, 2, 3, 7, 64, 1000, (size_t)1 << 20};
  for (size_t nb : counts) {
    for (int cons = 0; cons < 2; cons++) {
      const BlockMeta m(nb, cons != 0);
      CHECK(m.src_off.n == nb && m.dst_off.n == nb && m.src_len.n == nb && m.dst_cap.n == nb && m.out.n == nb && m.consumed.n == (cons ? nb : 0), "block counts");
      check_layout("block", nb, m.l, {span(m.src_off, false), span(m.dst_off, false), span(m.src_len, false), span(m.dst_cap, false), span(m.out, true), span(m.consumed, true)}, 0);
      CHECK(m.l.total == nb * (24 + 4 * (cons ? 2 : 1)), "block n=%zu: total %zu", nb, m.l.total);   // (no padding: the layout the kernels have always seen)
    }
    { const HashMeta<uint32_t> m(nb);
      check_layout("xxh32", nb, m.l, {span(m.off, false), span(m.len, false), span(m.hash, true)}, 0); }
    { const HashMeta<uint64_t> m(nb);
      check_layout("xxh64", nb, m.l, {span(m.off, false), span(m.len, false), span(m.hash, true)}, 0);
      CHECK(m.hash.off == ((nb * 12 + 7) & ~(size_t)7), "xxh64 n=%zu: hashes at %zu", nb, m.hash.off); }
    for (size_t nc : counts) {
      if (nc > nb + 1 && nb != 0) continue;   // (a few more chains than blocks -- empty chains -- is enough)
      { const ChainMeta m(nb, nc);
        CHECK(m.first.n == nc + 1 && m.stored.n == nb && m.chain_out.n == nc && m.out.n == nb && m.prefix.n == nc, "chain counts");
        check_layout("chain", nb * 31 + nc, m.l, {span(m.src_off, false), span(m.chain_dst_off, false), span(m.chain_dst_cap, false), span(m.src_len, false), span(m.dst_cap, false),
                                                  span(m.prefix, false), span(m.first, false), span(m.stored, false), span(m.chain_out, true), span(m.out, true)}, m.chain_out.bytes()); }
      { const CChainMeta m(nb, nc);
        CHECK(m.first.n == nc + 1 && m.consumed.n == nc && m.out.n == nb && m.chain_src_off.n == nc && m.dst_off.n == nb, "cchain counts");
        check_layout("cchain", nb * 31 + nc, m.l, {span(m.chain_src_off, false), span(m.dst_off, false), span(m.src_len, false), span(m.dst_cap, false), span(m.prefix, false),
                                                   span(m.first, false), span(m.consumed, true), span(m.out, true)}, m.l.results_bytes()); }
    }
  }
  // the same offset on both sides
  const ChainMeta m(5, 2);
  alignas(8) uint8_t host[512], dev[512];
  CHECK((uint8_t*)m.out.in(host) - host == (uint8_t*)m.out.in(dev) - dev && (size_t)((uint8_t*)m.out.in(host) - host) == m.out.off, "Region::in");
  // an array asked for out of order only widens the copies
  MetaLayout l;
  const Region<int32_t> a = l.input<int32_t>(3);
  const Region<uint64_t> r = l.result<uint64_t>(2);
  const Region<uint8_t> late = l.input<uint8_t>(5);
  const Region<int32_t> z = l.result<int32_t>(1, true);
  CHECK(a.off == 0 && r.off == 16 && late.off == 32 && z.off == 40 && l.total == 44, "out-of-order offsets");
  CHECK(l.upload == 44 && l.results == 16 && l.results_bytes() == 28, "out-of-order copies");
}

// ---- chunk cut ----
static void test_cut() {
  std::mt19937_64 rng(20240611);
  auto below = [&](uint64_t n) { return (size_t)(rng() % n); };
  size_t lists = 0, multi = 0, capped = 0, oversize = 0;
  for (int round = 0; round < 4000; round++) {
    const uint32_t n = (uint32_t)below(60), first = (uint32_t)below(1000);
    const size_t src_limit = round % 7 == 0 ? SIZE_MAX : 1 + below(5000), dst_limit = round % 3 == 0 ? SIZE_MAX : 1 + below(5000);
    const uint32_t max_units = round % 5 == 0 ? 1 + (uint32_t)below(8) : UINT32_MAX;
    std::vector<Cost> cost(n);
    for (Cost& c : cost) {
      const size_t kind = below(10);
      c.src = kind == 0 ? 0 : kind == 1 ? src_limit / 2 + below(6000) : al16(below(900));          // (zero cost; around or beyond the limit; ordinary)
      c.dst = kind == 2 ? 0 : kind == 3 ? dst_limit / 2 + below(6000) : al16(below(900));
      if (c.src > ((size_t)1 << 40)) c.src = 7000;
      if (c.dst > ((size_t)1 << 40)) c.dst = 7000;
    }
    auto cost_of = [&](uint32_t u) { CHECK(u >= first && u < first + n, "cost of unit %u outside [%u, %u)", u, first, first + n); return cost[u - first]; };
    uint32_t at = first;
    while (at < first + n) {
      const Chunk ck = cut_chunk(at, first + n, max_units, src_limit, dst_limit, cost_of);
      CHECK(ck.end > at && ck.end <= first + n, "round %d: chunk [%u, %u) of [%u, %u)", round, at, ck.end, first, first + n);   // in order, one unit at least
      size_t s = 0, d = 0;
      for (uint32_t u = at; u < ck.end; u++) { s += cost[u - first].src; d += cost[u - first].dst; }
      CHECK(s == ck.src && d == ck.dst, "round %d: chunk sums %zu / %zu, said %zu / %zu", round, s, d, ck.src, ck.dst);
      CHECK(ck.end - at <= max_units, "round %d: %u units, cap %u", round, ck.end - at, max_units);
      if (ck.end - at >= 2) { CHECK(s <= src_limit && d <= dst_limit, "round %d: chunk of %u units over a limit", round, ck.end - at); multi++; }
      else if (s > src_limit || d > dst_limit) oversize++;
      if (ck.end < first + n) {   // it could not have taken its successor
        const Cost nx = cost[ck.end - first];
        const bool full = ck.end - at == max_units;
        CHECK(full || s + nx.src > src_limit || d + nx.dst > dst_limit, "round %d: chunk [%u, %u) left its successor out", round, at, ck.end);
        capped += full;
      }
      at = ck.end;
    }
    CHECK(at == first + n, "round %d: units lost", round);
    const Chunk none = cut_chunk(at, at, max_units, src_limit, dst_limit, cost_of);
    CHECK(none.end == at && none.src == 0 && none.dst == 0, "round %d: the empty range", round);
    lists++;
  }
  CHECK(lists == 4000 && multi > 1000 && capped > 100 && oversize > 100, "cut coverage: %zu lists, %zu multi, %zu capped, %zu oversize", lists, multi, capped, oversize);
}

// ---- run plan ----
static void test_runs() {
  std::mt19937_64 rng(977);
  auto below = [&](uint64_t n) { return (size_t)(rng() % n); };
  size_t merged = 0, split = 0, exact = 0;
  for (int round = 0; round < 3000; round++) {
    const uint32_t n = (uint32_t)below(40);
    std::vector<Run> e(n);
    size_t at = below(3) * 16;
    for (Run& r : e) {
      const size_t room = al16(1 + below(3000));
      r.off = at;
      r.len = below(4) == 0 ? 0 : 1 + below(room);
      // the gap to the next entry's start, from this entry's produced end: around the rule's edge, or anything
      const size_t gaps[] = {4095, 4096, 4097, 0, 1, below(9000), below(9000)};
      const size_t gap = gaps[below(7)];
      at = std::max(r.off + room, r.off + r.len + gap);
    }
    std::vector<std::pair<size_t, size_t>> got;
    const int rc = for_each_run(n, [&](uint32_t t) { return e[t]; }, [&](size_t a, size_t b) { got.push_back({a, b}); return 0; });
    CHECK(rc == 0, "round %d: rc %d", round, rc);
    // naive: every produced entry is a range; neighbours at most 4096 bytes apart are joined
    std::vector<std::pair<size_t, size_t>> want;
    for (const Run& r : e) {
      if (!r.len) continue;
      if (!want.empty() && r.off <= want.back().second + 4096) want.back().second = r.off + r.len;
      else want.push_back({r.off, r.off + r.len});
    }
    CHECK(got == want, "round %d: %zu ranges, naive %zu", round, got.size(), want.size());
    for (size_t k = 0; k < got.size(); k++) {
      CHECK(got[k].first < got[k].second, "round %d: empty range", round);
      if (k) {
        CHECK(got[k].first > got[k - 1].second + 4096, "round %d: ranges %zu bytes apart", round, got[k].first - got[k - 1].second);
        exact += got[k].first == got[k - 1].second + 4097;
        split++;
      }
      bool starts = false, ends = false;
      for (const Run& r : e) { starts |= r.len && r.off == got[k].first; ends |= r.len && r.off + r.len == got[k].second; }
      CHECK(starts && ends, "round %d: range [%zu, %zu) not on entry boundaries", round, got[k].first, got[k].second);
    }
    for (const Run& r : e) {   // every produced byte is covered
      if (!r.len) continue;
      bool in = false;
      for (auto& g : got) in |= g.first <= r.off && r.off + r.len <= g.second;
      CHECK(in, "round %d: entry [%zu, +%zu) not covered", round, r.off, r.len);
    }
    size_t produced = 0;
    for (const Run& r : e) produced += r.len != 0;
    merged += produced - got.size();
  }
  CHECK(merged > 1000 && split > 1000 && exact > 100, "run coverage: %zu merged, %zu split, %zu at 4097", merged, split, exact);
  // an error ends the walk and is passed on
  const Run far[3] = {{0, 10}, {10000, 10}, {30000, 10}};
  int calls = 0;
  CHECK(for_each_run(3, [&](uint32_t t) { return far[t]; }, [&](size_t, size_t) { return ++calls == 2 ? 77 : 0; }) == 77 && calls == 2, "error from copy");
  CHECK(for_each_run(0, [&](uint32_t t) { return far[t]; }, [&](size_t, size_t) { return 1; }) == 0, "no entries");
}

// ---- chain shape ----
static void test_shape() {
  struct Case { std::vector<uint32_t> first; uint32_t n_blocks; std::vector<int32_t> prefix; std::vector<uint64_t> off; const char* dst; const char* src; };
  const char* const ends = "chain_first must start at 0 and end at n_blocks";
  const char* const asc = "chain_first must be ascending";
  const char* const neg = "negative chain_prefix_len";
  const Case cases[] = {
      {{0, 2, 5}, 5, {0, 3}, {0, 3}, nullptr, nullptr},
      {{0, 0, 0}, 0, {0, 0}, {0, 0}, nullptr, nullptr},                        // empty chains
      {{0, 2, 5}, 5, {}, {0, 0}, nullptr, nullptr},                            // no prefix array: the offsets are not looked at
      {{0}, 0, {}, {}, nullptr, nullptr},                                      // no chains
      {{1, 2, 5}, 5, {0, 0}, {0, 0}, ends, ends},
      {{0, 2, 4}, 5, {0, 0}, {0, 0}, ends, ends},
      {{0, 2, 6}, 5, {0, 0}, {0, 0}, ends, ends},
      {{0}, 3, {}, {}, ends, ends},
      {{0, 4, 2, 5}, 5, {0, 0, 0}, {0, 0, 0}, asc, asc},
      {{0, 6, 5}, 5, {-1, 0}, {0, 0}, neg, neg},                               // (chain 0's prefix is looked at before chain 1's range)
      {{0, 6, 5}, 5, {0, -1}, {0, 0}, asc, asc},
      {{0, 2, 5}, 5, {0, -1}, {0, 100}, neg, neg},
      {{0, 2, 5}, 5, {INT32_MIN, 0}, {9, 9}, neg, neg},
      {{0, 2, 5}, 5, {4, 0}, {3, 0}, "chain_prefix_len reaches in front of dst", "chain_prefix_len reaches in front of src"},
      {{0, 2, 5}, 5, {3, 1}, {3, 0}, "chain_prefix_len reaches in front of dst", "chain_prefix_len reaches in front of src"},
      {{0, 2, 5}, 5, {3, 70000}, {3, 70000}, nullptr, nullptr},
      {{0, 2, 5}, 5, {0, INT32_MAX}, {0, (uint64_t)INT32_MAX - 1}, "chain_prefix_len reaches in front of dst", "chain_prefix_len reaches in front of src"},
      {{0, 2, 1}, 5, {0, -1}, {0, 0}, ends, ends},                             // (the ends come first)
  };
  int k = 0;
  for (const Case& c : cases) {
    const uint32_t nc = (uint32_t)c.first.size() - 1;
    for (int in_dst = 0; in_dst < 2; in_dst++) {
      const char* got = chain_shape_error(c.first.data(), nc, c.n_blocks, c.prefix.empty() ? nullptr : c.prefix.data(), c.off.data(), in_dst != 0);
      const char* want = in_dst ? c.dst : c.src;
      CHECK((got == nullptr) == (want == nullptr) && (!got || std::string(got) == want), "shape case %d (%s): \"%s\", expected \"%s\"", k, in_dst ? "dst" : "src",
            got ? got : "(none)", want ? want : "(none)");
    }
    k++;
  }
}

// ---- what a chunk of chains calls its blocks, chains and slots ----
static void test_chain_frame() {
  int cases = 0;
  // packed offsets: negative and zero lengths take no bytes, every other block starts on the next 16-byte boundary
  const int32_t len[] = {5, -1, 0, 16, 17, INT32_MIN, 4096, 1, -7, 33};
  const uint64_t want_off[] = {0, 16, 16, 16, 32, 64, 64, 4160, 4176, 4176};
  std::vector<uint64_t> off(3, 99);   // (resized, not appended to)
  CHECK(packed_offsets(len, 10, off) == 4176 + 48 && off == std::vector<uint64_t>(want_off, want_off + 10), "packed offsets of 10 blocks"); cases++;
  CHECK(packed_offsets(len + 3, 2, off) == 48 && off == std::vector<uint64_t>({0, 16}), "packed offsets from block 3"); cases++;
  CHECK(packed_offsets(len, 0, off) == 0 && off.empty(), "packed offsets of no blocks"); cases++;
  std::mt19937_64 rng(31);
  for (int round = 0; round < 500; round++) {   // against the naive sum, and against chain_packed_bytes over any cut into chains
    const size_t n = rng() % 50;
    std::vector<int32_t> l(n);
    for (int32_t& v : l) v = (int32_t)(rng() % 5 == 0 ? -(int64_t)(rng() % 100000) : rng() % 3 ? rng() % 70 : rng() % 100000);
    const size_t total = packed_offsets(l.data(), n, off);
    size_t at = 0;
    for (size_t t = 0; t < n; t++) {
      CHECK(off[t] == at && at % 16 == 0, "round %d: block %zu at %zu, naive %zu", round, t, (size_t)off[t], at);
      at += l[t] > 0 ? ((size_t)l[t] + 15) / 16 * 16 : 0;
    }
    CHECK(total == at, "round %d: total %zu, naive %zu", round, total, at);
    std::vector<uint32_t> first{0};
    while (first.back() < n) first.push_back(std::min<uint32_t>((uint32_t)n, first.back() + (uint32_t)(rng() % 7)));   // (empty chains included)
    size_t sum = 0;
    for (uint32_t c = 0; c + 1 < first.size(); c++) {
      const size_t b = chain_packed_bytes(first.data(), c, l.data());
      CHECK(b == (first[c + 1] < n ? off[first[c + 1]] : total) - (first[c] < n ? off[first[c]] : total), "round %d: chain %u takes %zu", round, c, b);
      sum += b;
    }
    CHECK(sum == total, "round %d: the chains take %zu of %zu", round, sum, total);
    cases++;
  }
  // the per-chain sum: an empty chain at the front, in the middle and at the end takes nothing, whatever its neighbours hold
  const uint32_t cf[] = {0, 0, 2, 2, 5, 5};
  const int32_t cl[] = {100, -3, 7, 16, 0};
  const size_t want_sum[] = {0, 112, 0, 32, 0};
  for (uint32_t c = 0; c < 5; c++) { CHECK(chain_packed_bytes(cf, c, cl) == want_sum[c], "chain %u of the empty-chain case", c); cases++; }
  // first[] rebased: a chunk that starts at chain 0, one that does not, one of a single empty chain, one of no chains
  const uint32_t first[] = {0, 3, 3, 10, 11, 40, 40, 57};
  uint32_t out[9];
  auto rebased = [&](uint32_t c, uint32_t nc, std::vector<uint32_t> want) {
    std::fill(out, out + 9, 0xDEADu);
    rebase_first(first, c, nc, out);
    for (uint32_t t = 0; t <= nc; t++) CHECK(out[t] == want[t], "rebase_first(%u, %u)[%u] = %u", c, nc, t, out[t]);
    CHECK(out[nc + 1] == 0xDEADu, "rebase_first(%u, %u) wrote past first[nc]", c, nc);
    cases++;
  };
  rebased(0, 7, {0, 3, 3, 10, 11, 40, 40, 57});
  rebased(0, 2, {0, 3, 3});
  rebased(2, 3, {0, 7, 8, 37});
  rebased(3, 4, {0, 1, 30, 30, 47});
  rebased(5, 1, {0, 0});
  rebased(6, 1, {0, 17});
  rebased(4, 0, {0});
  // the slot words: a share whose slot 0 is stream 100 (and one whose slot 0 is stream 0), with and without marks; the marks are by id
  std::vector<uint8_t> poisoned(200, 0);
  poisoned[104] = 1; poisoned[4] = 1; poisoned[199] = 1;   // (4 = 104 - 100: a mark looked up by slot would stop the wrong stream)
  const uint32_t ids[] = {100, 101, 104, 150, 199};
  uint32_t slot[6] = {7, 7, 7, 7, 7, 7};
  stream_slots(ids, 5, 100, poisoned.data(), slot);
  CHECK(slot[0] == 0 && slot[1] == 1 && slot[2] == (4u | 0x80000000u) && slot[3] == 50 && slot[4] == (99u | 0x80000000u) && slot[5] == 7, "slots of a share from 100, marked"); cases++;
  stream_slots(ids, 5, 100, nullptr, slot);
  CHECK(slot[0] == 0 && slot[1] == 1 && slot[2] == 4 && slot[3] == 50 && slot[4] == 99 && slot[5] == 7, "slots of a share from 100, no marks"); cases++;
  stream_slots(ids + 2, 2, 100, poisoned.data(), slot);   // (a later chunk of the share: the ids from chain 2 on)
  CHECK(slot[0] == (4u | 0x80000000u) && slot[1] == 50 && slot[2] == 4, "slots of a chunk that starts at chain 2"); cases++;
  const uint32_t low[] = {0, 4, 5};
  stream_slots(low, 3, 0, poisoned.data(), slot);
  CHECK(slot[0] == 0 && slot[1] == (4u | 0x80000000u) && slot[2] == 5, "slots of a share from 0"); cases++;
  stream_slots(low, 0, 0, poisoned.data(), slot);
  CHECK(slot[0] == 0, "no chains, no slots"); cases++;
  CHECK(kSlotForceStop == 0x80000000u && pos(-1) == 0 && pos(0) == 0 && pos(INT32_MIN) == 0 && pos(INT32_MAX) == (size_t)INT32_MAX, "the mark and pos"); cases++;
  fprintf(stderr, "chain frame helpers (packed_offsets, chain_packed_bytes, rebase_first, stream_slots): %d cases\n", cases);
}

int main() {
  CHECK(al16(0) == 0 && al16(1) == 16 && al16(16) == 16 && al16(17) == 32, "al16");
  test_layouts();
  test_cut();
  test_runs();
  test_shape();
  test_chain_frame();
  puts("ok");
  return 0;
}
