// tests/cpp/hcstream_staging_test.cpp -- host code only, built with the address and undefined-behaviour sanitizers
// (tests/test_hcstream_abi.py).  The state machine and the linear image of lz4-java_amd/csrc/host_staging.h (HcsImage: what
// hcstream_host_shard stages for lz4hip_compress_hc_stream_batch) against a naive restatement: the stream's WHOLE life as one list that
// says, for every index liblz4 ever gave a byte, where that byte lies in the caller's memory, with liblz4's lowLimit and dictLimit and
// the run ends as indexes.  Random streams -- rings, jumps, contiguous runs, 0-byte blocks, blocks that cannot run, LZ4_loadDictHC,
// LZ4_saveDictHC -- cut into calls at random.  Per block: every byte the block can reach is in its view, at its place; low and dlim are
// liblz4's, cut to the view; the run ends in reach are the list's; behind every call the state is the list's.  Then several streams
// in one image behind a non-zero first stream: every stream's part is what the stream gives alone, at its place.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>
#include "../../lz4-java_amd/csrc/host_staging.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "hcstream_staging_test: line %d: %s (scenario %d)\n", __LINE__, #c, scenario); exit(1); } } while (0)
static int scenario = 0;

struct Naive {
  std::vector<uint64_t> addr;     // addr[i] = where the byte of index i lies
  std::vector<uint64_t> ends;     // indexes at which a jump ended a run
  uint64_t low = 0, dlim = 0;     // liblz4's lowLimit and dictLimit (index 0 = the stream's first byte)
  uint64_t at = 0;                // where the prefix ends (meaningful from the first block or load on)
  void jump(uint64_t s) { low = dlim; dlim = addr.size(); ends.push_back(addr.size()); at = s; }
  void enter(uint64_t s, uint64_t n, bool runs) {
    if (s != at) jump(s);
    if (runs && dlim > low) {
      const uint64_t dend = addr[dlim - 1] + 1, dbegin = dend - (dlim - low);
      if (s + n > dbegin && s < dend) {
        low = dlim - (dend - std::min(s + n, dend));
        if (dlim - low < 4) low = dlim;
      }
    }
  }
  void take(uint64_t s, uint64_t n) { for (uint64_t i = 0; i < n; i++) addr.push_back(s + i); at = s + n; }
  void load(uint64_t end, uint64_t len) {
    *this = Naive();
    const uint64_t k = std::min<uint64_t>(len, 65536);
    take(end - k, k);
  }
  int save(uint64_t buf, int k) {
    uint64_t kept = k < 0 ? 0 : std::min<uint64_t>((uint64_t)k, 65536);
    if (kept < 4) kept = 0;
    kept = std::min<uint64_t>(kept, addr.size() - dlim);
    for (uint64_t i = 0; i < kept; i++) addr[addr.size() - kept + i] = buf + i;
    dlim = low = addr.size() - kept;
    at = buf + kept;
    return (int)kept;
  }
  bool same(const staging::HcsState& st) const {
    if (st.index != addr.size() || st.prefix_len != addr.size() - dlim || st.ext_len != dlim - low || st.prefix_end != at) return false;
    return st.ext_len == 0 || st.ext_end == addr[dlim - 1] + 1;
  }
};

int main() {
  std::mt19937_64 rng(20261020);
  auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  const uint64_t ARENA = 400000;
  std::vector<uint8_t> arena(ARENA);
  for (auto& b : arena) b = (uint8_t)rng();
  long blocks_checked = 0, jumps = 0, trims = 0;
  for (scenario = 0; scenario < 300; scenario++) {
    Naive nv;
    staging::HcsState st{0, 0, 0, 0, 0};
    const uint64_t ring = 3000 + pick(80000);
    const int calls = 1 + (int)pick(8);
    for (int c = 0; c < calls; c++) {
      if (pick(6) == 0) {   // a state edit in front of the call
        if (pick(2) && nv.addr.size()) {
          const uint64_t buf = 300000 + pick(1000);
          const int k = (int)pick(5) == 0 ? (int)pick(8) : (int)pick(70000);
          const int kept = nv.save(buf, k);
          CHECK(staging::hcs_save_dict(st, buf, k) == kept);
        } else {
          const uint64_t len = pick(3) ? pick(5000) : pick(80000), end = len + pick(1000);
          nv.load(end, len);
          st = staging::hcs_load_dict(end, len);
        }
        CHECK(nv.same(st));
      }
      const uint32_t nb = (uint32_t)pick(7);
      std::vector<uint64_t> off(nb);
      std::vector<int32_t> len(nb);
      uint64_t cursor = nv.at;
      for (uint32_t i = 0; i < nb; i++) {
        const uint64_t r = pick(10);
        len[i] = r == 0 ? -1 - (int32_t)pick(5) : r == 1 ? (int32_t)pick(14) : r == 2 ? (int32_t)pick(70000) : (int32_t)pick(3000);
        if (pick(40) == 0) len[i] = 0x7E000001;
        const uint64_t n = staging::hcs_runs(len[i]) ? (uint64_t)len[i] : 0;
        if (pick(3) == 0 || cursor + n > ring) cursor = pick(5) ? 0 : pick(ring / 2);   // a jump: the ring wraps, or anywhere
        if (cursor + n > ARENA - 1) cursor = 0;
        off[i] = cursor;
        cursor += n;
      }
      const uint32_t first[2] = {0, nb};
      CHECK(staging::hcstream_shape_error(&st, first, 1, nb, len.data()) == nullptr);
      const staging::HcsImage im(&st, first, 0, 1, off.data(), len.data());
      CHECK(im.total == staging::hcstream_cost(st, first, 0, len.data()));
      std::vector<uint8_t> image(im.total);   // exactly: a piece that reached past it would be the sanitizer's finding
      for (const staging::HcsPiece& p : im.pieces) {
        CHECK(p.dev + p.len <= im.total && p.src + p.len <= ARENA);
        for (size_t i = 0; i < p.len; i++) image[p.dev + i] = arena[p.src + i];
      }
      CHECK(std::is_sorted(im.ends.begin(), im.ends.end()));
      for (uint32_t i = 0; i < nb; i++) {
        const bool runs = staging::hcs_runs(len[i]);
        const uint64_t n = runs ? (uint64_t)len[i] : 0;
        const uint64_t low0 = nv.low;
        const size_t e0 = nv.ends.size();
        nv.enter(off[i], n, runs);
        const bool jumped = nv.ends.size() != e0;
        jumps += jumped;
        trims += nv.low != low0 && nv.ends.size() == e0;
        const uint64_t blk = nv.addr.size();                                   // the block's first index
        const uint64_t hist = im.blk_hist[i], view = blk - hist;               // the view's first index
        CHECK(hist <= 65536 && hist <= blk && im.blk_start[i] >= im.buf_off[0] + hist);
        const uint64_t reach = std::max(nv.low, blk > 65535 ? blk - 65535 : 0);   // the lowest index the block's searches can name
        CHECK(view <= reach);
        CHECK(im.blk_low[i] == std::max(nv.low, view) - view && im.blk_dlim[i] == std::max(nv.dlim, view) - view);
        CHECK(im.blk_low[i] <= im.blk_dlim[i] && im.blk_dlim[i] <= hist);
        const uint64_t from = std::max(reach, view);
        for (uint64_t x = from; x < blk; x++) CHECK(image[im.blk_start[i] - (blk - x)] == arena[nv.addr[x]]);
        if (runs) {
          for (uint64_t x = 0; x < n; x++) CHECK(image[im.blk_start[i] + x] == arena[off[i] + x]);
          nv.take(off[i], n);
        }
        // the run ends in reach of the block, as buffer positions
        const uint64_t buf0 = blk - (im.blk_start[i] - im.buf_off[0]);        // the index of the buffer's first byte
        std::vector<uint64_t> want, got;
        for (uint64_t e : nv.ends) if (e > from && e < blk) want.push_back(e);
        for (uint32_t e : im.ends) if (buf0 + e > from && buf0 + e < blk) got.push_back(buf0 + e);
        want.erase(std::unique(want.begin(), want.end()), want.end());
        CHECK(want == got);
        // (an end AT the block's first index is this block's own jump -- or that of a later block behind blocks of no bytes)
        if (jumped && blk > buf0) CHECK(std::binary_search(im.ends.begin(), im.ends.end(), (uint32_t)(blk - buf0)));
        blocks_checked++;
      }
      CHECK(im.buf_len[0] <= im.total && im.after.size() == 1);
      st = im.after[0];
      CHECK(nv.same(st));
    }
  }
  // several streams in ONE image, behind streams the chunk does not hold (c0 > 0), as hcstream_host_shard builds it: every stream's part --
  // its buffer's offset, its blocks' numbers (rebased to the chunk's first block), its slice of the run ends, its pieces, its state -- is
  // what the stream gives alone (checked against the naive restatement above), moved to its place; total is the sum of the streams' costs
  long streams_checked = 0;
  for (scenario = 1000; scenario < 1120; scenario++) {
    const uint32_t c0 = (uint32_t)pick(4), ns = 2 + (uint32_t)pick(6), all = c0 + ns;
    std::vector<staging::HcsState> states(all);
    std::vector<uint32_t> first(all + 1, 0);
    std::vector<uint64_t> off;
    std::vector<int32_t> len;
    for (uint32_t c = 0; c < all; c++) {
      staging::HcsState st{0, 0, 0, 0, 0};
      if (pick(3) == 0) st = staging::hcs_load_dict(2000 + pick(70000), pick(2) ? pick(2000) : pick(70000) % 2000);
      if (pick(2)) {   // a stream that has run: a prefix and an external dictionary somewhere
        const uint64_t pl = pick(3) ? pick(5000) : 60000 + pick(10000), el = pick(3) ? pick(5000) : pick(70000);
        st = staging::HcsState{100000 + pl, pl, 90000 + el, el, pl + el + pick(100000)};
      }
      states[c] = st;
      const uint32_t nb = (uint32_t)pick(6);
      uint64_t cursor = st.prefix_end;
      for (uint32_t i = 0; i < nb; i++) {
        const uint64_t r = pick(10);
        const int32_t l = r == 0 ? -1 : r == 1 ? (int32_t)pick(14) : (int32_t)pick(3000);
        const uint64_t n = staging::hcs_runs(l) ? (uint64_t)l : 0;
        if (pick(3) == 0) cursor = 200000 + pick(100000);
        off.push_back(cursor); len.push_back(l);
        cursor += n;
      }
      first[c + 1] = (uint32_t)off.size();
    }
    CHECK(staging::hcstream_shape_error(states.data(), first.data(), all, first[all], len.data()) == nullptr);
    const staging::HcsImage im(states.data(), first.data(), c0, ns, off.data(), len.data());
    const uint32_t b0 = first[c0];
    CHECK(im.blk_start.size() == first[all] - b0 && im.buf_off.size() == ns && im.end_first.size() == ns + 1 && im.after.size() == ns);
    CHECK(im.end_first[0] == 0 && im.end_first[ns] == im.ends.size());
    size_t sum = 0, piece = 0;
    for (uint32_t t = 0; t < ns; t++) {
      const uint32_t f0 = first[c0 + t], nb = first[c0 + t + 1] - f0;
      const uint32_t one_first[2] = {0, nb};
      const staging::HcsImage one(&states[c0 + t], one_first, 0, 1, off.data() + f0, len.data() + f0);
      CHECK(im.buf_off[t] == sum && im.buf_len[t] == one.buf_len[0]);
      CHECK(memcmp(&im.after[t], &one.after[0], sizeof(staging::HcsState)) == 0);
      CHECK(im.end_first[t + 1] - im.end_first[t] == one.ends.size());
      for (size_t e = 0; e < one.ends.size(); e++) CHECK(im.ends[im.end_first[t] + e] == one.ends[e]);
      for (uint32_t i = 0; i < nb; i++) {
        const uint32_t g = f0 - b0 + i;
        CHECK(im.blk_start[g] == one.blk_start[i] + sum && im.blk_hist[g] == one.blk_hist[i] && im.blk_low[g] == one.blk_low[i] && im.blk_dlim[g] == one.blk_dlim[i]);
      }
      for (const staging::HcsPiece& q : one.pieces) {
        CHECK(piece < im.pieces.size());
        const staging::HcsPiece& m = im.pieces[piece++];
        CHECK(m.src == q.src && m.len == q.len && m.dev == q.dev + sum);
      }
      CHECK(one.total == staging::hcstream_cost(states[c0 + t], first.data(), c0 + t, len.data()));
      sum += one.total;
      streams_checked++;
    }
    CHECK(piece == im.pieces.size() && im.total == sum);
  }
  CHECK(streams_checked > 400);
  // the argument errors
  {
    const uint32_t first[2] = {0, 1}, bad_first[2] = {1, 1};
    const int32_t one[1] = {10};
    staging::HcsState a{5, 6, 0, 0, 6}, b{5, 2, 3, 4, 2}, c{0, 0, 0, 0, (1ull << 31) - 65536 - 9}, ok{0, 0, 0, 0, (1ull << 31) - 65536 - 10};
    CHECK(staging::hcstream_shape_error(&a, first, 1, 1, one) && staging::hcstream_shape_error(&b, first, 1, 1, one));
    CHECK(staging::hcstream_shape_error(&c, first, 1, 1, one) && !staging::hcstream_shape_error(&ok, first, 1, 1, one));
    CHECK(staging::hcstream_shape_error(&ok, bad_first, 1, 1, one));
  }
  CHECK(blocks_checked > 2000 && jumps > 500 && trims > 20);
  printf("hcstream staging ok: %ld blocks, %ld jumps, %ld trims\n", blocks_checked, jumps, trims);
  return 0;
}
