// tests/cpp/cxstream_staging_test.cpp -- TEST INFRASTRUCTURE ONLY.
// The staging arithmetic of the stream compressor for sources that land anywhere (lz4-java_amd/csrc/host_staging.h: cxstream_piece,
// cxstream_shape_error, cxstream_hull, cxstream_cost, CxImage, CXStreamMeta) against a naive restatement, on random windows, sources
// and histories.  Host code alone: built with the address and undefined-behaviour sanitizers by tests/test_cxstream_abi.py
// (support.build_sanitized) and run as a program of its own.
// Prints "cxstream staging ok: <cases> cases"; exit code 1 and a message on the first disagreement.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../lz4-java_amd/csrc/host_staging.h"

using namespace staging;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "cxstream_staging_test: line %d: %s (case %d)\n", __LINE__, #c, g_case); exit(1); } } while (0)
static int g_case = 0;

// byte by byte: 'i' every byte of [end - keep, end) lies in the window, 'o' none does, 's' some do
static char naive_where(uint64_t end, uint64_t keep, uint64_t wo, uint64_t wl) {
  if (wl == 0 && end - keep < wo && wo < end) return 's';   // (an empty window still has edges: a piece across them straddles)
  uint64_t in = 0;
  for (uint64_t b = end - keep; b < end; b++) in += (b >= wo && b < wo + wl) ? 1u : 0u;
  return in == keep ? 'i' : (in == 0 ? 'o' : 's');
}

int main() {
  std::mt19937_64 rng(4711);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  // ---- one piece against one window (small numbers, so that the byte-by-byte restatement is cheap; the 65536 cut apart) ----
  for (g_case = 0; g_case < 200000; g_case++) {
    const uint64_t wo = pick(0, 300), wl = pick(0, 200), end = pick(0, 700);
    const int32_t len = (int32_t)pick(0, 125) - 5;
    DsPiece p;
    const char* why = cxstream_piece(end, len, wo, wl, &p);
    if (len < 0) { CHECK(why != nullptr); continue; }
    if (len == 0) { CHECK(!why && p.kind == DS_NONE && p.keep == 0); continue; }
    if ((uint64_t)len > end) { CHECK(why != nullptr); continue; }
    const char w = naive_where(end, (uint64_t)len, wo, wl);
    if (w == 's') { CHECK(why != nullptr); continue; }
    CHECK(!why && p.keep == (uint64_t)len);
    if (w == 'i') CHECK(p.kind == DS_INSIDE);
    else CHECK(p.kind == (end == wo ? DS_LEAD : DS_APART));
  }
  { DsPiece p;   // only the last 65536 bytes are a piece: a history of 70000 bytes that BEGINS in front of the window is inside it
    CHECK(!cxstream_piece(170000, 70000, 104464, 100000, &p) && p.kind == DS_INSIDE && p.keep == 65536);
    CHECK(cxstream_piece(170000, 70000, 104465, 100000, &p) != nullptr);
    CHECK(!cxstream_piece(70000, 70000, 70000, 10, &p) && p.kind == DS_LEAD && p.keep == 65536); }
  // ---- whole chunks: hulls, placement, device offsets ----
  for (g_case = 0; g_case < 3000; g_case++) {
    const uint32_t nc = (uint32_t)pick(1, 12);
    std::vector<uint64_t> wo(nc), wl(nc), he(nc);
    std::vector<int32_t> hl(nc);
    const uint64_t shared_end = pick(1, 70000), shared_len = pick(1, shared_end);   // one dictionary in front of everything
    uint64_t at = 80000;
    std::vector<uint32_t> first{0};
    std::vector<uint64_t> so;
    std::vector<int32_t> sl;
    for (uint32_t t = 0; t < nc; t++) {
      at += pick(0, 300);
      wo[t] = at; wl[t] = pick(0, 5000); at += wl[t];
      switch (rng() % 5) {
        case 0: he[t] = pick(0, 1000); hl[t] = 0; break;                                                                  // none
        case 1: he[t] = shared_end; hl[t] = (int32_t)shared_len; break;                                                   // the shared dictionary
        case 2: if (wl[t]) { he[t] = wo[t] + pick(1, wl[t]); hl[t] = (int32_t)pick(1, he[t] - wo[t]); } else { he[t] = 0; hl[t] = 0; } break;   // inside
        case 3: he[t] = wo[t]; hl[t] = (int32_t)pick(1, 70000); break;                                                    // ends where the window begins
        default: he[t] = at + 100000 + pick(0, 999); hl[t] = (int32_t)pick(1, 70000); break;                              // behind everything
      }
      for (uint64_t k = pick(0, 4); k; k--) {
        const uint64_t o = pick(0, wl[t]);
        so.push_back(wo[t] + o);
        sl.push_back(rng() % 8 == 0 ? -(int32_t)pick(1, 9) : (int32_t)pick(0, wl[t] - o));
      }
      first.push_back((uint32_t)so.size());
    }
    so.push_back(0); sl.push_back(0);   // (never empty)
    CHECK(cxstream_shape_error(first.data(), nc, first.back(), so.data(), sl.data(), he.data(), hl.data(), wo.data(), wl.data()) == nullptr);
    const CxImage im(first.data(), 0, nc, so.data(), sl.data(), he.data(), hl.data(), wo.data(), wl.data());
    struct Reg { size_t b, e; };
    std::vector<Reg> regs;
    size_t cost = 0;
    for (uint32_t t = 0; t < nc; t++) {
      // the hull, restated: the lowest and highest byte any source or reachable piece names
      uint64_t lo = UINT64_MAX, hi = 0;
      for (uint32_t i = first[t]; i < first[t + 1]; i++) {
        const uint64_t n = sl[i] > 0 ? (uint64_t)sl[i] : 0;
        lo = std::min(lo, so[i]); hi = std::max(hi, so[i] + n);
      }
      const DsPiece& p = im.piece[t];
      if (p.kind == DS_INSIDE || p.kind == DS_LEAD) { lo = std::min(lo, he[t] - p.keep); hi = std::max(hi, he[t]); }
      if (lo == UINT64_MAX) { lo = hi = wo[t]; }
      CHECK(im.hull[t].lo == lo && im.hull[t].hi == hi);
      CHECK(im.base[t] % 16 == 0);
      regs.push_back(Reg{im.base[t], im.base[t] + (size_t)(hi - lo)});
      cost += cxstream_cost(im.hull[t], p);
      // every source and every piece byte has its place in the region, at the same distance from its neighbours
      for (uint32_t i = first[t]; i < first[t + 1]; i++) {
        const uint64_t n = sl[i] > 0 ? (uint64_t)sl[i] : 0;
        CHECK(im.to_dev(t, so[i]) >= regs.back().b && im.to_dev(t, so[i]) + n <= regs.back().e);
        CHECK(im.to_dev(t, so[i]) - im.base[t] == so[i] - lo);
      }
      if (p.kind == DS_NONE) CHECK(im.hist_dev[t] == 0 && hl[t] == 0);
      if (p.kind == DS_INSIDE || p.kind == DS_LEAD) CHECK(im.hist_dev[t] == im.to_dev(t, he[t]) && im.hist_dev[t] - p.keep >= regs.back().b && im.hist_dev[t] <= regs.back().e);
      if (p.kind == DS_APART) {
        bool found = false;
        for (const DsApart& a : im.apart) found |= a.end == he[t] && a.keep == p.keep && a.dev + a.keep == im.hist_dev[t];
        CHECK(found);
        // a piece apart lies behind every hull: its end is no source's offset, and no source ends inside it
        for (uint32_t i = first[t]; i < first[t + 1]; i++) CHECK(im.to_dev(t, so[i]) + (sl[i] > 0 ? (uint64_t)sl[i] : 0) <= im.hist_dev[t] - p.keep);
      }
    }
    for (const DsApart& a : im.apart) regs.push_back(Reg{a.dev, a.dev + (size_t)a.keep});
    for (size_t x = 0; x < regs.size(); x++) {
      CHECK(regs[x].e <= im.total);
      for (size_t y = 0; y < x; y++) CHECK(regs[x].e <= regs[y].b || regs[y].e <= regs[x].b);
    }
    CHECK(im.total <= cost);                       // (what cut_chunk adds up is never less than the image)
    for (size_t x = 0; x < im.apart.size(); x++)   // one copy of every distinct outside piece
      for (size_t y = 0; y < x; y++) CHECK(im.apart[x].end != im.apart[y].end || im.apart[x].keep != im.apart[y].keep);
    // the metadata: every array inside the buffer, aligned, none overlapping another
    const CXStreamMeta m(first.back(), nc);
    CHECK(m.l.upload <= m.l.total && m.l.results <= m.l.total && m.consumed.off % 8 == 0 && m.src_off.off % 8 == 0 && m.out.off % 4 == 0);
    CHECK(m.out.off + m.out.bytes() <= m.l.total && m.slot.off + m.slot.bytes() <= m.consumed.off && m.l.upload == m.l.total);
  }
  // ---- the argument errors ----
  { g_case = -1;
    uint32_t first[3] = {0, 1, 2};
    uint64_t so[2] = {10, 50}, wo[2] = {10, 40}, wl[2] = {20, 20}, he[2] = {0, 0};
    int32_t sl[2] = {20, 10}, hl[2] = {0, 0};
    CHECK(!cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl));
    first[0] = 1; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); first[0] = 0;
    first[1] = 3; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); first[1] = 1;
    CHECK(cxstream_shape_error(first, 2, 3, so, sl, he, hl, wo, wl));
    sl[0] = 21; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); sl[0] = 20;
    so[1] = 39; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); so[1] = 61; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); so[1] = 60;
    sl[1] = -3; CHECK(!cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); sl[1] = 0;   // (a negative length is the kernel's 0, not an argument error)
    he[1] = 45; hl[1] = 10; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl));   // straddles
    hl[1] = 5; CHECK(!cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl));
    he[1] = 3; hl[1] = 4; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl));     // longer than its end
    hl[1] = 3; CHECK(!cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl));
    hl[1] = -1; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); hl[1] = 0;
    wo[0] = UINT64_MAX - 5; CHECK(cxstream_shape_error(first, 2, 2, so, sl, he, hl, wo, wl)); }
  printf("cxstream staging ok: %d cases\n", 200000 + 3000);
  return 0;
}
