// tests/cpp/dstream_staging_test.cpp -- TEST INFRASTRUCTURE ONLY.
// The stream decoder's staging arithmetic (lz4-java_amd/csrc/host_staging.h: dstream_piece, dstream_shape_error, dstream_cost, DsImage,
// merge_runs) against a naive restatement, on random windows, states and runs.  Host code alone: built with the address and
// undefined-behaviour sanitizers by tests/test_dstream_abi.py (support.build_sanitized) and run as a program of its own.
// Prints "dstream staging ok: <cases> cases"; exit code 1 and a message on the first disagreement.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../lz4-java_amd/csrc/host_staging.h"

using namespace staging;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dstream_staging_test: line %d: %s (case %d)\n", __LINE__, #c, g_case); exit(1); } } while (0)
static int g_case = 0;

// byte by byte: 'i' every byte of [end - keep, end) lies in the window, 'o' none does, 's' some do
static char naive_where(uint64_t end, uint64_t keep, uint64_t wo, uint64_t wl) {
  if (wl == 0 && end - keep < wo && wo < end) return 's';   // (an empty window still has edges: a piece across them straddles)
  uint64_t in = 0;
  for (uint64_t b = end - keep; b < end; b++) in += (b >= wo && b < wo + wl) ? 1u : 0u;
  return in == keep ? 'i' : (in == 0 ? 'o' : 's');
}

int main() {
  std::mt19937_64 rng(12345);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  // ---- one piece against one window (small numbers, so that the byte-by-byte restatement is cheap; the 65535 cut apart) ----
  for (g_case = 0; g_case < 200000; g_case++) {
    const uint64_t wo = pick(0, 300), wl = pick(0, 200), end = pick(0, 700), len = pick(0, 120);
    const bool prefix = rng() & 1;
    DsPiece p;
    const char* why = dstream_piece(end, len, wo, wl, prefix, &p);
    if (len == 0) { CHECK(!why && p.kind == DS_NONE && p.keep == 0); continue; }
    if (len > end) { CHECK(why != nullptr); continue; }
    const char w = naive_where(end, len, wo, wl);
    if (w == 's') { CHECK(why != nullptr); continue; }
    CHECK(!why && p.keep == len);
    if (w == 'i') CHECK(p.kind == DS_INSIDE);
    else CHECK(p.kind == ((prefix && end == wo) ? DS_LEAD : DS_APART));
  }
  { DsPiece p;   // only the last 65535 bytes are a piece: a history of 70000 bytes that BEGINS in front of the window is inside it
    CHECK(!dstream_piece(170000, 70000, 104465, 100000, true, &p) && p.kind == DS_INSIDE && p.keep == 65535);
    CHECK(dstream_piece(170000, 70000, 104466, 100000, true, &p) != nullptr);
    CHECK(!dstream_piece(70000, 70000, 70000, 10, true, &p) && p.kind == DS_LEAD && p.keep == 65535);
    CHECK(!dstream_piece(70000, 70000, 70000, 10, false, &p) && p.kind == DS_APART); }
  // ---- whole chunks: placement, device states, the way back ----
  for (g_case = 0; g_case < 3000; g_case++) {
    const uint32_t nc = (uint32_t)pick(1, 12);
    std::vector<DsState> st(nc);
    std::vector<uint64_t> wo(nc), wl(nc);
    const uint64_t shared_end = pick(1, 70000), shared_len = pick(1, shared_end);   // one dictionary in front of everything
    uint64_t at = 80000;
    for (uint32_t t = 0; t < nc; t++) {
      at += pick(0, 300);
      wo[t] = at; wl[t] = pick(0, 5000); at += wl[t];
      auto history = [&](bool prefix, uint64_t& end, uint64_t& len) {
        switch (rng() % 5) {
          case 0: end = pick(0, 1000); len = 0; break;                                   // none (its end is whatever it was)
          case 1: end = shared_end; len = shared_len; break;                             // the shared dictionary
          case 2: if (wl[t]) { end = wo[t] + pick(1, wl[t]); len = pick(1, end - wo[t]); } else { end = 0; len = 0; } break;   // inside
          case 3: end = wo[t]; len = pick(1, 70000); (void)prefix; break;                // ends where the window begins
          default: end = at + 100000 + pick(0, 999); len = pick(1, 70000); break;        // behind everything
        }
      };
      history(true, st[t].prefix_end, st[t].prefix_len);
      history(false, st[t].ext_end, st[t].ext_len);
    }
    std::vector<uint32_t> first{0};
    std::vector<uint64_t> dof;
    std::vector<int32_t> dcap;
    for (uint32_t t = 0; t < nc; t++) {
      for (uint64_t k = pick(0, 3); k; k--) { const uint64_t o = pick(0, wl[t]); dof.push_back(wo[t] + o); dcap.push_back((int32_t)pick(0, wl[t] - o)); }
      first.push_back((uint32_t)dof.size());
    }
    dof.push_back(0); dcap.push_back(0);   // (never empty)
    CHECK(dstream_shape_error(st.data(), first.data(), nc, first.back(), dof.data(), dcap.data(), wo.data(), wl.data()) == nullptr);
    const DsImage im(st.data(), wo.data(), wl.data(), nc);
    // every region of the image: [begin, end) in device offsets; they are pairwise disjoint and lie inside the image
    struct Reg { size_t b, e; };
    std::vector<Reg> regs;
    size_t cost = 0;
    for (uint32_t t = 0; t < nc; t++) {
      const size_t lead = im.prefix[t].kind == DS_LEAD ? (size_t)im.prefix[t].keep : 0;
      CHECK(im.win[t] % 16 == 0 && im.win[t] >= lead);
      regs.push_back(Reg{im.win[t] - lead, im.win[t] + (size_t)wl[t]});
      cost += dstream_cost(st[t], wo[t], wl[t]);
    }
    for (const DsApart& a : im.apart) regs.push_back(Reg{a.dev, a.dev + (size_t)a.keep});
    for (size_t x = 0; x < regs.size(); x++) {
      CHECK(regs[x].e <= im.total);
      for (size_t y = 0; y < x; y++) CHECK(regs[x].e <= regs[y].b || regs[y].e <= regs[x].b);
    }
    CHECK(im.total <= cost);                       // (what cut_chunk adds up is never less than the image)
    for (size_t x = 0; x < im.apart.size(); x++)   // one copy of every distinct outside piece
      for (size_t y = 0; y < x; y++) CHECK(im.apart[x].end != im.apart[y].end || im.apart[x].keep != im.apart[y].keep);
    for (uint32_t t = 0; t < nc; t++) {
      const DsState& h = st[t]; const DsState& d = im.dev[t];
      CHECK(d.prefix_len == h.prefix_len && d.ext_len == h.ext_len);
      auto placed = [&](const DsPiece& p, uint64_t hend, uint64_t dend) {
        if (p.kind == DS_NONE) return;
        if (p.kind == DS_INSIDE || p.kind == DS_LEAD) { CHECK(dend - im.win[t] == hend - wo[t] || (p.kind == DS_LEAD && dend == im.win[t])); return; }
        bool found = false;
        for (const DsApart& a : im.apart) found |= a.end == hend && a.keep == p.keep && a.dev + a.keep == dend;
        CHECK(found);
      };
      placed(im.prefix[t], h.prefix_end, d.prefix_end);
      placed(im.ext[t], h.ext_end, d.ext_end);
      // the way back: the ends the stream came with, and every position of the window (its two ends included)
      CHECK(im.to_host(t, d.prefix_end, h, wo[t], wl[t]) == h.prefix_end);
      CHECK(im.to_host(t, d.ext_end, h, wo[t], wl[t]) == h.ext_end);
      for (uint64_t v : {(uint64_t)0, wl[t] / 2, wl[t]}) CHECK(im.to_host(t, im.win[t] + v, h, wo[t], wl[t]) == wo[t] + v);
    }
  }
  // ---- the argument errors ----
  { g_case = -1;
    DsState st[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    uint32_t first[3] = {0, 1, 2};
    uint64_t dof[2] = {10, 50}, wo[2] = {10, 40}, wl[2] = {20, 20};
    int32_t cap[2] = {20, 10};
    CHECK(!dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl));
    first[0] = 1; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); first[0] = 0;
    first[1] = 3; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); first[1] = 1;
    CHECK(dstream_shape_error(st, first, 2, 3, dof, cap, wo, wl));
    cap[0] = 21; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); cap[0] = 20;
    dof[1] = 39; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); dof[1] = 61; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); dof[1] = 60;
    cap[1] = -3; CHECK(!dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); cap[1] = 0;   // (a negative capacity is the kernel's -1, not an argument error)
    st[1].prefix_end = 45; st[1].prefix_len = 10; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl));   // straddles
    st[1].prefix_len = 5; CHECK(!dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl));
    st[1].ext_end = 3; st[1].ext_len = 4; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl));           // longer than its end
    st[1].ext_len = 3; CHECK(!dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl));
    wo[0] = UINT64_MAX - 5; CHECK(dstream_shape_error(st, first, 2, 2, dof, cap, wo, wl)); }
  // ---- merge_runs against a bitmap ----
  for (g_case = 0; g_case < 2000; g_case++) {
    std::vector<Run> r;
    std::vector<uint8_t> want(60000, 0), got(60000, 0);
    for (uint64_t k = pick(0, 12); k; k--) { const size_t o = (size_t)pick(0, 40000), n = (size_t)pick(0, 3000); r.push_back(Run{o, n}); for (size_t b = o; b < o + n; b++) want[b] = 1; }
    merge_runs(r);
    for (size_t x = 0; x < r.size(); x++) {
      CHECK(r[x].len > 0);
      if (x) CHECK(r[x].off > r[x - 1].off + r[x - 1].len + RUN_GAP);   // ascending, and more than the gap apart
      CHECK(want[r[x].off] && want[r[x].off + r[x].len - 1]);          // a run begins and ends with a byte somebody asked for
      for (size_t b = r[x].off; b < r[x].off + r[x].len; b++) got[b] = 1;
    }
    for (size_t b = 0; b < want.size(); b++) CHECK(!want[b] || got[b]);  // and every such byte travels
  }
  printf("dstream staging ok: %d cases\n", 200000 + 3000 + 2000);
  return 0;
}
