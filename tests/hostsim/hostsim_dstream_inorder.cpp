// tests/hostsim/hostsim_dstream_inorder.cpp -- TEST INFRASTRUCTURE ONLY.
// The in-order tier of the stream decoder (lz4-java_amd/csrc/lz4_decode_inorder.h) and the INORDER stream walk of lz4_decode_stream.h
// compiled against the lock-step host backend, in a library of its own (tests/test_dstream_inorder_hostsim.py), in the form
// decode_stream_inorder_kernel runs.  Nothing here is linked into liblz4hip.so.
//
// OrderedHost is the twin of what csrc/group_dev.h adds for the tier: copy_fwd (chunks of GL bytes, a byte per lane, a chunk's loads
// before its stores) and order().  It holds the tier to the ordering it claims to rely on: a store of an in-order block reaches memory
// only at the next order() and at the block's end, and loads read memory -- a load that depends on a store without an order() between
// them gets the old byte.  It keeps the highest address written since begin_block, so that a block decoded in order is held to "nothing
// is written at or behind d + r", not only to its capacity.
// -DLZ4HIP_INORDER_MUTANT=1: a literal copy rounds its last store up to the chunk (rule (b) broken).
// -DLZ4HIP_INORDER_NO_SYNC=1: the CORE's wait is compiled out (lz4_decode_inorder.h; rule (a) broken: a match source is loaded before
//                            the stores in front of it have landed).  The grid of the test must catch both.
#include <stdint.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_decode_stream.h"
#include "group_host.h"

#ifndef LZ4HIP_INORDER_MUTANT
#define LZ4HIP_INORDER_MUTANT 0
#endif

namespace {
constexpr size_t kGuard = 256, kGap = 16;
constexpr uint8_t kGuardByte = 0xA5, kGapByte = 0x3C;
constexpr uint64_t kDictEnd = 1ull << 62;

struct OrderedHost : hostsim::GroupHost {
  using hostsim::GroupHost::GroupHost;
  bool ino = false;                 // the block being decoded is an in-order one (SimIo::in_order)
  uint8_t* wr_top = nullptr;        // one past the highest byte an in-order copy has written since begin_block
  const uint8_t* stream_lo = nullptr; const uint8_t* stream_hi = nullptr;   // the compressed blocks: a copy from there is a literal run
  uint64_t orders = 0;
  std::vector<std::pair<uint8_t*, uint8_t>> pend;   // the stores issued since the last order(), not yet in memory

  void flush() { for (auto& w : pend) *w.first = w.second; pend.clear(); }
  void order() { orders++; flush(); }
  uint8_t get(const uint8_t* p) { return rd_ok(p, 1) ? *p : 0; }
  void put(uint8_t* p, uint8_t v) {
    if (!wr_ok(p, 1)) return;
    if (p + 1 > wr_top) wr_top = p + 1;
    pend.emplace_back(p, v);
  }
  // one copy, chunk by chunk: src(i) -> the address byte i comes from
  template <class Src>
  void chunks(uint8_t* d, uint32_t len, bool round_up, Src src) {
    for (uint32_t base = 0; base < len; base += (uint32_t)GL) {
      uint8_t v[64]; bool act[64];
      for (int l = 0; l < GL; l++) { const uint32_t i = base + (uint32_t)l; act[l] = i < len || round_up; v[l] = act[l] ? get(src(i)) : 0; }
      for (int l = 0; l < GL; l++) if (act[l]) put(d + base + l, v[l]);
    }
  }
  void copy_fwd(uint8_t* d, const uint8_t* s, uint32_t len) {
    const bool literal = s >= stream_lo && s < stream_hi;
    chunks(d, len, LZ4HIP_INORDER_MUTANT == 1 && literal && len != 0, [&](uint32_t i) { return s + i; });
  }
  void copy_match(uint8_t* dst, uint32_t op, uint32_t offset, uint32_t len, bool wild) {
    if (!ino) { hostsim::GroupHost::copy_match(dst, op, offset, len, wild); return; }
    uint8_t* const d = dst + op;
    if (offset == 0) { for (uint32_t i = 0; i < len; i++) put(d + i, 0); return; }   // (liblz4 1.9.3: an offset of 0 zero-fills)
    chunks(d, len, false, [&](uint32_t i) { return (const uint8_t*)(d - offset + i % offset); });   // replicate: only bytes in front of the match are read
  }
};
typedef lz4hip::InOrder<OrderedHost> Grp;

struct SimIo {
  Grp& g;
  const lz4hip::DStreamArgs& a;
  const uint8_t* lo; const uint8_t* hi;
  uint8_t* d = nullptr;
  uint64_t n_inorder = 0;
  bool past_r = false;
  void begin_block(uint8_t* d_, int cap) { d = d_; g.dst_lo = d_; g.dst_hi = d_ + cap; g.src_lo = lo; g.src_hi = hi; g.wr_top = nullptr; }
  void in_order(bool on) { if (!on) g.flush(); g.ino = on; n_inorder += on ? 1u : 0u; }
  lz4hip::DStreamState get_state(uint32_t c) const { return a.state[c]; }
  void put_state(uint32_t c, const lz4hip::DStreamState& s) { a.state[c] = s; }
  void put_out(uint32_t i, int r) {
    a.out[i] = r;
    g.flush();   // (the block's end: the kernel's fence, or its end)
    if (g.ino && r >= 0 && g.wr_top && g.wr_top > d + r) past_r = true;   // an in-order block stores nothing at or behind d + r
    g.ino = false;
  }
  void fence() {}
};
}  // namespace

extern "C" {

// hostsim_dstream.cpp's sim_dstream through the INORDER walk: `every` is the kernel's; *n_inorder comes back as the number of blocks that
// took the in-order tier, *n_orders as the number of order() waits.  form / gl / layout, the arena and the return value: as there; a byte
// stored at or behind d + r by an in-order block counts as out of bounds too.
int sim_dstream_inorder(const uint8_t* src, uint64_t src_bytes, const uint64_t* src_off, const int32_t* src_len, const uint64_t* dst_off,
                        const int32_t* dst_cap, uint32_t n, uint8_t* window, uint64_t win_len, const uint8_t* dict, uint64_t dict_len, int lead,
                        uint64_t* state, int form, int gl, int layout, int every, int32_t* out_len, uint64_t* n_inorder, uint64_t* n_orders) {
  const size_t ns = (size_t)src_bytes, nw = (size_t)win_len, nd = (size_t)(dict_len > 65535 ? 65535 : dict_len), gap = (nd && !lead) ? kGap : 0;
  std::vector<uint8_t> arena(kGuard + ns + nd + gap + nw + kGuard + 1, kGuardByte);
  uint8_t *s, *dp;
  if (layout == 0) { dp = arena.data() + kGuard; s = dp + nd + gap + nw; }
  else { s = arena.data() + kGuard; dp = s + ns; }
  uint8_t* const win = dp + nd + gap;
  if (ns) memcpy(s, src, ns);
  if (nd) memcpy(dp, dict + (dict_len - nd), nd);
  memset(dp + nd, kGapByte, gap);
  if (nw) memcpy(win, window, nw);
  const uint64_t wbase = (uint64_t)(win - arena.data()), dend = (uint64_t)(dp + nd - arena.data());
  std::vector<uint64_t> doff(n);
  for (uint32_t i = 0; i < n; i++) doff[i] = wbase + dst_off[i];
  auto in = [&](uint64_t e, uint64_t len) { return len == 0 ? 0 : (e == kDictEnd ? dend : wbase + e); };
  lz4hip::DStreamState st{in(state[0], state[1]), state[1], in(state[2], state[3]), state[3]};
  const uint32_t first[2] = {0u, n};
  lz4hip::DStreamArgs a{s, src_off, src_len, first, arena.data(), doff.data(), dst_cap, &st, out_len, n, 1u};
  Grp g(gl, s, (long)ns, win, 0);
  g.stream_lo = s; g.stream_hi = s + ns;
  SimIo io{g, a, layout == 0 ? dp : s, layout == 0 ? s + ns : win + nw};
  if (form == 2) lz4hip::dstream_walk<Grp, SimIo, 2, true>(g, io, a, 0u, g.stg_buf, every != 0);
  else if (form == 1) lz4hip::dstream_walk<Grp, SimIo, 1, true>(g, io, a, 0u, nullptr, every != 0);
  else lz4hip::dstream_walk<Grp, SimIo, 0, true>(g, io, a, 0u, nullptr, every != 0);
  g.flush();
  if (nw) memcpy(window, win, nw);
  auto back = [&](uint64_t e, uint64_t len) { return len == 0 ? 0 : ((e == dend && gap) ? kDictEnd : e - wbase); };
  state[0] = back(st.prefix_end, st.prefix_len); state[1] = st.prefix_len; state[2] = back(st.ext_end, st.ext_len); state[3] = st.ext_len;
  *n_inorder = io.n_inorder;
  *n_orders = g.orders;
  bool bad = g.oob || io.past_r || hostsim::GroupHost::walk_mismatch.load() != 0;
  if (nd && memcmp(dp, dict + (dict_len - nd), nd) != 0) bad = true;
  if (ns && memcmp(s, src, ns) != 0) bad = true;
  for (size_t k = 0; k < gap; k++) if (dp[nd + k] != kGapByte) bad = true;
  for (size_t k = 0; k < kGuard; k++) {
    if (arena[k] != kGuardByte) bad = true;
    if (arena[kGuard + ns + nd + gap + nw + k] != kGuardByte) bad = true;
  }
  return bad ? -1000000 : 0;
}

int sim_dstream_inorder_mutant() { return LZ4HIP_INORDER_NO_SYNC ? 2 : LZ4HIP_INORDER_MUTANT; }

}  // extern "C"
