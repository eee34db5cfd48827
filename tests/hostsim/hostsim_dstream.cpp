// tests/hostsim/hostsim_dstream.cpp -- TEST INFRASTRUCTURE ONLY.
// The stream walk of lz4-java_amd/csrc/lz4_decode_stream.h (LZ4_decompress_safe_continue in every mode of LZ4_streamDecode_t) and the
// PREFIX && DICT switch of lz4_decode_core.h compiled against the lock-step host backend, in a library of its own
// (tests/test_dstream_hostsim.py), in the forms decode_stream_kernel runs.  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_decode_stream.h"
#include "group_host.h"

namespace {
constexpr size_t kGuard = 256, kGap = 16;
constexpr uint8_t kGuardByte = 0xA5, kGapByte = 0x3C;
constexpr uint64_t kDictEnd = 1ull << 62;   // a state's end offset that means "the end of the outside dictionary"

// The simulator knows ONE readable range besides the block's own slot, so the dictionary piece, the window and the streams share an
// arena with nothing but kGap bytes between the first two (none where the dictionary leads into the window):
// layout 0 = [guard][dictionary piece][gap][window][streams][guard], layout 1 = [guard][streams][dictionary piece][gap][window][guard].
// Only the last 65535 bytes of the dictionary are in the arena: a read in front of them is out of bounds, as is one behind the window
// (layout 1) or in front of the streams / behind them.  Writes are legal inside the current block's [d, d + cap) only.
struct SimIo {
  hostsim::GroupHost& g;
  const lz4hip::DStreamArgs& a;
  const uint8_t* lo; const uint8_t* hi;
  void begin_block(uint8_t* d, int cap) { g.dst_lo = d; g.dst_hi = d + cap; g.src_lo = lo; g.src_hi = hi; }
  lz4hip::DStreamState get_state(uint32_t c) const { return a.state[c]; }
  void put_state(uint32_t c, const lz4hip::DStreamState& s) { a.state[c] = s; }
  void put_out(uint32_t i, int r) { a.out[i] = r; }
  void fence() {}
};
}  // namespace

extern "C" {

// One stream's n blocks of one call through dstream_walk: streams src + src_off[i] (src_bytes in all), block i to window + dst_off[i];
// the window (win_len bytes) comes in as the calls before left it and goes back as this one leaves it; dict[0 .. dict_len) is the
// outside dictionary (lead != 0: directly in front of the window).  state[4] in and out: lengths as they are, ends relative to the
// window, kDictEnd for the dictionary's end.  form / gl: as sim_chain's.  Returns 0, or -1000000 if the simulated group touched
// memory outside its bounds, or a guard, gap, dictionary or stream byte changed.
int sim_dstream(const uint8_t* src, uint64_t src_bytes, const uint64_t* src_off, const int32_t* src_len, const uint64_t* dst_off, const int32_t* dst_cap,
                uint32_t n, uint8_t* window, uint64_t win_len, const uint8_t* dict, uint64_t dict_len, int lead, uint64_t* state, int form, int gl,
                int layout, int32_t* out_len) {
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
  hostsim::GroupHost g(gl, s, (long)ns, win, 0);
  SimIo io{g, a, layout == 0 ? dp : s, layout == 0 ? s + ns : win + nw};
  if (form == 2) lz4hip::dstream_walk<hostsim::GroupHost, SimIo, 2>(g, io, a, 0u, g.stg_buf);
  else if (form == 1) lz4hip::dstream_walk<hostsim::GroupHost, SimIo, 1>(g, io, a, 0u, nullptr);
  else lz4hip::dstream_walk<hostsim::GroupHost, SimIo, 0>(g, io, a, 0u, nullptr);
  if (nw) memcpy(window, win, nw);
  auto back = [&](uint64_t e, uint64_t len) { return len == 0 ? 0 : ((e == dend && gap) ? kDictEnd : e - wbase); };
  state[0] = back(st.prefix_end, st.prefix_len); state[1] = st.prefix_len; state[2] = back(st.ext_end, st.ext_len); state[3] = st.ext_len;
  bool bad = g.oob || hostsim::GroupHost::walk_mismatch.load() != 0;
  if (nd && memcmp(dp, dict + (dict_len - nd), nd) != 0) bad = true;
  if (ns && memcmp(s, src, ns) != 0) bad = true;
  for (size_t k = 0; k < gap; k++) if (dp[nd + k] != kGapByte) bad = true;
  for (size_t k = 0; k < kGuard; k++) {
    if (arena[k] != kGuardByte) bad = true;
    if (arena[kGuard + ns + nd + gap + nw + k] != kGuardByte) bad = true;
  }
  return bad ? -1000000 : 0;
}

// decode_block's PREFIX && DICT instance alone (LZ4_decompress_safe_doubleDict): the block src[0 .. src_len) decoded behind prefix[0 ..
// prefix_len) with the external dictionary ext[0 .. ext_len) (ext_len as liblz4 gets it: it may exceed what is kept, the last 65535
// bytes), capacity cap; out[cap] comes back pre-filled with `fill`.  -> the block's result; *status = 0 or -1000000 as above
int sim_double_dict(const uint8_t* src, int src_len, const uint8_t* prefix, int prefix_len, const uint8_t* ext, uint64_t ext_len, int cap, int form, int gl,
                    uint8_t fill, uint8_t* out, int* status) {
  const size_t ns = (size_t)src_len, np = (size_t)prefix_len, ne = (size_t)(ext_len > 65535 ? 65535 : ext_len), nc = (size_t)(cap > 0 ? cap : 0);
  // [guard][ext piece][gap][prefix][block][streams][guard]
  std::vector<uint8_t> arena(kGuard + ne + kGap + np + nc + ns + kGuard + 1, kGuardByte);
  uint8_t* const e = arena.data() + kGuard, *const p = e + ne + kGap, *const d = p + np, *const s = d + nc;
  if (ne) memcpy(e, ext + (ext_len - ne), ne);
  memset(e + ne, kGapByte, kGap);
  if (np) memcpy(p, prefix, np);
  memset(d, fill, nc);
  if (ns) memcpy(s, src, ns);
  hostsim::GroupHost g(gl, e, (long)(s + ns - e), d, cap);
  const int dl = ext_len >= 65536 ? 65536 : (int)ext_len;
  int r;
  if (form == 2) r = lz4hip::decode_block<hostsim::GroupHost, true, 2, false, false, true, true>(g, s, src_len, d, cap, g.stg_buf, e + ne, dl, prefix_len);
  else if (form == 1) r = lz4hip::decode_block<hostsim::GroupHost, true, 1, false, false, true, true>(g, s, src_len, d, cap, nullptr, e + ne, dl, prefix_len);
  else r = lz4hip::decode_block<hostsim::GroupHost, true, 0, false, false, true, true>(g, s, src_len, d, cap, nullptr, e + ne, dl, prefix_len);
  memcpy(out, d, nc);
  bool bad = g.oob || hostsim::GroupHost::walk_mismatch.load() != 0;
  if (ne && memcmp(e, ext + (ext_len - ne), ne) != 0) bad = true;
  if (np && memcmp(p, prefix, np) != 0) bad = true;
  if (ns && memcmp(s, src, ns) != 0) bad = true;
  for (size_t k = 0; k < kGap; k++) if (e[ne + k] != kGapByte) bad = true;
  for (size_t k = 0; k < kGuard; k++) if (arena[k] != kGuardByte || s[ns + k] != kGuardByte) bad = true;
  *status = bad ? -1000000 : 0;
  return r;
}

// the number of deep-loop trips the simulator has run (tests assert that the deep loop really ran)
uint64_t sim_dstream_deep_trips() { return hostsim::GroupHost::deep_trips; }

}  // extern "C"
