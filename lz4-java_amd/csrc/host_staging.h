// host_staging.h -- the arithmetic of staging a host batch (api.cpp's shard functions), free of HIP so that it is compiled and tested
// without a device (tests/cpp/host_staging_test.cpp): where a chunk's metadata arrays lie in their one buffer, where a chunk ends,
// which produced bytes travel back in one copy, and the shape the arrays of a chain call must have.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace staging {

inline size_t al16(size_t v) { return (v + 15u) & ~(size_t)15u; }   // (every packed source and slot starts on a 16-byte boundary)

// n elements of T at byte `off` of a metadata buffer: the same offset in the pinned host copy and in the device copy
template <class T>
struct Region {
  size_t off = 0, n = 0;
  size_t bytes() const { return n * sizeof(T); }
  T* in(void* base) const { return (T*)((uint8_t*)base + off); }
};

// A chunk's metadata in ONE buffer, handed out front to back, every array aligned to its element type: the inputs first, then the
// results (one at least).  One H2D takes [0, upload), one D2H takes [results, total).  A result its kernel expects zeroed goes up as
// well: zero_results(host copy), before the inputs are filled in.  Nothing depends on neighbours by hand: an array asked for out of
// order only widens the two copies (upload ends behind the last input or zeroed result, results starts at the first result).
struct MetaLayout {
  size_t total = 0, upload = 0, results = SIZE_MAX;
  template <class T>
  Region<T> take(size_t n, bool goes_up, bool comes_back) {
    total = (total + alignof(T) - 1) & ~(alignof(T) - 1);
    const Region<T> r{total, n};
    if (comes_back && results == SIZE_MAX) results = r.off;
    total += r.bytes();
    if (goes_up) upload = total;
    return r;
  }
  template <class T> Region<T> input(size_t n) { return take<T>(n, true, false); }
  template <class T> Region<T> result(size_t n, bool zeroed = false) { return take<T>(n, zeroed, true); }
  size_t results_bytes() const { return total - results; }
  void zero_results(void* host) const { if (upload > results) memset((uint8_t*)host + results, 0, upload - results); }
};
// The four layouts.  (Members are initialised in the order they are declared: that order is the order in the buffer.)
struct BlockMeta {   // the block operations (host_shard): nb blocks; consumed[] only where the operation has a second result
  MetaLayout l;
  Region<uint64_t> src_off, dst_off; Region<int32_t> src_len, dst_cap, out, consumed;
  BlockMeta(size_t nb, bool has_consumed) : src_off(l.input<uint64_t>(nb)), dst_off(l.input<uint64_t>(nb)), src_len(l.input<int32_t>(nb)), dst_cap(l.input<int32_t>(nb)),
        out(l.result<int32_t>(nb)), consumed(l.result<int32_t>(has_consumed ? nb : 0)) {}
};
struct ChainMeta {   // chain decode (chain_host_shard): nb blocks in nc chains; chain_out[] goes up zeroed
  MetaLayout l;
  Region<uint64_t> src_off, chain_dst_off, chain_dst_cap; Region<int32_t> src_len, dst_cap, prefix; Region<uint32_t> first; Region<uint8_t> stored; Region<uint64_t> chain_out; Region<int32_t> out;
  ChainMeta(size_t nb, size_t nc)
      : src_off(l.input<uint64_t>(nb)), chain_dst_off(l.input<uint64_t>(nc)), chain_dst_cap(l.input<uint64_t>(nc)), src_len(l.input<int32_t>(nb)),
        dst_cap(l.input<int32_t>(nb)), prefix(l.input<int32_t>(nc)), first(l.input<uint32_t>(nc + 1)), stored(l.input<uint8_t>(nb)),
        chain_out(l.result<uint64_t>(nc, true)), out(l.result<int32_t>(nb)) {}
};
struct CChainMeta {   // chain compress (cchain_host_shard): out[] and chain_consumed[] go up zeroed; slot[] only for resident streams
  MetaLayout l;
  Region<uint64_t> chain_src_off, dst_off; Region<int32_t> src_len, dst_cap, prefix; Region<uint32_t> first, slot; Region<uint64_t> consumed; Region<int32_t> out;
  CChainMeta(size_t nb, size_t nc, bool has_slot = false)
      : chain_src_off(l.input<uint64_t>(nc)), dst_off(l.input<uint64_t>(nb)), src_len(l.input<int32_t>(nb)), dst_cap(l.input<int32_t>(nb)),
        prefix(l.input<int32_t>(nc)), first(l.input<uint32_t>(nc + 1)), slot(l.input<uint32_t>(has_slot ? nc : 0)),
        consumed(l.result<uint64_t>(nc, true)), out(l.result<int32_t>(nb, true)) {}
};
template <class T>
struct HashMeta {   // the hashes (xxh_shard): T = uint32_t / uint64_t
  MetaLayout l;
  Region<uint64_t> off; Region<int32_t> len; Region<T> hash;
  explicit HashMeta(size_t nb) : off(l.input<uint64_t>(nb)), len(l.input<int32_t>(nb)), hash(l.result<T>(nb)) {}
};

// The scratch of the HC chain compressor's layout kernel (compress_hc.hip) for n_blocks blocks in n_chains chains whose regions end at or
// before `span`, with build segments of `seg` positions (4096 .. 2^30): byte offsets of its arrays, 8-byte ones first.  max_items: a
// chain of N buffer bytes lists ceil((N - 3) / seg) <= N / seg + 1 items, and the chains' buffers lie side by side inside the span,
// so span / seg + n_chains + 1 is never exceeded (capped where a uint32_t ends; the layout kernel lists nothing past it).
struct HcChainScratchLayout {
  uint32_t max_items;
  size_t blk_start, chain_buf, chain_len, items, blk_hist, words, total;
  HcChainScratchLayout(uint64_t span, uint32_t n_blocks, uint32_t n_chains, uint32_t seg) {
    const uint64_t m = span / (seg ? seg : 1u) + (uint64_t)n_chains + 1u;
    max_items = m > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)m;
    blk_start = 0;                                        // u64[n_blocks]
    chain_buf = blk_start + 8u * (size_t)n_blocks;        // u64[n_chains]
    chain_len = chain_buf + 8u * (size_t)n_chains;        // u64[n_chains]
    items = chain_len + 8u * (size_t)n_chains;            // {u32, u32}[max_items]
    blk_hist = items + 8u * (size_t)max_items;            // u32[n_blocks]
    words = blk_hist + 4u * (size_t)n_blocks;             // u32[2]
    total = words + 8u;
  }
};

// The next chunk of the units [begin, end) -- blocks, chains, buffers: units are taken while the chunk stays within src_limit and
// dst_limit bytes and max_units units; the first unit is taken whatever it costs, so a single unit always fits.  cost(u) -> the
// bytes unit u takes in the packed source and destination, rounded as the caller packs them.
struct Cost { size_t src, dst; };
struct Chunk { uint32_t end; size_t src, dst; };
template <class CostOf>
Chunk cut_chunk(uint32_t begin, uint32_t end, uint32_t max_units, size_t src_limit, size_t dst_limit, CostOf cost) {
  Chunk c{begin, 0, 0};
  while (c.end < end && c.end - begin < max_units) {
    const Cost u = cost(c.end);
    if (c.end > begin && (c.src + u.src > src_limit || c.dst + u.dst > dst_limit)) break;
    c.src += u.src; c.dst += u.dst; c.end++;
  }
  return c;
}

// Only the bytes produced come back: entry(t) -> where entry t starts in the packed destination and how much it produced (0: skipped),
// offsets ascending; runs whose gap is at most RUN_GAP bytes travel as one copy(begin, end).  copy returns 0 or an error, which ends the walk.
constexpr size_t RUN_GAP = 4096;
struct Run { size_t off, len; };
template <class Entry, class Copy>
int for_each_run(uint32_t n, Entry entry, Copy copy) {
  size_t r0 = 0, r1 = 0;
  for (uint32_t t = 0; t < n; t++) {
    const Run e = entry(t);
    if (!e.len) continue;
    if (r1 > r0 && e.off <= r1 + RUN_GAP) { r1 = e.off + e.len; continue; }
    if (r1 > r0) { const int rc = copy(r0, r1); if (rc) return rc; }
    r0 = e.off; r1 = e.off + e.len;
  }
  return r1 > r0 ? copy(r0, r1) : 0;
}

// What can be said about the chain arrays of a host call without a device: chain_first runs from 0 to n_blocks and ascends, and no
// chain's prefix is negative or longer than its offset chain_off[c] (in_dst: the offsets into dst -- the decoder's history lies in
// front of its output -- and not into src, the compressor's).  -> a message, or nullptr
inline const char* chain_shape_error(const uint32_t* chain_first, uint32_t n_chains, uint32_t n_blocks, const int32_t* chain_prefix_len,
                                     const uint64_t* chain_off, bool in_dst) {
  if (chain_first[0] != 0u || chain_first[n_chains] != n_blocks) return "chain_first must start at 0 and end at n_blocks";
  for (uint32_t c = 0; c < n_chains; c++) {
    if (chain_first[c] > chain_first[c + 1]) return "chain_first must be ascending";
    if (chain_prefix_len && chain_prefix_len[c] < 0) return "negative chain_prefix_len";
    if (chain_prefix_len && (uint64_t)chain_prefix_len[c] > chain_off[c])
      return in_dst ? "chain_prefix_len reaches in front of dst" : "chain_prefix_len reaches in front of src";
  }
  return nullptr;
}

}  // namespace staging
