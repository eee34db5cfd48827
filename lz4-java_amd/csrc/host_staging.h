// host_staging.h -- the arithmetic of staging a host batch (api.cpp's shard functions), free of HIP so that it is compiled and tested
// without a device (tests/cpp/host_staging_test.cpp): where a chunk's metadata arrays lie in their one buffer, where a chunk ends,
// where its blocks lie packed and what a chunk of chains calls its chains and slots, which produced bytes travel back in one copy, the shape the arrays of a chain call must have, where the windows and history
// pieces of a stream-decode call lie in the device image, and where the used parts of the windows and the history pieces of a
// stream-compress call whose sources land anywhere lie in theirs, and the state machine and the linear image of an HC stream-compress
// call (one buffer per stream in liblz4's index space).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace staging {

inline size_t al16(size_t v) { return (v + 15u) & ~(size_t)15u; }   // (every packed source and slot starts on a 16-byte boundary)
inline size_t pos(int32_t v) { return v > 0 ? (size_t)v : 0; }      // (a negative length or capacity takes no bytes in the staging)

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
// The layouts.  (Members are initialised in the order they are declared: that order is the order in the buffer.)
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
struct CXStreamMeta {   // resident streams whose sources land anywhere (cxstream_host_shard): out[] and chain_consumed[] go up zeroed
  MetaLayout l;
  Region<uint64_t> src_off, dst_off, hist_end; Region<int32_t> src_len, dst_cap, hist_len; Region<uint32_t> first, slot; Region<uint64_t> consumed; Region<int32_t> out;
  CXStreamMeta(size_t nb, size_t nc)
      : src_off(l.input<uint64_t>(nb)), dst_off(l.input<uint64_t>(nb)), hist_end(l.input<uint64_t>(nc)), src_len(l.input<int32_t>(nb)), dst_cap(l.input<int32_t>(nb)),
        hist_len(l.input<int32_t>(nc)), first(l.input<uint32_t>(nc + 1)), slot(l.input<uint32_t>(nc)),
        consumed(l.result<uint64_t>(nc, true)), out(l.result<int32_t>(nb, true)) {}
};
struct HcStreamMeta {   // HC streams whose sources land anywhere (hcstream_host_shard): the image's arrays; the build's queue word goes up zeroed
  MetaLayout l;
  Region<uint64_t> blk_start, dst_off, buf_off, buf_len; Region<int32_t> src_len, dst_cap; Region<uint32_t> blk_hist, blk_low, blk_dlim, end_first, ends, items, queue;
  Region<int32_t> out;
  HcStreamMeta(size_t nb, size_t nc, size_t n_ends, size_t n_items)
      : blk_start(l.input<uint64_t>(nb)), dst_off(l.input<uint64_t>(nb)), buf_off(l.input<uint64_t>(nc)), buf_len(l.input<uint64_t>(nc)),
        src_len(l.input<int32_t>(nb)), dst_cap(l.input<int32_t>(nb)), blk_hist(l.input<uint32_t>(nb)), blk_low(l.input<uint32_t>(nb)),
        blk_dlim(l.input<uint32_t>(nb)), end_first(l.input<uint32_t>(nc + 1)), ends(l.input<uint32_t>(n_ends)), items(l.input<uint32_t>(2 * n_items)),
        queue(l.result<uint32_t>(1, true)), out(l.result<int32_t>(nb)) {}
};
template <class T>
struct HashMeta {   // the hashes (xxh_shard): T = uint32_t / uint64_t
  MetaLayout l;
  Region<uint64_t> off; Region<int32_t> len; Region<T> hash;
  explicit HashMeta(size_t nb) : off(l.input<uint64_t>(nb)), len(l.input<int32_t>(nb)), hash(l.result<T>(nb)) {}
};
struct ContainerManyMeta {   // many containers per call (container_many_shard): nc items that own ne entries of the batch arrays
  MetaLayout l;
  Region<uint64_t> body_off, body_len, dst_base; Region<uint32_t> slot, max_block, first; Region<uint8_t> flags;
  Region<uint64_t> info, item_dst_off; Region<uint32_t> item_first; Region<int32_t> sizes;
  ContainerManyMeta(size_t nc, size_t ne)
      : body_off(l.input<uint64_t>(nc)), body_len(l.input<uint64_t>(nc)), dst_base(l.input<uint64_t>(nc)), slot(l.input<uint32_t>(nc)),
        max_block(l.input<uint32_t>(nc)), first(l.input<uint32_t>(nc + 1)), flags(l.input<uint8_t>(nc)),
        info(l.result<uint64_t>(5 * nc)), item_dst_off(l.result<uint64_t>(nc + 1)), item_first(l.result<uint32_t>(nc + 1)), sizes(l.result<int32_t>(ne)) {}
};
struct ContainerWriteManyMeta {   // many containers written per call (container_write_many_shard): nc items
  MetaLayout l;
  Region<uint64_t> src_off, slot_base; Region<int32_t> src_len, hash_len; Region<uint32_t> block_size, first, gap_head, gap_tail; Region<uint8_t> flags;
  Region<uint64_t> item_dst_off; Region<uint32_t> content_hash;
  explicit ContainerWriteManyMeta(size_t nc)
      : src_off(l.input<uint64_t>(nc)), slot_base(l.input<uint64_t>(nc)), src_len(l.input<int32_t>(nc)), hash_len(l.input<int32_t>(nc)),
        block_size(l.input<uint32_t>(nc)), first(l.input<uint32_t>(nc + 1)), gap_head(l.input<uint32_t>(nc)), gap_tail(l.input<uint32_t>(nc)), flags(l.input<uint8_t>(nc)),
        item_dst_off(l.result<uint64_t>(nc + 1)), content_hash(l.result<uint32_t>(nc)) {}
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

// Blocks packed one behind the other, each from a 16-byte boundary, a negative length as no bytes: where each of the n blocks starts
// (off is resized to n) -> the bytes they take together
inline size_t packed_offsets(const int32_t* len, size_t n, std::vector<uint64_t>& off) {
  off.resize(n);
  size_t o = 0;
  for (size_t t = 0; t < n; t++) { off[t] = o; o += al16(pos(len[t])); }
  return o;
}
// ... and what the blocks of chain c take of that: [chain_first[c], chain_first[c + 1]) of len[]
inline size_t chain_packed_bytes(const uint32_t* chain_first, uint32_t c, const int32_t* len) {
  size_t sum = 0;
  for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) sum += al16(pos(len[i]));
  return sum;
}
// chain_first[] of the chunk that holds the chains [c, c + nc) and nothing else: first[0 .. nc], counted from the chunk's first block
inline void rebase_first(const uint32_t* chain_first, uint32_t c, uint32_t nc, uint32_t* first) {
  for (uint32_t t = 0; t <= nc; t++) first[t] = chain_first[c + t] - chain_first[c];
}
// The slot words of nc chains that continue resident streams: stream ids[t] lies in slot ids[t] - id0 of its device's share of the set
// (id0: the id of the share's slot 0); a stream marked in poisoned[] (by id; may be nullptr) is told to stop (kSlotForceStop: the
// kernels' kStreamForceStop)
constexpr uint32_t kSlotForceStop = 0x80000000u;
inline void stream_slots(const uint32_t* ids, uint32_t nc, uint32_t id0, const uint8_t* poisoned, uint32_t* slot) {
  for (uint32_t t = 0; t < nc; t++) slot[t] = (ids[t] - id0) | (poisoned && poisoned[ids[t]] ? kSlotForceStop : 0u);
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

// ---- the stream decoder's device image (api.cpp dstream_host_shard) ----
// A stream's state is liblz4's four fields as offsets into the caller's destination base (include/lz4hip.h lz4hip_dstream_state).  Of
// each history -- the prefix and the external dictionary -- only the PIECE [end - min(len, 65535), end) can be read.  A stream's window
// [win_off, win_off + win_len) is mirrored whole on the device; a piece lies inside it (DS_INSIDE), or outside it: a prefix that ends
// exactly at win_off stays contiguous with the window, in lead room in front of the mirror (DS_LEAD), every other outside piece is
// uploaded apart (DS_APART), once per chunk however many streams name it.  A piece that straddles a window edge is an error.
struct DsState { uint64_t prefix_end, prefix_len, ext_end, ext_len; };
constexpr uint64_t kDsKeep = 65535;
constexpr uint64_t kDsNoPrefix = UINT64_MAX, kDsNoExt = UINT64_MAX - 1u;   // the device's word for the end of a history of no bytes
enum DsKind : uint8_t { DS_NONE, DS_INSIDE, DS_LEAD, DS_APART };
struct DsPiece { DsKind kind = DS_NONE; uint64_t keep = 0; };
struct DsMetaLayout {   // stream decode (dstream_host_shard): nb blocks in nc streams; the state records go up and come back
  MetaLayout l;
  Region<uint64_t> src_off, dst_off; Region<int32_t> src_len, dst_cap; Region<uint32_t> first; Region<DsState> state; Region<int32_t> out;
  DsMetaLayout(size_t nb, size_t nc)
      : src_off(l.input<uint64_t>(nb)), dst_off(l.input<uint64_t>(nb)), src_len(l.input<int32_t>(nb)), dst_cap(l.input<int32_t>(nb)),
        first(l.input<uint32_t>(nc + 1)), state(l.take<DsState>(nc, true, true)), out(l.result<int32_t>(nb)) {}
};

// the piece of the history (end, len) against the window -> a message, or nullptr with *p filled in
inline const char* dstream_piece(uint64_t end, uint64_t len, uint64_t win_off, uint64_t win_len, bool is_prefix, DsPiece* p) {
  *p = DsPiece{};
  if (len == 0) return nullptr;
  if (len > end) return is_prefix ? "prefix_len reaches in front of dst" : "ext_len reaches in front of dst";
  p->keep = len < kDsKeep ? len : kDsKeep;
  const uint64_t start = end - p->keep, wend = win_off + win_len;
  if (start >= win_off && end <= wend) p->kind = DS_INSIDE;
  else if (end <= win_off) p->kind = is_prefix && end == win_off ? DS_LEAD : DS_APART;
  else if (start >= wend) p->kind = DS_APART;
  else return is_prefix ? "the prefix straddles an edge of the stream's window" : "the external dictionary straddles an edge of the stream's window";
  return nullptr;
}

// What can be said about a stream-decode call without a device: chain_first runs from 0 to n_blocks and ascends, every window has
// an end, every slot lies inside its stream's window, every history piece is placeable.  -> a message, or nullptr
inline const char* dstream_shape_error(const DsState* state, const uint32_t* chain_first, uint32_t n_chains, uint32_t n_blocks, const uint64_t* dst_off,
                                       const int32_t* dst_cap, const uint64_t* win_off, const uint64_t* win_len) {
  if (chain_first[0] != 0u || chain_first[n_chains] != n_blocks) return "chain_first must start at 0 and end at n_blocks";
  for (uint32_t c = 0; c < n_chains; c++)
    if (chain_first[c] > chain_first[c + 1]) return "chain_first must be ascending";
  for (uint32_t c = 0; c < n_chains; c++) {
    if (win_off[c] + win_len[c] < win_off[c]) return "a stream's window wraps around the address space";
    const uint64_t wend = win_off[c] + win_len[c];
    for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) {
      const uint64_t cap = dst_cap[i] > 0 ? (uint64_t)dst_cap[i] : 0u;
      if (dst_off[i] < win_off[c] || dst_off[i] > wend || cap > wend - dst_off[i]) return "a block's slot lies outside its stream's window";
    }
    DsPiece p;
    if (const char* why = dstream_piece(state[c].prefix_end, state[c].prefix_len, win_off[c], win_len[c], true, &p)) return why;
    if (const char* why = dstream_piece(state[c].ext_end, state[c].ext_len, win_off[c], win_len[c], false, &p)) return why;
  }
  return nullptr;
}

// the bytes stream c takes in the device image when it stands alone (cut_chunk's cost: shared pieces are counted once per stream)
inline size_t dstream_cost(const DsState& s, uint64_t win_off, uint64_t win_len) {
  DsPiece p, e;
  (void)dstream_piece(s.prefix_end, s.prefix_len, win_off, win_len, true, &p);
  (void)dstream_piece(s.ext_end, s.ext_len, win_off, win_len, false, &e);
  return al16((size_t)(p.kind == DS_LEAD ? p.keep : 0u)) + al16((size_t)win_len) + (p.kind == DS_APART ? al16((size_t)p.keep) : 0u) +
         (e.kind == DS_APART ? al16((size_t)e.keep) : 0u);
}

// One chunk's image: stream t's window is mirrored at device offset win[t] (16-aligned, its lead room directly in front of it); the
// pieces uploaded apart follow the windows.  dev[t] is the state the kernel gets: lengths as they are, ends as device offsets.
struct DsApart { uint64_t end, keep; size_t dev; };   // the caller's bytes [end - keep, end) at device offset dev
struct DsImage {
  std::vector<size_t> win;
  std::vector<DsPiece> prefix, ext;
  std::vector<DsApart> apart;
  std::vector<DsState> dev;
  size_t total = 0;
  size_t apart_at(uint64_t end, uint64_t keep) {   // (chunks hold few distinct outside pieces -- a shared dictionary is one)
    for (const DsApart& a : apart) if (a.end == end && a.keep == keep) return a.dev;
    apart.push_back(DsApart{end, keep, total});
    total += al16((size_t)keep);
    return apart.back().dev;
  }
  // state / win_off / win_len: the chunk's first stream's (nc streams); the call has passed dstream_shape_error
  DsImage(const DsState* state, const uint64_t* win_off, const uint64_t* win_len, uint32_t nc) : win(nc), prefix(nc), ext(nc), dev(nc) {
    for (uint32_t t = 0; t < nc; t++) {
      (void)dstream_piece(state[t].prefix_end, state[t].prefix_len, win_off[t], win_len[t], true, &prefix[t]);
      (void)dstream_piece(state[t].ext_end, state[t].ext_len, win_off[t], win_len[t], false, &ext[t]);
      win[t] = total + al16((size_t)(prefix[t].kind == DS_LEAD ? prefix[t].keep : 0u));
      total = win[t] + al16((size_t)win_len[t]);
    }
    for (uint32_t t = 0; t < nc; t++) {
      dev[t] = DsState{kDsNoPrefix, state[t].prefix_len, kDsNoExt, state[t].ext_len};
      if (prefix[t].kind == DS_INSIDE || prefix[t].kind == DS_LEAD) dev[t].prefix_end = win[t] + (state[t].prefix_end - win_off[t]);
      if (prefix[t].kind == DS_APART) dev[t].prefix_end = apart_at(state[t].prefix_end, prefix[t].keep) + prefix[t].keep;
      if (ext[t].kind == DS_INSIDE) dev[t].ext_end = win[t] + (state[t].ext_end - win_off[t]);
      if (ext[t].kind == DS_APART) dev[t].ext_end = apart_at(state[t].ext_end, ext[t].keep) + ext[t].keep;
    }
  }
  // an end offset the kernel wrote back, in the caller's terms: a position of the mirrored window (its two ends included), or one of
  // the two ends the stream came with (host: its state before the call)
  uint64_t to_host(uint32_t t, uint64_t v, const DsState& host, uint64_t win_off, uint64_t win_len) const {
    if (v == kDsNoPrefix) return host.prefix_end;
    if (v == kDsNoExt) return host.ext_end;
    if (v >= win[t] && v - win[t] <= win_len) return win_off + (v - win[t]);
    return v == dev[t].prefix_end ? host.prefix_end : host.ext_end;
  }
};

// ---- the stream compressor's device image when sources land anywhere (api.cpp cxstream_host_shard) ----
// Per call and stream the caller says where the stream's history ends in src and how much of it is there; the PIECE that can be read is
// its last min(len, 65536) bytes (LZ4_loadDict's and LZ4_saveDict's 64 KB: one byte more than the decoder's piece).  Against the
// stream's window it is placed as the decoder's pieces are: inside, contiguous in front of it (it ends at win_off), or apart.  Of a window
// only the USED part is mirrored: the hull [lo, hi) of the call's sources and of a piece that is inside or contiguous, at the device
// offset base; x in the hull is base + (x - lo), so every comparison of offsets the walk makes holds on the device as it does in the
// caller's terms.  Pieces apart follow the hulls, each once per chunk.
constexpr uint64_t kCxKeep = 65536;
inline const char* cxstream_piece(uint64_t end, int32_t len, uint64_t win_off, uint64_t win_len, DsPiece* p) {
  *p = DsPiece{};
  if (len < 0) return "negative chain_hist_len";
  if (len == 0) return nullptr;
  if ((uint64_t)len > end) return "chain_hist_len reaches in front of src";
  p->keep = (uint64_t)len < kCxKeep ? (uint64_t)len : kCxKeep;
  const uint64_t start = end - p->keep, wend = win_off + win_len;
  if (start >= win_off && end <= wend) p->kind = DS_INSIDE;
  else if (end <= win_off) p->kind = end == win_off ? DS_LEAD : DS_APART;
  else if (start >= wend) p->kind = DS_APART;
  else return "the history straddles an edge of the stream's window";
  return nullptr;
}
// What can be said about a call without a device: the shape of chain_first, every window has an end, every source lies inside its
// stream's window (a negative length: its offset does), every history piece is placeable.  -> a message, or nullptr
inline const char* cxstream_shape_error(const uint32_t* chain_first, uint32_t n_chains, uint32_t n_blocks, const uint64_t* src_off, const int32_t* src_len,
                                        const uint64_t* hist_end, const int32_t* hist_len, const uint64_t* win_off, const uint64_t* win_len) {
  if (chain_first[0] != 0u || chain_first[n_chains] != n_blocks) return "chain_first must start at 0 and end at n_blocks";
  for (uint32_t c = 0; c < n_chains; c++)
    if (chain_first[c] > chain_first[c + 1]) return "chain_first must be ascending";
  for (uint32_t c = 0; c < n_chains; c++) {
    if (win_off[c] + win_len[c] < win_off[c]) return "a stream's window wraps around the address space";
    const uint64_t wend = win_off[c] + win_len[c];
    for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) {
      const uint64_t n = src_len[i] > 0 ? (uint64_t)src_len[i] : 0u;
      if (src_off[i] < win_off[c] || src_off[i] > wend || n > wend - src_off[i]) return "a block's source lies outside its stream's window";
    }
    DsPiece p;
    if (const char* why = cxstream_piece(hist_end[c], hist_len[c], win_off[c], win_len[c], &p)) return why;
  }
  return nullptr;
}
struct CxHull { uint64_t lo = 0, hi = 0; };
// the used part of stream c's window: the call has passed cxstream_shape_error.  A block that cannot run -- a negative length --
// counts with its offset alone; a stream without blocks and without a piece in reach of its window has an empty hull at win_off
inline CxHull cxstream_hull(const uint32_t* chain_first, uint32_t c, const uint64_t* src_off, const int32_t* src_len, uint64_t hist_end, const DsPiece& p,
                            uint64_t win_off) {
  CxHull h;
  bool any = false;
  auto take = [&](uint64_t a, uint64_t b) { if (!any) { h.lo = a; h.hi = b; any = true; } else { if (a < h.lo) h.lo = a; if (b > h.hi) h.hi = b; } };
  for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) take(src_off[i], src_off[i] + (src_len[i] > 0 ? (uint64_t)src_len[i] : 0u));
  if (p.kind == DS_INSIDE || p.kind == DS_LEAD) take(hist_end - p.keep, hist_end);
  if (!any) h.lo = h.hi = win_off;
  return h;
}
// the bytes stream c takes in the device image when it stands alone (cut_chunk's cost: shared pieces are counted once per stream)
inline size_t cxstream_cost(const CxHull& h, const DsPiece& p) { return al16((size_t)(h.hi - h.lo)) + (p.kind == DS_APART ? al16((size_t)p.keep) : 0u); }
// One chunk's image: nc streams from the chunk's first on.  hist_dev[t]: where stream t's history ends on the device (0 with no piece:
// the walk looks at no byte of a history of length 0)
struct CxImage {
  std::vector<CxHull> hull;
  std::vector<size_t> base;
  std::vector<DsPiece> piece;
  std::vector<DsApart> apart;
  std::vector<uint64_t> hist_dev;
  size_t total = 0;
  size_t apart_at(uint64_t end, uint64_t keep) {   // (chunks hold few distinct outside pieces -- a shared dictionary is one)
    for (const DsApart& a : apart) if (a.end == end && a.keep == keep) return a.dev;
    apart.push_back(DsApart{end, keep, total});
    total += al16((size_t)keep);
    return apart.back().dev;
  }
  CxImage(const uint32_t* chain_first, uint32_t c0, uint32_t nc, const uint64_t* src_off, const int32_t* src_len, const uint64_t* hist_end,
          const int32_t* hist_len, const uint64_t* win_off, const uint64_t* win_len)
      : hull(nc), base(nc), piece(nc), hist_dev(nc) {
    for (uint32_t t = 0; t < nc; t++) {
      (void)cxstream_piece(hist_end[c0 + t], hist_len[c0 + t], win_off[c0 + t], win_len[c0 + t], &piece[t]);
      hull[t] = cxstream_hull(chain_first, c0 + t, src_off, src_len, hist_end[c0 + t], piece[t], win_off[c0 + t]);
      base[t] = total;
      total += al16((size_t)(hull[t].hi - hull[t].lo));
    }
    for (uint32_t t = 0; t < nc; t++) {
      hist_dev[t] = 0;
      if (piece[t].kind == DS_INSIDE || piece[t].kind == DS_LEAD) hist_dev[t] = to_dev(t, hist_end[c0 + t]);
      if (piece[t].kind == DS_APART) hist_dev[t] = apart_at(hist_end[c0 + t], piece[t].keep) + piece[t].keep;
    }
  }
  uint64_t to_dev(uint32_t t, uint64_t x) const { return base[t] + (x - hull[t].lo); }
};

// ---- the HC stream compressor when sources land anywhere (api.cpp hcstream_host_shard) ----
// A stream's state is liblz4's bookkeeping as offsets into the caller's source base (include/lz4hip.h lz4hip_hcstream_state): the prefix
// [prefix_end - prefix_len, prefix_end), the external dictionary [ext_end - ext_len, ext_end), and the bytes loaded plus consumed.  It is
// a function of addresses and lengths alone, so the whole call is walked here, before anything is compressed.
struct HcsState { uint64_t prefix_end, prefix_len, ext_end, ext_len, index; };
constexpr uint64_t kHcsKeep = 65536, kHcsMaxBlock = 0x7E000000ull, kHcsLife = 0x80000000ull;
inline bool hcs_runs(int32_t n) { return n >= 0 && (uint64_t)n <= kHcsMaxBlock; }   // otherwise: 0, step 1 only, nothing consumed
// LZ4_loadDictHC / LZ4_saveDictHC as state edits
inline HcsState hcs_load_dict(uint64_t dict_end, uint64_t dict_len) {
  const uint64_t k = dict_len < kHcsKeep ? dict_len : kHcsKeep;
  return HcsState{dict_end, k, 0, 0, k};
}
inline int hcs_save_dict(HcsState& st, uint64_t buf_off, int k) {
  uint64_t kept = k < 0 ? 0u : ((uint64_t)k < kHcsKeep ? (uint64_t)k : kHcsKeep);
  if (kept < 4u) kept = 0;
  if (kept > st.prefix_len) kept = st.prefix_len;
  st.prefix_end = buf_off + kept;
  st.prefix_len = kept;
  st.ext_len = 0;
  return (int)kept;
}
// steps 1 and 2 of the state machine in front of the block [s, s + n) -> true at a jump; n = 0 for a block that cannot run
inline bool hcs_enter(HcsState& st, uint64_t s, uint64_t n, bool runs) {
  const bool jump = s != st.prefix_end;
  if (jump) { st.ext_end = st.prefix_end; st.ext_len = st.prefix_len; st.prefix_len = 0; st.prefix_end = s; }
  if (runs && st.ext_len > 0 && s + n > st.ext_end - st.ext_len && s < st.ext_end) {
    st.ext_len = st.ext_end - (s + n < st.ext_end ? s + n : st.ext_end);
    if (st.ext_len < 4u) st.ext_len = 0;
  }
  return jump;
}
inline void hcs_leave(HcsState& st, uint64_t s, uint64_t n) { st.prefix_len += n; st.prefix_end = s + n; st.index += n; }
// what of a state's histories a call stages: the prefix's last 64 KB, and of the external piece what the first block can still reach
// while the prefix is shorter than 65535 bytes
inline uint64_t hcs_prefix_keep(const HcsState& st) { return st.prefix_len < kHcsKeep ? st.prefix_len : kHcsKeep; }
inline uint64_t hcs_ext_keep(const HcsState& st) {
  const uint64_t pk = hcs_prefix_keep(st);
  if (pk >= kHcsKeep - 1u) return 0;
  return st.ext_len < kHcsKeep - pk ? st.ext_len : kHcsKeep - pk;
}
// What can be said about a call without a device -> a message, or nullptr
inline const char* hcstream_shape_error(const HcsState* state, const uint32_t* chain_first, uint32_t n_chains, uint32_t n_blocks, const int32_t* src_len) {
  if (chain_first[0] != 0u || chain_first[n_chains] != n_blocks) return "chain_first must start at 0 and end at n_blocks";
  for (uint32_t c = 0; c < n_chains; c++)
    if (chain_first[c] > chain_first[c + 1]) return "chain_first must be ascending";
  for (uint32_t c = 0; c < n_chains; c++) {
    if (state[c].prefix_len > state[c].prefix_end) return "prefix_len reaches in front of src";
    if (state[c].ext_len > state[c].ext_end) return "ext_len reaches in front of src";
    uint64_t index = state[c].index;
    if (index > kHcsLife) return "a stream past the 2 GiB index limit (liblz4 reloads its dictionary there: out of scope)";
    for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) {
      if (hcs_runs(src_len[i])) index += (uint64_t)src_len[i];
      if (kHcsKeep + index > kHcsLife) return "a stream would pass the 2 GiB index limit during the call (liblz4 reloads its dictionary there: out of scope)";
    }
  }
  return nullptr;
}
// the bytes stream c's linear buffer takes (cut_chunk's cost)
inline size_t hcstream_cost(const HcsState& st, const uint32_t* chain_first, uint32_t c, const int32_t* src_len) {
  uint64_t n = hcs_ext_keep(st) + hcs_prefix_keep(st);
  for (uint32_t i = chain_first[c]; i < chain_first[c + 1]; i++) if (hcs_runs(src_len[i])) n += (uint64_t)src_len[i];
  return al16((size_t)n);
}
// One chunk's image.  Every stream gets ONE buffer in liblz4's own index space: the kept external piece, the kept prefix piece, then the
// call's blocks in order -- a jump is contiguous there.  Per block: where it starts in the image, how much lies in front of it in its
// VIEW (hist = min(65536, what the buffer holds in front of it)), and liblz4's lowLimit and dictLimit as positions of that view, cut to
// its start (what lies below the view cannot be reached: 65535 is the longest distance, and the backward extension of a match ends
// at the pending literals, which begin inside the block).  Per stream: the buffer, its run ends (positions at which a jump ended a
// contiguous run, ascending, counted from the buffer's start) and the state behind its last block.
struct HcsPiece { uint64_t src; size_t dev, len; };   // the caller's bytes [src, src + len) at image offset dev
struct HcsImage {
  std::vector<HcsPiece> pieces;
  std::vector<uint64_t> blk_start;
  std::vector<uint32_t> blk_hist, blk_low, blk_dlim;
  std::vector<uint64_t> buf_off, buf_len;
  std::vector<uint32_t> end_first, ends;
  std::vector<HcsState> after;
  size_t total = 0;
  // stream c0 + t is blocks [chain_first[c0 + t], chain_first[c0 + t + 1]); the call has passed hcstream_shape_error
  HcsImage(const HcsState* state, const uint32_t* chain_first, uint32_t c0, uint32_t nc, const uint64_t* src_off, const int32_t* src_len) {
    const uint32_t b0 = chain_first[c0], nb = chain_first[c0 + nc] - b0;
    blk_start.resize(nb); blk_hist.resize(nb); blk_low.resize(nb); blk_dlim.resize(nb);
    buf_off.resize(nc); buf_len.resize(nc); end_first.resize(nc + 1); after.resize(nc);
    for (uint32_t t = 0; t < nc; t++) {
      HcsState st = state[c0 + t];
      const uint64_t ek = hcs_ext_keep(st), pk = hcs_prefix_keep(st);
      const size_t base = total;
      end_first[t] = (uint32_t)ends.size();
      if (ek) pieces.push_back(HcsPiece{st.ext_end - ek, base, (size_t)ek});
      if (pk) pieces.push_back(HcsPiece{st.prefix_end - pk, base + (size_t)ek, (size_t)pk});
      if (ek) ends.push_back((uint32_t)ek);
      uint64_t L = ek + pk;          // the buffer's length so far
      uint64_t dlim = ek;            // where the prefix begins in the buffer
      uint64_t ext_avail = ek;       // bytes of the external piece the buffer holds in front of dlim
      for (uint32_t i = chain_first[c0 + t]; i < chain_first[c0 + t + 1]; i++) {
        const bool runs = hcs_runs(src_len[i]);
        const uint64_t s = src_off[i], n = runs ? (uint64_t)src_len[i] : 0u;
        if (hcs_enter(st, s, n, runs)) {
          ext_avail = L - dlim;
          dlim = L;
          if (ends.size() == end_first[t] || ends.back() != (uint32_t)L) ends.push_back((uint32_t)L);
        }
        const uint64_t low = dlim - (st.ext_len < ext_avail ? st.ext_len : ext_avail);
        const uint64_t hist = L < kHcsKeep ? L : kHcsKeep, view = L - hist;
        blk_start[i - b0] = base + L;
        blk_hist[i - b0] = (uint32_t)hist;
        blk_low[i - b0] = (uint32_t)((low > view ? low : view) - view);
        blk_dlim[i - b0] = (uint32_t)((dlim > view ? dlim : view) - view);
        if (!runs) continue;
        if (n) pieces.push_back(HcsPiece{s, base + (size_t)L, (size_t)n});
        L += n;
        hcs_leave(st, s, n);
      }
      buf_off[t] = base; buf_len[t] = L; after[t] = st;
      total += al16((size_t)L);
    }
    end_first[nc] = (uint32_t)ends.size();
  }
};

// runs in any order, overlapping ones included -> ascending, disjoint, those at most RUN_GAP bytes apart joined
inline void merge_runs(std::vector<Run>& r) {
  std::sort(r.begin(), r.end(), [](const Run& a, const Run& b) { return a.off < b.off; });
  size_t n = 0;
  for (const Run& e : r) {
    if (!e.len) continue;
    if (n && e.off <= r[n - 1].off + r[n - 1].len + RUN_GAP) {
      const size_t end = std::max(r[n - 1].off + r[n - 1].len, e.off + e.len);
      r[n - 1].len = end - r[n - 1].off;
    } else r[n++] = e;
  }
  r.resize(n);
}

}  // namespace staging
