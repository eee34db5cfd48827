// lz4_fast_chain.h -- the walk over one chain of linked blocks on the compressing side (LZ4_compress_fast_continue, liblz4 1.9.3,
// acceleration 1), shared by compress_fast.hip (compress_fast_chain_cu_kernel) and the CPU lane simulator
// (tests/hostsim/hostsim_cchain.cpp); behind it, the same walk for streams whose state stays on the device between launches
// (cstream_walk: compress_fast_stream_cu_kernel, tests/hostsim/hostsim_cstream.cpp), and for such streams when their sources land
// anywhere (cxstream_walk: compress_fast_xstream_cu_kernel, tests/hostsim/hostsim_cxstream.cpp).
//
// A chain is a run of blocks whose SOURCES lie back to back; block k may match into the blocks before it and into the history that
// lies directly in front of the chain.  liblz4 defines block k's result as
//   s = LZ4_createStream();  if (P > 0) LZ4_loadDict(s, chain_src - P, P);
//   r_k = LZ4_compress_fast_continue(s, chain_src + sum(src_len_j, j < k), dst_k, src_len_k, dst_cap_k, 1);
// which is its prefix mode throughout (the very first block of a stream without a dictionary runs in external-dictionary mode against
// an empty dictionary, which parses the same way).  The rules, each confirmed against the reference library by the tests:
//   * byU32 with the 5-byte hash at every size; ONE table for the whole chain, never cleared between its blocks;
//   * without a prefix the stream's offset starts at 0: chain position p is index p, and an empty bucket is index 0 -- a real
//     candidate, the plain core's "every bucket starts as position 0";
//   * with P > 0 the offset starts at 65536 (LZ4_loadDict adds 64 KB even where it loads nothing).  P < 8 loads nothing and the prefix
//     bytes are unreachable: keep = 0, empty buckets fall to the lower bound.  P >= 8 inserts the last keep = min(P, 65536) bytes at
//     stride 3 (dict_table_build); the history's first byte is index 65536 - keep, which is also the lower bound of a candidate
//     (liblz4 checks it while history plus consumed bytes are under 64 KB; beyond that the 65535-byte distance rule implies it);
//   * a block under 13 bytes is one literal run and inserts nothing, but the index space moves on;
//   * a block whose result is 0 (it does not fit; a negative length or capacity; history + consumed + src_len above 0x7E000000, so that
//     liblz4's index renormalisation is never reached) ends the chain: the blocks behind it get kChainStopped.
// The table is built at the first block that probes it (13 bytes and more): until then nothing reads it, and the four bytes at
// chain position 0 -- the fingerprint of the empty buckets of a chain without a prefix -- exist by then.
//
// ONE wavefront walks a chain from its first block to its last and waits for nobody; parallelism comes from the number of chains.
// Nothing outside [chain_src - keep, chain_src + sum src_len) is read, nothing at or past the current block's end, and nothing outside
// a block's slot is written.
//
// ACC (every walk here): the call's acceleration, 2 .. 65537 after the caller's clamp, in `accel` -- the last argument of
// LZ4_compress_fast_continue.  liblz4 lets it touch nothing but where a miss run probes (FastCore's ACC switch), so the walks are the
// same text: returns, stop rule, span limit, short blocks, history rules, the record's words and the table image's format do not
// change, and calls at different accelerations -- the acceleration-1 kernels among them -- alternate on one stream.  ACC = false is the
// walk the acceleration-1 kernels run, instruction for instruction (profiles/caccel_kernel_diff.txt); `accel` is not read there.
//
// Io: uni(v) / uni_ptr(p): a wave-uniform value back in scalar registers (identity on the host); put_out(i, r) / put_chain(c, bytes):
// the results (lane 0 writes them, vector stores); begin_block(buf, end, d, cap): the block about to run may read [buf, buf + end) and
// write [d, d + cap) (the simulator's bounds; nothing on the device).
#pragma once
#include <stdint.h>
#include "kernels.h"
#include "lz4_fast_core.h"

namespace lz4hip {

constexpr uint32_t kChainSpanMax = 0x7E000000u;   // kept history + the chain's source: liblz4's indexes stay below their renormalisation

// the table a chain starts with, in w's LDS: [buf, buf + keep) is the kept history (keep = 0 or 8 .. 65536), prefixed: P > 0
template <class W>
LZ4HIP_DEV void link_table_init(W& w, const uint8_t* buf, uint32_t keep, bool prefixed) {
  using Core = FastCore<W, false, DirectOut<W>, false, false, false, true>;
  if (keep) {
    dict_table_build(w, buf, keep);
  } else {
    // no prefix: every bucket is {index 0, fingerprint of the bytes at position 0}; a prefix under 8 bytes: empty entries, index 0,
    // below the lower bound
    const uint64_t e0 = prefixed ? 0u : (uint64_t)(((w.sld32(buf, 0) * 2654435761u) >> 16) & Core::FPM);
    w.template lds_fill<false>(1u << Core::HLOG, e0);
    w.sync();
  }
}

// (cstream_walk below holds a copy of this block loop, and cxstream_walk behind it a copy of its prefix-mode branch: a change here is
// to be made there as well)
template <bool ACC = false, class W, class Io>
LZ4HIP_DEV void cchain_walk(W& w, Io& io, const CChainArgs& a, uint32_t c, [[maybe_unused]] uint32_t accel = 1u) {
  using Core = FastCore<W, false, DirectOut<W>, false, ACC, false, true>;
  uint32_t b1 = io.uni(a.chain_first[c + 1]), b0 = io.uni(a.chain_first[c]);
  if (b1 > a.n_blocks) b1 = a.n_blocks;
  if (b0 > b1) b0 = b1;
  const uint64_t soff = io.uni64(a.chain_src_off[c]);
  uint64_t P = 0;
  if (a.chain_prefix_len) { const int32_t p = (int32_t)io.uni((uint32_t)a.chain_prefix_len[c]); P = p > 0 ? (uint64_t)p : 0u; }
  if (P > soff) P = soff;
  const uint32_t keep = P < 8u ? 0u : (P > 65536u ? 65536u : (uint32_t)P);
  const uint32_t ibase = P ? 65536u - keep : 0u;
  const uint8_t* const buf = io.uni_ptr(a.src + soff - keep);
  uint32_t pos = keep;       // where the next block starts in buf
  bool table_ready = false;
  uint32_t i = b0;
  while (i < b1) {
    const int32_t sl = (int32_t)io.uni((uint32_t)a.src_len[i]), dc = (int32_t)io.uni((uint32_t)a.dst_cap[i]);
    uint32_t r = 0;
    if (sl >= 0 && dc >= 0 && (uint64_t)pos + (uint32_t)sl <= kChainSpanMax) {
      const uint32_t end = pos + (uint32_t)sl;
      uint8_t* d = io.uni_ptr(a.dst + io.uni64(a.dst_off[i]));
      io.begin_block(buf, end, d, (uint32_t)dc);
      if (sl >= 13 && !table_ready) { link_table_init(w, buf, keep, P != 0u); table_ready = true; }
      DirectOut<W> out(w, buf, end, d, (uint32_t)dc);
      out.limited = (uint32_t)dc < (uint32_t)sl + (uint32_t)sl / 255u + 16u;   // (by the block's length, not by its end in buf)
      Core core(w, out, buf, end);
      core.blk = pos; core.ibase = ibase; core.lowidx = ibase;
      if constexpr (ACC) core.accel = accel;
      r = core.run();
    }
    io.put_out(i, (int32_t)r);
    i++;
    if (r == 0u) break;
    pos += (uint32_t)sl;
  }
  for (; i < b1; i++) io.put_out(i, kChainStopped);
  io.put_chain(c, (uint64_t)(pos - keep));
}

// ---------------------------------------------------------------------------------------------------
// The same walk for a stream whose state outlives the launch (compress_fast_stream_cu_kernel, tests/hostsim/hostsim_cstream.cpp):
// chain c of the call is the next run of blocks of the stream in slot s.slot[c], and what ONE LZ4_stream_t would carry from call to call
// -- its table, its index position, the history it holds -- is loaded from the slot before the walk and stored back behind it
// (kernels.h CStreamArgs: the record's words).  (A walk of its own beside cchain_walk, not a switch in it: cchain_walk's kernel keeps
// the instructions it has -- even the per-block body alone, as one inline helper for both walks, changed them: 3202 -> 3189, DESIGN.md
// 2.1.  A change to the block loop there is to be made here as well, and one to the prologue and epilogue here -- the record, the image,
// the stop -- in cxstream_walk, which holds a copy of them.)
//   * a fresh stream (a record of zeros) is cchain_walk's chain, rule for rule; with a prefix of 8 bytes and more its table is built
//     before the first block, not at the first block that probes: the loaded bytes need not be in front of a later call's source;
//   * a stream that has run continues in liblz4's prefix mode: the source follows kept = min(chain_prefix_len, 65536, held) bytes of its
//     history (no 8-byte minimum: that is LZ4_loadDict's).  kept < held is LZ4_saveDict with a smaller size.  buf[0] is index
//     idx - kept, and that is the lower bound of a candidate whatever the table holds: where liblz4 does not check it (held >= 64 KB, or
//     held == idx) the 65535-byte distance rule or index 0 imply it, so an entry that points in front of this call's buf is never read;
//   * a stream that has seen only blocks under 13 bytes has no table yet.  Its empty buckets are index 0.  With idx - kept > 0 index 0 is
//     below the bound for good (the bound never falls: held only grows by what is consumed), so the fingerprint does not matter and
//     the buckets are zeros; with idx - kept == 0 the stream's first four bytes are buf[0 .. 4) and the fingerprint is theirs;
//   * the 0x7E000000 limit counts loaded history + everything consumed since the reset + src_len: the one-call chain's count;
//   * a block whose result is 0 stops the STREAM: the record keeps kStreamStopped until the host zeroes it (reset).
// Io, beyond cchain_walk's: begin_state(image) / end_state(): the walk is about to read or write the slot's 32 KB image, and is done
// (the simulator's bounds); table_load(w, image) / table_store(w, image): the image to and from w's table, wave-wide; put_rec(rec, ...):
// the record's words, from lane 0.
template <bool ACC = false, class W, class Io>
LZ4HIP_DEV void cstream_walk(W& w, Io& io, const CStreamArgs& s, uint32_t c, [[maybe_unused]] uint32_t accel = 1u) {
  using Core = FastCore<W, false, DirectOut<W>, false, ACC, false, true>;
  const CChainArgs& a = s.c;
  uint32_t b1 = io.uni(a.chain_first[c + 1]), b0 = io.uni(a.chain_first[c]);
  if (b1 > a.n_blocks) b1 = a.n_blocks;
  if (b0 > b1) b0 = b1;
  const uint32_t sv = io.uni(s.slot[c]), slot = sv & ~kStreamForceStop;
  uint32_t* const rec = io.uni_ptr(s.rec + (size_t)slot * kStreamRecWords);
  uint8_t* const image = (uint8_t*)io.uni_ptr(s.tables + (size_t)slot * (1u << Core::HLOG));
  uint32_t idx = io.uni(rec[0]), held = io.uni(rec[1]), flags = io.uni(rec[2]), span = io.uni(rec[3]);
  uint64_t total = ((uint64_t)io.uni(rec[5]) << 32) | io.uni(rec[4]);
  uint32_t i = b0;
  if ((sv & kStreamForceStop) || (flags & kStreamStopped)) {
    for (; i < b1; i++) io.put_out(i, kChainStopped);
    io.put_chain(c, 0u);
    io.put_rec(rec, idx, held, flags | kStreamStopped, span, total);
    return;
  }
  const uint64_t soff = io.uni64(a.chain_src_off[c]);
  uint64_t P = 0;
  if (a.chain_prefix_len) { const int32_t p = (int32_t)io.uni((uint32_t)a.chain_prefix_len[c]); P = p > 0 ? (uint64_t)p : 0u; }
  if (P > soff) P = soff;
  const bool fresh = !(flags & kStreamUsed);
  uint32_t kept;
  if (fresh) {
    kept = P < 8u ? 0u : (P > 65536u ? 65536u : (uint32_t)P);
    idx = P ? 65536u : 0u;
    held = kept; span = kept; total = 0u;
    flags = kStreamUsed | (P ? kStreamPrefixed : 0u);
  } else {
    kept = P > held ? held : (uint32_t)P;   // (held <= 65536)
  }
  const uint32_t ibase = idx - kept;
  const uint8_t* const buf = io.uni_ptr(a.src + soff - kept);
  uint32_t pos = kept;       // where the next block starts in buf
  bool table_ready = (flags & kStreamTable) != 0u, dirty = false;
  if (table_ready) {
    io.begin_state(image);
    io.table_load(w, image);
    io.end_state();
  } else if (fresh && kept) {
    io.begin_block(buf, kept, nullptr, 0u);
    link_table_init(w, buf, kept, true);
    table_ready = dirty = true;
  }
  bool stopped = false;
  while (i < b1) {
    const int32_t sl = (int32_t)io.uni((uint32_t)a.src_len[i]), dc = (int32_t)io.uni((uint32_t)a.dst_cap[i]);
    uint32_t r = 0;
    if (sl >= 0 && dc >= 0 && (uint64_t)span + (uint32_t)sl <= kChainSpanMax) {
      const uint32_t end = pos + (uint32_t)sl;
      uint8_t* d = io.uni_ptr(a.dst + io.uni64(a.dst_off[i]));
      io.begin_block(buf, end, d, (uint32_t)dc);
      if (sl >= 13) {
        if (!table_ready) { link_table_init(w, buf, 0u, (flags & kStreamPrefixed) != 0u || ibase != 0u); table_ready = true; }
        dirty = true;
      }
      DirectOut<W> out(w, buf, end, d, (uint32_t)dc);
      out.limited = (uint32_t)dc < (uint32_t)sl + (uint32_t)sl / 255u + 16u;   // (by the block's length, not by its end in buf)
      Core core(w, out, buf, end);
      core.blk = pos; core.ibase = ibase; core.lowidx = ibase;
      if constexpr (ACC) core.accel = accel;
      r = core.run();
    }
    io.put_out(i, (int32_t)r);
    i++;
    if (r == 0u) { stopped = true; break; }
    pos += (uint32_t)sl; span += (uint32_t)sl;
  }
  for (; i < b1; i++) io.put_out(i, kChainStopped);
  io.put_chain(c, (uint64_t)(pos - kept));
  // a stopped stream's table is never read again
  if (table_ready && dirty && !stopped) {
    w.sync();
    io.begin_state(image);
    io.table_store(w, image);
    io.end_state();
  }
  io.put_rec(rec, ibase + pos, pos > 65536u ? 65536u : pos, flags | (table_ready ? kStreamTable : 0u) | (stopped ? kStreamStopped : 0u), span,
             total + (uint64_t)(pos - kept));
}

// ---------------------------------------------------------------------------------------------------
// The walk for a resident stream whose sources land ANYWHERE (compress_fast_xstream_cu_kernel, tests/hostsim/hostsim_cxstream.cpp): every
// block has its own source offset, and the stream's history D = [D_end - D_len, D_end) lies wherever the blocks before left it -- a
// ring that wraps, two alternating buffers, a save area.  Same record, same 32 KB image, same rules as cstream_walk (the two walks
// alternate on one slot); what is new is liblz4's per-block state machine (LZ4_compress_fast_continue, 1.9.3), applied to offsets into
// a.s.c.src.  At the stream's first block of the launch D_end = chain_hist_end[c] and D_len = min(chain_hist_len[c], 65536, what the
// record holds); a fresh stream loads those bytes as LZ4_loadDict does (8-byte minimum, indexes from 65536).  Then, for a block [s, s + n):
//   1. D_len < 4 and D_end != s: the history is dropped;
//   2. s + n inside (D_end - D_len, D_end): the source overlaps its history, of which [s + n, D_end) stays -- at most 64 KB, nothing
//      under 4 bytes;
//   3. D_end == s: prefix mode, cstream_walk's LINK block on the buffer that begins at D's first byte; D grows by the block;
//   4. otherwise external-dictionary mode: the LINK + DICT core (lz4_fast_core.h) -- indexes [idx - D_len, idx) name D's bytes, the block
//      starts at idx; afterwards D is the block alone (a 0-byte block: nothing);
//   5. idx += n.
// In both modes idx - D_len is the lower bound of a candidate, whatever the table holds: where liblz4 does not check it (D_len >= 64 KB,
// or D_len == idx) the distance rule or index 0 imply it.  D_len is capped at 64 KB from call to call and in front of an external block:
// nothing further back can be reached, and liblz4's own cap in rule 2 makes the trimmed size the same.  A block in external mode whose
// bytes overlap D's (rule 2 does not catch a source that runs over D's END) reads D as it is now, as liblz4 does: FastCore's alias_hi.
// ONE EXCEPTION, not reproduced: such a source that begins EXACTLY at D's first byte (one reused buffer, a longer block than the one
// before).  liblz4 tells a match in the external dictionary by `lowLimit == dictionary`, which then holds for matches inside the block
// too, so it cuts their forward count at D's would-be end; the engine's matches are the longer, ordinary ones.  Both outputs are
// valid LZ4 of an input that is misuse either way (D was overwritten: liblz4's own output does not decode there).
// A stream without a table (blocks under 13 bytes only) builds it at its first block that probes: empty buckets are index 0, a real
// candidate only while idx - D_len == 0, when the stream's first four bytes are D's (or, with no history at all, the block's).
// Io, beyond cstream_walk's: begin_xblock(hist, hist_len, blk, n, d, cap): the block about to run may read both pieces.
template <bool ACC = false, class W, class Io>
LZ4HIP_DEV void cxstream_walk(W& w, Io& io, const CXStreamArgs& x, uint32_t c, [[maybe_unused]] uint32_t accel = 1u) {
  using Link = FastCore<W, false, DirectOut<W>, false, ACC, false, true>;
  using Ext = FastCore<W, false, DirectOut<W>, false, ACC, true, true>;
  const CStreamArgs& s = x.s;
  const CChainArgs& a = s.c;
  uint32_t b1 = io.uni(a.chain_first[c + 1]), b0 = io.uni(a.chain_first[c]);
  if (b1 > a.n_blocks) b1 = a.n_blocks;
  if (b0 > b1) b0 = b1;
  const uint32_t sv = io.uni(s.slot[c]), slot = sv & ~kStreamForceStop;
  uint32_t* const rec = io.uni_ptr(s.rec + (size_t)slot * kStreamRecWords);
  uint8_t* const image = (uint8_t*)io.uni_ptr(s.tables + (size_t)slot * (1u << Link::HLOG));
  uint32_t idx = io.uni(rec[0]), held = io.uni(rec[1]), flags = io.uni(rec[2]), span = io.uni(rec[3]);
  uint64_t total = ((uint64_t)io.uni(rec[5]) << 32) | io.uni(rec[4]);
  uint32_t i = b0;
  if ((sv & kStreamForceStop) || (flags & kStreamStopped)) {
    for (; i < b1; i++) io.put_out(i, kChainStopped);
    io.put_chain(c, 0u);
    io.put_rec(rec, idx, held, flags | kStreamStopped, span, total);
    return;
  }
  uint64_t De = io.uni64(x.chain_hist_end[c]);
  uint64_t P = 0;
  { const int32_t p = (int32_t)io.uni((uint32_t)a.chain_prefix_len[c]); P = p > 0 ? (uint64_t)p : 0u; }
  if (P > De) P = De;
  const bool fresh = !(flags & kStreamUsed);
  uint32_t Dl;
  if (fresh) {
    Dl = P < 8u ? 0u : (P > 65536u ? 65536u : (uint32_t)P);
    idx = P ? 65536u : 0u;
    span = Dl; total = 0u;
    flags = kStreamUsed | (P ? kStreamPrefixed : 0u);
  } else {
    Dl = P > held ? held : (uint32_t)P;   // (held <= 65536)
  }
  bool table_ready = (flags & kStreamTable) != 0u, dirty = false;
  if (table_ready) {
    io.begin_state(image);
    io.table_load(w, image);
    io.end_state();
  } else if (fresh && Dl) {
    const uint8_t* const hist = io.uni_ptr(a.src + De - Dl);
    io.begin_block(hist, Dl, nullptr, 0u);
    link_table_init(w, hist, Dl, true);
    table_ready = dirty = true;
  }
  bool stopped = false;
  uint64_t consumed = 0;
  while (i < b1) {
    const int32_t sl = (int32_t)io.uni((uint32_t)a.src_len[i]), dc = (int32_t)io.uni((uint32_t)a.dst_cap[i]);
    uint32_t r = 0;
    if (sl >= 0 && dc >= 0 && (uint64_t)span + (uint32_t)sl <= kChainSpanMax) {
      const uint32_t n = (uint32_t)sl;
      const uint64_t so = io.uni64(x.src_off[i]);
      if (Dl < 4u && De != so) Dl = 0u;                          // rule 1
      if (so + n > De - Dl && so + n < De) {                     // rule 2
        const uint64_t t = De - (so + n);
        Dl = t > 65536u ? 65536u : (uint32_t)t;
        if (Dl < 4u) Dl = 0u;
      }
      uint8_t* d = io.uni_ptr(a.dst + io.uni64(a.dst_off[i]));
      const bool probes = sl >= 13;
      if (De == so) {                                            // rule 3: the block follows its history
        const uint8_t* const buf = io.uni_ptr(a.src + so - Dl);
        const uint32_t end = Dl + n, ibase = idx - Dl;
        io.begin_block(buf, end, d, (uint32_t)dc);
        if (probes) {
          if (!table_ready) { link_table_init(w, buf, 0u, (flags & kStreamPrefixed) != 0u || ibase != 0u); table_ready = true; }
          dirty = true;
        }
        DirectOut<W> out(w, buf, end, d, (uint32_t)dc);
        out.limited = (uint32_t)dc < n + n / 255u + 16u;   // (by the block's length, not by its end in buf)
        Link core(w, out, buf, end);
        core.blk = Dl; core.ibase = ibase; core.lowidx = ibase;
        if constexpr (ACC) core.accel = accel;
        r = core.run();
        if (r) { Dl += n; De = so + n; }
      } else {                                                   // rule 4: the history lies elsewhere
        if (Dl > 65536u) Dl = 65536u;
        const uint8_t* const blk = io.uni_ptr(a.src + so);
        const uint8_t* const hist = io.uni_ptr(a.src + De - Dl);
        const uint32_t low = idx - Dl;
        io.begin_xblock(hist, Dl, blk, n, d, (uint32_t)dc);
        if (probes) {
          if (!table_ready) { link_table_init(w, Dl ? hist : blk, 0u, (flags & kStreamPrefixed) != 0u || low != 0u); table_ready = true; }
          dirty = true;
        }
        DirectOut<W> out(w, blk, n, d, (uint32_t)dc);
        Ext core(w, out, blk, n);
        core.dict = hist; core.keep = Dl; core.ibase = idx; core.lowidx = low;
        core.alias_hi = (Dl != 0u && so < De && so + n > De - Dl) ? idx : 0u;
        if constexpr (ACC) core.accel = accel;
        r = core.run();
        if (r) { Dl = n; De = so + n; }
      }
    }
    io.put_out(i, (int32_t)r);
    i++;
    if (r == 0u) { stopped = true; break; }
    idx += (uint32_t)sl; span += (uint32_t)sl; consumed += (uint32_t)sl;
  }
  for (; i < b1; i++) io.put_out(i, kChainStopped);
  io.put_chain(c, consumed);
  // a stopped stream's table is never read again
  if (table_ready && dirty && !stopped) {
    w.sync();
    io.begin_state(image);
    io.table_store(w, image);
    io.end_state();
  }
  io.put_rec(rec, idx, Dl > 65536u ? 65536u : Dl, flags | (table_ready ? kStreamTable : 0u) | (stopped ? kStreamStopped : 0u), span, total + consumed);
}

}  // namespace lz4hip
