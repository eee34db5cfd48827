// tests/cpp/chain_mirror_test.cpp -- exercises LZ4HIPBatch::decompressSafeChain of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).
// Built and run by tests/test_gpu_chain.py with one chain in a file:
//   chain_mirror_test <chain> <out>
// <chain>: u32 n_blocks, u32 prefix_len, u64 chain capacity, then per block {u32 stream length, u32 stored, i32 capacity}, the history
// bytes, the streams back to back (little endian).  The chain is decoded TWICE in one call (two chains, the second behind guard bytes);
// both must agree.  Prints "<out_len ...> | <chain_out_len>" and writes the decoded bytes to <out>.
//   chain_mirror_test --frame <frame> <out> <batchBlocks>   reads an LZ4 frame WITHOUT block independence through
//                     LZ4FrameInputStream(linkedBlocks = true) of lz4hip_streams.hpp and writes what it decodes; the default reader must
//                     refuse the same frame with the reference's message
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "../../lz4-java_amd/host/lz4hip_streams.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

template <class T> static T rd(const bytes& b, size_t& p) { T v; memcpy(&v, b.data() + p, sizeof v); p += sizeof v; return v; }

static int frame_mode(const char* path, const char* out, size_t batch) {
  bytes in;
  if (!slurp(path, in)) return 2;
  const std::string all(in.begin(), in.end());
  try {
    {
      std::istringstream s(all);
      lz4::LZ4FrameInputStream refuses(s);
      bool threw = false;
      try { (void)refuses.readAll(); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("BLOCK_INDEPENDENCE") != std::string::npos; }
      if (!threw) { fprintf(stderr, "the default reader did not refuse the frame\n"); return 1; }
    }
    std::istringstream s(all);
    lz4::LZ4FrameInputStream rd(s, false, lz4::BatchEngine(), batch, true);
    const bytes got = rd.readAll();
    std::ofstream o(out, std::ios::binary);
    o.write((const char*)got.data(), (std::streamsize)got.size());
    printf("%zu\n", got.size());
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}

int main(int argc, char** argv) {
  if (argc >= 5 && std::string(argv[1]) == "--frame") return frame_mode(argv[2], argv[3], (size_t)atoi(argv[4]));
  if (argc < 3) { fprintf(stderr, "usage: chain_mirror_test <chain> <out>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const uint32_t n = rd<uint32_t>(in, p), prefix = rd<uint32_t>(in, p);
  const uint64_t ccap = rd<uint64_t>(in, p);
  std::vector<int32_t> len(n), cap(n);
  std::vector<uint8_t> stored(n);
  for (uint32_t i = 0; i < n; i++) { len[i] = (int32_t)rd<uint32_t>(in, p); stored[i] = (uint8_t)rd<uint32_t>(in, p); cap[i] = rd<int32_t>(in, p); }
  const size_t guard = 32, hist_at = p;
  p += prefix;
  // two chains over the same streams: blocks [0, n) and [n, 2n)
  bytes src(in.begin() + p, in.end());
  std::vector<uint64_t> off(2 * n);
  std::vector<int32_t> len2(2 * n), cap2(2 * n);
  std::vector<uint8_t> stored2(2 * n);
  uint64_t o = 0;
  for (uint32_t i = 0; i < n; i++) { off[i] = off[n + i] = o; o += (uint64_t)len[i]; len2[i] = len2[n + i] = len[i]; cap2[i] = cap2[n + i] = cap[i]; stored2[i] = stored2[n + i] = stored[i]; }
  const size_t span = guard + prefix + (size_t)ccap;
  bytes dst(2 * span + guard, 0xEE);
  for (int k = 0; k < 2; k++) memcpy(dst.data() + k * span + guard, in.data() + hist_at, prefix);
  const std::vector<uint64_t> cdo = {guard + prefix, span + guard + prefix}, cc = {ccap, ccap};
  const std::vector<int32_t> pre = {(int32_t)prefix, (int32_t)prefix};
  try {   // the argument checks need no device
    bool threw = false;
    try { (void)lz4::LZ4HIPBatch::decompressSafeChain(src, off, len2, cap2, {0, n, 2 * n + 1}, dst, cdo, cc, pre, stored2); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::decompressSafeChain(src, off, len2, cap2, {0, n, 2 * n}, dst, {cdo[0], (uint64_t)dst.size()}, {ccap, ccap + 1}, pre, stored2); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::decompressSafeChain(src, off, len2, cap2, {0, n, 2 * n}, dst, cdo, cc, {(int32_t)(guard + prefix + 1), 0}, stored2); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::decompressSafeChain(src, off, len2, cap2, {0, n, 2 * n}, dst, cdo, cc, pre, {1}); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    const lz4::LZ4HIPBatch::Chains r = lz4::LZ4HIPBatch::decompressSafeChain(src, off, len2, cap2, {0, n, 2 * n}, dst, cdo, cc, pre, stored2);
    for (uint32_t i = 0; i < n; i++)
      if (r.lengths[i] != r.lengths[n + i]) { fprintf(stderr, "the two chains differ at block %u\n", i); return 1; }
    if (r.chainLengths[0] != r.chainLengths[1] || r.chainLengths[0] > ccap) return 1;
    const size_t done = (size_t)r.chainLengths[0];
    if (memcmp(dst.data() + cdo[0], dst.data() + cdo[1], done) != 0) { fprintf(stderr, "the two chains' bytes differ\n"); return 1; }
    for (int k = 0; k < 2; k++) {
      const uint8_t* q = dst.data() + k * span;
      for (size_t i = 0; i < guard; i++) if (q[i] != 0xEE) { fprintf(stderr, "guard byte changed\n"); return 1; }
      if (memcmp(q + guard, in.data() + hist_at, prefix) != 0) { fprintf(stderr, "history changed\n"); return 1; }
      for (size_t i = done; i < ccap; i++) if (q[guard + prefix + i] != 0xEE) { fprintf(stderr, "byte behind the decoded ones changed\n"); return 1; }
    }
    for (size_t i = 0; i < guard; i++) if (dst[2 * span + i] != 0xEE) return 1;
    if (!dump(argv[2], dst.data() + cdo[0], done)) return 1;
    for (uint32_t i = 0; i < n; i++) printf("%d ", r.lengths[i]);
    printf("| %llu\n", (unsigned long long)r.chainLengths[0]);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
