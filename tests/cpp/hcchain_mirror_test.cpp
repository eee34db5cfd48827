// tests/cpp/hcchain_mirror_test.cpp -- exercises LZ4HIPBatch::compressHCChain of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).
// Built and run by tests/test_hcchain_abi.py and tests/test_gpu_hcchain.py with one chain in a file:
//   hcchain_mirror_test <chain> <out> <level>
// <chain>: u32 n_blocks, u32 prefix_len, then per block {i32 src_len, i32 dst_cap}, the history bytes, the source (little endian).
// The chain is compressed TWICE in one call (two chains, the second behind guard bytes); both must agree.  Prints "<out_len ...>" and
// writes the bytes of the blocks that succeeded, back to back, to <out>.
//   hcchain_mirror_test --frame <data> <out> <blockSize 4..7> <batchBlocks> <level>   writes <data> through
//                     LZ4FrameOutputStream(linkedBlocks = true, level) of lz4hip_streams.hpp, in pieces of batchBlocks blocks, reads the
//                     frame back through LZ4FrameInputStream(linkedBlocks = true) and writes the frame to <out>
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "../../lz4-java_amd/host/lz4hip_streams.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

template <class T> static T rd(const bytes& b, size_t& p) { T v; memcpy(&v, b.data() + p, sizeof v); p += sizeof v; return v; }

static int frame_mode(const char* path, const char* out, int blockSize, size_t batch, int level) {
  bytes in;
  if (!slurp(path, in)) return 2;
  try {
    std::ostringstream sink;
    {
      bool threw = false;   // a level without linked blocks is refused before anything is written
      try { lz4::LZ4FrameOutputStream bad(sink, (lz4::frame::BLOCKSIZE)blockSize, -1, {lz4::frame::BLOCK_INDEPENDENCE}, lz4::BatchEngine(), batch, false, level); }
      catch (const std::invalid_argument&) { threw = true; }
      if (!threw || !sink.str().empty()) { fprintf(stderr, "a level without linkedBlocks was accepted\n"); return 1; }
      lz4::LZ4FrameOutputStream w(sink, (lz4::frame::BLOCKSIZE)blockSize, -1, {lz4::frame::BLOCK_CHECKSUM, lz4::frame::CONTENT_CHECKSUM}, lz4::BatchEngine(), batch, true,
                                  level);
      const size_t piece = batch << (2 * blockSize + 8);
      for (size_t a = 0; a < in.size(); a += piece) w.write(in.data() + a, in.size() - a < piece ? in.size() - a : piece);
      w.close();
    }
    const std::string frame = sink.str();
    if ((uint8_t)frame[4] & 0x20) { fprintf(stderr, "the frame carries the block-independence flag\n"); return 1; }
    std::istringstream s(frame);
    lz4::LZ4FrameInputStream r(s, false, lz4::BatchEngine(), 64, true);
    if (r.readAll() != in) { fprintf(stderr, "the frame does not read back\n"); return 1; }
    if (!dump(out, (const uint8_t*)frame.data(), frame.size())) return 1;
    printf("%zu\n", frame.size());
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}

int main(int argc, char** argv) {
  if (argc >= 7 && std::string(argv[1]) == "--frame") return frame_mode(argv[2], argv[3], atoi(argv[4]), (size_t)atoi(argv[5]), atoi(argv[6]));
  if (argc < 4) { fprintf(stderr, "usage: hcchain_mirror_test <chain> <out> <level>\n"); return 2; }
  const int level = atoi(argv[3]);
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const uint32_t n = rd<uint32_t>(in, p), prefix = rd<uint32_t>(in, p);
  std::vector<int32_t> len(2 * n), cap(2 * n);
  size_t total = 0, room = 0;
  for (uint32_t i = 0; i < n; i++) {
    len[i] = len[n + i] = rd<int32_t>(in, p); cap[i] = cap[n + i] = rd<int32_t>(in, p);
    total += (size_t)len[i]; room += (size_t)cap[i];
  }
  const size_t guard = 32, span = guard + prefix + total;
  if (in.size() - p != prefix + total) { fprintf(stderr, "bad chain file\n"); return 2; }
  // two chains over copies of the same history and source
  bytes src(2 * span + guard, 0xA5);
  for (int k = 0; k < 2; k++) memcpy(src.data() + k * span + guard, in.data() + p, prefix + total);
  const std::vector<uint64_t> cso = {guard + prefix, span + guard + prefix};
  const std::vector<int32_t> pre = {(int32_t)prefix, (int32_t)prefix};
  std::vector<uint64_t> doff(2 * n);
  bytes dst(2 * (room + n * guard) + guard, 0xEE);
  { uint64_t o = guard; for (uint32_t i = 0; i < 2 * n; i++) { doff[i] = o; o += (uint64_t)cap[i] + guard; } }
  const bytes src_before = src;
  try {   // the argument checks need no device
    bool threw = false;
    try { (void)lz4::LZ4HIPBatch::compressHCChain(src, cso, len, {0, n, 2 * n + 1}, dst, doff, cap, pre, level); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::compressHCChain(src, {cso[0], (uint64_t)src.size() + 1}, len, {0, n, 2 * n}, dst, doff, cap, pre, level); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::compressHCChain(src, cso, len, {0, n, 2 * n}, dst, doff, cap, {(int32_t)(guard + prefix + 1), 0}, level); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::compressHCChain(src, cso, len, {0, n, 2 * n}, dst, doff, cap, {1}, level); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    const std::vector<int32_t> r = lz4::LZ4HIPBatch::compressHCChain(src, cso, len, {0, n, 2 * n}, dst, doff, cap, pre, level);
    if (src != src_before) { fprintf(stderr, "the source changed\n"); return 1; }
    bytes produced;
    size_t at = 0;   // every byte of dst is a guard, a block's result, or untouched
    for (uint32_t i = 0; i < 2 * n; i++) {
      if (r[i] != r[(i + n) % (2 * n)]) { fprintf(stderr, "the two chains differ at block %u\n", i % n); return 1; }
      const size_t got = r[i] > 0 ? (size_t)r[i] : 0;
      if (got > (size_t)cap[i]) return 1;
      for (; at < doff[i]; at++) if (dst[at] != 0xEE) { fprintf(stderr, "guard byte changed\n"); return 1; }
      for (size_t k = got; k < (size_t)cap[i]; k++) if (dst[doff[i] + k] != 0xEE) { fprintf(stderr, "byte behind block %u's result changed\n", i); return 1; }
      at = doff[i] + (size_t)cap[i];
      if (i < n) produced.insert(produced.end(), dst.begin() + doff[i], dst.begin() + doff[i] + got);
      else if (memcmp(dst.data() + doff[i], dst.data() + doff[i - n], got) != 0) { fprintf(stderr, "the two chains' bytes differ\n"); return 1; }
    }
    for (; at < dst.size(); at++) if (dst[at] != 0xEE) { fprintf(stderr, "guard byte changed\n"); return 1; }
    if (!dump(argv[2], produced.data(), produced.size())) return 1;
    for (uint32_t i = 0; i < n; i++) printf("%d ", r[i]);
    printf("\n");
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
