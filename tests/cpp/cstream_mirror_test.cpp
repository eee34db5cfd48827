// tests/cpp/cstream_mirror_test.cpp -- exercises CompressStreams of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).
// Built by tests/test_cstream_abi.py and run by tests/test_gpu_cstream.py with one chain in a file:
//   cstream_mirror_test <chain> <out>
// <chain>: u32 n_blocks, u32 prefix_len, then per block {i32 src_len, i32 dst_cap}, the history bytes, the source (little endian): the
// file of cchain_mirror_test.  The blocks go through stream 1 of a set of three, cut into two calls behind everything the stream holds,
// and through LZ4HIPBatch::compressFastChain in one call; both must agree.  Prints "<out_len ...> | <consumed>" and writes the bytes of
// the blocks that succeeded, back to back, to <out>.
//   cstream_mirror_test --frame <data> <out> <blockSize 4..7> <batchBlocks> <flushEvery>   writes <data> through
//                     LZ4FrameOutputStream(linkedBlocks = true) with streamState(true) of lz4hip_streams.hpp, block by block, flushing
//                     every flushEvery blocks (0: never), reads the frame back and writes it to <out>
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

static int frame_mode(const char* path, const char* out, int blockSize, size_t batch, size_t flushEvery) {
  bytes in;
  if (!slurp(path, in)) return 2;
  try {
    std::ostringstream sink;
    {
      lz4::LZ4FrameOutputStream w(sink, (lz4::frame::BLOCKSIZE)blockSize, -1, {lz4::frame::BLOCK_CHECKSUM, lz4::frame::CONTENT_CHECKSUM}, lz4::BatchEngine(), batch, true);
      w.streamState(true);
      const size_t bs = (size_t)1 << (2 * blockSize + 8);
      size_t k = 0;
      for (size_t a = 0; a < in.size(); a += bs) {
        w.write(in.data() + a, in.size() - a < bs ? in.size() - a : bs);
        if (flushEvery && ++k % flushEvery == 0) w.flush();
      }
      w.close();
    }
    const std::string frame = sink.str();
    std::istringstream s(frame);
    lz4::LZ4FrameInputStream r(s, false, lz4::BatchEngine(), 64, true);
    if (r.readAll() != in) { fprintf(stderr, "the frame does not read back\n"); return 1; }
    if (!dump(out, (const uint8_t*)frame.data(), frame.size())) return 1;
    bool threw = false;   // the switch needs linked blocks and the fast chain
    try { std::ostringstream o2; lz4::LZ4FrameOutputStream w2(o2, (lz4::frame::BLOCKSIZE)blockSize); w2.streamState(true); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    printf("%zu\n", frame.size());
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}

int main(int argc, char** argv) {
  if (argc >= 7 && std::string(argv[1]) == "--frame") return frame_mode(argv[2], argv[3], atoi(argv[4]), (size_t)atoi(argv[5]), (size_t)atoi(argv[6]));
  if (argc < 3) { fprintf(stderr, "usage: cstream_mirror_test <chain> <out>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const uint32_t n = rd<uint32_t>(in, p), prefix = rd<uint32_t>(in, p);
  std::vector<int32_t> len(n), cap(n);
  std::vector<uint64_t> doff(n);
  size_t total = 0, room = 0;
  const size_t guard = 32;
  for (uint32_t i = 0; i < n; i++) {
    len[i] = rd<int32_t>(in, p); cap[i] = rd<int32_t>(in, p);
    doff[i] = guard + room + i * guard;
    total += (size_t)len[i]; room += (size_t)cap[i];
  }
  if (in.size() - p != prefix + total || n < 2) { fprintf(stderr, "bad chain file\n"); return 2; }
  bytes src(guard + prefix + total + guard, 0xA5);
  memcpy(src.data() + guard, in.data() + p, prefix + total);
  const uint32_t cut = n / 2;
  size_t first_bytes = 0;
  for (uint32_t i = 0; i < cut; i++) first_bytes += (size_t)len[i];
  bytes one(room + (n + 1) * guard, 0xEE), two = one;
  try {
    const lz4::LZ4HIPBatch::Chains want = lz4::LZ4HIPBatch::compressFastChain(src, {guard + prefix}, len, {0, n}, one, doff, cap, {(int32_t)prefix});
    lz4::CompressStreams streams(3);
    if (streams.size() != 3) return 1;
    bool threw = false;   // the id checks come before the library
    try { (void)streams.compress({3}, src, {guard + prefix}, len, {0, n}, two, doff, cap, {(int32_t)prefix}); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    const std::vector<int32_t> len_a(len.begin(), len.begin() + cut), len_b(len.begin() + cut, len.end());
    const std::vector<int32_t> cap_a(cap.begin(), cap.begin() + cut), cap_b(cap.begin() + cut, cap.end());
    const std::vector<uint64_t> off_a(doff.begin(), doff.begin() + cut), off_b(doff.begin() + cut, doff.end());
    const lz4::LZ4HIPBatch::Chains a = streams.compress({1}, src, {guard + prefix}, len_a, {0, cut}, two, off_a, cap_a, {(int32_t)prefix});
    // everything the stream holds (at most 64 KB) lies in front of the second call's source
    const size_t held = (prefix < 8 ? 0 : (prefix > 65536 ? 65536 : prefix)) + (size_t)a.chainLengths[0];
    const lz4::LZ4HIPBatch::Chains b = streams.compress({1}, src, {guard + prefix + first_bytes}, len_b, {0, n - cut}, two, off_b, cap_b,
                                                        {(int32_t)(held > 65536 ? 65536 : held)});
    std::vector<int32_t> got = a.lengths;
    got.insert(got.end(), b.lengths.begin(), b.lengths.end());
    if (got != want.lengths || a.chainLengths[0] + b.chainLengths[0] != want.chainLengths[0]) { fprintf(stderr, "the stream's results differ from the chain's\n"); return 1; }
    if (two != one) { fprintf(stderr, "the stream's bytes differ from the chain's\n"); return 1; }
    const lz4::CompressStreams::State s = streams.consumed(0, 3);
    const bool stopped = want.chainLengths[0] != total;
    if (s.consumed[1] != want.chainLengths[0] || s.consumed[0] != 0 || s.consumed[2] != 0 || (s.stopped[1] != 0) != stopped) return 1;
    streams.reset({1});
    if (streams.consumed(1, 1).consumed[0] != 0) return 1;
    bytes produced;
    for (uint32_t i = 0; i < n; i++)
      if (got[i] > 0) produced.insert(produced.end(), two.begin() + doff[i], two.begin() + doff[i] + got[i]);
    if (!dump(argv[2], produced.data(), produced.size())) return 1;
    for (uint32_t i = 0; i < n; i++) printf("%d ", got[i]);
    printf("| %llu\n", (unsigned long long)want.chainLengths[0]);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
