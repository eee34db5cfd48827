// tests/cpp/caccel_mirror_test.cpp -- exercises the acceleration parameter of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp:
// LZ4HIPBatch::compressFastChain, CompressStreams::compress and compressAt; lz4hip_streams.hpp: LZ4FrameOutputStream::acceleration).
// Built and run by tests/test_caccel_abi.py / tests/test_gpu_caccel.py with one chain in a file:
//   caccel_mirror_test <chain> <out> <acceleration>
// <chain>: u32 n_blocks, u32 prefix_len, then per block {i32 src_len, i32 dst_cap}, the history bytes, the source (little endian).
// The chain is compressed three times at the acceleration: as one chain, as a resident stream cut into two calls, and as a resident
// stream through compressAt in one call; all three must agree.  Prints "<out_len ...> | <chain_consumed>" and writes the bytes of the
// blocks that succeeded, back to back, to <out> (the test compares them with the reference's LZ4_compress_fast_continue).
//   caccel_mirror_test --frame <data> <out> <acceleration> <streamState 0|1>   writes <data> in 64 KiB blocks through
//                     LZ4FrameOutputStream(linkedBlocks = true) with acceleration(N), reads the frame back and writes it to <out>
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

static int frame_mode(const char* path, const char* out, int accel, bool state) {
  bytes in;
  if (!slurp(path, in)) return 2;
  try {
    {   // the setter's own checks need no device
      std::ostringstream s0;
      lz4::LZ4FrameOutputStream plain(s0);
      bool threw = false;
      try { plain.acceleration(8); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;
      plain.acceleration(1);
      lz4::LZ4FrameOutputStream hc(s0, lz4::frame::SIZE_64KB, -1, {}, lz4::BatchEngine(), 64, true, 9);
      threw = false;
      try { hc.acceleration(8); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;
    }
    std::ostringstream sink;
    {
      lz4::LZ4FrameOutputStream w(sink, lz4::frame::SIZE_64KB, -1, {}, lz4::BatchEngine(), 64, true);
      w.streamState(state);
      w.acceleration(accel);
      w.write(in);
      w.close();
    }
    const std::string frame = sink.str();
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
  if (argc >= 6 && std::string(argv[1]) == "--frame") return frame_mode(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]) != 0);
  if (argc < 4) { fprintf(stderr, "usage: caccel_mirror_test <chain> <out> <acceleration>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  const int accel = atoi(argv[3]);
  size_t p = 0;
  const uint32_t n = rd<uint32_t>(in, p), prefix = rd<uint32_t>(in, p);
  if (n < 2) { fprintf(stderr, "the chain needs two blocks\n"); return 2; }
  std::vector<int32_t> len(n), cap(n);
  size_t total = 0, room = 0;
  for (uint32_t i = 0; i < n; i++) { len[i] = rd<int32_t>(in, p); cap[i] = rd<int32_t>(in, p); total += (size_t)len[i]; room += (size_t)cap[i]; }
  const size_t guard = 32;
  if (in.size() - p != prefix + total) { fprintf(stderr, "bad chain file\n"); return 2; }
  bytes src(guard + prefix + total + guard, 0xA5);
  memcpy(src.data() + guard, in.data() + p, prefix + total);
  std::vector<uint64_t> doff(n), soff(n);
  { uint64_t o = guard, s = guard + prefix; for (uint32_t i = 0; i < n; i++) { doff[i] = o; o += (uint64_t)cap[i] + guard; soff[i] = s; s += (uint64_t)len[i]; } }
  const size_t dst_size = room + (n + 1) * guard;
  try {
    bytes d1(dst_size, 0xEE), d2(dst_size, 0xEE), d3(dst_size, 0xEE);
    const lz4::LZ4HIPBatch::Chains one = lz4::LZ4HIPBatch::compressFastChain(src, {guard + prefix}, len, {0, n}, d1, doff, cap, {(int32_t)prefix}, accel);
    // the same blocks as a resident stream in two calls, the second with everything the stream holds in front of its source
    const uint32_t h = n / 2;
    lz4::CompressStreams set(2);
    const std::vector<int32_t> len_a(len.begin(), len.begin() + h), len_b(len.begin() + h, len.end());
    const std::vector<int32_t> cap_a(cap.begin(), cap.begin() + h), cap_b(cap.begin() + h, cap.end());
    const std::vector<uint64_t> doff_a(doff.begin(), doff.begin() + h), doff_b(doff.begin() + h, doff.end());
    const lz4::LZ4HIPBatch::Chains a = set.compress({1u}, src, {guard + prefix}, len_a, {0, h}, d2, doff_a, cap_a, {(int32_t)prefix}, accel);
    const lz4::LZ4HIPBatch::Chains b = set.compress({1u}, src, {soff[h]}, len_b, {0, n - h}, d2, doff_b, cap_b, {(int32_t)(soff[h] - guard)}, accel);
    // and through compressAt on the set's other stream, one call
    const lz4::LZ4HIPBatch::Chains at = set.compressAt({0u}, src, soff, len, {0, n}, {guard + prefix}, {(int32_t)prefix}, {0}, {(uint64_t)src.size()}, d3, doff, cap, accel);
    std::vector<int32_t> two(a.lengths);
    two.insert(two.end(), b.lengths.begin(), b.lengths.end());
    if (two != one.lengths || at.lengths != one.lengths || a.chainLengths[0] + b.chainLengths[0] != one.chainLengths[0] || at.chainLengths[0] != one.chainLengths[0]) {
      fprintf(stderr, "the chain, the stream in two calls and compressAt differ in their values\n");
      return 1;
    }
    if (d2 != d1 || d3 != d1) { fprintf(stderr, "the chain, the stream in two calls and compressAt differ in their bytes\n"); return 1; }
    const lz4::CompressStreams::State st = set.consumed(0, 2);
    if (st.consumed[0] != one.chainLengths[0] || st.consumed[1] != one.chainLengths[0]) return 1;
    bytes produced;
    size_t pos = 0;   // every byte of dst is a guard, a block's result, or untouched
    for (uint32_t i = 0; i < n; i++) {
      const size_t got = one.lengths[i] > 0 ? (size_t)one.lengths[i] : 0;
      if (got > (size_t)cap[i]) return 1;
      for (; pos < doff[i]; pos++) if (d1[pos] != 0xEE) { fprintf(stderr, "guard byte changed\n"); return 1; }
      for (size_t k = got; k < (size_t)cap[i]; k++) if (d1[doff[i] + k] != 0xEE) { fprintf(stderr, "byte behind block %u's result changed\n", i); return 1; }
      pos = doff[i] + (size_t)cap[i];
      produced.insert(produced.end(), d1.begin() + doff[i], d1.begin() + doff[i] + got);
    }
    for (; pos < d1.size(); pos++) if (d1[pos] != 0xEE) { fprintf(stderr, "guard byte changed\n"); return 1; }
    if (!dump(argv[2], produced.data(), produced.size())) return 1;
    for (uint32_t i = 0; i < n; i++) printf("%d ", one.lengths[i]);
    printf("| %llu\n", (unsigned long long)one.chainLengths[0]);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
