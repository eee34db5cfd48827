// tests/cpp/cxstream_mirror_test.cpp -- exercises CompressStreams::compressAt of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).
// Built by tests/test_cxstream_abi.py and run by tests/test_gpu_cxstream.py with one stream in a file:
//   cxstream_mirror_test <stream> <out>
// <stream>: i64 win_len, n_blocks, n_calls; per call {i64 end block, hist_end (relative to the window), hist_len}; per block {i64 off, len,
// cap}; the blocks' bytes (little endian): the file of fake_jni_cxstream.  The blocks go through stream 1 of a set of three, call after
// call, the producer writing each call's blocks into the window first.  Prints the out_len values and writes the bytes of the blocks
// that succeeded, back to back, to <out>.
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

static int64_t rd(const bytes& b, size_t& p) { int64_t v; memcpy(&v, b.data() + p, sizeof v); p += sizeof v; return v; }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: cxstream_mirror_test <stream> <out>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const int64_t win_len = rd(in, p), n = rd(in, p), calls = rd(in, p);
  if (win_len < 0 || n < 0 || calls < 1 || in.size() < 24 + 24 * (size_t)(calls + n)) { fprintf(stderr, "bad stream file\n"); return 2; }
  const size_t calls_at = p, blocks_at = calls_at + 24 * (size_t)calls;
  size_t data_p = blocks_at + 24 * (size_t)n;
  const uint64_t guard = 32, win = guard;
  bytes src(guard + (size_t)win_len + guard, 0xA5);
  size_t room = guard;
  for (int64_t i = 0; i < n; i++) { size_t q = blocks_at + 24 * (size_t)i + 16; room += (size_t)rd(in, q) + guard; }
  bytes dst(room, 0xEE);
  try {
    lz4::CompressStreams streams(3);
    bool threw = false;   // the shape checks come before the library
    try { (void)streams.compressAt({3}, src, {}, {}, {0, 0}, {0}, {0}, {win}, {(uint64_t)win_len}, dst, {}, {}); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    bytes produced;
    int64_t k = 0;
    size_t slot = guard;
    for (int64_t ci = 0; ci < calls; ci++) {
      p = calls_at + 24 * (size_t)ci;
      const int64_t cut = rd(in, p), hist_end = rd(in, p), hist_len = rd(in, p), nb = cut - k;
      if (nb < 0 || cut > n) return 2;
      std::vector<uint64_t> so, doff;
      std::vector<int32_t> sl, dc;
      for (int64_t i = 0; i < nb; i++) {
        p = blocks_at + 24 * (size_t)(k + i);
        const int64_t off = rd(in, p), len = rd(in, p), cap = rd(in, p);
        if (off < 0 || len < 0 || cap < 0 || off + len > win_len || data_p + (size_t)len > in.size()) return 2;
        memcpy(src.data() + win + (size_t)off, in.data() + data_p, (size_t)len);   // the producer writes the block into its place
        data_p += (size_t)len;
        so.push_back(win + (uint64_t)off); sl.push_back((int32_t)len); doff.push_back(slot); dc.push_back((int32_t)cap);
        slot += (size_t)cap + guard;
      }
      const lz4::LZ4HIPBatch::Chains r = streams.compressAt({1}, src, so, sl, {0, (uint32_t)nb}, {hist_len ? win + (uint64_t)hist_end : 0}, {(int32_t)hist_len}, {win},
                                                            {(uint64_t)win_len}, dst, doff, dc);
      for (int64_t i = 0; i < nb; i++) {
        printf("%d ", r.lengths[i]);
        if (r.lengths[i] > 0) produced.insert(produced.end(), dst.begin() + doff[i], dst.begin() + doff[i] + r.lengths[i]);
        for (size_t g = (size_t)(r.lengths[i] > 0 ? r.lengths[i] : 0); r.lengths[i] != 0 && g < (size_t)dc[i] + guard; g++)
          if (dst[doff[i] + g] != 0xEE) { fprintf(stderr, "written past a result\n"); return 1; }
      }
      k = cut;
    }
    printf("\n");
    if (!dump(argv[2], produced.data(), produced.size())) return 1;
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
