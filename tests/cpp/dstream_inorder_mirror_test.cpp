// tests/cpp/dstream_inorder_mirror_test.cpp -- exercises DecodeStreams(n, inOrder) / LZ4HIPBatch::decompressSafeStream(.., inOrder) /
// LZ4HIPBatch::decoderRingBufferSize of the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).  Built and run by
// tests/test_gpu_dstream_inorder.py (and, without a GPU, tests/test_dstream_inorder_abi.py) with one stream in a file:
//   dstream_inorder_mirror_test <stream> <out> [alt]
// <stream>: the file dstream_mirror_test.cpp describes, without a dictionary.  The stream is decoded as stream 1 of an in-order set of
// three, call after call, into [128 x 0xEE][window][128 x 0xEE]; with `alt` every second call names the existing entry point (a stream
// none of whose slots overlaps).  Prints the out_len values and the state behind the last call ("prefix_end prefix_len ext_end ext_len",
// ends relative to the window) and writes the window to <out>.  Exit code 0 = all good, 1 = a guard byte changed or a ring size is
// wrong; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstring>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

static int64_t rd(const bytes& b, size_t& p) { int64_t v; memcpy(&v, b.data() + p, sizeof v); p += sizeof v; return v; }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: dstream_inorder_mirror_test <stream> <out> [alt]\n"); return 2; }
  const bool alt = argc > 3 && std::string(argv[3]) == "alt";
  if (lz4::LZ4HIPBatch::decoderRingBufferSize(4096) != 65536 + 14 + 4096 || lz4::LZ4HIPBatch::decoderRingBufferSize(-1) != 0 ||
      lz4::LZ4HIPBatch::decoderRingBufferSize(3) != 65536 + 14 + 16) { fprintf(stderr, "decoderRingBufferSize\n"); return 1; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const int64_t win_len = rd(in, p), dict_len = rd(in, p), lead = rd(in, p), n = rd(in, p), calls = rd(in, p);
  int64_t st[4];
  for (int64_t& v : st) v = rd(in, p);
  if (dict_len || lead || st[1]) return 2;
  std::vector<int64_t> cuts((size_t)calls), off((size_t)n), cap((size_t)n), len((size_t)n);
  for (int64_t& v : cuts) v = rd(in, p);
  for (int64_t i = 0; i < n; i++) { off[(size_t)i] = rd(in, p); cap[(size_t)i] = rd(in, p); len[(size_t)i] = rd(in, p); }
  const size_t guard = 128, win = guard;
  bytes dest(win + (size_t)win_len + guard, 0xEE);
  const bytes src(in.begin() + (long)p, in.end());
  try {
    lz4::DecodeStreams ds(3, true);
    int64_t k = 0, ci = 0;
    uint64_t so = 0;
    for (int64_t cut : cuts) {
      std::vector<uint64_t> srcOff, destOff;
      std::vector<int32_t> srcLen, maxDestLen;
      for (; k < cut; k++) {
        srcOff.push_back(so); srcLen.push_back((int32_t)len[(size_t)k]); so += (uint64_t)len[(size_t)k];
        destOff.push_back(win + (uint64_t)off[(size_t)k]); maxDestLen.push_back((int32_t)cap[(size_t)k]);
      }
      const std::vector<uint32_t> first{0u, (uint32_t)srcOff.size()};
      const std::vector<int32_t> r = (alt && (ci & 1))
          ? ds.decompress({1u}, src, srcOff, srcLen, first, dest, destOff, maxDestLen, {(uint64_t)win}, {(uint64_t)win_len}, false)
          : ds.decompress({1u}, src, srcOff, srcLen, first, dest, destOff, maxDestLen, {(uint64_t)win}, {(uint64_t)win_len});
      for (int32_t v : r) printf("%d ", v);
      ci++;
    }
    const lz4hip_dstream_state& s = ds.state(1);
    printf("\n%lld %llu %lld %llu\n", (long long)s.prefix_end - (long long)win, (unsigned long long)s.prefix_len, (long long)s.ext_end - (long long)win,
           (unsigned long long)s.ext_len);
    if (ds.state(0).prefix_len || ds.state(2).prefix_len) { fprintf(stderr, "another stream's state changed\n"); return 1; }
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  for (size_t i = 0; i < guard; i++)
    if (dest[i] != 0xEE || dest[win + (size_t)win_len + i] != 0xEE) { fprintf(stderr, "a guard byte changed\n"); return 1; }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(dest.data() + win, 1, (size_t)win_len, o) != (size_t)win_len) return 2;
  fclose(o);
  return 0;
}
