// tests/cpp/dstream_mirror_test.cpp -- exercises DecodeStreams / LZ4HIPBatch::decompressSafeStream of the C++ host mirror
// (lz4-java_amd/host/lz4hip.hpp).  Built and run by tests/test_gpu_dstream.py with one stream in a file:
//   dstream_mirror_test <stream>
// <stream> (tests/dstream_common.py stream_file; every number an i64, little endian): window length, dictionary length, lead (the
// dictionary lies directly in front of the window), n_blocks, n_calls, the state {prefix_end, prefix_len, ext_end, ext_len} (ends
// relative to the window; -1: the dictionary's end), the calls' cut points, per block {window offset, capacity, stream length}, the
// dictionary, the streams back to back.  The stream is decoded as stream 1 of a set of three, call after call, into
// [dictionary][128 x 0xEE][window][128 x 0xEE].  Prints the out_len values and the state behind the last call ("prefix_end prefix_len
// ext_end ext_len", ends relative to the window).  Exit code 0 = all good, 1 = a guard byte changed; with no GPU it must fail loudly
// (exit code 3).
#include <cstdio>
#include <cstring>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

static int64_t rd(const bytes& b, size_t& p) { int64_t v; memcpy(&v, b.data() + p, sizeof v); p += sizeof v; return v; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: dstream_mirror_test <stream>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  size_t p = 0;
  const int64_t win_len = rd(in, p), dict_len = rd(in, p), lead = rd(in, p), n = rd(in, p), calls = rd(in, p);
  int64_t st[4];
  for (int64_t& v : st) v = rd(in, p);
  std::vector<int64_t> cuts((size_t)calls), off((size_t)n), cap((size_t)n), len((size_t)n);
  for (int64_t& v : cuts) v = rd(in, p);
  for (int64_t i = 0; i < n; i++) { off[(size_t)i] = rd(in, p); cap[(size_t)i] = rd(in, p); len[(size_t)i] = rd(in, p); }
  const size_t guard = 128, gap = lead ? 0 : guard, win = (size_t)dict_len + gap;
  bytes dest(win + (size_t)win_len + guard, 0xEE);
  memcpy(dest.data(), in.data() + p, (size_t)dict_len);
  p += (size_t)dict_len;
  const bytes src(in.begin() + (long)p, in.end());
  try {
    lz4::DecodeStreams ds(3);
    if (st[1]) ds.set(1, st[0] < 0 ? (uint64_t)dict_len : win + (uint64_t)st[0], (uint64_t)st[1]);
    int64_t k = 0;
    uint64_t so = 0;
    for (int64_t cut : cuts) {
      std::vector<uint64_t> srcOff, destOff;
      std::vector<int32_t> srcLen, maxDestLen;
      for (; k < cut; k++) {
        srcOff.push_back(so); srcLen.push_back((int32_t)len[(size_t)k]); so += (uint64_t)len[(size_t)k];
        destOff.push_back(win + (uint64_t)off[(size_t)k]); maxDestLen.push_back((int32_t)cap[(size_t)k]);
      }
      // (a window that begins at the dictionary once the prefix can reach across the window's first edge: the header's rule)
      const uint64_t wbeg = (lead && k != cuts[0]) ? 0u : (uint64_t)win;
      const std::vector<int32_t> r = ds.decompress({1u}, src, srcOff, srcLen, {0u, (uint32_t)srcOff.size()}, dest, destOff, maxDestLen, {wbeg},
                                                   {(uint64_t)win + (uint64_t)win_len - wbeg});
      for (int32_t v : r) printf("%d ", v);
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
    if ((gap && dest[(size_t)dict_len + i] != 0xEE) || dest[win + (size_t)win_len + i] != 0xEE) { fprintf(stderr, "a guard byte changed\n"); return 1; }
  if (dict_len && memcmp(dest.data(), in.data() + (p - (size_t)dict_len), (size_t)dict_len) != 0) { fprintf(stderr, "the dictionary changed\n"); return 1; }
  return 0;
}
