// tests/cpp/partial_mirror_test.cpp -- exercises LZ4SafeDecompressor::decompressPartial of the C++ host mirror
// (lz4-java_amd/host/lz4hip.hpp).  Built and run by tests/test_gpu_partial.py with an LZ4 block, a target and a capacity:
//   partial_mirror_test <stream> <target> <cap> <out>   writes the decoded bytes to <out> and prints the count, or prints
//                                                       "error <message>" for a stream liblz4 rejects
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: partial_mirror_test <stream> <target> <cap> <out>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in)) return 2;
  const int t = atoi(argv[2]), cap = atoi(argv[3]);
  const int room = t < cap ? t : cap;
  const int off = 3, doff = 5;                   // regions away from byte 0 of both vectors
  bytes src(in.size() + off);
  std::copy(in.begin(), in.end(), src.begin() + off);
  bytes dst((size_t)cap + doff + 16, 0xEE);
  try {
    const lz4::LZ4SafeDecompressor& d = lz4::LZ4Factory::hipInstance().safeDecompressor();
    bool threw = false;
    try { (void)d.decompressPartial(src, off, (int)in.size() + 1, dst, doff, t, cap); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)d.decompressPartial(src, off, (int)in.size(), dst, doff, t, cap + 17); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    int w;
    try {
      w = d.decompressPartial(src, off, (int)in.size(), dst, doff, t, cap);
    } catch (const lz4::LZ4Exception& e) {
      if (std::string(e.what()).rfind("Error decoding offset ", 0) != 0) throw;
      if (!untouched(dst, (size_t)doff, (size_t)room)) return 1;
      printf("error %s\n", e.what());
      return 0;
    }
    if (w < 0 || w > room) return 1;
    if (!untouched(dst, (size_t)doff, (size_t)room)) return 1;
    if (!dump(argv[4], dst.data() + doff, (size_t)w)) return 1;
    printf("%d\n", w);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
