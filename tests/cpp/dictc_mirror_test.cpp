// tests/cpp/dictc_mirror_test.cpp -- exercises LZ4HIPCompressor::compressWithDict and LZ4HIPBatch::compressDict of the C++ host mirror
// (lz4-java_amd/host/lz4hip.hpp).  Built and run by tests/test_dictc_abi.py (argument checks, no device) and tests/test_gpu_dictc.py:
//   dictc_mirror_test <dictionary> <record> <out>   writes the compressed bytes to <out> and prints their count
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: dictc_mirror_test <dictionary> <record> <out>\n"); return 2; }
  bytes dictBytes, in;
  if (!slurp(argv[1], dictBytes) || !slurp(argv[2], in)) return 2;
  const int off = 3, doff = 5;                   // regions away from byte 0 of both vectors
  bytes src(in.size() + off);
  std::copy(in.begin(), in.end(), src.begin() + off);
  const lz4::LZ4HIPCompressor c;
  const int cap = c.maxCompressedLength((int)in.size());
  bytes dst((size_t)cap + doff + 16, 0xEE);
  try {   // the argument checks need no device
    lz4::LZ4Dictionary dict(dictBytes);
    bool threw = false;
    try { (void)c.compressWithDict(dict, src, off, (int)in.size() + 1, dst, doff, cap); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)c.compressWithDict(dict, src, off, (int)in.size(), dst, doff, cap + 17); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPCompressor(4).compressWithDict(dict, src, off, (int)in.size(), dst, doff, cap); } catch (const std::logic_error&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::compressDict(src, {(uint64_t)off}, {(int32_t)in.size(), 1}, dst, {0}, {cap}, dict); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)lz4::LZ4HIPBatch::compressDict(src, {(uint64_t)off}, {(int32_t)in.size()}, dst, {(uint64_t)doff + 17}, {cap}, dict); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    // the batch of two: the same record twice, the second slot one byte too small for anything but an empty record
    bytes dst2((size_t)cap + 8 + 1, 0xEE);
    const std::vector<int32_t> got = lz4::LZ4HIPBatch::compressDict(src, {(uint64_t)off, (uint64_t)off}, {(int32_t)in.size(), (int32_t)in.size()}, dst2,
                                                                    {0, (uint64_t)cap + 8}, {cap, 1}, dict);
    const int w = c.compressWithDict(dict, src, off, (int)in.size(), dst, doff, cap);
    if (w <= 0 || w > cap) return 1;
    if (got[0] != w || got[1] != (in.empty() ? 1 : 0)) { fprintf(stderr, "batch %d %d, single %d\n", got[0], got[1], w); return 1; }
    for (int i = 0; i < w; i++)
      if (dst2[(size_t)i] != dst[(size_t)(doff + i)]) { fprintf(stderr, "batch differs at %d\n", i); return 1; }
    for (size_t i = (size_t)cap; i < (size_t)cap + 8; i++)
      if (dst2[i] != 0xEE) { fprintf(stderr, "batch: byte %zu outside the slots changed\n", i); return 1; }
    if (!untouched(dst, (size_t)doff, (size_t)cap)) return 1;
    try { (void)c.compressWithDict(dict, src, off, (int)in.size(), dst, doff, w - 1); return 1; }
    catch (const lz4::LZ4Exception& e) { if (std::string(e.what()) != "maxDestLen is too small") throw; }
    if (!dump(argv[3], dst.data() + doff, (size_t)w)) return 1;
    printf("%d\n", w);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
