// tests/cpp/dict_mirror_test.cpp -- exercises LZ4Dictionary, LZ4SafeDecompressor::decompressWithDict and LZ4HIPBatch::decompressSafeDict of
// the C++ host mirror (lz4-java_amd/host/lz4hip.hpp).  Built and run by tests/test_gpu_dict.py with a dictionary, an LZ4 block that was
// compressed against it and a capacity:
//   dict_mirror_test <dictionary> <stream> <cap> <out>   writes the decoded bytes to <out> and prints the count, or prints
//                                                        "error <message>" for a stream liblz4 rejects
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: dict_mirror_test <dictionary> <stream> <cap> <out>\n"); return 2; }
  bytes dictBytes, in;
  if (!slurp(argv[1], dictBytes) || !slurp(argv[2], in)) return 2;
  const int cap = atoi(argv[3]);
  const int off = 3, doff = 5;                   // regions away from byte 0 of both vectors
  bytes src(in.size() + off);
  std::copy(in.begin(), in.end(), src.begin() + off);
  bytes dst((size_t)cap + doff + 16, 0xEE);
  try {   // the argument checks need no device
    bool threw = false;
    try { lz4::LZ4Dictionary bad(dictBytes.data(), -1); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { lz4::LZ4Dictionary bad(nullptr, 4); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    lz4::LZ4Dictionary dict(dictBytes);
    if (dict.size() != (int)dictBytes.size()) { fprintf(stderr, "size() = %d\n", dict.size()); return 1; }
    lz4::LZ4Dictionary moved(std::move(dict));
    if (moved.size() != (int)dictBytes.size() || dict.handle() != nullptr) return 1;
    const lz4::LZ4SafeDecompressor& d = lz4::LZ4Factory::hipInstance().safeDecompressor();
    threw = false;
    try { (void)d.decompressWithDict(moved, src, off, (int)in.size() + 1, dst, doff, cap); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    threw = false;
    try { (void)d.decompressWithDict(moved, src, off, (int)in.size(), dst, doff, cap + 17); } catch (const std::out_of_range&) { threw = true; }
    if (!threw) return 1;
    // the batch of two: the same block twice, into two slots of a second buffer
    bytes dst2((size_t)2 * cap + 24, 0xEE);
    const std::vector<int32_t> got = lz4::LZ4HIPBatch::decompressSafeDict(src, {(uint64_t)off, (uint64_t)off}, {(int32_t)in.size(), (int32_t)in.size()}, dst2,
                                                                          {0, (uint64_t)cap + 8}, {cap, cap}, moved);
    int w;
    try {
      w = d.decompressWithDict(moved, src, off, (int)in.size(), dst, doff, cap);
    } catch (const lz4::LZ4Exception& e) {
      if (std::string(e.what()).rfind("Error decoding offset ", 0) != 0) throw;
      const int code = -(atoi(e.what() + 22) - off);
      if (got[0] != code || got[1] != code) { fprintf(stderr, "batch %d %d, single %d\n", got[0], got[1], code); return 1; }
      if (!untouched(dst, (size_t)doff, (size_t)cap)) return 1;
      printf("error %s\n", e.what());
      return 0;
    }
    if (w < 0 || w > cap) return 1;
    if (got[0] != w || got[1] != w) { fprintf(stderr, "batch %d %d, single %d\n", got[0], got[1], w); return 1; }
    for (int k = 0; k < 2; k++)
      for (int i = 0; i < w; i++)
        if (dst2[(size_t)k * (cap + 8) + i] != dst[doff + i]) { fprintf(stderr, "batch slot %d differs at %d\n", k, i); return 1; }
    for (size_t i = 0; i < dst2.size(); i++) {
      const bool in0 = i < (size_t)cap, in1 = i >= (size_t)cap + 8 && i < (size_t)2 * cap + 8;
      if (!in0 && !in1 && dst2[i] != 0xEE) { fprintf(stderr, "batch: byte %zu outside the slots changed\n", i); return 1; }
    }
    if (!untouched(dst, (size_t)doff, (size_t)cap)) return 1;
    if (!dump(argv[4], dst.data() + doff, (size_t)w)) return 1;
    printf("%d\n", w);
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
