// tests/cpp/hcstream_mirror_test.cpp -- CompressStreamsHC of lz4-java_amd/host/lz4hip.hpp (the C++ twin of the Python class) driven by a
// script file that tests/test_gpu_hcstream.py writes: ONE stream, a call per block, LZ4_loadDictHC and LZ4_saveDictHC as state edits.
//   in : int64 level, arena, n_ops; per op int64 kind (0 block, 1 loadDict, 2 saveDict), off, n, cap, k; then the blocks' bytes in order
//        (an op of kind 1 carries its dictionary's n bytes, which lie at [off - n, off) from the start)
//   out: per op int64 r (a block's result, saveDict's kept, 0), then the state's five words; then the blocks' output bytes in order
// Exit status 3: no device (the loud failure every entry point has).
#include <stdio.h>
#include <string.h>
#include <fstream>
#include <iterator>
#include "../../lz4-java_amd/host/lz4hip.hpp"

using namespace net::jpountz;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int64_t* q = (const int64_t*)in.data();
  const int64_t level = q[0], arena_size = q[1], n_ops = q[2];
  const uint8_t* data = in.data() + 8 * (3 + 5 * n_ops);
  bytes arena((size_t)arena_size, 0xA5);
  for (int64_t i = 0; i < n_ops; i++) {   // the dictionaries lie in the arena from the start
    const int64_t* op = q + 3 + 5 * i;
    if (op[0] == 1) memcpy(arena.data() + op[1] - op[2], data, (size_t)op[2]);
    if (op[0] != 2) data += op[2] > 0 && op[2] <= 0x7E000000 ? op[2] : 0;
  }
  data = in.data() + 8 * (3 + 5 * n_ops);
  std::vector<int64_t> head;
  std::vector<uint8_t> body;
  try {
    lz4::CompressStreamsHC hs(1, (int)level);
    for (int64_t i = 0; i < n_ops; i++) {
      const int64_t* op = q + 3 + 5 * i;
      const int64_t held = op[0] != 2 && op[2] > 0 && op[2] <= 0x7E000000 ? op[2] : 0;
      int64_t r = 0;
      if (op[0] == 1) {
        hs.loadDict(0, (uint64_t)op[1], (uint64_t)op[2]);
      } else if (op[0] == 2) {
        const uint64_t end = hs.state(0).prefix_end;
        r = hs.saveDict(0, (uint64_t)op[1], (int)op[4]);
        memmove(arena.data() + op[1], arena.data() + end - r, (size_t)r);   // (the caller's part of LZ4_saveDictHC: the copy)
      } else {
        memcpy(arena.data() + op[1], data, (size_t)held);
        bytes dst((size_t)(op[3] > 0 ? op[3] : 0) + 1);
        r = hs.compress({0}, arena, {(uint64_t)op[1]}, {(int32_t)op[2]}, {0, 1}, dst, {0}, {(int32_t)op[3]})[0];
        body.insert(body.end(), dst.begin(), dst.begin() + (r > 0 ? r : 0));
      }
      data += held;
      const lz4hip_hcstream_state& s = hs.state(0);
      head.insert(head.end(), {r, (int64_t)s.prefix_end, (int64_t)s.prefix_len, (int64_t)s.ext_end, (int64_t)s.ext_len, (int64_t)s.index});
    }
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char*)head.data(), (std::streamsize)(head.size() * 8));
  o.write((const char*)body.data(), (std::streamsize)body.size());
  return o.good() ? 0 : 1;
}
