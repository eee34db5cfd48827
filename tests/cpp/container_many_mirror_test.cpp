// tests/cpp/container_many_mirror_test.cpp -- exercises BatchEngine::containerDecodeMany of the C++ host mirror
// (lz4-java_amd/host/lz4hip_streams.hpp).  Built and run by tests/test_container_many_abi.py / tests/test_gpu_container_many.py:
//   container_many_mirror_test --streams <kind> <batchBlocks> <items> <out>
//     readFrames (kind 0) / readBlockStreams (kind 1) over <items>: u32 count, then per item {u64 len, bytes} of whole streams; every
//     result is compared here with the sequential reader of the same item (bytes, exception class and message); prints per item
//     "R <bytes> <class or -> <message>" and writes the bytes, item after item, to <out>
//   container_many_mirror_test <cases> <out>
//     <cases>: tests/cpp/container_rules_test.cpp's file -- u32 count, then per item {u32 kind, u32 flags, u32 max_block, u32 n_max,
//              u64 (unused), u64 len, bytes}; one kind and one n_max for all items
//     prints per item "I <blocks> <consumed> <why> <code> <decoded bytes> <sizes...>", writes all decoded bytes, item after item, to <out>
// Exit code 0 = all good; with no GPU it must fail loudly (exit code 3).
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip_streams.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

template <class Reader> static Reader make(std::istream& in, size_t batch);
template <> lz4::LZ4FrameInputStream make<lz4::LZ4FrameInputStream>(std::istream& in, size_t batch) { return lz4::LZ4FrameInputStream(in, false, lz4::BatchEngine(), batch); }
template <> lz4::LZ4BlockInputStream make<lz4::LZ4BlockInputStream>(std::istream& in, size_t batch) { return lz4::LZ4BlockInputStream(in, true, lz4::BatchEngine(), batch); }

// the sequential reader over one item, as ManyDriver records a reader's end
template <class Reader>
static lz4::ReadResult sequential(const bytes& item, size_t batch) {
  lz4::ReadResult r;
  std::istringstream in(std::string(item.begin(), item.end()));
  try {
    Reader rd = make<Reader>(in, batch);
    uint8_t buf[4096];
    for (size_t k; (k = rd.read(buf, sizeof buf)) != 0;) r.data.insert(r.data.end(), buf, buf + k);
  } catch (const lz4::EOFException& e) { r.errorClass = "EOFException"; r.error = e.what(); }
  catch (const lz4::IOException& e) { r.errorClass = "IOException"; r.error = e.what(); }
  catch (const lz4::LZ4Exception&) { throw; }
  catch (const std::exception& e) { r.errorClass = "exception"; r.error = e.what(); }
  return r;
}

static int streams(int kind, size_t batch, const char* path, const char* outPath) {
  bytes in;
  if (!slurp(path, in) || in.size() < 4) return 2;
  uint32_t count;
  memcpy(&count, in.data(), 4);
  size_t p = 4;
  std::vector<bytes> items;
  for (uint32_t i = 0; i < count; i++) {
    uint64_t len;
    if (p + 8 > in.size()) return 2;
    memcpy(&len, in.data() + p, 8); p += 8;
    if (p + len > in.size()) return 2;
    items.emplace_back(in.begin() + (ptrdiff_t)p, in.begin() + (ptrdiff_t)(p + len));
    p += len;
  }
  const std::vector<lz4::ReadResult> got = kind == 0 ? lz4::readFrames(items, lz4::BatchEngine(), batch) : lz4::readBlockStreams(items, lz4::BatchEngine(), batch);
  if (got.size() != items.size()) return 1;
  bytes all;
  for (size_t i = 0; i < items.size(); i++) {
    const lz4::ReadResult want = kind == 0 ? sequential<lz4::LZ4FrameInputStream>(items[i], batch) : sequential<lz4::LZ4BlockInputStream>(items[i], batch);
    if (got[i].data != want.data || got[i].errorClass != want.errorClass || got[i].error != want.error) {
      fprintf(stderr, "item %zu: %zu bytes, %s \"%s\"; the sequential reader: %zu bytes, %s \"%s\"\n", i, got[i].data.size(), got[i].errorClass.c_str(),
              got[i].error.c_str(), want.data.size(), want.errorClass.c_str(), want.error.c_str());
      return 1;
    }
    printf("R %zu %s %s\n", got[i].data.size(), got[i].errorClass.empty() ? "-" : got[i].errorClass.c_str(), got[i].error.c_str());
    all.insert(all.end(), got[i].data.begin(), got[i].data.end());
  }
  return dump(outPath, all.data(), all.size()) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc >= 6 && std::string(argv[1]) == "--streams") {
    try { return streams(atoi(argv[2]), (size_t)atoi(argv[3]), argv[4], argv[5]); }
    catch (const lz4::LZ4Exception& e) { fprintf(stderr, "%s\n", e.what()); return 3; }
  }
  if (argc < 3) { fprintf(stderr, "usage: container_many_mirror_test <cases> <out>\n"); return 2; }
  bytes in;
  if (!slurp(argv[1], in) || in.size() < 4) return 2;
  uint32_t count;
  memcpy(&count, in.data(), 4);
  size_t p = 4;
  std::vector<bytes> bodies;
  std::vector<uint32_t> maxBlock;
  std::vector<uint8_t> cks;
  uint32_t kind = 0, nMax = 1;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t h[4];
    uint64_t len;
    if (p + 32 > in.size()) return 2;
    memcpy(h, in.data() + p, 16); memcpy(&len, in.data() + p + 24, 8); p += 32;
    if (p + len > in.size()) return 2;
    kind = h[0]; nMax = h[3];
    cks.push_back((uint8_t)h[1]); maxBlock.push_back(h[2]);
    bodies.emplace_back(in.begin() + (ptrdiff_t)p, in.begin() + (ptrdiff_t)(p + len));
    p += len;
  }
  try {
    lz4::BatchEngine e;
    bool threw = false;
    try { (void)e.containerDecodeMany((int)kind, bodies, std::vector<uint32_t>(bodies.size() + 1, 1u), nMax, cks); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return 1;
    if (!e.containerDecodeMany((int)kind, {}, {}, nMax, {}).empty()) return 1;
    const std::vector<lz4::BatchEngine::ContainerRun> runs = e.containerDecodeMany((int)kind, bodies, maxBlock, nMax, cks);
    if (runs.size() != bodies.size()) return 1;
    bytes all;
    for (const auto& r : runs) {
      printf("I %zu %llu %d %lld %zu", r.sizes.size(), (unsigned long long)r.consumed, r.why, (long long)r.code, r.decoded.size());
      for (int32_t s : r.sizes) printf(" %d", s);
      printf("\n");
      all.insert(all.end(), r.decoded.begin(), r.decoded.end());
    }
    if (!dump(argv[2], all.data(), all.size())) return 1;
    return 0;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
