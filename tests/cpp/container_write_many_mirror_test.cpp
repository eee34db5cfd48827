// tests/cpp/container_write_many_mirror_test.cpp -- exercises BatchEngine::containerBlocksMany, writeFrames and writeBlockStreams of the C++
// host mirror (lz4-java_amd/host/lz4hip_streams.hpp).  Built and run by tests/test_container_write_many_mirrors.py and
// tests/test_gpu_container_write_many.py:
//   container_write_many_mirror_test --args
//     the argument errors (they need no device), then one well-formed call: prints "checks ok" and "call ok" or "call failed: <message>"
//   container_write_many_mirror_test --streams <kind> <blockSize> <flg bits> <items> <out>
//     writeFrames (kind 0; blockSize 4..7; flg bits: 0x10 block checksums, 0x08 content size, 0x04 content checksum) / writeBlockStreams
//     (kind 1) over <items>: u32 count, then per item {u64 len, bytes}; every container is compared here with the per-payload writer's;
//     prints per item "R <bytes>" and writes the containers, item after item, to <out>
//   container_write_many_mirror_test <cases> <out>
//     <cases>: u32 kind, u32 level, u32 count, then per item {u32 block_size, u32 flags, u32 gap_head, u32 gap_tail, u64 len, bytes}
//     prints per item "I <item bytes> <content hash>", writes the items' bytes (gaps included), item after item, to <out>
// Exit code 0 = all good; a library failure (no GPU, for one) is loud: exit code 3.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include "../../lz4-java_amd/host/lz4hip_streams.hpp"
#include "mirror_io.h"

using namespace net::jpountz;

static bool says(const std::function<void()>& f, const char* what) {
  try { f(); } catch (const lz4::LZ4Exception& e) { return strstr(e.what(), what) != nullptr; }
  return false;
}

static int args() {
  lz4::BatchEngine e;
  const std::vector<bytes> two = {bytes(3000, 'x'), bytes(70, 'y')};
  bool threw = false;
  try { (void)e.containerBlocksMany(0, two, {1000}, {1, 0}, {0, 0}, {0, 0}); } catch (const std::invalid_argument&) { threw = true; }
  if (!threw) return 1;
  const lz4::LZ4HIPBatch::ManyWritten none = e.containerBlocksMany(1, {}, {}, {}, {}, {});
  if (!none.data.empty() || none.offsets != std::vector<uint64_t>{0} || !none.contentHash.empty()) return 1;
  if (!lz4::writeFrames({}).empty() || !lz4::writeBlockStreams({}).empty()) return 1;
  if (!says([&] { (void)e.containerBlocksMany(2, two, {1000, 64}, {1, 0}, {0, 0}, {0, 0}); }, "kind")) return 1;
  if (!says([&] { (void)e.containerBlocksMany(0, two, {1000, 63}, {1, 0}, {0, 0}, {0, 0}); }, "block size must be 64 .. 32 MiB")) return 1;
  if (!says([&] { (void)e.containerBlocksMany(0, two, {1000, 64}, {1, 4}, {0, 0}, {0, 0}); }, "bit 1 (content hash) are defined")) return 1;
  if (!says([&] { (void)e.containerBlocksMany(1, two, {1000, 64}, {1, 0}, {0, 0}, {0, 0}); }, "belongs to kind 0")) return 1;
  printf("checks ok\n");
  try {
    const lz4::LZ4HIPBatch::ManyWritten w = e.containerBlocksMany(0, two, {1000, 64}, {3, 0}, {7, 0}, {19, 0});
    if (w.offsets.size() != 3 || w.offsets[2] != w.data.size() || w.contentHash[0] == 0 || w.contentHash[1] != 0) return 1;
    printf("call ok\n");
  } catch (const lz4::LZ4Exception& x) { printf("call failed: %s\n", x.what()); }
  return 0;
}

static bool items_of(const char* path, std::vector<bytes>& items) {
  bytes in;
  if (!slurp(path, in) || in.size() < 4) return false;
  uint32_t count;
  memcpy(&count, in.data(), 4);
  size_t p = 4;
  for (uint32_t i = 0; i < count; i++) {
    uint64_t len;
    if (p + 8 > in.size()) return false;
    memcpy(&len, in.data() + p, 8); p += 8;
    if (p + len > in.size()) return false;
    items.emplace_back(in.begin() + (ptrdiff_t)p, in.begin() + (ptrdiff_t)(p + len));
    p += len;
  }
  return true;
}

static std::vector<bytes> frames(const std::vector<bytes>& items, int bs, int flg) {
  const lz4::frame::BLOCKSIZE b = (lz4::frame::BLOCKSIZE)bs;
  using namespace lz4::frame;
  switch (flg) {
    case 0x00: return lz4::writeFrames(items, lz4::BatchEngine(), b);
    case 0x04: return lz4::writeFrames(items, lz4::BatchEngine(), b, {BLOCK_INDEPENDENCE, CONTENT_CHECKSUM});
    case 0x10: return lz4::writeFrames(items, lz4::BatchEngine(), b, {BLOCK_INDEPENDENCE, BLOCK_CHECKSUM});
    case 0x1C: return lz4::writeFrames(items, lz4::BatchEngine(), b, {BLOCK_INDEPENDENCE, BLOCK_CHECKSUM, CONTENT_SIZE, CONTENT_CHECKSUM});
  }
  throw std::invalid_argument("flg bits");
}
static bytes frame_alone(const bytes& p, int bs, int flg) {
  const lz4::frame::BLOCKSIZE b = (lz4::frame::BLOCKSIZE)bs;
  using namespace lz4::frame;
  std::ostringstream sink;
  const int64_t known = (flg & 0x08) ? (int64_t)p.size() : -1;
  std::unique_ptr<lz4::LZ4FrameOutputStream> w;
  switch (flg) {
    case 0x00: w.reset(new lz4::LZ4FrameOutputStream(sink, b, known)); break;
    case 0x04: w.reset(new lz4::LZ4FrameOutputStream(sink, b, known, {BLOCK_INDEPENDENCE, CONTENT_CHECKSUM})); break;
    case 0x10: w.reset(new lz4::LZ4FrameOutputStream(sink, b, known, {BLOCK_INDEPENDENCE, BLOCK_CHECKSUM})); break;
    default: w.reset(new lz4::LZ4FrameOutputStream(sink, b, known, {BLOCK_INDEPENDENCE, BLOCK_CHECKSUM, CONTENT_SIZE, CONTENT_CHECKSUM})); break;
  }
  w->write(p);
  w->close();
  const std::string s = sink.str();
  return bytes(s.begin(), s.end());
}

static int streams(int kind, int bs, int flg, const char* path, const char* outPath) {
  std::vector<bytes> items;
  if (!items_of(path, items)) return 2;
  const std::vector<bytes> got = kind == 0 ? frames(items, bs, flg) : lz4::writeBlockStreams(items, lz4::BatchEngine(), bs);
  if (got.size() != items.size()) return 1;
  lz4::BatchEngine host;
  host.hostAssembly = true;
  const std::vector<bytes> slow = kind == 0 ? std::vector<bytes>() : lz4::writeBlockStreams(items, host, bs);   // (the fall-back: writer by writer)
  bytes all;
  for (size_t i = 0; i < items.size(); i++) {
    bytes want;
    if (kind == 0) want = frame_alone(items[i], bs, flg);
    else {
      std::ostringstream sink;
      { lz4::LZ4BlockOutputStream w(sink, bs); w.write(items[i]); w.close(); }
      const std::string s = sink.str();
      want.assign(s.begin(), s.end());
      if (slow[i] != want) { fprintf(stderr, "item %zu: the fall-back differs from the writer\n", i); return 1; }
    }
    if (got[i] != want) { fprintf(stderr, "item %zu: %zu bytes; the per-payload writer: %zu bytes\n", i, got[i].size(), want.size()); return 1; }
    printf("R %zu\n", got[i].size());
    all.insert(all.end(), got[i].begin(), got[i].end());
  }
  return dump(outPath, all.data(), all.size()) ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && std::string(argv[1]) == "--args") return args();
    if (argc >= 7 && std::string(argv[1]) == "--streams") return streams(atoi(argv[2]), atoi(argv[3]), (int)strtol(argv[4], nullptr, 0), argv[5], argv[6]);
    if (argc < 3) { fprintf(stderr, "usage: container_write_many_mirror_test <cases> <out>\n"); return 2; }
    bytes in;
    if (!slurp(argv[1], in) || in.size() < 12) return 2;
    uint32_t head[3];
    memcpy(head, in.data(), 12);
    size_t p = 12;
    std::vector<bytes> items;
    std::vector<uint32_t> bs, gh, gt;
    std::vector<uint8_t> fl;
    for (uint32_t i = 0; i < head[2]; i++) {
      uint32_t h[4];
      uint64_t len;
      if (p + 24 > in.size()) return 2;
      memcpy(h, in.data() + p, 16); memcpy(&len, in.data() + p + 16, 8); p += 24;
      if (p + len > in.size()) return 2;
      bs.push_back(h[0]); fl.push_back((uint8_t)h[1]); gh.push_back(h[2]); gt.push_back(h[3]);
      items.emplace_back(in.begin() + (ptrdiff_t)p, in.begin() + (ptrdiff_t)(p + len));
      p += len;
    }
    lz4::BatchEngine e;
    e.hcLevel = (int)head[1];
    const lz4::LZ4HIPBatch::ManyWritten w = e.containerBlocksMany((int)head[0], items, bs, fl, gh, gt);
    if (w.offsets.size() != items.size() + 1 || w.offsets.back() != w.data.size()) return 1;
    for (size_t c = 0; c < items.size(); c++) printf("I %llu %u\n", (unsigned long long)(w.offsets[c + 1] - w.offsets[c]), w.contentHash[c]);
    return dump(argv[2], w.data.data(), w.data.size()) ? 0 : 1;
  } catch (const lz4::LZ4Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}
