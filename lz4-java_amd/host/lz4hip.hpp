// lz4hip.hpp -- C++ host-side mirror of lz4-java's plugin interface for the "HIP" family, header-only
// over the C ABI (include/lz4hip.h).  The reference's host side is compiled (JVM) code; this image has
// no JDK, so this header is the compiled-language mirror (the Java twins live in ../java):
//
//   net::jpountz::lz4::LZ4Factory::hipInstance()     <- LZ4Factory.java:91-126 (new fourth accessor), :229-291
//   LZ4Compressor::compress / maxCompressedLength   <- LZ4Compressor.java:36,59 ; LZ4JNICompressor.java:35-43
//   LZ4SafeDecompressor::decompress                 <- LZ4SafeDecompressor.java:45 ; LZ4JNISafeDecompressor.java:34-43
//   LZ4SafeDecompressor::decompressPartial          =  LZ4_decompress_safe_partial of liblz4's main API (no reference entry reaches it)
//   LZ4Dictionary, LZ4SafeDecompressor::decompressWithDict, LZ4HIPBatch::decompressSafeDict
//                                                   =  LZ4_decompress_safe_usingDict of liblz4's main API against a dictionary that is not
//                                                      contiguous with the destination (no reference entry reaches it)
//   LZ4HIPBatch::compressFastChain                  =  LZ4_compress_fast_continue over chains of linked blocks (liblz4's prefix mode)
//   CompressStreams                                 =  LZ4_compress_fast_continue on streams that go on from call to call: ONE LZ4_stream_t each,
//                                                      its state resident on the device (LZ4_saveDict through chainPrefixLen)
//   LZ4HIPBatch::compressHCChain                    =  LZ4_compress_HC_continue over chains of linked blocks (prefix mode; not serial)
//   LZ4HIPBatch::compressHCStream, CompressStreamsHC =  LZ4_compress_HC_continue on streams whose sources land anywhere (rings, alternating
//                                                      buffers, save areas with LZ4_saveDictHC, dictionaries elsewhere): ONE LZ4_streamHC_t each
//   LZ4HIPBatch::decompressSafeChain                =  LZ4_decompress_safe_continue over chains of linked blocks (liblz4's rolling-prefix
//                                                      mode; no reference entry reaches it)
//   LZ4HIPBatch::decompressSafeStream, DecodeStreams =  LZ4_decompress_safe_continue on streams whose blocks land anywhere (rings, alternating
//                                                      buffers, save areas, dictionaries elsewhere): every mode of LZ4_streamDecode_t
//   LZ4HIPCompressor::compressWithDict, LZ4HIPBatch::compressDict
//                                                   =  LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream per block: the writer
//                                                      of the records decompressWithDict reads (no reference entry reaches it)
//   LZ4HCHIPCompressor::compressWithDict, LZ4HIPBatch::compressHCDict
//                                                   =  LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream per block, at the
//                                                      compressor's level (no reference entry reaches it)
//   LZ4SafeDecompressor::decompressedLength, LZ4HIPBatch::decompressedLengths / decompressSafeSized
//                                                   =  the decoded size without a destination; the batch twin of the allocating
//                                                      overloads LZ4SafeDecompressor.java:117-137 without their worst-case buffer
//   LZ4FastDecompressor::decompress                 <- LZ4FastDecompressor.java:48 ; LZ4JNIFastDecompressor.java:35-44
//   LZ4Exception                                    <- LZ4Exception.java
//   net::jpountz::xxhash::XXHashFactory::hipInstance().hash32()/hash64()  <- XXHashFactory.java:80,211,220
// Same names, argument meaning (byte array + offset + length) and error behaviour: range violations throw
// std::out_of_range / std::invalid_argument (ArrayIndexOutOfBounds / IllegalArgument, SafeUtils.java:24-42),
// codec failures throw LZ4Exception with the reference's messages.  No CPU path: a missing GPU throws.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/lz4hip.h"

namespace net { namespace jpountz {

using bytes = std::vector<uint8_t>;

namespace util {
inline void checkLength(int len) { if (len < 0) throw std::invalid_argument("lengths must be >= 0"); }
inline void checkRange(const bytes& buf, int off) { if (off < 0 || off >= (int)buf.size()) throw std::out_of_range(std::to_string(off)); }
inline void checkRange(const bytes& buf, int off, int len) {
  checkLength(len);
  if (len > 0) { checkRange(buf, off); checkRange(buf, off + len - 1); }
}
}  // namespace util

namespace lz4 {

struct LZ4Exception : std::runtime_error { using std::runtime_error::runtime_error; };

inline int libCheck(int ret) {
  if (LZ4HIP_IS_LIB_ERROR(ret)) throw LZ4Exception(std::string("liblz4hip: ") + lz4hip_last_error());
  return ret;
}

class LZ4Compressor {
 public:
  virtual ~LZ4Compressor() {}
  int maxCompressedLength(int length) const {  // LZ4Utils.java:34-41
    if (length < 0) throw std::invalid_argument("length must be >= 0, got " + std::to_string(length));
    if (length >= 0x7E000000) throw std::invalid_argument("length must be < 0x7E000000");
    return length + length / 255 + 16;
  }
  virtual int compress(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const = 0;
  int compress(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff) const {
    return compress(src, srcOff, srcLen, dest, destOff, (int)dest.size() - destOff);
  }
  int compress(const bytes& src, bytes& dest) const { return compress(src, 0, (int)src.size(), dest, 0); }
  bytes compress(const bytes& src, int srcOff, int srcLen) const {
    bytes out((size_t)maxCompressedLength(srcLen));
    out.resize((size_t)compress(src, srcOff, srcLen, out, 0, (int)out.size()));
    return out;
  }
  bytes compress(const bytes& src) const { return compress(src, 0, (int)src.size()); }
};

class LZ4Dictionary;
// acceleration != 1: the bytes of liblz4's LZ4_compress_fast(..., acceleration) (lz4hip_compress_fast_accel; < 1 acts as 1, > 65537 as 65537)
class LZ4HIPCompressor final : public LZ4Compressor {
  int accel_;
 public:
  using LZ4Compressor::compress;
  explicit LZ4HIPCompressor(int acceleration = 1) : accel_(acceleration) {}
  int acceleration() const { return accel_; }
  int compress(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const override {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, maxDestLen);
    const int result = libCheck(accel_ == 1 ? lz4hip_compress_fast(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen)
                                            : lz4hip_compress_fast_accel(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen, accel_));
    if (result <= 0) throw LZ4Exception("maxDestLen is too small");
    return result;
  }
  // liblz4's LZ4_compress_destSize: compresses as much of src[srcOff, srcOff + srcLen) as fits in exactly targetDestSize bytes at
  // dest + destOff; returns the bytes written and sets srcLen to the source bytes they cover (lz4hip_compress_dest_size).  liblz4
  // has no accelerated destSize: an accelerated compressor throws std::logic_error.
  int compressDestSize(const bytes& src, int srcOff, int& srcLen, bytes& dest, int destOff, int targetDestSize) const {
    if (accel_ > 1) throw std::logic_error("compressDestSize: liblz4 has no accelerated destSize");
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, targetDestSize);
    int size = srcLen;
    const int result = libCheck(lz4hip_compress_dest_size(src.data() + srcOff, &size, dest.data() + destOff, targetDestSize));
    srcLen = size;
    return result;
  }
  // liblz4's LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream: src[srcOff, srcOff + srcLen) compressed alone against `dict`
  // (which is not contiguous with src) into dest + destOff; returns the compressed size (lz4hip_compress_fast_dict).  There is no
  // accelerated form: an accelerated compressor throws std::logic_error.
  int compressWithDict(const LZ4Dictionary& dict, const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const;
};

class LZ4HCHIPCompressor final : public LZ4Compressor {
  int level_;
 public:
  using LZ4Compressor::compress;
  explicit LZ4HCHIPCompressor(int compressionLevel = 9) : level_(compressionLevel) {}
  int compress(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const override {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, maxDestLen);
    const int result = libCheck(lz4hip_compress_hc(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen, level_));
    if (result <= 0) throw LZ4Exception("");
    return result;
  }
  // liblz4's LZ4_compress_HC_destSize at this compressor's level: compresses as much of src[srcOff, srcOff + srcLen) as fits in
  // exactly targetDestSize bytes at dest + destOff; returns the bytes written and sets srcLen to the source bytes they cover
  // (lz4hip_compress_hc_dest_size)
  int compressDestSize(const bytes& src, int srcOff, int& srcLen, bytes& dest, int destOff, int targetDestSize) const {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, targetDestSize);
    int size = srcLen;
    const int result = libCheck(lz4hip_compress_hc_dest_size(src.data() + srcOff, &size, dest.data() + destOff, targetDestSize, level_));
    srcLen = size;
    return result;
  }
  // liblz4's LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream at this compressor's level: src[srcOff, srcOff + srcLen)
  // compressed alone against `dict` (which is not contiguous with src) into dest + destOff; returns the compressed size
  // (lz4hip_compress_hc_dict)
  int compressWithDict(const LZ4Dictionary& dict, const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const;
};

// A shared dictionary for LZ4_decompress_safe_usingDict, LZ4_loadDict + LZ4_compress_fast_continue and LZ4_loadDictHC +
// LZ4_compress_HC_continue (lz4hip_dict_create): the handle keeps the true length and the last 64 KB, resident on every initialised
// device (and the tables LZ4_loadDict / LZ4_loadDictHC leave, from its first fast / HC compress on a device).  Immutable: any number of threads may compress and decode against it; it must outlive the calls that use it.
class LZ4Dictionary {
  lz4hip_dict* h_ = nullptr;
 public:
  LZ4Dictionary(const uint8_t* data, int length) {
    const int rc = lz4hip_dict_create(data, length, &h_);
    if (rc == LZ4HIP_E_ARG) throw std::invalid_argument(std::string("LZ4Dictionary: ") + lz4hip_last_error());
    if (rc != 0) throw LZ4Exception(std::string("liblz4hip status ") + std::to_string(rc) + ": " + lz4hip_last_error());
  }
  explicit LZ4Dictionary(const bytes& data) : LZ4Dictionary(data.empty() ? reinterpret_cast<const uint8_t*>("") : data.data(), (int)data.size()) {}
  LZ4Dictionary(const LZ4Dictionary&) = delete;
  LZ4Dictionary& operator=(const LZ4Dictionary&) = delete;
  LZ4Dictionary(LZ4Dictionary&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~LZ4Dictionary() { lz4hip_dict_free(h_); }
  int size() const { return lz4hip_dict_size(h_); }
  const lz4hip_dict* handle() const { return h_; }
};

inline int LZ4HIPCompressor::compressWithDict(const LZ4Dictionary& dict, const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff,
                                              int maxDestLen) const {
  if (accel_ > 1) throw std::logic_error("compressWithDict: no accelerated form");
  util::checkRange(src, srcOff, srcLen);
  util::checkRange(dest, destOff, maxDestLen);
  const int result = libCheck(lz4hip_compress_fast_dict(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen, dict.handle()));
  if (result <= 0) throw LZ4Exception("maxDestLen is too small");
  return result;
}

inline int LZ4HCHIPCompressor::compressWithDict(const LZ4Dictionary& dict, const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff,
                                                int maxDestLen) const {
  util::checkRange(src, srcOff, srcLen);
  util::checkRange(dest, destOff, maxDestLen);
  const int result = libCheck(lz4hip_compress_hc_dict(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen, level_, dict.handle()));
  if (result <= 0) throw LZ4Exception("");
  return result;
}

class LZ4SafeDecompressor {
 public:
  int decompress(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, maxDestLen);
    const int result = libCheck(lz4hip_decompress_safe(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen));
    if (result < 0) throw LZ4Exception("Error decoding offset " + std::to_string(srcOff - result) + " of input buffer");
    return result;
  }
  int decompress(const bytes& src, bytes& dest) const { return decompress(src, 0, (int)src.size(), dest, 0, (int)dest.size()); }
  bytes decompress(const bytes& src, int maxDestLen) const {
    bytes out((size_t)maxDestLen);
    out.resize((size_t)decompress(src, 0, (int)src.size(), out, 0, maxDestLen));
    return out;
  }
  // liblz4's LZ4_decompress_safe_usingDict: decodes a block that was compressed against `dict` (which is not contiguous with dest)
  // into dest + destOff and returns the decoded size (lz4hip_decompress_safe_dict)
  int decompressWithDict(const LZ4Dictionary& dict, const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int maxDestLen) const {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, maxDestLen);
    const int result = libCheck(lz4hip_decompress_safe_dict(src.data() + srcOff, srcLen, dest.data() + destOff, maxDestLen, dict.handle()));
    if (result < 0) throw LZ4Exception("Error decoding offset " + std::to_string(srcOff - result) + " of input buffer");
    return result;
  }
  // liblz4's LZ4_decompress_safe_partial: decodes the first min(targetLen, maxDestLen) bytes of the block (fewer where a cut stream
  // ends first) into dest + destOff and returns the count; nothing is written past destOff + min(targetLen, maxDestLen)
  int decompressPartial(const bytes& src, int srcOff, int srcLen, bytes& dest, int destOff, int targetLen, int maxDestLen) const {
    util::checkRange(src, srcOff, srcLen);
    util::checkRange(dest, destOff, maxDestLen);
    const int result = libCheck(lz4hip_decompress_safe_partial(src.data() + srcOff, srcLen, dest.data() + destOff, targetLen, maxDestLen));
    if (result < 0) throw LZ4Exception("Error decoding offset " + std::to_string(srcOff - result) + " of input buffer");
    return result;
  }
  // what decompress(src, srcOff, srcLen, dest, destOff, maxDestLen) would return, without a destination: nothing is decoded into
  // memory (lz4hip_decompressed_size).  A stream that decompress() rejects with that capacity throws the same LZ4Exception
  int decompressedLength(const bytes& src, int srcOff, int srcLen, int maxDestLen) const {
    util::checkRange(src, srcOff, srcLen);
    util::checkLength(maxDestLen);
    const int result = libCheck(lz4hip_decompressed_size(src.data() + srcOff, srcLen, maxDestLen));
    if (result < 0) throw LZ4Exception("Error decoding offset " + std::to_string(srcOff - result) + " of input buffer");
    return result;
  }
};

// Many blocks per call, host memory.  decompressedLengths: what LZ4_decompress_safe would return per block for a capacity of
// maxDestLen[i] -- no destination exists (lz4hip_decompressed_size_batch).  decompressSafeSized: the batch twin of
// LZ4SafeDecompressor::decompress(src, maxDestLen) -> right-sized vector: the sizes are queried, exactly sum(max(size, 0)) bytes are
// allocated with the blocks packed back to back, and every block that decodes is decoded into its slot; lengths[i] < 0 (liblz4's
// code) marks a block that does not decode with capacity maxDestLen[i], its slot is empty.
struct LZ4HIPBatch {
  struct Sized { bytes data; std::vector<uint64_t> offsets; std::vector<int32_t> lengths; };
  static void checkBlocks(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen, const std::vector<int32_t>& maxDestLen) {
    if (srcLen.size() != srcOff.size() || maxDestLen.size() != srcOff.size()) throw std::invalid_argument("per-block arrays differ in length");
    for (size_t i = 0; i < srcOff.size(); i++) {
      if (srcLen[i] < 0 || maxDestLen[i] < 0) throw std::invalid_argument("lengths must be >= 0");
      if (srcOff[i] > src.size() || (uint64_t)srcLen[i] > src.size() - srcOff[i]) throw std::out_of_range("block " + std::to_string(i));
    }
  }
  static void status(int rc) { if (rc != 0) throw LZ4Exception(std::string("liblz4hip status ") + std::to_string(rc) + ": " + lz4hip_last_error()); }
  // The blocks of MANY LZ4 Frames (kind 0) or LZ4Block streams (kind 1) in one call (lz4hip_container_blocks_many): item c is items[c]
  // cut into pieces of blockSize[c] bytes at `level` (0: fast, else lz4-java's HC level); flags[c]: bit 0 block checksums (kind 0), bit
  // 1 the XXH32 (seed 0) of the item is wanted; gapHead[c] / gapTail[c] zero bytes lie in front of and behind its blocks.  Item c is
  // data[offsets[c], offsets[c + 1]); contentHash[c] is 0 where flags[c] has no bit 1.
  struct ManyWritten { bytes data; std::vector<uint64_t> offsets; std::vector<uint32_t> contentHash; };
  static ManyWritten containerBlocksMany(int kind, int level, const std::vector<bytes>& items, const std::vector<uint32_t>& blockSize,
                                         const std::vector<uint8_t>& flags, const std::vector<uint32_t>& gapHead, const std::vector<uint32_t>& gapTail) {
    const size_t n = items.size();
    if (blockSize.size() != n || flags.size() != n || gapHead.size() != n || gapTail.size() != n) throw std::invalid_argument("per-item lists differ in length");
    ManyWritten w;
    w.offsets.assign(n + 1, 0);
    w.contentHash.assign(n, 0);
    if (n == 0) return w;
    std::vector<uint64_t> off(n), len(n), need(n);
    std::vector<uint32_t> nb(n);
    bytes blob;
    for (size_t c = 0; c < n; c++) { off[c] = blob.size(); len[c] = items[c].size(); blob.insert(blob.end(), items[c].begin(), items[c].end()); }
    blob.push_back(0);                            // (empty buffers still hand the library a pointer)
    status(lz4hip_container_blocks_many_bound(kind, len.data(), blockSize.data(), flags.data(), gapHead.data(), gapTail.data(), (uint32_t)n, nb.data(), need.data()));
    uint64_t cap = 0;
    for (size_t c = 0; c < n; c++) cap += need[c];
    w.data.resize((size_t)cap + 1u);
    status(lz4hip_container_blocks_many(kind, level, blob.data(), off.data(), len.data(), blockSize.data(), flags.data(), gapHead.data(), gapTail.data(),
                                        (uint32_t)n, w.data.data(), cap, w.offsets.data(), w.contentHash.data()));
    w.data.resize((size_t)w.offsets[n]);
    return w;
  }
  // LZ4_loadDict + LZ4_compress_fast_continue per block, a fresh stream each, against one dictionary: block i is compressed into
  // dest[destOff[i], + maxDestLen[i]); returns the compressed sizes, 0 where the slot is too small (lz4hip_compress_fast_dict_batch)
  static std::vector<int32_t> compressDict(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen, bytes& dest,
                                           const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen, const LZ4Dictionary& dict) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    if (destOff.size() != srcOff.size()) throw std::invalid_argument("per-block arrays differ in length");
    for (size_t i = 0; i < destOff.size(); i++)
      if (destOff[i] > dest.size() || (uint64_t)maxDestLen[i] > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    std::vector<int32_t> out(srcOff.size(), 0);
    bytes one(1);                                 // (empty buffers still hand the library a pointer)
    status(lz4hip_compress_fast_dict_batch(src.empty() ? one.data() : src.data(), srcOff.data(), srcLen.data(), dest.empty() ? one.data() : dest.data(),
                                           destOff.data(), maxDestLen.data(), out.data(), (uint32_t)srcOff.size(), dict.handle()));
    return out;
  }
  // LZ4_loadDictHC + LZ4_compress_HC_continue per block at HC level `level`, a fresh stream each, against one dictionary: block i is
  // compressed into dest[destOff[i], + maxDestLen[i]); returns the compressed sizes, 0 where liblz4 returns 0
  // (lz4hip_compress_hc_dict_batch)
  static std::vector<int32_t> compressHCDict(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen, bytes& dest,
                                             const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen, const LZ4Dictionary& dict,
                                             int level = 9) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    if (destOff.size() != srcOff.size()) throw std::invalid_argument("per-block arrays differ in length");
    for (size_t i = 0; i < destOff.size(); i++)
      if (destOff[i] > dest.size() || (uint64_t)maxDestLen[i] > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    std::vector<int32_t> out(srcOff.size(), 0);
    bytes one(1);                                 // (empty buffers still hand the library a pointer)
    status(lz4hip_compress_hc_dict_batch(src.empty() ? one.data() : src.data(), srcOff.data(), srcLen.data(), dest.empty() ? one.data() : dest.data(),
                                         destOff.data(), maxDestLen.data(), out.data(), (uint32_t)srcOff.size(), level, dict.handle()));
    return out;
  }
  // LZ4_decompress_safe_usingDict per block against one dictionary: block i decodes into dest[destOff[i], + maxDestLen[i]); returns
  // liblz4's values (lz4hip_decompress_safe_dict_batch)
  static std::vector<int32_t> decompressSafeDict(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen, bytes& dest,
                                                 const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen, const LZ4Dictionary& dict) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    if (destOff.size() != srcOff.size()) throw std::invalid_argument("per-block arrays differ in length");
    for (size_t i = 0; i < destOff.size(); i++)
      if (destOff[i] > dest.size() || (uint64_t)maxDestLen[i] > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    std::vector<int32_t> out(srcOff.size(), 0);
    bytes one(1);                                 // (an empty destination still hands the library a pointer)
    status(lz4hip_decompress_safe_dict_batch(src.data(), srcOff.data(), srcLen.data(), dest.empty() ? one.data() : dest.data(), destOff.data(),
                                             maxDestLen.data(), out.data(), (uint32_t)srcOff.size(), dict.handle()));
    return out;
  }
  // LZ4_decompress_safe_continue over chains of linked blocks (lz4hip_decompress_safe_chain_batch): chain c is the blocks
  // [chainFirst[c], chainFirst[c + 1]), decoded back to back into dest[chainDestOff[c], + chainDestCap[c]) behind chainPrefixLen[c] bytes of
  // history that lie in front of it in dest (an empty vector: no history); maxDestLen[i] is the capacity liblz4 would be given for block
  // i; stored[i] != 0 (an empty vector: no block is) marks a raw block that is copied.  lengths[i] = liblz4's return value,
  // LZ4HIP_CHAIN_STOPPED behind a chain's first negative one; chainLengths[c] = the bytes chain c decoded
  struct Chains { std::vector<int32_t> lengths; std::vector<uint64_t> chainLengths; };
  static Chains decompressSafeChain(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen,
                                    const std::vector<int32_t>& maxDestLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                    const std::vector<uint64_t>& chainDestOff, const std::vector<uint64_t>& chainDestCap,
                                    const std::vector<int32_t>& chainPrefixLen = {}, const std::vector<uint8_t>& stored = {}) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    const size_t n = srcOff.size(), nc = chainDestOff.size();
    if (!stored.empty() && stored.size() != n) throw std::invalid_argument("per-block arrays differ in length");
    if (chainFirst.size() != nc + 1 || chainDestCap.size() != nc || (!chainPrefixLen.empty() && chainPrefixLen.size() != nc))
      throw std::invalid_argument("per-chain arrays differ in length");
    if (chainFirst[0] != 0 || chainFirst[nc] != n) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
    for (size_t c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
      if (chainDestOff[c] > dest.size() || chainDestCap[c] > dest.size() - chainDestOff[c]) throw std::out_of_range("chain " + std::to_string(c));
      if (!chainPrefixLen.empty()) {
        if (chainPrefixLen[c] < 0) throw std::invalid_argument("lengths must be >= 0");
        if ((uint64_t)chainPrefixLen[c] > chainDestOff[c]) throw std::out_of_range("history of chain " + std::to_string(c));
      }
    }
    Chains r;
    r.lengths.assign(n, 0);
    r.chainLengths.assign(nc, 0);
    bytes one(1);                                 // (an empty destination still hands the library a pointer)
    int32_t none = 0;
    uint64_t none64 = 0;
    status(lz4hip_decompress_safe_chain_batch(src.empty() ? one.data() : src.data(), n ? srcOff.data() : &none64, n ? srcLen.data() : &none,
                                              stored.empty() ? nullptr : stored.data(), n ? maxDestLen.data() : &none, chainFirst.data(),
                                              dest.empty() ? one.data() : dest.data(), nc ? chainDestOff.data() : &none64, nc ? chainDestCap.data() : &none64,
                                              chainPrefixLen.empty() ? nullptr : chainPrefixLen.data(), n ? r.lengths.data() : &none,
                                              nc ? r.chainLengths.data() : &none64, (uint32_t)n, (uint32_t)nc));
    return r;
  }
  // LZ4_decompress_safe_continue on streams whose blocks land anywhere (lz4hip_decompress_safe_stream_batch): stream c is the blocks
  // [chainFirst[c], chainFirst[c + 1]) of this call, block i is decoded to dest[destOff[i], + maxDestLen[i]), inside the stream's window
  // dest[chainWinOff[c], + chainWinLen[c]).  state[c] is liblz4's LZ4_streamDecode_t as offsets into dest -- all zero: a fresh stream,
  // LZ4_setStreamDecode(dest + p, n): {p + n, n, 0, 0} -- read and written back.  -> liblz4's return value per block,
  // LZ4HIP_CHAIN_STOPPED behind a stream's first negative one of the call.  The header says when the bytes are liblz4's (the ring rule).
  // inOrder: the twin lz4hip_decompress_safe_stream_inorder_batch -- the same call for streams whose slots overlap the history they can
  // reach (the ring of decoderRingBufferSize(maxBlock) bytes, rings in step with the writer's); the two may alternate on one stream
  static std::vector<int32_t> decompressSafeStream(std::vector<lz4hip_dstream_state>& state, const bytes& src, const std::vector<uint64_t>& srcOff,
                                                   const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                                   const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen,
                                                   const std::vector<uint64_t>& chainWinOff, const std::vector<uint64_t>& chainWinLen,
                                                   bool inOrder = false) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    const size_t n = srcOff.size(), nc = state.size();
    if (destOff.size() != n) throw std::invalid_argument("per-block arrays differ in length");
    if (chainFirst.size() != nc + 1 || chainWinOff.size() != nc || chainWinLen.size() != nc) throw std::invalid_argument("per-stream arrays differ in length");
    if (chainFirst[0] != 0 || chainFirst[nc] != n) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
    for (size_t c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
      if (chainWinOff[c] > dest.size() || chainWinLen[c] > dest.size() - chainWinOff[c]) throw std::out_of_range("window of stream " + std::to_string(c));
      const lz4hip_dstream_state& s = state[c];
      if (s.prefix_len > s.prefix_end || s.ext_len > s.ext_end || (s.prefix_len && s.prefix_end > dest.size()) || (s.ext_len && s.ext_end > dest.size()))
        throw std::out_of_range("history of stream " + std::to_string(c));
    }
    for (size_t i = 0; i < n; i++)
      if (destOff[i] > dest.size() || (uint64_t)maxDestLen[i] > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    std::vector<int32_t> lengths(n, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint64_t none64 = 0;
    lz4hip_dstream_state none_state{0, 0, 0, 0};
    // (one call, through lz4hip_decompress_safe_stream_batch(state, ...) or its in-order twin: the two take the same arguments)
    const auto entry = inOrder ? lz4hip_decompress_safe_stream_inorder_batch : lz4hip_decompress_safe_stream_batch;
    status(entry(nc ? state.data() : &none_state, src.empty() ? one.data() : src.data(), n ? srcOff.data() : &none64, n ? srcLen.data() : &none,
                 chainFirst.data(), dest.empty() ? one.data() : dest.data(), n ? destOff.data() : &none64, n ? maxDestLen.data() : &none,
                 nc ? chainWinOff.data() : &none64, nc ? chainWinLen.data() : &none64, n ? lengths.data() : &none, (uint32_t)n, (uint32_t)nc));
    return lengths;
  }
  // LZ4_decoderRingBufferSize: the smallest ring a stream of blocks of up to maxBlock bytes is decoded into (inOrder); 0: no such ring
  static int decoderRingBufferSize(int maxBlock) { return lz4hip_decoder_ring_buffer_size(maxBlock); }
  // LZ4_compress_fast_continue over chains of linked blocks (lz4hip_compress_fast_chain_batch): chain c is the blocks
  // [chainFirst[c], chainFirst[c + 1]), whose sources lie back to back from src[chainSrcOff[c]] on, behind chainPrefixLen[c] bytes of
  // history that lie in front of it in src (an empty vector: no history; the stream loads it with LZ4_loadDict); block i owns the slot
  // dest[destOff[i], + maxDestLen[i]).  lengths[i] = liblz4's return value (0: it did not fit, which ends the chain),
  // LZ4HIP_CHAIN_STOPPED behind a chain's first 0; chainLengths[c] = the source bytes of chain c's blocks that succeeded.
  // acceleration: LZ4_compress_fast_continue's last argument for every block of the call (lz4hip_compress_fast_chain_accel_batch, which
  // clamps it to 1 .. 65537 as liblz4 does; 1 is lz4hip_compress_fast_chain_batch, called as such)
  static Chains compressFastChain(const bytes& src, const std::vector<uint64_t>& chainSrcOff, const std::vector<int32_t>& srcLen,
                                  const std::vector<uint32_t>& chainFirst, bytes& dest, const std::vector<uint64_t>& destOff,
                                  const std::vector<int32_t>& maxDestLen, const std::vector<int32_t>& chainPrefixLen = {}, int acceleration = 1) {
    checkChains(src, chainSrcOff, srcLen, chainFirst, dest, destOff, maxDestLen, chainPrefixLen);
    const size_t n = srcLen.size(), nc = chainSrcOff.size();
    Chains r;
    r.lengths.assign(n, 0);
    r.chainLengths.assign(nc, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint64_t none64 = 0;
    const uint8_t* sp = src.empty() ? one.data() : src.data();
    const uint64_t* cso = nc ? chainSrcOff.data() : &none64;
    const int32_t* pre = chainPrefixLen.empty() ? nullptr : chainPrefixLen.data();
    uint8_t* dp = dest.empty() ? one.data() : dest.data();
    if (acceleration == 1)
      status(lz4hip_compress_fast_chain_batch(sp, cso, pre, n ? srcLen.data() : &none, chainFirst.data(), dp, n ? destOff.data() : &none64,
                                              n ? maxDestLen.data() : &none, n ? r.lengths.data() : &none, nc ? r.chainLengths.data() : &none64,
                                              (uint32_t)n, (uint32_t)nc));
    else
      status(lz4hip_compress_fast_chain_accel_batch(sp, cso, pre, n ? srcLen.data() : &none, chainFirst.data(), dp, n ? destOff.data() : &none64,
                                                    n ? maxDestLen.data() : &none, n ? r.lengths.data() : &none, nc ? r.chainLengths.data() : &none64,
                                                    (uint32_t)n, (uint32_t)nc, acceleration));
    return r;
  }
  // LZ4_compress_HC_continue over chains of linked blocks, prefix mode (lz4hip_compress_hc_chain_batch): compressFastChain's arrays
  // and an HC level (< 1 -> 9, > 12 -> 12) -> liblz4's return value per block.  A block whose result is 0 -- it did not fit -- does
  // NOT end its chain: its source is history for the blocks behind it, and there is no LZ4HIP_CHAIN_STOPPED here.  Not serial: every
  // block of every chain is parsed at once
  static std::vector<int32_t> compressHCChain(const bytes& src, const std::vector<uint64_t>& chainSrcOff, const std::vector<int32_t>& srcLen,
                                              const std::vector<uint32_t>& chainFirst, bytes& dest, const std::vector<uint64_t>& destOff,
                                              const std::vector<int32_t>& maxDestLen, const std::vector<int32_t>& chainPrefixLen = {}, int level = 9) {
    checkChains(src, chainSrcOff, srcLen, chainFirst, dest, destOff, maxDestLen, chainPrefixLen);
    const size_t n = srcLen.size(), nc = chainSrcOff.size();
    std::vector<int32_t> lengths(n, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint64_t none64 = 0;
    status(lz4hip_compress_hc_chain_batch(src.empty() ? one.data() : src.data(), nc ? chainSrcOff.data() : &none64,
                                          chainPrefixLen.empty() ? nullptr : chainPrefixLen.data(), n ? srcLen.data() : &none, chainFirst.data(),
                                          dest.empty() ? one.data() : dest.data(), n ? destOff.data() : &none64, n ? maxDestLen.data() : &none,
                                          n ? lengths.data() : &none, (uint32_t)n, (uint32_t)nc, level));
    return lengths;
  }
  // LZ4_compress_HC_continue on streams whose sources land anywhere -- a ring that wraps, alternating buffers, a save area, a dictionary
  // elsewhere (lz4hip_compress_hc_stream_batch): stream c is the blocks [chainFirst[c], chainFirst[c + 1]) of this call, block i is
  // src[srcOff[i], + srcLen[i]) and owns the slot dest[destOff[i], + maxDestLen[i]).  state[c] is liblz4's bookkeeping as offsets into src
  // -- all zero: a fresh stream -- read and written back.  -> liblz4's return value per block (0: it did not fit, which does not end the
  // stream).  A call is a snapshot of src; the header states the exceptions to byte equality
  static std::vector<int32_t> compressHCStream(std::vector<lz4hip_hcstream_state>& state, const bytes& src, const std::vector<uint64_t>& srcOff,
                                               const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                               const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen, int level = 9) {
    const size_t n = srcOff.size(), nc = state.size();
    if (srcLen.size() != n || destOff.size() != n || maxDestLen.size() != n) throw std::invalid_argument("per-block arrays differ in length");
    if (chainFirst.size() != nc + 1) throw std::invalid_argument("per-stream arrays differ in length");
    if (chainFirst[0] != 0 || chainFirst[nc] != n) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
    for (size_t c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
      const lz4hip_hcstream_state& s = state[c];
      if (s.prefix_len > s.prefix_end || s.ext_len > s.ext_end || (s.prefix_len && s.prefix_end > src.size()) || (s.ext_len && s.ext_end > src.size()))
        throw std::out_of_range("history of stream " + std::to_string(c));
    }
    for (size_t i = 0; i < n; i++) {
      const uint64_t len = srcLen[i] >= 0 && srcLen[i] <= 0x7E000000 ? (uint64_t)srcLen[i] : 0u;   // (any other length reads nothing: the engine's rule)
      if (srcOff[i] > src.size() || len > src.size() - srcOff[i]) throw std::out_of_range("source " + std::to_string(i));
      const uint64_t cap = maxDestLen[i] > 0 ? (uint64_t)maxDestLen[i] : 0u;
      if (destOff[i] > dest.size() || cap > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    }
    std::vector<int32_t> lengths(n, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint64_t none64 = 0;
    lz4hip_hcstream_state none_state{0, 0, 0, 0, 0};
    status(lz4hip_compress_hc_stream_batch(nc ? state.data() : &none_state, src.empty() ? one.data() : src.data(), n ? srcOff.data() : &none64,
                                           n ? srcLen.data() : &none, chainFirst.data(), dest.empty() ? one.data() : dest.data(),
                                           n ? destOff.data() : &none64, n ? maxDestLen.data() : &none, n ? lengths.data() : &none, (uint32_t)n,
                                           (uint32_t)nc, level));
    return lengths;
  }
  // the argument checks of the two chain compressors
  static void checkChains(const bytes& src, const std::vector<uint64_t>& chainSrcOff, const std::vector<int32_t>& srcLen,
                          const std::vector<uint32_t>& chainFirst, const bytes& dest, const std::vector<uint64_t>& destOff,
                          const std::vector<int32_t>& maxDestLen, const std::vector<int32_t>& chainPrefixLen) {
    const size_t n = srcLen.size(), nc = chainSrcOff.size();
    if (destOff.size() != n || maxDestLen.size() != n) throw std::invalid_argument("per-block arrays differ in length");
    if (chainFirst.size() != nc + 1 || (!chainPrefixLen.empty() && chainPrefixLen.size() != nc))
      throw std::invalid_argument("per-chain arrays differ in length");
    if (chainFirst[0] != 0 || chainFirst[nc] != n) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
    for (size_t c = 0; c < nc; c++) {
      if (chainFirst[c] > chainFirst[c + 1]) throw std::invalid_argument("chainFirst must ascend from 0 to the number of blocks");
      uint64_t total = 0;
      for (uint32_t i = chainFirst[c]; i < chainFirst[c + 1]; i++) {
        if (srcLen[i] < 0) throw std::invalid_argument("lengths must be >= 0");
        total += (uint64_t)srcLen[i];
      }
      if (chainSrcOff[c] > src.size() || total > src.size() - chainSrcOff[c]) throw std::out_of_range("chain " + std::to_string(c));
      if (!chainPrefixLen.empty()) {
        if (chainPrefixLen[c] < 0) throw std::invalid_argument("lengths must be >= 0");
        if ((uint64_t)chainPrefixLen[c] > chainSrcOff[c]) throw std::out_of_range("history of chain " + std::to_string(c));
      }
    }
    for (size_t i = 0; i < n; i++) {
      if (maxDestLen[i] < 0) throw std::invalid_argument("lengths must be >= 0");
      if (destOff[i] > dest.size() || (uint64_t)maxDestLen[i] > dest.size() - destOff[i]) throw std::out_of_range("slot " + std::to_string(i));
    }
  }
  static std::vector<int32_t> decompressedLengths(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen,
                                                  const std::vector<int32_t>& maxDestLen) {
    checkBlocks(src, srcOff, srcLen, maxDestLen);
    std::vector<int32_t> out(srcOff.size(), 0);
    status(lz4hip_decompressed_size_batch(src.data(), srcOff.data(), srcLen.data(), maxDestLen.data(), out.data(), (uint32_t)srcOff.size()));
    return out;
  }
  static Sized decompressSafeSized(const bytes& src, const std::vector<uint64_t>& srcOff, const std::vector<int32_t>& srcLen,
                                   const std::vector<int32_t>& maxDestLen) {
    Sized r;
    r.lengths = decompressedLengths(src, srcOff, srcLen, maxDestLen);
    const size_t n = srcOff.size();
    r.offsets.resize(n);
    uint64_t total = 0;
    std::vector<uint64_t> so, dof;
    std::vector<int32_t> sl, dc;
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; i++) {
      r.offsets[i] = total;
      if (r.lengths[i] < 0) continue;
      so.push_back(srcOff[i]); sl.push_back(srcLen[i]); dof.push_back(total); dc.push_back(r.lengths[i]); idx.push_back(i);
      total += (uint64_t)r.lengths[i];
    }
    r.data.resize((size_t)total);
    if (idx.empty()) return r;
    bytes one(1);                                 // (an all-empty result still hands the library a destination pointer)
    uint8_t* dst = total ? r.data.data() : one.data();
    std::vector<int32_t> got(idx.size(), 0);
    status(lz4hip_decompress_safe_batch(src.data(), so.data(), sl.data(), dst, dof.data(), dc.data(), got.data(), (uint32_t)idx.size()));
    for (size_t k = 0; k < idx.size(); k++) {
      if (got[k] == dc[k]) continue;
      // a stream liblz4 accepts only with room to spare (it breaks the format's end rules): once more, alone, with its maxDestLen
      const size_t i = idx[k];
      bytes scratch((size_t)maxDestLen[i] + 1);
      const int r2 = libCheck(lz4hip_decompress_safe(src.data() + srcOff[i], srcLen[i], scratch.data(), maxDestLen[i]));
      if (r2 != r.lengths[i]) throw LZ4Exception("block " + std::to_string(i) + ": the decoder disagrees with the size query");
      std::copy(scratch.begin(), scratch.begin() + r2, r.data.begin() + (size_t)r.offsets[i]);
    }
    return r;
  }
};

// A set of n compress streams whose state -- the hash table and index position an LZ4_stream_t carries beside its history -- is resident
// on the device between calls (lz4hip_cstreams_create; about 32 KB of device memory per stream).  compress(): the arrays of
// LZ4HIPBatch::compressFastChain, and chain c is the next run of blocks of stream streamId[c] (strictly ascending).  Every stream gives,
// over all the calls that name it, the bytes ONE LZ4_stream_t of liblz4 gives, however its blocks are cut into calls; for a stream
// that has run, chainPrefixLen[c] is how many of the last bytes it consumed lie in front of the source (LZ4_saveDict's size; 0 is
// legal and no reset).  A block whose result is 0 stops its stream until reset().  Calls on one set are serialised; the set is
// destroyed before lz4hip_shutdown().  acceleration (compress and compressAt): LZ4_compress_fast_continue's last argument for every block
// of THAT call (the *_accel_batch entry points, which clamp it to 1 .. 65537; 1 is the call without it); a stream may get another in every call.
class CompressStreams {
 public:
  explicit CompressStreams(uint32_t n) { LZ4HIPBatch::status(lz4hip_cstreams_create(n, &h_)); }
  ~CompressStreams() { lz4hip_cstreams_free(h_); }
  CompressStreams(const CompressStreams&) = delete;
  CompressStreams& operator=(const CompressStreams&) = delete;
  uint32_t size() const { return (uint32_t)lz4hip_cstreams_count(h_); }
  LZ4HIPBatch::Chains compress(const std::vector<uint32_t>& streamId, const bytes& src, const std::vector<uint64_t>& chainSrcOff,
                               const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                               const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen,
                               const std::vector<int32_t>& chainPrefixLen = {}, int acceleration = 1) {
    LZ4HIPBatch::checkChains(src, chainSrcOff, srcLen, chainFirst, dest, destOff, maxDestLen, chainPrefixLen);
    const size_t n = srcLen.size(), nc = chainSrcOff.size();
    if (streamId.size() != nc) throw std::invalid_argument("per-chain arrays differ in length");
    for (size_t c = 0; c < nc; c++)
      if (streamId[c] >= size() || (c && streamId[c] <= streamId[c - 1]))
        throw std::invalid_argument("streamId must be strictly ascending and below the number of streams");
    LZ4HIPBatch::Chains r;
    r.lengths.assign(n, 0);
    r.chainLengths.assign(nc, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint32_t none32 = 0;
    uint64_t none64 = 0;
    const uint32_t* ids = nc ? streamId.data() : &none32;
    const uint8_t* sp = src.empty() ? one.data() : src.data();
    const uint64_t* cso = nc ? chainSrcOff.data() : &none64;
    const int32_t* pre = chainPrefixLen.empty() ? nullptr : chainPrefixLen.data();
    uint8_t* dp = dest.empty() ? one.data() : dest.data();
    if (acceleration == 1)
      LZ4HIPBatch::status(lz4hip_compress_fast_stream_batch(h_, ids, sp, cso, pre, n ? srcLen.data() : &none, chainFirst.data(), dp,
                                                            n ? destOff.data() : &none64, n ? maxDestLen.data() : &none, n ? r.lengths.data() : &none,
                                                            nc ? r.chainLengths.data() : &none64, (uint32_t)n, (uint32_t)nc));
    else
      LZ4HIPBatch::status(lz4hip_compress_fast_stream_accel_batch(h_, ids, sp, cso, pre, n ? srcLen.data() : &none, chainFirst.data(), dp,
                                                                  n ? destOff.data() : &none64, n ? maxDestLen.data() : &none, n ? r.lengths.data() : &none,
                                                                  nc ? r.chainLengths.data() : &none64, (uint32_t)n, (uint32_t)nc, acceleration));
    return r;
  }
  // The same streams when their sources land anywhere -- a ring that wraps, alternating buffers, a dictionary elsewhere
  // (lz4hip_compress_fast_stream_ext_batch): every block has its own srcOff[i] inside its stream's window [chainWinOff[c],
  // + chainWinLen[c]); the stream's history ends at chainHistEnd[c] in src, with chainHistLen[c] bytes of it present.  A block that
  // does not follow its history runs in liblz4's external-dictionary mode.  A call is a snapshot of src.
  LZ4HIPBatch::Chains compressAt(const std::vector<uint32_t>& streamId, const bytes& src, const std::vector<uint64_t>& srcOff,
                                 const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst,
                                 const std::vector<uint64_t>& chainHistEnd, const std::vector<int32_t>& chainHistLen,
                                 const std::vector<uint64_t>& chainWinOff, const std::vector<uint64_t>& chainWinLen, bytes& dest,
                                 const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen, int acceleration = 1) {
    const size_t n = srcLen.size(), nc = streamId.size();
    if (srcOff.size() != n || destOff.size() != n || maxDestLen.size() != n) throw std::invalid_argument("per-block arrays differ in length");
    if (chainHistEnd.size() != nc || chainHistLen.size() != nc || chainWinOff.size() != nc || chainWinLen.size() != nc || chainFirst.size() != nc + 1)
      throw std::invalid_argument("per-chain arrays differ in length");
    for (size_t c = 0; c < nc; c++)
      if (streamId[c] >= size() || (c && streamId[c] <= streamId[c - 1]))
        throw std::invalid_argument("streamId must be strictly ascending and below the number of streams");
    LZ4HIPBatch::Chains r;
    r.lengths.assign(n, 0);
    r.chainLengths.assign(nc, 0);
    bytes one(1);                                 // (an empty buffer still hands the library a pointer)
    int32_t none = 0;
    uint32_t none32 = 0;
    uint64_t none64 = 0;
    const uint32_t* ids = nc ? streamId.data() : &none32;
    const uint8_t* sp = src.empty() ? one.data() : src.data();
    const uint64_t* he = nc ? chainHistEnd.data() : &none64;
    const int32_t* hl = nc ? chainHistLen.data() : &none;
    const uint64_t* wo = nc ? chainWinOff.data() : &none64;
    const uint64_t* wl = nc ? chainWinLen.data() : &none64;
    uint8_t* dp = dest.empty() ? one.data() : dest.data();
    if (acceleration == 1)
      LZ4HIPBatch::status(lz4hip_compress_fast_stream_ext_batch(h_, ids, sp, n ? srcOff.data() : &none64, n ? srcLen.data() : &none, chainFirst.data(), he, hl,
                                                                wo, wl, dp, n ? destOff.data() : &none64, n ? maxDestLen.data() : &none,
                                                                n ? r.lengths.data() : &none, nc ? r.chainLengths.data() : &none64, (uint32_t)n, (uint32_t)nc));
    else
      LZ4HIPBatch::status(lz4hip_compress_fast_stream_ext_accel_batch(h_, ids, sp, n ? srcOff.data() : &none64, n ? srcLen.data() : &none, chainFirst.data(),
                                                                      he, hl, wo, wl, dp, n ? destOff.data() : &none64, n ? maxDestLen.data() : &none,
                                                                      n ? r.lengths.data() : &none, nc ? r.chainLengths.data() : &none64, (uint32_t)n,
                                                                      (uint32_t)nc, acceleration));
    return r;
  }
  void reset() { LZ4HIPBatch::status(lz4hip_cstreams_reset(h_, nullptr, 0)); }
  void reset(const std::vector<uint32_t>& streamId) {
    if (!streamId.empty()) LZ4HIPBatch::status(lz4hip_cstreams_reset(h_, streamId.data(), (uint32_t)streamId.size()));
  }
  struct State { std::vector<uint64_t> consumed; std::vector<uint8_t> stopped; };
  State consumed(uint32_t first, uint32_t n) {
    State s;
    s.consumed.assign(n, 0);
    s.stopped.assign(n, 0);
    if (n) LZ4HIPBatch::status(lz4hip_cstreams_consumed(h_, first, n, s.consumed.data(), s.stopped.data()));
    return s;
  }

 private:
  lz4hip_cstreams* h_ = nullptr;
};

// The states of n decode streams: per stream what an LZ4_streamDecode_t of liblz4 holds, as offsets into the one destination its caller
// decodes into.  Plain host data: nothing on a device, nothing to destroy.  decompress(): the arrays of LZ4HIPBatch::decompressSafeStream,
// and chain c of the call is the next run of blocks of stream streamId[c] (distinct ids).  Every stream gives, over all the calls that
// name it, the values ONE LZ4_streamDecode_t gives, however its blocks are cut into calls.  inOrder: the set's calls go to the in-order
// twin (LZ4HIPBatch::decompressSafeStream(.., inOrder)); a call may say otherwise, and the two may alternate on a stream.
class DecodeStreams {
 public:
  explicit DecodeStreams(uint32_t n, bool inOrder = false) : state_(n, lz4hip_dstream_state{0, 0, 0, 0}), inOrder_(inOrder) {
    if (!n) throw std::invalid_argument("a set has at least one stream");
  }
  uint32_t size() const { return (uint32_t)state_.size(); }
  // LZ4_setStreamDecode: the stream starts behind the prefixLen bytes of dictionary that end at dest[prefixEnd]
  void set(uint32_t streamId, uint64_t prefixEnd, uint64_t prefixLen) {
    if (prefixLen > prefixEnd) throw std::out_of_range("history of stream " + std::to_string(streamId));
    state_.at(streamId) = lz4hip_dstream_state{prefixEnd, prefixLen, 0, 0};
  }
  void reset() { for (lz4hip_dstream_state& s : state_) s = lz4hip_dstream_state{0, 0, 0, 0}; }
  void reset(const std::vector<uint32_t>& streamId) { for (uint32_t c : streamId) state_.at(c) = lz4hip_dstream_state{0, 0, 0, 0}; }
  const lz4hip_dstream_state& state(uint32_t streamId) const { return state_.at(streamId); }
  std::vector<int32_t> decompress(const std::vector<uint32_t>& streamId, const bytes& src, const std::vector<uint64_t>& srcOff,
                                  const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                  const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen,
                                  const std::vector<uint64_t>& chainWinOff, const std::vector<uint64_t>& chainWinLen) {
    return decompress(streamId, src, srcOff, srcLen, chainFirst, dest, destOff, maxDestLen, chainWinOff, chainWinLen, inOrder_);
  }
  std::vector<int32_t> decompress(const std::vector<uint32_t>& streamId, const bytes& src, const std::vector<uint64_t>& srcOff,
                                  const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                  const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen,
                                  const std::vector<uint64_t>& chainWinOff, const std::vector<uint64_t>& chainWinLen, bool inOrder) {
    std::vector<lz4hip_dstream_state> st;
    std::vector<uint8_t> seen(state_.size(), 0);
    for (uint32_t c : streamId) {
      if (c >= state_.size() || seen[c]) throw std::invalid_argument("streamId must be distinct and below the number of streams");
      seen[c] = 1;
      st.push_back(state_[c]);
    }
    std::vector<int32_t> r = LZ4HIPBatch::decompressSafeStream(st, src, srcOff, srcLen, chainFirst, dest, destOff, maxDestLen, chainWinOff, chainWinLen, inOrder);
    for (size_t k = 0; k < streamId.size(); k++) state_[streamId[k]] = st[k];
    return r;
  }

 private:
  std::vector<lz4hip_dstream_state> state_;
  bool inOrder_;
};

// The states of n HC compress streams whose sources land anywhere: per stream what an LZ4_streamHC_t of liblz4 keeps beside its tables,
// as offsets into the one source its caller compresses from.  Plain host data: nothing on a device, nothing to destroy.  compress(): the
// arrays of LZ4HIPBatch::compressHCStream at the set's level, and chain c of the call is the next run of blocks of stream streamId[c]
// (distinct ids).  Every stream gives, over all the calls that name it, the values ONE LZ4_streamHC_t gives, however its blocks are cut
// into calls (include/lz4hip.h states the exceptions).
class CompressStreamsHC {
 public:
  explicit CompressStreamsHC(uint32_t n, int level = 9) : level_(level), state_(n, lz4hip_hcstream_state{0, 0, 0, 0, 0}) {
    if (!n) throw std::invalid_argument("a set has at least one stream");
  }
  uint32_t size() const { return (uint32_t)state_.size(); }
  int level() const { return level_; }
  // LZ4_loadDictHC: the stream is fresh behind the dictLen bytes of dictionary that end at src[dictEnd]
  void loadDict(uint32_t streamId, uint64_t dictEnd, uint64_t dictLen) {
    if (dictLen > dictEnd) throw std::out_of_range("history of stream " + std::to_string(streamId));
    LZ4HIPBatch::status(lz4hip_hcstream_load_dict(&state_.at(streamId), dictEnd, dictLen));
  }
  // LZ4_saveDictHC for the caller who has copied the last k bytes the stream consumed to src[bufOff ..] -> the bytes kept
  int saveDict(uint32_t streamId, uint64_t bufOff, int k) {
    const int kept = lz4hip_hcstream_save_dict(&state_.at(streamId), bufOff, k);
    if (kept < 0) LZ4HIPBatch::status(kept);
    return kept;
  }
  void reset() { for (lz4hip_hcstream_state& s : state_) s = lz4hip_hcstream_state{0, 0, 0, 0, 0}; }
  void reset(const std::vector<uint32_t>& streamId) { for (uint32_t c : streamId) state_.at(c) = lz4hip_hcstream_state{0, 0, 0, 0, 0}; }
  const lz4hip_hcstream_state& state(uint32_t streamId) const { return state_.at(streamId); }
  std::vector<int32_t> compress(const std::vector<uint32_t>& streamId, const bytes& src, const std::vector<uint64_t>& srcOff,
                                const std::vector<int32_t>& srcLen, const std::vector<uint32_t>& chainFirst, bytes& dest,
                                const std::vector<uint64_t>& destOff, const std::vector<int32_t>& maxDestLen) {
    std::vector<lz4hip_hcstream_state> st;
    std::vector<uint8_t> seen(state_.size(), 0);
    for (uint32_t c : streamId) {
      if (c >= state_.size() || seen[c]) throw std::invalid_argument("streamId must be distinct and below the number of streams");
      seen[c] = 1;
      st.push_back(state_[c]);
    }
    std::vector<int32_t> r = LZ4HIPBatch::compressHCStream(st, src, srcOff, srcLen, chainFirst, dest, destOff, maxDestLen, level_);
    for (size_t k = 0; k < streamId.size(); k++) state_[streamId[k]] = st[k];
    return r;
  }

 private:
  int level_;
  std::vector<lz4hip_hcstream_state> state_;
};

class LZ4FastDecompressor {
 public:
  int decompress(const bytes& src, int srcOff, bytes& dest, int destOff, int destLen) const {
    if (!src.empty() || srcOff) util::checkRange(src, srcOff);
    util::checkRange(dest, destOff, destLen);
    const int result = libCheck(lz4hip_decompress_fast(src.data() + srcOff, (int)src.size() - srcOff, dest.data() + destOff, destLen));
    if (result < 0) throw LZ4Exception("Error decoding offset " + std::to_string(srcOff - result) + " of input buffer");
    return result;
  }
  bytes decompress(const bytes& src, int destLen) const {
    bytes out((size_t)destLen);
    decompress(src, 0, out, 0, destLen);
    return out;
  }
};

class LZ4Factory {
  LZ4HIPCompressor fast_;
  LZ4HCHIPCompressor high_;
  LZ4FastDecompressor fastDec_;
  LZ4SafeDecompressor safeDec_;
  LZ4Factory() {
    // LZ4Factory.java:204-220: round-trip a 20-byte vector through the members before handing them out
    const bytes original = {'a','b','c','d',' ',' ',' ',' ',' ',' ','a','b','c','d','e','f','g','h','i','j'};
    const LZ4Compressor* both[2] = {&fast_, &high_};
    for (const LZ4Compressor* c : both) {
      const bytes compressed = c->compress(original);
      if (fastDec_.decompress(compressed, (int)original.size()) != original) throw std::logic_error("AssertionError");
      if (safeDec_.decompress(compressed, (int)original.size()) != original) throw std::logic_error("AssertionError");
    }
  }
 public:
  static LZ4Factory& hipInstance() { static LZ4Factory f; return f; }
  const LZ4Compressor& fastCompressor() const { return fast_; }
  // a fast compressor bound to LZ4_compress_fast's acceleration (1 = the bytes of fastCompressor())
  std::unique_ptr<LZ4Compressor> fastCompressor(int acceleration) const {
    return std::unique_ptr<LZ4Compressor>(new LZ4HIPCompressor(acceleration));
  }
  std::unique_ptr<LZ4Compressor> highCompressor(int compressionLevel = 9) const {  // clamp: LZ4Factory.java:263-270
    if (compressionLevel > 17) compressionLevel = 17; else if (compressionLevel < 1) compressionLevel = 9;
    return std::unique_ptr<LZ4Compressor>(new LZ4HCHIPCompressor(compressionLevel));
  }
  const LZ4FastDecompressor& fastDecompressor() const { return fastDec_; }
  const LZ4SafeDecompressor& safeDecompressor() const { return safeDec_; }
  std::string toString() const { return "LZ4Factory:HIP"; }
};

}  // namespace lz4

namespace xxhash {
struct XXHash32 {
  int32_t hash(const bytes& buf, int off, int len, int32_t seed) const {
    util::checkRange(buf, off, len);
    uint32_t h = 0;
    if (lz4hip_xxh32(buf.data() + off, len, (uint32_t)seed, &h) != 0) throw std::runtime_error(std::string("liblz4hip: ") + lz4hip_last_error());
    return (int32_t)h;
  }
};
struct XXHash64 {
  int64_t hash(const bytes& buf, int off, int len, int64_t seed) const {
    util::checkRange(buf, off, len);
    uint64_t h = 0;
    if (lz4hip_xxh64(buf.data() + off, len, (uint64_t)seed, &h) != 0) throw std::runtime_error(std::string("liblz4hip: ") + lz4hip_last_error());
    return (int64_t)h;
  }
};
// StreamingXXHash32.java:38-129 / StreamingXXHash64.java (JNI twins StreamingXXHash32JNI.java:28-104): the state is a device
// record behind a lz4hip_xxh_stream handle; update() continues it with one launch.
namespace detail {
inline void xchk(int rc) { if (rc != 0) throw std::runtime_error(std::string("liblz4hip: ") + lz4hip_last_error()); }
class StreamingBase {
 public:
  StreamingBase(const StreamingBase&) = delete;
  StreamingBase& operator=(const StreamingBase&) = delete;
  ~StreamingBase() { close(); }
  void update(const bytes& buf, int off, int len) {
    checkState();
    util::checkRange(buf, off, len);
    xchk(lz4hip_xxh_stream_update(st_, buf.data() + off, len));
  }
  void update(const uint8_t* p, size_t n) {  // raw overload for the stream classes (pieces of <= 1 GiB)
    checkState();
    while (n) { const size_t part = n < (1u << 30) ? n : (1u << 30); xchk(lz4hip_xxh_stream_update(st_, p, (int)part)); p += part; n -= part; }
  }
  void close() { if (st_) { lz4hip_xxh_stream_free(st_); st_ = nullptr; } }
 protected:
  StreamingBase() = default;
  void checkState() const { if (!st_) throw std::logic_error("Already finalized"); }  // StreamingXXHash32JNI.java:47-51
  lz4hip_xxh_stream* st_ = nullptr;
};
}  // namespace detail
class StreamingXXHash32 final : public detail::StreamingBase {
 public:
  explicit StreamingXXHash32(int32_t seed) : seed_(seed) { detail::xchk(lz4hip_xxh32_stream_create((uint32_t)seed, &st_)); }
  int32_t getValue() { checkState(); uint32_t h = 0; detail::xchk(lz4hip_xxh32_stream_digest(st_, &h)); return (int32_t)h; }
  void reset() { checkState(); detail::xchk(lz4hip_xxh_stream_reset(st_, (uint32_t)seed_)); }
  int64_t checksumValue() { return (int64_t)((uint32_t)getValue() & 0xFFFFFFFu); }  // asChecksum().getValue(): 28 bits (:101-107)
 private:
  int32_t seed_;
};
class StreamingXXHash64 final : public detail::StreamingBase {
 public:
  explicit StreamingXXHash64(int64_t seed) : seed_(seed) { detail::xchk(lz4hip_xxh64_stream_create((uint64_t)seed, &st_)); }
  int64_t getValue() { checkState(); uint64_t h = 0; detail::xchk(lz4hip_xxh64_stream_digest(st_, &h)); return (int64_t)h; }
  void reset() { checkState(); detail::xchk(lz4hip_xxh_stream_reset(st_, (uint64_t)seed_)); }
 private:
  int64_t seed_;
};
struct XXHashFactory {
  static XXHashFactory& hipInstance() { static XXHashFactory f; return f; }
  XXHash32 hash32() const { return XXHash32(); }
  XXHash64 hash64() const { return XXHash64(); }
  std::unique_ptr<StreamingXXHash32> newStreamingHash32(int32_t seed) const { return std::unique_ptr<StreamingXXHash32>(new StreamingXXHash32(seed)); }  // XXHashFactory.java:230
  std::unique_ptr<StreamingXXHash64> newStreamingHash64(int64_t seed) const { return std::unique_ptr<StreamingXXHash64>(new StreamingXXHash64(seed)); }  // :240
};
}  // namespace xxhash

}}  // namespace net::jpountz
