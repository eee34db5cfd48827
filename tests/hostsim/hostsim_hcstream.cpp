// tests/hostsim/hostsim_hcstream.cpp -- TEST INFRASTRUCTURE ONLY.
// The HC stream compressor for sources that land anywhere, on the CPU: the state machine and the linear image of host_staging.h
// (HcsImage) and the two cores of lz4_hc_core.h (hc_stream_build_segment = HcBuild<..., false, SEG = true, RUNS = true>,
// hc_stream_parse_block = HcParse<..., false, DICT = true, PREFIX = true>) compiled against the lock-step host backend, in a library of
// its own (tests/test_hcstream_hostsim.py).  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/host_staging.h"
#include "../../lz4-java_amd/csrc/lz4_hc_core.h"
#include "wave_host.h"

extern "C" {

// One call on ONE stream, as hcstream_host_shard stages it and the two kernels run it: state5 = the stream's record (read, and written
// back), block i = src[src_off[i], + src_len[i]) -> dst[dst_off[i], + dst_cap[i]), out[i] = the result.  The image is a buffer of
// exactly its size: what the call reads of `src` is what the pieces name.  delta[] is built in segments of `seg` positions.  -> 0,
// -1 for a call hcstream_shape_error refuses, -1000 if the simulated wave read outside a block's view (or the build outside the
// stream's buffer) or wrote outside a slot.  info[0] = the image's bytes, info[1] = its run ends, info[2] = its pieces.
int sim_hcstream_call(uint64_t* state5, const uint8_t* src, const uint64_t* src_off, const int32_t* src_len, uint32_t nb, uint8_t* dst,
                      const uint64_t* dst_off, const int32_t* dst_cap, int32_t* out, int level, uint32_t seg, uint64_t rng_seed, uint64_t* info) {
  staging::HcsState st;
  memcpy(&st, state5, sizeof st);
  const uint32_t first[2] = {0u, nb};
  if (staging::hcstream_shape_error(&st, first, 1, nb, src_len)) return -1;
  if (level < 1) level = 9;
  if (level > 12) level = 12;
  const staging::HcsImage im(&st, first, 0, 1, src_off, src_len);
  std::vector<uint8_t> image(im.total ? im.total : 1u, 0xA5);
  for (const staging::HcsPiece& p : im.pieces) memcpy(image.data() + p.dev, src + p.src, p.len);
  const uint64_t len = im.buf_len[0];
  std::vector<uint16_t> delta((size_t)len + 8u, 0xFFFF);
  bool oob = false;
  {
    hostsim::WaveHost w;
    if (rng_seed) w.rng = rng_seed;
    w.bounds(image.data(), (size_t)len, nullptr, 0);
    const uint64_t nseg = len >= 4u ? (len - 3u + seg - 1u) / seg : 0u;
    for (uint64_t k = 0; k < nseg; k++) {
      w.lds.assign(16384, 0);
      lz4hip::hc_stream_build_segment(w, image.data(), len, seg, (uint32_t)(nseg - 1u - k), delta.data(), im.ends.data(), (uint32_t)im.ends.size());
    }
    oob |= w.oob;
  }
  std::vector<int> opt(level >= 10 ? (size_t)lz4hip::HC_OPT_INTS : 1u, 0x55555555);
  for (uint32_t i = 0; i < nb; i++) {
    const int32_t n = src_len[i], cap = dst_cap[i];
    int r = 0;
    if (staging::hcs_runs(n) && cap >= 0) {
      const uint32_t hist = im.blk_hist[i];
      const uint64_t view = im.blk_start[i] - hist;
      hostsim::WaveHost w;
      if (rng_seed) w.rng = rng_seed + i;
      w.bounds(image.data() + view, (size_t)hist + (size_t)n, dst + dst_off[i], (size_t)cap);
      r = lz4hip::hc_stream_parse_block(w, image.data() + view, hist, im.blk_low[i], im.blk_dlim[i], n, delta.data() + view, dst + dst_off[i], cap, level,
                                        opt.data());
      oob |= w.oob;
    }
    out[i] = r;
  }
  memcpy(state5, &im.after[0], sizeof st);
  if (info) { info[0] = im.total; info[1] = im.ends.size(); info[2] = im.pieces.size(); }
  return oob ? -1000 : 0;
}

// the two state edits, as the C ABI's helpers make them
void sim_hcs_load_dict(uint64_t* state5, uint64_t dict_end, uint64_t dict_len) {
  const staging::HcsState v = staging::hcs_load_dict(dict_end, dict_len);
  memcpy(state5, &v, sizeof v);
}
int sim_hcs_save_dict(uint64_t* state5, uint64_t buf_off, int k) {
  staging::HcsState v;
  memcpy(&v, state5, sizeof v);
  const int kept = staging::hcs_save_dict(v, buf_off, k);
  memcpy(state5, &v, sizeof v);
  return kept;
}

}  // extern "C"
