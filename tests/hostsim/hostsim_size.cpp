// tests/hostsim/hostsim_size.cpp -- TEST INFRASTRUCTURE ONLY.
// The decoded-size query of lz4-java_amd/csrc/lz4_decode_size.h compiled against the lock-step host backend, in a library of its own
// (tests/test_size_hostsim.py), in its two forms: the exact path alone, and the fast interior in front of it.  The backend is the
// wave backend of group_host.h with copies that do nothing -- what group_dev.h's SizeWaveDev is on the device -- and NO destination:
// any access outside [src, src + src_size) counts as out of bounds.  Nothing here is linked into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_decode_core.h"
#include "group_host.h"

namespace {

struct SizeHost : hostsim::GroupHost {
  uint32_t sz_lo = 1u, sz_avail = 0u;   // the stream ring holds [sz_lo, sz_avail): nothing yet
  uint64_t copies = 0;
  static constexpr bool kExactLengthSum = true;   // (as SizeWaveDev)
  SizeHost(const uint8_t* s, long n, uint32_t ks) : hostsim::GroupHost(64, s, n, nullptr, 0) { kWs = ks; }
  void sz_begin(uint8_t*) { if (!wave_mode) wv_begin(nullptr, nullptr); }
  void copy_lits(uint8_t*, const uint8_t*, uint32_t, bool) { copies++; }
  void copy_lits_wide(uint8_t*, const uint8_t*, uint32_t) { copies++; }
  void copy_match(uint8_t*, uint32_t, uint32_t, uint32_t, bool) { copies++; }
  void copy_match_wide(uint8_t*, uint32_t, uint32_t, uint32_t) { copies++; }
};

}  // namespace

extern "C" {

// the decoded-size query: fast = 0 the exact path alone, 1 the fast interior + the exact path; ks = bytes of the stream ring (the
// device uses 2048).  Returns the value, or -1000000 if the simulated wavefront touched memory outside [src, src + src_size) or its
// LDS.  *exact_calls (may be NULL): how many runs the exact code went through -- few where the fast interior did the block.
int sim_decoded_size(const uint8_t* src, int src_size, int cap, int fast, int ks, long long* exact_calls) {
  SizeHost g(src, src_size > 0 ? src_size : 0, (uint32_t)ks);
  const int r = fast ? lz4hip::decoded_size<SizeHost, true>(g, src, src_size, cap, nullptr)
                     : lz4hip::decoded_size<SizeHost, false>(g, src, src_size, cap, nullptr);
  if (exact_calls) *exact_calls = (long long)g.copies;
  if (g.oob || hostsim::GroupHost::walk_mismatch.load() != 0) return -1000000;
  return r;
}

}  // extern "C"
