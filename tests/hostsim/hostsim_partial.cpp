// tests/hostsim/hostsim_partial.cpp -- TEST INFRASTRUCTURE ONLY.
// The PARTIAL switch of lz4-java_amd/csrc/lz4_decode_core.h (LZ4_decompress_safe_partial) compiled against the lock-step host
// backend, in a library of its own (tests/test_partial_hostsim.py), in the three forms the partial kernels run.  Nothing here is
// linked into liblz4hip.so.
#include <stdint.h>
#include "../../lz4-java_amd/csrc/lz4_decode_core.h"
#include "group_host.h"

extern "C" {

// LZ4_decompress_safe_partial(src, dst, src_size, target, cap) as decode_partial_kernel / decode_partial_deep_kernel run it:
// form 0 = the plain interior loop, 1 = the staged loop (decode_partial_kernel<4, 0, true>), 2 = the deep loop
// (decode_partial_deep_kernel<8>); gl = lanes per block.  Returns liblz4's value, or -1000000 if the simulated group touched
// memory outside [src, src + src_size) / [dst, dst + min(target, cap)).
int sim_decompress_partial(const uint8_t* src, int src_size, uint8_t* dst, int target, int cap, int form, int gl) {
  const int out_size = (target < 0 || cap < 0) ? -1 : (target < cap ? target : cap);
  hostsim::GroupHost g(gl, src, src_size, dst, out_size > 0 ? out_size : 0);
  int r;
  if (form == 2) r = lz4hip::decode_block<hostsim::GroupHost, true, 2, false, true>(g, src, src_size, dst, out_size, g.stg_buf);
  else if (form == 1) r = lz4hip::decode_block<hostsim::GroupHost, true, 0, true, true>(g, src, src_size, dst, out_size, g.stg_buf);
  else r = lz4hip::decode_block<hostsim::GroupHost, true, 0, false, true>(g, src, src_size, dst, out_size);
  if (g.oob || hostsim::GroupHost::walk_mismatch.load() != 0) return -1000000;
  return r;
}

}  // extern "C"
