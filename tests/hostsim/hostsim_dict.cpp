// tests/hostsim/hostsim_dict.cpp -- TEST INFRASTRUCTURE ONLY.
// The DICT switch of lz4-java_amd/csrc/lz4_decode_core.h (LZ4_decompress_safe_usingDict, external dictionary) compiled against the
// lock-step host backend, in a library of its own (tests/test_dict_hostsim.py), in the forms the dictionary kernels run.  Nothing here
// is linked into liblz4hip.so.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/lz4_decode_core.h"
#include "group_host.h"

extern "C" {

// LZ4_decompress_safe_usingDict(src, dst, src_size, cap, dict, dict_len) as decode_dict_kernel / decode_dict_deep_kernel run it:
// form 0 = the plain interior loop (built with -DLZ4HIP_DECODE_INTERIOR=0, libhostsim_dict_exact.so: the exact tiers alone), 1 = the staged
// loop (decode_dict_kernel<4, 0, true>), 2 = the deep loop with the pipelined loop behind it (decode_dict_deep_kernel<8>), 3 = the
// pipelined loop alone; gl = lanes per block.
// The simulator knows ONE readable range besides dst, so stream and dictionary share an arena: layout 0 = [dictionary][stream] (a read
// in front of the dictionary or behind the stream is out of bounds), layout 1 = [stream][dictionary] (a read behind the dictionary's
// end or in front of the stream is).  A case is run in both.  Returns liblz4's value, or -1000000 if the simulated group touched
// memory outside the arena / [dst, dst + cap).
int sim_decompress_dict(const uint8_t* src, int src_size, uint8_t* dst, int cap, const uint8_t* dict, int dict_len, int form, int gl, int layout) {
  const size_t ns = src_size > 0 ? (size_t)src_size : 0, nd = dict_len > 0 ? (size_t)dict_len : 0;
  std::vector<uint8_t> arena(ns + nd + 1);
  uint8_t* const s = arena.data() + (layout == 0 ? nd : 0);
  uint8_t* const d = arena.data() + (layout == 0 ? 0 : ns);
  if (ns) memcpy(s, src, ns);
  if (nd) memcpy(d, dict, nd);
  hostsim::GroupHost g(gl, arena.data(), (long)(ns + nd), dst, cap > 0 ? cap : 0);
  const uint8_t* const dict_end = d + nd;
  int r;
  if (form == 2) r = lz4hip::decode_block<hostsim::GroupHost, true, 2, false, false, true>(g, s, src_size, dst, cap, g.stg_buf, dict_end, dict_len);
  else if (form == 1) r = lz4hip::decode_block<hostsim::GroupHost, true, 0, true, false, true>(g, s, src_size, dst, cap, g.stg_buf, dict_end, dict_len);
  else if (form == 3) r = lz4hip::decode_block<hostsim::GroupHost, true, 1, false, false, true>(g, s, src_size, dst, cap, nullptr, dict_end, dict_len);
  else r = lz4hip::decode_block<hostsim::GroupHost, true, 0, false, false, true>(g, s, src_size, dst, cap, nullptr, dict_end, dict_len);
  if (g.oob || hostsim::GroupHost::walk_mismatch.load() != 0) return -1000000;
  return r;
}

}  // extern "C"
