// container_rules_test.cpp -- csrc/container_rules.h as the host compiles it, alone: a stand-alone program (address and
// undefined-behaviour sanitizers, tests/support.py build_sanitized) that walks every body of a case file and prints what the walk
// took.  Every body sits in an allocation of exactly its length, so a rule that reads one byte past a body is a finding.
//   argv[1]: the case file -- u32 count, then per case {u32 kind, u32 flags, u32 max_block, u32 n_max, u64 slot_bytes, u64 len, bytes}
//   stdout : per case "C blocks why pos dst_bytes slot_max" and per block "B raw pay_off pay_len cap stored next bound"
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../lz4-java_amd/csrc/container_rules.h"

namespace cr = lz4hip::container_rules;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t h[4];
    uint64_t slot = 0, len = 0;
    if (fread(h, 4, 4, f) != 4 || fread(&slot, 8, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    uint8_t* body = new uint8_t[len];                     // exactly its length
    if (len && fread(body, 1, len, f) != len) return 2;
    std::vector<cr::Block> table(h[3]);
    const cr::Walk w = cr::walk(body, len, (int)h[0], h[1], h[2], slot, h[3], table.data());
    printf("C %u %u %llu %llu %llu\n", w.blocks, w.why, (unsigned long long)w.pos, (unsigned long long)w.dst_bytes, (unsigned long long)w.slot_max);
    for (uint32_t k = 0; k < w.blocks; k++) {
      const cr::Block& b = table[k];
      printf("B %u %llu %u %u %u %llu %llu\n", b.raw, (unsigned long long)b.pay_off, b.pay_len, b.cap, b.stored, (unsigned long long)b.next,
             (unsigned long long)b.bound);
    }
    delete[] body;
  }
  fclose(f);
  return 0;
}
