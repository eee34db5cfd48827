// tests/cpp/mirror_io.h -- TEST INFRASTRUCTURE ONLY.  What the *_mirror_test.cpp programs do alike around their calls into the C++ host
// mirror: read an input file, check that nothing outside a destination's slot was written, write the result file.
#ifndef MIRROR_IO_H
#define MIRROR_IO_H
#include <cstdint>
#include <cstdio>
#include <vector>

// the file's bytes appended to `out`; false where it cannot be opened
static inline bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (int c; (c = fgetc(f)) != EOF;) out.push_back((uint8_t)c);
  fclose(f);
  return true;
}

// every byte of `b` outside [off, off + room) still holds `fill`; else "byte <i> outside the <what> changed" on stderr and false
static inline bool untouched(const std::vector<uint8_t>& b, size_t off, size_t room, const char* what = "slot", uint8_t fill = 0xEE) {
  for (size_t i = 0; i < b.size(); i++)
    if ((i < off || i >= off + room) && b[i] != fill) { fprintf(stderr, "byte %zu outside the %s changed\n", i, what); return false; }
  return true;
}

// n bytes at p -> the file `path`
static inline bool dump(const char* path, const uint8_t* p, size_t n) {
  FILE* o = fopen(path, "wb");
  const bool ok = o && fwrite(p, 1, n, o) == n;
  if (o) fclose(o);
  return ok;
}
#endif
