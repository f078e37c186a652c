// The loaders of rvtests_amd/csrc/rvt_bed_codes.h (bed_load4, bed_load16) over heap buffers of exactly end - base bytes: every
// length 1 .. 40, every start offset inside the buffer.  Host code only; built with the address and undefined-behaviour
// sanitizers (tests/test_bed_codes_cpu.py), so a byte touched outside [base, end) shows as a report, and every value is held to a
// byte-wise read with zeros behind `end`.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rvtests_amd/csrc tools/bed_codes_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "rvt_bed_codes.h"

static int g_failed = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      std::fprintf(stderr, "line %d: %s (length %d, offset %d)\n", __LINE__, #cond, len, off); \
      ++g_failed;                                                                            \
    }                                                                                        \
  } while (0)

// bytes [off + 4 k, off + 4 k + 4) of the buffer as a little-endian word, zero from `len` on
static uint32_t bytewise(const unsigned char* base, int len, int off, int k) {
  uint32_t v = 0;
  for (int b = 0; b < 4; ++b)
    if (off + 4 * k + b < len) v |= (uint32_t)base[off + 4 * k + b] << (8 * b);
  return v;
}

int main() {
  for (int len = 1; len <= 40; ++len) {
    unsigned char* base = static_cast<unsigned char*>(std::malloc((size_t)len));  // (16-byte aligned: off & 3 is p's alignment)
    if (!base) return 2;
    for (int i = 0; i < len; ++i) base[i] = (unsigned char)(37 * i + 11 * len + 1);
    const unsigned char* end = base + len;
    for (int off = 0; off < len; ++off) {
      CHECK(rvt::bed_load4(base + off, base, end) == bytewise(base, len, off, 0));
      uint32_t w[4];
      rvt::bed_load16(base + off, base, end, w);
      for (int k = 0; k < 4; ++k) CHECK(w[k] == bytewise(base, len, off, k));
      // a piece that starts at p itself, at any alignment: the branch that may not reach down to the aligned dword below p
      if (off > 0) {
        CHECK(rvt::bed_load4(base + off, base + off, end) == bytewise(base, len, off, 0));
        rvt::bed_load16(base + off, base + off, end, w);
        for (int k = 0; k < 4; ++k) CHECK(w[k] == bytewise(base, len, off, k));
      }
    }
    std::free(base);
  }
  if (g_failed) return 1;
  std::puts("bed codes: ok");
  return 0;
}
