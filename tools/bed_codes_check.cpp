// The loaders of rvtests_amd/csrc/rvt_bed_codes.h (bed_load4, bed_load16) over heap buffers of exactly end - base bytes: every
// length 1 .. 40, every start offset inside the buffer; and bed_span, where V rows at an address lie in a matrix, against 128-bit
// arithmetic.  Host code only; built with the address and undefined-behaviour sanitizers (tests/test_bed_codes_cpu.py), so a byte
// touched outside [base, end) or an index that overflows shows as a report, and every value is held to a byte-wise read with
// zeros behind `end`.
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

// bed_span's answer in arithmetic that cannot overflow
static long long span_wide(uint64_t base, long long nv, long long pitch, uint64_t at, long long V) {
  const __int128 off = (__int128)at - (__int128)base;
  if (off < 0 || off >= (__int128)nv * pitch) return rvt::kBedSpanOutside;
  if (off % pitch != 0) return rvt::kBedSpanOffRow;
  const __int128 first = off / pitch;
  return first + (__int128)V > (__int128)nv ? rvt::kBedSpanLeaves : (long long)first;
}

// pitches 1, 129, 125 000 x 1, 2, 4 099 rows x bases low and near 2^47 x addresses around both ends and the row boundaries x
// V from 1 to one past the end, 2^30 and 2^62
static int check_spans() {
  int bad = 0, cases = 0;
  const long long pitches[] = {1, 129, 125000}, nvs[] = {1, 2, 4099};
  const uint64_t bases[] = {4096, ((uint64_t)1 << 47) - 4096, ((uint64_t)1 << 47) - 1};
  for (long long pitch : pitches)
    for (long long nv : nvs)
      for (uint64_t base : bases) {
        const uint64_t end = base + (uint64_t)(nv * pitch);
        const long long rows[] = {0, 1, nv / 2, nv - 2, nv - 1};
        uint64_t at[5 * 3 + 4];
        int na = 0;
        for (long long r : rows)
          if (r >= 0)
            for (long long d = -1; d <= 1; ++d) at[na++] = base + (uint64_t)(r * pitch + d);
        at[na++] = end - 1, at[na++] = end, at[na++] = end + rvt::kBedSlackBytes - 1, at[na++] = end + rvt::kBedSlackBytes;
        for (int a = 0; a < na; ++a) {
          const long long left = nv - (long long)((at[a] - base) / (uint64_t)pitch);
          const long long Vs[] = {0, 1, left - 1, left, left + 1, nv, nv + 1, 1LL << 30, 1LL << 62, INT64_MAX};
          for (long long V : Vs) {
            if (V < 0) continue;
            ++cases;
            if (rvt::bed_span(base, nv, pitch, at[a], V) != span_wide(base, nv, pitch, at[a], V)) {
              std::fprintf(stderr, "bed_span(base %llu, %lld rows of %lld, at base%+lld, V %lld)\n", (unsigned long long)base, nv,
                           pitch, (long long)(at[a] - base), V);
              ++bad;
            }
          }
        }
      }
  if (cases < 300) ++bad;
  return bad;
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
  g_failed += check_spans();
  if (g_failed) return 1;
  std::puts("bed codes: ok");
  return 0;
}
