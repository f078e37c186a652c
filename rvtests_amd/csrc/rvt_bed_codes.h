// rvtests_amd — rows of a device-resident PLINK .bed matrix (rvt_bed_alloc): the one statement of the format and of what every
// reader of such rows does with it.
//
// Row r lies at rows + r * pitch with pitch = ceil(N / 4) bytes; rows are NOT aligned (N = 515: pitch 129, consecutive rows start
// at all four byte alignments).  Sample i of a row sits in bits 2 (i & 3), 2 (i & 3) + 1 of byte i >> 2; the 2-bit codes are
// 00 -> 0, 10 -> 1, 11 -> 2, 01 -> missing (lo = bit 0, hi = bit 1 of a pair: call = hi + (hi & lo), missing = lo & ~hi).  The
// pairs of a row's last byte behind sample N - 1 are padding: they hold anything and must not count — a reader either never
// indexes them or masks them with one of the live masks below.
//
// Here: the value of a code, the site pass on the four counts of a row (BedSite), the live masks, the population counts, the
// spread of a code byte into byte lanes and the loaders of 4 and 16 bytes of codes from any byte address.  (The nibble form of
// MetaCov's MXFP4 band, with its own per-nibble mask bed_live_mask, is rvt_bed_nibbles.h.)  The kinship tiles read nine aligned
// words per row, which may reach past the last row's end (kin_stage, kinship_kernels.hip.h): rvt_bed_alloc leaves kBedSlackBytes
// behind the matrix for them.  Also here, for the host: the pitch (bed_pitch) and where V rows at an address lie in a matrix of
// known extent (bed_span) — what the engine's record of a matrix (rvt_ctx::BedMatrix) and bed_rows_span are made of.
// No HIP types in any signature: compiled by hipcc for the kernels and by g++ for the harness (hostcheck.cpp) and for
// tools/bed_codes_check.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RVT_BC_HD __host__ __device__ __forceinline__
#else
#define RVT_BC_HD inline
#endif

namespace rvt {

// bytes of a row of N samples: the one place that writes it
constexpr long long bed_pitch(long long N) { return (N + 3) / 4; }
// bytes rvt_bed_alloc leaves behind the last row (kin_stage's aligned words)
constexpr int kBedSlackBytes = 16;

// Where V rows at address `at` lie in the matrix of n_variants rows of `pitch` bytes at `base` (addresses as integers): the index
// of the first row, or one of the three refusals.  In row indices throughout — V is never multiplied by the pitch, so any V of
// an int64_t caller is answered without overflow.  The slack is not part of the rows: an address in it is outside.
constexpr long long kBedSpanOutside = -1, kBedSpanOffRow = -2, kBedSpanLeaves = -3;
inline long long bed_span(uint64_t base, long long n_variants, long long pitch, uint64_t at, long long V) {
  if (at < base || pitch < 1) return kBedSpanOutside;
  const uint64_t off = at - base, first = off / (uint64_t)pitch;
  if (first >= (uint64_t)n_variants) return kBedSpanOutside;
  if (off % (uint64_t)pitch != 0) return kBedSpanOffRow;
  return V > n_variants - (long long)first ? kBedSpanLeaves : (long long)first;
}

// the value of the 2-bit code q with `fill` for a missing call
RVT_BC_HD double bed_value(unsigned q, double fill) { return q == 0u ? 0.0 : (q == 2u ? 1.0 : (q == 3u ? 2.0 : fill)); }

// What the counts n0 n1 n2 missing of a row decide.  mean is the fill value of a mean-imputed column (0.0 for a row with no
// called sample); poly = at least two of n0, n1, n2 are non-zero, i.e. the imputed column has two distinct values (one called
// value v makes the mean v exactly); flip = the coded allele is the major one (ac > called).  Every consumer's own twist — a mean
// of 0 for a row without a missing call, af = ac / (2 called), a fixed-point fill — is written at the consumer on top of this.
struct BedSite {
  long long called, ac, missing;  // n0 + n1 + n2, n1 + 2 n2, the missing calls
  bool poly, flip;
  double mean;  // ac / called
};

RVT_BC_HD BedSite bed_site(long long n0, long long n1, long long n2, long long nm) {
  BedSite s;
  s.called = n0 + n1 + n2;
  s.ac = n1 + 2 * n2;
  s.missing = nm;
  s.poly = ((n0 > 0) + (n1 > 0) + (n2 > 0)) >= 2;
  s.flip = s.ac > s.called;
  s.mean = s.called > 0 ? (double)s.ac / (double)s.called : 0.0;
  return s;
}

// "The first `left` samples of this group exist" (left <= 0: none): bit 0 of every 2-bit pair of a dword of codes, 16 samples ...
RVT_BC_HD uint32_t bed_live_pairs(long long left) {
  return left >= 16 ? 0x55555555u : (left <= 0 ? 0u : (0x55555555u & ((1u << (2 * (int)left)) - 1u)));
}
// ... and bit 0 of every byte lane of a dword that holds one sample per byte, 4 samples
RVT_BC_HD uint32_t bed_live_lanes(long long left) {
  return left >= 4 ? 0x01010101u : (left <= 0 ? 0u : (0x01010101u & ((1u << (8 * (int)left)) - 1u)));
}

RVT_BC_HD int bed_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}

// n[0 .. 3] += the calls of 0 / 1 / 2 / missing among the samples of `code` (up to 16) that live_pairs names
RVT_BC_HD void bed_counts16(uint32_t code, uint32_t live_pairs, int (&n)[4]) {
  const uint32_t lo = code & 0x55555555u, hi = (code >> 1) & 0x55555555u;
  n[0] += bed_popc(live_pairs & ~lo & ~hi);
  n[1] += bed_popc(live_pairs & hi & ~lo);
  n[2] += bed_popc(live_pairs & hi & lo);
  n[3] += bed_popc(live_pairs & lo & ~hi);
}

// The four bits at 0, 2, 4, 6 of byte k of x -> bit 0 of the four byte lanes of a dword (sample e of the byte in lane e): the
// lo bits of a dword of codes x, the hi bits of x >> 1.  The copies of the byte at shifts 0, 6, 12, 18 (one 24-bit
// multiplication) overlap in a bit that can carry only into an odd bit, which the mask drops.
RVT_BC_HD uint32_t bed_spread(uint32_t x, int k) {
  const uint32_t b = (x >> (8 * k)) & 0x55u;
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(b, 0x41041u) & 0x01010101u;
#else
  return (b * 0x41041u) & 0x01010101u;
#endif
}

// the dword at the 4-byte aligned address a
RVT_BC_HD uint32_t bed_dword(const unsigned char* a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const uint32_t*>(a);
#else
  uint32_t v;
  memcpy(&v, a, sizeof(v));
  return v;
#endif
}

// The loaders.  Contract of both: p has any alignment, no byte outside [base, end) is touched, bytes at or behind `end` read as
// zero (p >= base).  Inside the buffer they read aligned dwords and shift them together; at its first and last few bytes they go
// byte by byte.
//
// 4 bytes of codes at p: one dword where p is aligned, else two.
RVT_BC_HD uint32_t bed_load4(const unsigned char* p, const unsigned char* base, const unsigned char* end) {
  const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
  const unsigned char* a = p - sh;
  if (sh == 0u && p + 4 <= end) return bed_dword(p);
  if (sh != 0u && a >= base && a + 8 <= end) {
    const uint32_t lo = bed_dword(a), hi = bed_dword(a + 4);
    return (lo >> (8u * sh)) | (hi << (32u - 8u * sh));
  }
  uint32_t code = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int e = 0; e < 4; ++e)
    if (p + e < end) code |= (uint32_t)p[e] << (8 * e);
  return code;
}

// bytes sh .. sh + 3 of the eight bytes hi : lo
RVT_BC_HD uint32_t bed_funnel(uint32_t hi, uint32_t lo, unsigned sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | (uint64_t)lo) >> (8u * sh));
#endif
}

// 16 bytes of codes at p: five aligned dwords shifted together (four when p is aligned)
RVT_BC_HD void bed_load16(const unsigned char* p, const unsigned char* base, const unsigned char* end, uint32_t (&w)[4]) {
  const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
  const unsigned char* q = p - sh;
  if (q >= base && q + (sh ? 20 : 16) <= end) {
    const uint32_t a0 = bed_dword(q), a1 = bed_dword(q + 4), a2 = bed_dword(q + 8), a3 = bed_dword(q + 12);
    const uint32_t a4 = sh ? bed_dword(q + 16) : 0u;
    w[0] = bed_funnel(a1, a0, sh);
    w[1] = bed_funnel(a2, a1, sh);
    w[2] = bed_funnel(a3, a2, sh);
    w[3] = bed_funnel(a4, a3, sh);
  } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
      uint32_t v = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int b = 0; b < 4; ++b)
        if (p + 4 * k + b < end) v |= (uint32_t)p[4 * k + b] << (8 * b);
      w[k] = v;
    }
  }
}

// Where the rows of a kernel's job lie — consecutive in the matrix, or listed by address with a flip to the minor allele (the
// kept rows of a gene batch): a kernel over "rows" takes one of the two as a template parameter.
struct BedRowsAt {
  const unsigned char* base;
  long long pitch;
  RVT_BC_HD const unsigned char* row(int j) const { return base + (long long)j * pitch; }
  RVT_BC_HD bool flip(int) const { return false; }
};
struct BedRowList {
  const unsigned char* const* rows;
  const int* flips;
  RVT_BC_HD const unsigned char* row(int j) const { return rows[j]; }
  RVT_BC_HD bool flip(int j) const { return flips[j] != 0; }
};

}  // namespace rvt
