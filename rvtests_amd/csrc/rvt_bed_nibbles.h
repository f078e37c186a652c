// rvtests_amd — one byte of a PLINK .bed row (four 2-bit calls, sample e in bits 2 e: 00 -> 0, 10 -> 1, 11 -> 2, 01 -> missing)
// as what MetaCov's MXFP4 band reads of a mean-imputed column g = h + mu m (band_gemm.hip.h, band_rows.hip.h): four E2M1 codes
// of the calls h (value << 1, missing -> 0) and four of the missing mask m (0x2 = 1.0 where the call is missing), sample e in
// bits 4 e of the 16 — sample 2 i in the low nibble of byte i of a nibble row — and the numbers of 0 / 1 / 2 / missing calls.
// `live` (1 .. 4) says how many of the four samples exist: a row's last byte carries N - 4 (ceil(N / 4) - 1) of them, and the
// pairs behind them are padding, which is neither counted nor coded whatever it holds.
// No HIP types: compiled by hipcc for the device (bed_band_kernels.hip.h) and by g++ for the harness (hostcheck.cpp).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RVT_BN_HD __host__ __device__ inline
#else
#define RVT_BN_HD inline
#endif

namespace rvt {

struct BedNibbles {
  unsigned h;     // 16 bits: the calls' E2M1 codes (0 -> 0x0, 1 -> 0x2, 2 -> 0x4, missing -> 0x0)
  unsigned m;     // 16 bits: 0x2 where the call is missing
  unsigned one;   // bit 4 e: sample e is a call of 1 (likewise two, miss, zero) — the counts are the population counts
  unsigned two;
  unsigned miss;
  unsigned zero;
};

// the low bit of every nibble of the `live` first samples
RVT_BN_HD unsigned bed_live_mask(int live) { return live >= 4 ? 0x1111u : (0x1111u & ((1u << (4 * live)) - 1u)); }

RVT_BN_HD BedNibbles bed_byte_nibbles(unsigned byte, unsigned live_mask) {
  // pair e -> the low two bits of nibble e
  unsigned x = byte & 0xffu;
  x = (x | (x << 4)) & 0x0f0fu;
  x = (x | (x << 2)) & 0x3333u;
  const unsigned lo = x & 0x1111u, hi = (x >> 1) & 0x1111u;
  BedNibbles r;
  r.one = live_mask & hi & ~lo;
  r.two = live_mask & hi & lo;
  r.miss = live_mask & lo & ~hi;
  r.zero = live_mask & ~lo & ~hi;
  r.h = (r.one << 1) | (r.two << 2);
  r.m = r.miss << 1;
  return r;
}

RVT_BN_HD int bed_popc16(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  int n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
#endif
}

}  // namespace rvt
