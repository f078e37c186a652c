// rvtests_amd — famGrammarGamma from rows of a resident .bed matrix (rvt_grammar_bed_dev): the arithmetic that is not a kernel.
//
// No HIP types: compiled by hipcc for the kernels (grammar_bed_kernels.hip.h) and by g++ into the host test harness
// (hostcheck.cpp: hc_grammar_ty_planes, hc_grammar_bed_finish, hc_grammar_bed_plan), where the CPU tests hold it to numpy.
//
// GrammarGamma::TestCovariate (regression/GrammarGamma.cpp:122-152) needs of a column g only (g - gbar)'ty and
// (g - gbar)'(g - gbar).  A mean-imputed column of PLINK codes (rvt_bed_codes.h; hi = bit 1, lo = bit 0 of a pair) is
// g = c + mu m with c the calls (missing -> 0), m the missing indicator and mu = ac / called, and gbar = mu.  With
// the 0 / 1 bit planes H = hi, L = lo, HL = hi & lo of a row:  c = H + HL,  m = L - HL,  so
//     sum c ty = S_H + S_HL,    sum m ty = S_L - S_HL,    (g - gbar)'ty = (S_H + S_HL) + mu (S_L - S_HL - T),   T = sum ty,
//     (g - gbar)'(g - gbar) = (called (n1 + 4 n2) - ac^2) / called,
// where S_X = sum X_i ty_i.  ty is ONE vector per null fit; it is held as a signed 56-bit fixed-point number per sample, cut into
// eight base-128 digits (int8 each), and the S_X are exact integer sums per digit plane (the int8 matrix cores form them).
#pragma once
#include <stdint.h>
#include "rvt_bed_codes.h"
#include "rvt_special.h"

namespace rvt {

constexpr int kGgPlanes = 8;        // base-128 digits of a ty entry: the top one signed (-64 .. 63), the others 0 .. 127
constexpr int kGgBits = 55;         // q_i = rint(ty_i 2^(55 - e)), |q_i| < 2^55
constexpr int kGgCols = 9;          // columns of the B operand that are not padding: the eight planes and the ones column
constexpr int kGgKstep = 64;        // samples of one matrix instruction (v_mfma_i32_16x16x64_i8): the unit of a slice's length
constexpr int kGgTileRows = 16;     // rows of one row tile
constexpr int kGgMaxSlice = 7168;   // samples of the longest slice: 9 bytes each in LDS (63 KB), and 127 * 7168 < 2^31
constexpr int kGgMinSlice = 2048;   // the shortest slice the plan chooses by itself (108 bytes of partial sums per row and slice)
constexpr int kGgTiles = 16;        // row tiles per workgroup the plan chooses (two per wave): B is staged once for 256 rows
constexpr int kGgMaxTiles = 64;
constexpr int64_t kGgMaxN = 1 << 23;  // samples: keeps the four-plane integer sums of grammar_bed_finish below 2^53

// e with maxabs < 2^e (0 for maxabs == 0): the largest entries then have |q| in [2^54, 2^55), so their 53 bits are kept whole
RVT_HD int grammar_ty_exp(double maxabs) {
  if (!(maxabs > 0.0)) return 0;
  int e = 0;
  (void)frexp(maxabs, &e);  // maxabs = f 2^e, f in [1/2, 1)
  return e;
}

// q = rint(ty 2^(55 - e)) and its digits: q = sum_p d[p] 128^(7 - p), d[0] = floor(q / 128^7) signed, the others 0 .. 127
RVT_HD int64_t grammar_ty_digits(double ty, int e, signed char* d) {
  const int64_t q = (int64_t)llrint(ldexp(ty, kGgBits - e));
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int p = 0; p < kGgPlanes; ++p) {
    const int sh = 7 * (kGgPlanes - 1 - p);
    const int64_t v = q >> sh;  // (arithmetic: floor)
    d[p] = (signed char)(p == 0 ? v : (v & 127));
  }
  return q;
}

// The planes of a whole vector, as the device builds them (grammar_ty_planes_kernel runs the two functions above): planes[p * ld
// + i] for i < N, *exp2 = e, totals[p] = T_p = sum_i planes[p][i].  Returns 0 when an entry of ty is not finite (nothing written).
inline int grammar_ty_planes(const double* ty, int64_t N, signed char* planes, int64_t ld, int* exp2, long long* totals) {
  double mx = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    if (!(fabs(ty[i]) <= DBL_MAX)) return 0;
    mx = fmax(mx, fabs(ty[i]));
  }
  const int e = grammar_ty_exp(mx);
  *exp2 = e;
  for (int p = 0; p < kGgPlanes; ++p) totals[p] = 0;
  for (int64_t i = 0; i < N; ++i) {
    signed char d[kGgPlanes];
    (void)grammar_ty_digits(ty[i], e, d);
    for (int p = 0; p < kGgPlanes; ++p) {
      planes[p * ld + i] = d[p];
      totals[p] += d[p];
    }
  }
  return 1;
}

// sum_p x[p] 128^(7 - p) of eight plane sums with |x[p]| <= 2 * 127 * kGgMaxN < 2^31, in ONE fixed order: the four upper and the
// four lower planes are combined exactly in int64 (each below 2^53), converted exactly and joined by one fma — one rounding.
RVT_HD double grammar_planes_value(const int64_t* x) {
  const int64_t hi = ((x[0] * 128 + x[1]) * 128 + x[2]) * 128 + x[3];
  const int64_t lo = ((x[4] * 128 + x[5]) * 128 + x[6]) * 128 + x[7];
  return fma((double)hi, 268435456.0 /* 128^4 */, (double)lo);
}

// One row: the counts, the plane sums S[0..7] = S_H, S[8..15] = S_L, S[16..23] = S_HL, the totals T, e, and the null fit's gamma
// and ySigmaY -> ok, af (af=mean), beta, beta_var, p.  ok = 0 (beta, beta_var, p NaN) when fewer than two of n0, n1, n2 are
// non-zero: the imputed column is then constant.
//
// Error of the centred g'ty against the exact sum over the samples, in units of ty:
//   * the digits: |ty_i - q_i 2^(e - 55)| <= 2^(e - 56), hence at most sum_i |g_i - mu| 2^(e - 56) <= 2^-55 (ac + mu nm) max|ty|
//     (2^(e - 1) <= max|ty|); the integer sums add nothing;
//   * four roundings, one fixed order: the join of the c part C = sum c q, the join of the m part M = sum m q - sum q (T is
//     folded in BEFORE the join, so that mu multiplies one number; both joins: grammar_planes_value), mu = ac / called, and the
//     fma mu M + C: at most 2^-53 (|C| + 2 mu |M| + |mu M + C|) in units of 2^(e - 55).  The scaling by 2^(e - 55) is exact.
// With |C| <= ac max|q|, mu |M| <= mu called max|q| = ac max|q| and max|q| 2^(e - 55) = max|ty|, both kinds together stay below
// 6 * 2^-53 ac max|ty|: a few ulp of the LARGER of the two terms that cancel in mu M + C — the cancellation g'ty has in any route
// that centres after the sum (the block route subtracts mean * sum ty) —, inside the floor 8 * 2^-53 (ac + mu nm) max|ty| of
// the tests' beta tolerance.  g'g is one rounding of an exact integer quotient.  The last lines are grammar_stream_kernel's own
// (fam_single.hip.h).
RVT_HD void grammar_bed_finish(long long n0, long long n1, long long n2, long long nm, const int64_t* S, const long long* T, int e,
                               double gamma, double ysy, int* ok, double* af, double* beta, double* beta_var, double* p) {
  const BedSite site = bed_site(n0, n1, n2, nm);
  const long long called = site.called, ac = site.ac;
  *af = called > 0 ? (double)ac / (2.0 * (double)called) : 0.0;
  if (!site.poly) {
    *ok = 0;
    *beta = *beta_var = *p = NAN;
    return;
  }
  const double mu = site.mean;
  int64_t xc[kGgPlanes], xm[kGgPlanes];
  for (int q = 0; q < kGgPlanes; ++q) {
    xc[q] = S[q] + S[2 * kGgPlanes + q];                               // sum c ty
    xm[q] = S[kGgPlanes + q] - S[2 * kGgPlanes + q] - (int64_t)T[q];   // sum m ty - sum ty
  }
  const double gty = ldexp(fma(mu, grammar_planes_value(xm), grammar_planes_value(xc)), e - kGgBits);
  const double gg = (double)(called * (n1 + 4 * n2) - ac * ac) / (double)called;
  *beta = gty / gg / gamma;
  *beta_var = ysy / gg / gamma;
  *p = chisq_Q(gty * gty / gg / gamma, 1.0);
  *ok = 1;
}

// The launch plan of grammar_bed_kernel for V rows of N samples on a chip of `cus` compute units: the sample axis [0, Npad),
// Npad = N rounded up to the K-step, is cut into `slices` slices of `slice` samples (a multiple of the K-step, the last one
// shorter), the ceil(V / 16) row tiles into `groups` workgroups of `tiles` consecutive tiles; grid = (groups, slices), and every
// (row, sample) belongs to exactly one workgroup.  By itself the plan takes kGgTiles tiles (fewer when V has fewer) and the slice
// that gives about six workgroups per compute unit, between kGgMinSlice and kGgMaxSlice; slice_req / tiles_req > 0 (the caller
// reads RVT_GG_BED_SLICE / RVT_GG_BED_TILES at every call) replace them, rounded up to the K-step and cut to what the kernel
// holds.  127 * slice < 2^31: a slice's sums fit the int32 accumulators.
struct GgBedPlan {
  long long npad, slice;
  int slices, row_tiles, tiles, groups;
};

RVT_HD GgBedPlan grammar_bed_plan(long long N, long long V, int cus, long long slice_req, int tiles_req) {
  GgBedPlan P;
  P.npad = (N + kGgKstep - 1) / kGgKstep * kGgKstep;
  P.row_tiles = (int)((V + kGgTileRows - 1) / kGgTileRows);
  int tiles = tiles_req > 0 ? tiles_req : kGgTiles;
  if (tiles > kGgMaxTiles) tiles = kGgMaxTiles;
  if (tiles > P.row_tiles) tiles = P.row_tiles;
  if (tiles < 1) tiles = 1;
  P.tiles = tiles;
  P.groups = (P.row_tiles + tiles - 1) / tiles;
  long long slice;
  if (slice_req > 0) {
    slice = (slice_req + kGgKstep - 1) / kGgKstep * kGgKstep;
  } else {
    const long long want = (6LL * (cus > 0 ? cus : 1) + P.groups - 1) / P.groups;  // slices for six workgroups per unit
    slice = ((P.npad + want - 1) / want + kGgKstep - 1) / kGgKstep * kGgKstep;
    if (slice < kGgMinSlice) slice = kGgMinSlice;
  }
  if (slice > kGgMaxSlice) slice = kGgMaxSlice;
  if (slice > P.npad) slice = P.npad;
  if (slice < kGgKstep) slice = kGgKstep;
  P.slice = slice;
  P.slices = (int)((P.npad + slice - 1) / slice);
  return P;
}

}  // namespace rvt
