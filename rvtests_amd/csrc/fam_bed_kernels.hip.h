// rvtests_amd — the family tests' front stage over rows of a resident .bed matrix (rvt_score_bed_dev_fam, rvt_lrt_bed_dev_fam):
// what raw_colstat_kernel + rotate_columns give for fp64 columns — the rotated columns U'G, the raw column sums and the
// polymorphic flags — formed from the 2-bit codes where they lie (the format, its loaders and the row sources: rvt_bed_codes.h).
// The column a caller would have uploaded is the calls with missing imputed to the mean of the called ones
// (DataConsolidator.cpp:217-245), i.e. exactly  g = c + mu m  with c = the calls (missing -> 0), m = the missing indicator and
// mu = (n1 + 2 n2) / (N - missing):
//   * family form (rvt_set_kinship_families): rot_fam_bed_kernel, rot_fam_kernel's tile filled from the codes;
//   * dense U on digit planes: fam_bed_unpack_kernel writes c and m as single-plane int8 operands of planes_gemm, U'c and U'm
//     are exact integer products and fam_bed_combine_kernel forms U'c + mu U'm (mu in the planes' fixed point, see
//     fam_bed_fill_fixed) — 6 x 2 plane pairs where the fp64 route's quantised imputed column costs 6 x 6, and no fp64 read
//     of the column at all;
//   * column-compressed U with scattered supports: no kernel here — the piece is expanded to fp64 columns with
//     bed_expand_columns_kernel and goes through rotate_columns (rot_sparse_kernel); the form is not worth one of its own.
// Bytes per column: N / 4 of codes instead of 8 N of doubles in, 8 N out (family form; the dense form adds 2 N of planes).
// Rows start at any byte address, so every kernel here loads single bytes; the padding pairs of a row's last byte are never
// looked at (family form: no member index reaches them) or masked out.
// The gene side (rvt_run_fam_tests_bed_dev: FamSKAT, FamCMC, FamZeggini) adds the flip to the minor allele and the drop of
// monomorphic rows from the counts, and runs the same kernels over a LIST of kept rows (they are scattered after the drop, and
// genes lie anywhere) with the flip applied: every kernel over rows takes its row source (BedRowsAt, BedRowList) as a template
// parameter.  Last, the burden collapse from the codes.
// Included by rvt_fam.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bed_expand.hip.h"

namespace rvt {

// The fill value f of a missing call in the fixed point the digit planes give a non-integer column (quantize_columns: entries
// scaled by 2^s, s = 7 kRotPlanesG - 3 - ilogb(max |g|), and the largest entry of an imputed column is its largest call — top2:
// that call is 2): rint(f 2^s) 2^-s.  The dense rotation multiplies with it, so that it stays the integer product the fp64 route
// forms of the same column (tests/rotref.py states it) — U'g = 2^-s (2^s U'c + rint(f 2^s) U'm) — whose bound then holds here
// as well; the other forms take the fill value itself.
__device__ __forceinline__ double fam_bed_fill_fixed(double f, bool top2) {
  const int s = 7 * kRotPlanesG - 3 - (top2 ? 1 : 0);
  return ldexp(rint(ldexp(f, s)), -s);
}

// The site pass: counts[4 v ..] = n0 n1 n2 missing of row v (recode_bed_count_kernel) -> the fill value, the column sum and the
// polymorphic flag of the imputed column.  sum = n1 + 2 n2 + missing mu; polymorphic = at least two of n0, n1, n2 non-zero,
// which is raw_colstat_kernel's min != max on the imputed column (one called value: the mean is that value).  A row with no
// called sample gets mu = 0 and is monomorphic: its rotated column is all zero and no NaN reaches a neighbour.
// muq = mu in the digit planes' fixed point (fam_bed_fill_fixed; ac > 0: the largest call is 1 or 2; ac == 0: mu is 0 anyway).
static __global__ __launch_bounds__(256) void fam_bed_site_kernel(const unsigned long long* __restrict__ counts, int n,
                                                                  double* __restrict__ mu, double* __restrict__ muq,
                                                                  double* __restrict__ colsum, int* __restrict__ poly) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const long long n2 = (long long)counts[4 * v + 2];
  const BedSite s = bed_site((long long)counts[4 * v], (long long)counts[4 * v + 1], n2, (long long)counts[4 * v + 3]);
  mu[v] = s.mean;
  muq[v] = fam_bed_fill_fixed(s.mean, n2 > 0);
  colsum[v] = fma((double)s.missing, s.mean, (double)s.ac);
  poly[v] = s.poly ? 1 : 0;
}

// rot_fam_kernel over codes: the same grid (runs of families x tiles of kRotFamCols columns), the same thread-to-eigenpair
// map, the same fma chain (rot_fam_chain) and the same stores; only step 1 differs — thread t decodes the pair of sample
// members[e0 + t] from byte members[e0 + t] >> 2 of each of the tile's rows, missing -> mu[col], and flips the value where the
// row source says so: flip ? 2.0 - v : v with v = bed_value(code, mu).  A tile therefore holds the very doubles the fp64 route
// reads from an uploaded imputed column (after fam_flip_compact_kernel, on the gene side), and the outputs agree with it bit
// for bit.
// Traffic per column: the bytes of the members' pairs (N / 4 when every sample belongs to a family of the run) and 8 N out.
template <class Rows>
static __global__ __launch_bounds__(kRotFamRows) void rot_fam_bed_kernel(
    const int* __restrict__ run_ptr, const int* __restrict__ pair_fam, const long long* __restrict__ fam_ptr,
    const int* __restrict__ members, const long long* __restrict__ colptr, const double* __restrict__ vals, const Rows src,
    const double* __restrict__ mu, int ncols, double* __restrict__ out, long long ld_dst) {
  __shared__ double g[kRotFamCols][kRotFamRows];
  const int e0 = run_ptr[blockIdx.x], nrows = run_ptr[blockIdx.x + 1] - e0;  // nrows <= kRotFamRows
  const int t = threadIdx.x, col0 = blockIdx.y * kRotFamCols;
  const int nc = min(kRotFamCols, ncols - col0);
  const bool active = t < nrows;
  int k = 0, row0 = 0;
  const double* u = vals;
  if (active) {
    const int e = e0 + t, f = pair_fam[e];
    const long long fs = fam_ptr[f];
    k = (int)(fam_ptr[f + 1] - fs);
    row0 = (int)(fs - e0);
    u = vals + colptr[e];
    const int s = members[e], sh = 2 * (s & 3);
#pragma unroll
    for (int c = 0; c < kRotFamCols; ++c)
      if (c < nc) {
        const double v = bed_value(((unsigned)src.row(col0 + c)[s >> 2] >> sh) & 3u, mu[col0 + c]);
        g[c][t] = src.flip(col0 + c) ? 2.0 - v : v;
      }
  }
  __syncthreads();
  if (!active) return;
  double acc[kRotFamCols];
  rot_fam_chain(u, k, row0, g, acc);
  double* dst = out + (e0 + t) + (long long)col0 * ld_dst;
#pragma unroll
  for (int c = 0; c < kRotFamCols; ++c)
    if (c < nc) dst[(long long)c * ld_dst] = acc[c];
}

// n rows -> the B operand of planes_gemm, one int8 plane: column j = c', the calls of row j (2 - call where the row source flips
// it) with missing -> 0, and — with_m — column n + j = its missing indicator m (the flipped imputed column is c' + mu' m); column j
// at B + j * ldk, sample i at byte i.  A thread takes one byte of a row (four samples) and stores four int8 per column as one
// dword (ldk is a multiple of 128 and 4 ceil(N / 4) <= ldk); the pairs past sample N - 1 are written as zeros whatever the byte
// holds.  The rest of B (bytes from 4 ceil(N / 4) on, the pad columns) is zeroed by the caller.  grid (ceil(pitch / 256), n).
template <class Rows>
static __global__ __launch_bounds__(256) void fam_bed_unpack_kernel(const Rows src, long long pitch, long long N, int n,
                                                                    int with_m, signed char* __restrict__ B, long long ldk) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= pitch) return;
  const int j = blockIdx.y;
  const unsigned code = src.row(j)[b];
  const bool fl = src.flip(j);
  const long long left = N - 4 * b;  // > 0
  uint32_t cw = 0u, mw = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned q = (code >> (2 * e)) & 3u;
    if (e < left) {
      const unsigned call = q == 2u ? 1u : (q == 3u ? 2u : 0u);
      cw |= (q == 1u ? 0u : (fl ? 2u - call : call)) << (8 * e);
      mw |= (q == 1u ? 1u : 0u) << (8 * e);
    }
  }
  *reinterpret_cast<uint32_t*>(B + (long long)j * ldk + 4 * b) = cw;
  if (with_m) *reinterpret_cast<uint32_t*>(B + (long long)(n + j) * ldk + 4 * b) = mw;
}

// out[:, h] = fma(mu[h], C[:, n + h], C[:, h]) for the N rows of n columns: U'g = U'c + mu U'm (the caller passes muq).
// grid (ceil(N / 256), n).
static __global__ __launch_bounds__(256) void fam_bed_combine_kernel(const double* __restrict__ C, long long ldc, long long N,
                                                                     int n, const double* __restrict__ mu,
                                                                     double* __restrict__ out, long long ld_dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int h = blockIdx.y;
  out[i + (long long)h * ld_dst] = fma(mu[h], C[i + (long long)(n + h) * ldc], C[i + (long long)h * ldc]);
}

// ---- the gene-based family tests over resident rows (rvt_run_fam_tests_bed_dev) -----------------------------------------------------
// Step 1 of rvt_run_fam_tests (DataConsolidator.cpp:46-69,94-142) decided from the four counts of a row, in integers, with
// called = n0 + n1 + n2 and a = n1 + 2 n2: flags[v] bit 0 = flip to the minor allele, bit 1 = keep (polymorphic, the rule of
// fam_bed_site_kernel), bit 2 = no missing call (a kept row then holds hard calls only: fam_colstat_kernel's bit 2).
// flip = a > called.  That is the reference's s > rows and fam_colstat_kernel's !(sum <= N) on the imputed column in every case:
// the imputed column sums to a N / called, which differs from N by at least N / called >= 1 unless a == called — far beyond the
// rounding of any summation order of N values in [0, 2] — and when a == called the fill value is exactly 1.0, every entry is an
// integer and the sum is exactly N in any order.  No rounding of either route can decide differently.
static __global__ __launch_bounds__(256) void fam_bed_gene_site_kernel(const unsigned long long* __restrict__ counts, long long n,
                                                                       int* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const BedSite s = bed_site((long long)counts[4 * v], (long long)counts[4 * v + 1], (long long)counts[4 * v + 2],
                             (long long)counts[4 * v + 3]);
  flags[v] = (s.flip ? 1 : 0) | (s.poly ? 2 : 0) | (s.missing == 0 ? 4 : 0);
}

// The kept rows of a batch, column k of the compact matrix = row src[k] of the site pass: flip[k]; mu[k] = a / called, the fill
// value of a missing call BEFORE the flip (the family form and the expansion flip the decoded value, 2.0 - v: the one fp64
// subtraction of fam_flip_compact_kernel); fillq[k] = the fill value AFTER the flip, mu' = 2.0 - mu where flipped, in the fixed
// point the digit planes give the column (fam_bed_fill_fixed; the largest entry of a flipped kept column is 2 when n0 > 0,
// else 1).
static __global__ __launch_bounds__(256) void fam_bed_kept_kernel(const unsigned long long* __restrict__ counts,
                                                                  const int* __restrict__ src, long long T,
                                                                  int* __restrict__ flip, double* __restrict__ mu,
                                                                  double* __restrict__ fillq) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= T) return;
  const long long v = src[k];
  const long long n0 = (long long)counts[4 * v], n2 = (long long)counts[4 * v + 2];
  const BedSite s = bed_site(n0, (long long)counts[4 * v + 1], n2, 0);  // (kept: called >= 2)
  flip[k] = s.flip ? 1 : 0;
  mu[k] = s.mean;
  fillq[k] = fam_bed_fill_fixed(s.flip ? 2.0 - s.mean : s.mean, (s.flip ? n0 : n2) > 0);
}

// cmcCollapse / zegginiCollapse (src/Model.cpp:73-89,115-130) from the codes: gene k owns kept rows [off[k], off[k] + m[k]) of
// the list and writes its two collapsed columns to out + (2k) * ld and out + (2k+1) * ld, as fam_collapse_kernel does from the
// flipped fp64 block.  A thread takes one byte position (four samples) and walks the gene's kept rows; a sample counts where
// (int)value > 0 on the flipped, imputed value: a called one when flip ? call < 2 : call > 0, a missing one when its fill value
// (flip ? 2.0 - mu : mu) is >= 1 — only an unflipped row with a == called, mu = 1.0, gets there.  Reads m N / 4 bytes per gene
// where the fp64 route reads 8 m N.  grid (ceil(pitch / 256), genes).
static __global__ __launch_bounds__(256) void fam_bed_collapse_kernel(const unsigned char* const* __restrict__ rows,
                                                                      const int* __restrict__ flip,
                                                                      const double* __restrict__ mu, const int* __restrict__ off,
                                                                      const int* __restrict__ m, long long pitch, long long N,
                                                                      long long ld, double* __restrict__ out) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x, i = 4 * b;
  if (b >= pitch) return;
  const int k = blockIdx.y, j0 = off[k], mk = m[k];
  int n[4] = {0, 0, 0, 0};
  for (int j = j0; j < j0 + mk; ++j) {
    const unsigned code = rows[j][b];
    const bool fl = flip[j] != 0;
    const int miss = (int)(fl ? 2.0 - mu[j] : mu[j]) > 0 ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned q = (code >> (2 * e)) & 3u;  // 0 -> 0, 2 -> 1, 3 -> 2, 1 -> missing
      n[e] += q == 1u ? miss : (fl ? (q != 3u ? 1 : 0) : (q != 0u ? 1 : 0));
    }
  }
  double* cmc = out + (long long)(2 * k) * ld + i;
  double* zeg = out + (long long)(2 * k + 1) * ld + i;
  for (int e = 0; e < 4 && i + e < N; ++e) {
    cmc[e] = n[e] > 0 ? 1.0 : 0.0;
    zeg[e] = (double)n[e];
  }
}

}  // namespace rvt
