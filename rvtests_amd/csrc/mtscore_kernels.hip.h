// rvtests_amd — kernels of the multiple-trait score test (rvt_mtscore.hip; `--single fastmtscore`,
// regression/FastMultipleTraitLinearRegressionScoreTest.cpp).
//
// Once per analysis: the traits and covariates are centred over their observed entries and stored as six signed base-128 digit
// planes per column, one ROW of the A operand of rot_gemm.hip.h each ([plane][row][ldk], per-row binary exponent: the layout
// and the digits of rot_quantize_f64_kernel).  Per piece of a genotype block: one pass over the fp64 columns that tests every
// value for 0 / 1 / 2, writes the one-plane int8 B operand and leaves the exact integer column sums; the products G'[Yc | Zc]
// and G'indModel run on the int8 matrix cores (rvt_planes_gemm); mt_finish_kernel forms u, v and p of every (variant, test) cell
// with the shared arithmetic of rvt_mtscore.h.  Rows of a resident .bed matrix (rvt_mt_score_bed_dev) take the front stage of
// the file's second half instead of that pass: the same B operand and moments from the 2-bit codes and their counts, plus a
// compact second operand for the rows with missing calls.  Every kernel is wave-size agnostic except for the 64-lane shuffles of the
// block reductions (256 threads = four waves of 64, as everywhere in the engine).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rvt_bed_codes.h"
#include "rvt_mtscore.h"
#include "rot_gemm.hip.h"

namespace rvt {

constexpr int kMtPlanes = 6;        // digits of a trait / covariate row (40 bits below the row's largest entry)
constexpr int kMtFinTests = 16;     // tests x variants of one workgroup of mt_finish_kernel
constexpr int kMtFinVars = 16;
constexpr int kMtPassRows = 16384;  // rows of a column one workgroup of mt_geno_pass_kernel converts (16 x 256 threads x 4)

// sum over the 256 threads of a workgroup in a FIXED order (lanes by shuffle, the four waves in order); every thread gets it
template <class T>
__device__ __forceinline__ T mt_block_sum(T v, T* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (red may still be read from an earlier call)
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T s = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}
__device__ __forceinline__ double mt_block_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = fmax(s, red[w]);
  return s;
}

// Observed count, mean over the observed entries (0 when there is none) and max |x - mean| of every column of a column-major
// n x ncols matrix (NaN = missing; center(), :93-126).  stat[4 col + {0, 1, 2}]; grid = ncols, 256 threads.
static __global__ __launch_bounds__(256) void mt_colstat_kernel(const double* __restrict__ src, long long n,
                                                                double* __restrict__ stat) {
  __shared__ double red[4];
  const double* s = src + (long long)blockIdx.x * n;
  double sum = 0.0, cnt = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = s[i];
    if (x == x) sum += x, cnt += 1.0;
  }
  sum = mt_block_sum(sum, red);
  cnt = mt_block_sum(cnt, red);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double mx = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = s[i];
    if (x == x) mx = fmax(mx, fabs(x - mean));
  }
  mx = mt_block_max(mx, red);
  if (threadIdx.x == 0) {
    stat[4 * blockIdx.x] = cnt;
    stat[4 * blockIdx.x + 1] = mean;
    stat[4 * blockIdx.x + 2] = mx;
  }
}

// Column blockIdx.x of src, centred by stat's mean with its missing entries set to 0, scaled by 2^sexp[col] and rounded, as
// kMtPlanes digits into row (row0 + col) of the planes; the bytes behind n stay as they are (zero).  Leaves per row the exact
// integer sum of the stored values (rowsum_q, in units of 2^-sexp) and the sum of squares of the centred values.
static __global__ __launch_bounds__(256) void mt_quantize_rows_kernel(const double* __restrict__ src, long long n,
                                                                      const double* __restrict__ stat,
                                                                      const int* __restrict__ sexp, int row0,
                                                                      signed char* __restrict__ planes, long long ldk,
                                                                      long long plane_stride, long long* __restrict__ rowsum_q,
                                                                      double* __restrict__ sumsq) {
  __shared__ double redd[4];
  __shared__ long long redl[4];
  const int col = blockIdx.x;
  const double* s = src + (long long)col * n;
  const double mean = stat[4 * col + 1];
  const int e = sexp[col];
  signed char* dst = planes + (long long)(row0 + col) * ldk;
  long long qs = 0;
  double ss = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = s[i];
    const double xc = (x == x) ? x - mean : 0.0;
    const long long q = llrint(ldexp(xc, e));
    signed char d[8];
    rot_digits(q, kMtPlanes, d);
#pragma unroll
    for (int p = 0; p < kMtPlanes; ++p) dst[p * plane_stride + i] = d[p];
    qs += q;
    ss += xc * xc;
  }
  qs = mt_block_sum(qs, redl);
  ss = mt_block_sum(ss, redd);
  if (threadIdx.x == 0) {
    rowsum_q[col] = qs;
    sumsq[col] = ss;
  }
}

// One read of V fp64 columns (column-major, leading dimension ld, n rows): every value is tested for 0 / 1 / 2 (bad[0] is set
// when one is anything else), the int8 copy goes to out8[col * ldk + i] for i < ldk (zero behind n), and isum[2 col], [2 col + 1]
// receive sum g and sum g^2 as exact integers (integer atomics: the same sums in any order).  grid = (V, ceil(ldk /
// kMtPassRows)), 256 threads, four rows per thread and store.
static __global__ __launch_bounds__(256) void mt_geno_pass_kernel(const double* __restrict__ G, long long n, long long ld,
                                                                  signed char* __restrict__ out8, long long ldk,
                                                                  unsigned long long* __restrict__ isum, int* __restrict__ bad) {
  __shared__ unsigned red[4];
  const int col = blockIdx.x;
  const double* g = G + (long long)col * ld;
  unsigned* o = reinterpret_cast<unsigned*>(out8 + (long long)col * ldk);
  const long long i_lo = (long long)blockIdx.y * kMtPassRows;
  const long long i_hi = (i_lo + kMtPassRows < ldk) ? i_lo + kMtPassRows : ldk;
  unsigned s1 = 0, s2 = 0;
  bool notint = false;
  for (long long i = i_lo + 4 * (long long)threadIdx.x; i < i_hi; i += 4 * 256) {  // (ldk is a multiple of 128: whole words)
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double x = (i + k < n) ? g[i + k] : 0.0;
      const bool okv = (x == 0.0) || (x == 1.0) || (x == 2.0);
      notint = notint || !okv;
      const unsigned v = okv ? (unsigned)x : 0u;
      word |= v << (8 * k);
      s1 += v;
      s2 += v * v;
    }
    o[i >> 2] = word;
  }
  s1 = mt_block_sum(s1, red);
  s2 = mt_block_sum(s2, red);
  if (threadIdx.x == 0) {
    if (s1) atomicAdd(&isum[2 * col], (unsigned long long)s1);
    if (s2) atomicAdd(&isum[2 * col + 1], (unsigned long long)s2);
  }
  if (notint) atomicOr(bad, 1);
}

// hard calls: gsum = sum g, gg = |g - mean|^2 = sum g^2 - (sum g)^2 / n from the exact integers (one rounding each)
static __global__ void mt_int_moments_kernel(const unsigned long long* __restrict__ isum, int V, double n, double* __restrict__ gsum,
                                             double* __restrict__ gg) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const double s1 = (double)isum[2 * v], s2 = (double)isum[2 * v + 1];
  gsum[v] = s1;
  gg[v] = s2 - s1 * s1 / n;
}

// anything else: the column's sum and the sum of squares around its mean in two passes (fixed order); grid = V, 256 threads
static __global__ __launch_bounds__(256) void mt_col_moments_kernel(const double* __restrict__ G, long long n, long long ld,
                                                                    double* __restrict__ gsum, double* __restrict__ gg) {
  __shared__ double red[4];
  const double* g = G + (long long)blockIdx.x * ld;
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) s += g[i];
  s = mt_block_sum(s, red);
  const double mean = s / (double)n;
  double q = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const double dlt = g[i] - mean;
    q += dlt * dlt;
  }
  q = mt_block_sum(q, red);
  if (threadIdx.x == 0) {
    gsum[blockIdx.x] = s;
    gg[blockIdx.x] = q;
  }
}

// One thread per (variant, test): u, v, p (V x T row-major each) from GYZ = C1 (resident rows x variants, leading dimension
// ldc1: g'[Yc | Zc] of the UNCENTRED g), nm = C2 (patterns x variants, ldc2), the row sums of the stored [Yc | Zc] (the centring
// term gbar 1'[Yc | Zc]) and the column moments.  The constants of a workgroup's kMtFinTests tests are staged in LDS.
// grid = (ceil(T / kMtFinTests), ceil(V / kMtFinVars)), 256 threads.
// kMean: gsum holds the columns' means themselves (rows of a .bed matrix: mt_bed_site_kernel's mu), not their sums.
template <bool kMean>
static __global__ __launch_bounds__(256) void mt_finish_kernel(const double* __restrict__ C1, long long ldc1,
                                                               const double* __restrict__ C2, long long ldc2,
                                                               const double* __restrict__ rowsum, const double* __restrict__ gsum,
                                                               const double* __restrict__ gg, const MtTest* __restrict__ tests,
                                                               int T, int V, double n, double* __restrict__ u_out,
                                                               double* __restrict__ v_out, double* __restrict__ p_out) {
  static_assert(sizeof(MtTest) % sizeof(double) == 0, "MtTest is copied as doubles");
  __shared__ MtTest sh[kMtFinTests];
  const int t0 = blockIdx.x * kMtFinTests;
  const int nt = (T - t0 < kMtFinTests) ? T - t0 : kMtFinTests;
  {
    const double* src = reinterpret_cast<const double*>(tests + t0);
    double* dst = reinterpret_cast<double*>(sh);
    const int words = nt * (int)(sizeof(MtTest) / sizeof(double));
    for (int w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
  }
  __syncthreads();
  const int tl = threadIdx.x % kMtFinTests, vl = threadIdx.x / kMtFinTests;
  const int v = blockIdx.y * kMtFinVars + vl;
  if (tl >= nt || v >= V) return;
  const MtTest& t = sh[tl];
  const double gbar = kMean ? gsum[v] : gsum[v] / n;
  const double* c1 = C1 + (long long)v * ldc1;
  const double gy = c1[t.y] - gbar * rowsum[t.y];
  double gz[kMtMaxCov];
  for (int a = 0; a < t.ncov; ++a) gz[a] = c1[t.z[a]] - gbar * rowsum[t.z[a]];
  const double nm = C2[(long long)v * ldc2 + t.pattern];
  double u, vv, p;
  mt_cell(n, nm, gy, gz, gg[v], t, &u, &vv, &p);
  const long long o = (long long)v * T + t0 + tl;
  u_out[o] = u;
  v_out[o] = vv;
  p_out[o] = p;
}

// ---- rows of a resident .bed matrix (rvt_mt_score_bed_dev) ---------------------------------------------------------------------------
// Rows pitch = ceil(n / 4) bytes apart (the format: rvt_bed_codes.h).  The column a caller of
// rvt_mt_score_block uploads is exactly g = c + mu m: c = the calls with missing -> 0, m = the missing indicator, mu = the mean of
// the called ones.  c and m are one int8 plane each, so G'[Yc | Zc] and G'indModel are exact integer products of c, plus mu
// times those of m for the rows that have a missing call at all.

// The moments of the imputed column from the counts[4 v ..] = n0 n1 n2 missing of row v: mu[v] = a / called with a = n1 + 2 n2
// and called = n0 + n1 + n2 (bed_site), gg[v] = sum (g - mu)^2 = (n1 + 4 n2) - a a / called (the missing entries sit on the
// mean) — exact integers and one rounding each; with called = n, mt_int_moments_kernel's expressions.  No called sample: mu = 0,
// gg = 0.
static __global__ void mt_bed_site_kernel(const unsigned long long* __restrict__ counts, int V, double* __restrict__ mu,
                                          double* __restrict__ gg) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const long long n1 = (long long)counts[4 * v + 1], n2 = (long long)counts[4 * v + 2];
  const BedSite s = bed_site((long long)counts[4 * v], n1, n2, 0);
  const double s1 = (double)s.ac, s2 = (double)(n1 + 4 * n2), nc = (double)s.called;
  mu[v] = s.mean;
  gg[v] = s.called > 0 ? s2 - s1 * s1 / nc : 0.0;
}

// Row blockIdx.x of the piece -> column blockIdx.x of Bc (the calls, missing -> 0) and, when slot[row] >= 0, column slot[row] of
// Bm (the missing indicator): the one-plane B operands of rvt_planes_gemm, column j at B + j * ldk, sample i at byte i, zero
// from sample n to ldk whatever the padding pairs of the row's last byte hold.  A thread takes 16 samples per step: four bytes
// of codes in (bed_load4 inside the piece [rows, rows + bytes)), one 16-byte store per operand out (ldk is a multiple of 128, the
// operands are 256-byte aligned).  Bytes of a dword that belong to the next row are samples >= n and are masked with the padding
// pairs.  grid = (rows of the piece, ceil(ldk / kMtPassRows)), 256 threads.
static __global__ __launch_bounds__(256) void mt_bed_unpack_kernel(const unsigned char* __restrict__ rows, long long pitch,
                                                                   long long n, long long bytes, const int* __restrict__ slot,
                                                                   signed char* __restrict__ Bc, signed char* __restrict__ Bm,
                                                                   long long ldk) {
  const int col = blockIdx.x;
  const unsigned char* r = rows + (long long)col * pitch;
  const unsigned char* end = rows + bytes;
  const int sl = slot[col];
  uint4* oc = reinterpret_cast<uint4*>(Bc + (long long)col * ldk);
  uint4* om = sl >= 0 ? reinterpret_cast<uint4*>(Bm + (long long)sl * ldk) : nullptr;
  const long long i_lo = (long long)blockIdx.y * kMtPassRows;
  const long long i_hi = (i_lo + kMtPassRows < ldk) ? i_lo + kMtPassRows : ldk;
  for (long long i = i_lo + 16 * (long long)threadIdx.x; i < i_hi; i += 16 * 256) {
    const long long b0 = i >> 2;
    const uint32_t code = b0 < pitch ? bed_load4(r + b0, rows, end) : 0u;
    const long long left = n - i;  // samples of this group that exist (may be <= 0: zeros up to ldk)
    uint32_t cw[4], mw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t live = bed_live_lanes(left - 4 * k);
      const uint32_t lo = bed_spread(code, k) & live, hi = bed_spread(code >> 1, k) & live;
      cw[k] = hi + (hi & lo);
      mw[k] = lo & ~hi;
    }
    oc[i >> 4] = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    if (om) om[i >> 4] = make_uint4(mw[0], mw[1], mw[2], mw[3]);
  }
}

// C = Cc + mu Cm for the rows that have a missing call: column idx[j] of C1 (R rows) and of C2 (K rows) receives
// fma(mu[idx[j]], column j of C1m / C2m, itself).  The columns of the other rows are not touched.  grid = (ceil((R + K) / 256),
// rows with a missing call), 256 threads.
static __global__ __launch_bounds__(256) void mt_bed_combine_kernel(double* __restrict__ C1, const double* __restrict__ C1m,
                                                                    long long ldc1, int R, double* __restrict__ C2,
                                                                    const double* __restrict__ C2m, long long ldc2, int K,
                                                                    const int* __restrict__ idx, const double* __restrict__ mu) {
  const int row = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  const int v = idx[j];
  const double m = mu[v];
  if (row < R) {
    const long long o = (long long)v * ldc1 + row;
    C1[o] = fma(m, C1m[(long long)j * ldc1 + row], C1[o]);
  } else if (row - R < K) {
    const long long o = (long long)v * ldc2 + (row - R);
    C2[o] = fma(m, C2m[(long long)j * ldc2 + (row - R)], C2[o]);
  }
}

}  // namespace rvt
