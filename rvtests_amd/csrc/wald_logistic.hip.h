// rvtests_amd — SingleVariantWaldTest for a binary trait: one logistic regression per variant, batched.
//
// Every variant h of a batch replays LogisticRegression::FitLogisticModel(A, y, 100) (regression/LogisticRegression.cpp:279-336)
// on A = [1, g_h, X_1 .. X_{d-1}] (the reference's copyGenotypeWithCovariateAndIntercept order, src/ModelUtil.h:70-96), P = d + 1
// parameters:
//   beta = 0; per round: p = 1 / (1 + exp(-A beta)), v = p (1 - p), D = A'VA, step = D^-1 A'(y - p), beta += step;
//   deviance = -2 sum [y log p + (1 - y) log(1 - p)] on the p of the round (before the update), non-finite terms dropped
//   (safeSum, regression/EigenMatrixInterface.cpp:138-150); converged when rounds > 1 and |deviance change| < 1e-3; failed on a
//   deviance that is not FP_NORMAL or after 100 rounds; covB = D^-1 of the last executed round.
// Difference: a D that is not positive definite ends the fit as failed (Eigen's LLT does not report it; the reference goes on
// with whatever its solve returned).
//
// The variants advance in lockstep, one pair of launches per round:
//   wald_logistic_round_kernel   grid (slices of kWaldSlice active variants, sample chunks of kWaldChunk): the workgroup holds the
//                                X rows of a 256-sample tile in LDS once and reuses them for every variant of its slice; each thread
//                                forms p, v, y - p and the log-likelihood term of one sample, then every thread sums ONE entry of
//                                [Gram upper triangle | gradient | log-likelihood] ((P + 1)(P + 2) / 2 entries) over a fixed
//                                subset of the tile; the subsets are added in a fixed order at the end of the chunk
//   wald_logistic_step_kernel    one thread per active variant: the chunk partials in chunk order (bit-reproducible: the chunk
//                                length is a constant, so a variant's sums do not depend on the batch it is in), Cholesky in
//                                registers, update, round state, and the next list of active variants (converged and failed
//                                variants leave it, so they cost nothing in later rounds)
// The work space is allocated once per context (rvt_wald_block); nothing is allocated inside the round loop.
#pragma once
#include <hip/hip_runtime.h>
#include "rvt_special.h"

namespace rvt_wald {

constexpr int kWaldMaxP = RVT_MAX_COV + 1;                     // parameters: intercept, g, up to 15 covariates
constexpr int kWaldMaxE = (kWaldMaxP + 1) * (kWaldMaxP + 2) / 2;  // Gram upper triangle + gradient + log-likelihood
constexpr int kWaldSlice = 8;                                  // variants per workgroup of the round kernel
constexpr int kWaldTile = 256;                                 // samples per LDS tile (one per thread)
constexpr int kWaldLds = kWaldTile + 1;                        // LDS row stride (doubles): rows fall into different banks
constexpr long long kWaldChunk = 32LL * kWaldTile;             // samples per chunk partial
constexpr int kWaldRounds = 100;                               // FitLogisticModel(X, y, 100)

static inline __host__ __device__ int wald_entries(int P) { return (P + 1) * (P + 2) / 2; }

// entry e of the enumeration a <= b over 0..P (index P stands for the right-hand side): LDS rows of its three factors
// (rows: X_0 .. X_{d-1} | g | v | y - p | loglik | ones)
static __device__ __forceinline__ void wald_entry_rows(int e, int d, int* r1, int* r2, int* r3) {
  const int P = d + 1;
  int a = 0, b = 0, k = 0;
  for (a = 0; a <= P; ++a) {
    const int n = P + 1 - a;
    if (e < k + n) {
      b = a + (e - k);
      break;
    }
    k += n;
  }
  auto row = [d](int j) { return j == 0 ? 0 : (j == 1 ? d : j - 1); };
  const int rv = d + 1, rr = d + 2, rl = d + 3, r1s = d + 4;
  if (b < P) {  // Gram: A_a A_b v
    *r1 = row(a);
    *r2 = row(b);
    *r3 = rv;
  } else if (a < P) {  // gradient: A_a (y - p)
    *r1 = row(a);
    *r2 = rr;
    *r3 = r1s;
  } else {  // log-likelihood
    *r1 = rl;
    *r2 = r1s;
    *r3 = r1s;
  }
}

// Per batch variant h (grid = variants, 256 threads): isMonomorphicMarker (src/DataConsolidator.cpp:94-116: every non-missing
// value equals the first), the start of the fit (beta = 0) and the first list of active variants.  Monomorphic variants are
// finished here: ok = 0, rounds = 0, outputs 0 / 0 / 1.
static __global__ __launch_bounds__(256) void wald_logistic_init_kernel(const double* __restrict__ dG, long long ld, int col0,
                                                                        long long N, int d, double* __restrict__ beta,
                                                                        double* __restrict__ last_dev, int* __restrict__ iter,
                                                                        int* __restrict__ list, int* __restrict__ count,
                                                                        int* __restrict__ ok, int* __restrict__ rounds,
                                                                        double* __restrict__ ob, double* __restrict__ os,
                                                                        double* __restrict__ op) {
  __shared__ double smn[256], smx[256];
  const int h = blockIdx.x, t = threadIdx.x;
  const double* g = dG + (long long)(col0 + h) * ld;
  double mn = INFINITY, mx = -INFINITY;
  for (long long i = t; i < N; i += 256) {
    const double x = g[i];
    if (x >= 0.0) {
      mn = fmin(mn, x);
      mx = fmax(mx, x);
    }
  }
  smn[t] = mn;
  smx[t] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      smn[t] = fmin(smn[t], smn[t + s]);
      smx[t] = fmax(smx[t], smx[t + s]);
    }
    __syncthreads();
  }
  if (t < kWaldMaxP) beta[(long long)h * kWaldMaxP + t] = 0.0;
  if (t < d) {
    ob[(long long)h * d + t] = 0.0;
    os[(long long)h * d + t] = 0.0;
    op[(long long)h * d + t] = 1.0;
  }
  if (t == 0) {
    const bool mono = !(smn[0] < smx[0]);  // (also: no non-missing value at all)
    last_dev[h] = -99999.0;
    iter[h] = 0;
    rounds[h] = 0;
    ok[h] = mono ? 0 : -1;  // (-1 until the fit ends)
    if (!mono) list[atomicAdd(count, 1)] = h;
  }
}

// dynamic LDS of wald_logistic_round_kernel: 21 KB at d = 4, 46 KB at d = 16 (d = 4: the registers, not the LDS, cap it at four
// workgroups per CU)
static inline size_t wald_round_lds_bytes(int d) {
  return sizeof(double) * ((size_t)(d + 5) * kWaldLds + kWaldTile + (size_t)kWaldSlice * kWaldMaxP) + sizeof(int) * kWaldSlice;
}

// One IRLS round of the active variants list[0 .. n_active): grid (ceil(n_active / kWaldSlice), n_chunks), 256 threads.
// part[(q * n_chunks + chunk) * E + e]: entry e of active position q summed over the chunk's samples.
static __global__ __launch_bounds__(256) void wald_logistic_round_kernel(
    const double* __restrict__ dG, long long ld, int col0, const double* __restrict__ X, const double* __restrict__ y, long long N,
    int d, const int* __restrict__ list, int n_active, const double* __restrict__ beta, int n_chunks, double* __restrict__ part) {
  // LDS sized by d (wald_round_lds_bytes): rows X_0 .. X_{d-1} | g | v | y - p | loglik | ones, then the reduction buffer,
  // the slice's estimates and variant indices
  extern __shared__ double wald_lds[];
  double* sx = wald_lds;
  double* sred = sx + (d + 5) * kWaldLds;
  double* sbeta = sred + kWaldTile;
  int* svar = reinterpret_cast<int*>(sbeta + kWaldSlice * kWaldMaxP);
  const int P = d + 1, E = wald_entries(P), G = kWaldTile / E;
  const int t = threadIdx.x;
  const int pos0 = blockIdx.x * kWaldSlice;
  const int ns = min(kWaldSlice, n_active - pos0);
  const int chunk = blockIdx.y;
  if (t < kWaldSlice * kWaldMaxP) {
    const int vv = t / kWaldMaxP, a = t % kWaldMaxP;
    sbeta[t] = (vv < ns && a < P) ? beta[(long long)list[pos0 + vv] * kWaldMaxP + a] : 0.0;
  }
  if (t < kWaldSlice) svar[t] = t < ns ? list[pos0 + t] : 0;
  sx[(d + 4) * kWaldLds + t] = 1.0;
  const int e = t % E, grp = t / E;
  const bool acc_on = grp < G;
  int r1 = 0, r2 = 0, r3 = 0;
  if (acc_on) wald_entry_rows(e, d, &r1, &r2, &r3);
  const double* s1 = sx + r1 * kWaldLds;
  const double* s2 = sx + r2 * kWaldLds;
  const double* s3 = sx + r3 * kWaldLds;
  double acc[kWaldSlice];
#pragma unroll
  for (int vv = 0; vv < kWaldSlice; ++vv) acc[vv] = 0.0;
  const long long i_begin = (long long)chunk * kWaldChunk;
  const long long i_end = min(N, i_begin + kWaldChunk);
  for (long long i0 = i_begin; i0 < i_end; i0 += kWaldTile) {
    const long long i = i0 + t;
    const bool in = i < i_end;
    __syncthreads();  // (the previous tile's readers are done)
    for (int k = 0; k < d; ++k) sx[k * kWaldLds + t] = in ? X[(long long)k * ld + i] : 0.0;
    const double yi = in ? y[i] : 0.0;
#pragma unroll
    for (int vv = 0; vv < kWaldSlice; ++vv) {
      if (vv < ns) {
        const double* b = sbeta + vv * kWaldMaxP;
        const double g = in ? dG[(long long)(col0 + svar[vv]) * ld + i] : 0.0;
        // A beta in the column order of A: 1, g, X_1 ..
        double eta = sx[t] * b[0];
        eta += g * b[1];
        for (int k = 1; k < d; ++k) eta += sx[k * kWaldLds + t] * b[k + 1];
        const double p = 1.0 / (1.0 + exp(-eta));
        double v = p * (1.0 - p), r = yi - p;
        double l = yi * log(p) + (1.0 - yi) * log(1.0 - p);
        if (!in) v = r = 0.0;
        if (!in || !isfinite(l)) l = 0.0;  // safeSum
        sx[d * kWaldLds + t] = g;
        sx[(d + 1) * kWaldLds + t] = v;
        sx[(d + 2) * kWaldLds + t] = r;
        sx[(d + 3) * kWaldLds + t] = l;
        __syncthreads();
        if (acc_on) {
          double a = acc[vv];
          for (int j = grp; j < kWaldTile; j += G) a += s1[j] * s2[j] * s3[j];
          acc[vv] = a;
        }
        __syncthreads();
      }
    }
  }
#pragma unroll
  for (int vv = 0; vv < kWaldSlice; ++vv) {
    if (vv < ns) {
      __syncthreads();
      if (acc_on) sred[grp * E + e] = acc[vv];
      __syncthreads();
      if (t < E) {
        double s = 0.0;
        for (int q = 0; q < G; ++q) s += sred[q * E + t];
        part[((long long)(pos0 + vv) * n_chunks + chunk) * E + t] = s;
      }
    }
  }
}

// The step of every active variant (one thread each): sums, Cholesky of D, beta update, convergence, outputs.
static __global__ __launch_bounds__(64) void wald_logistic_step_kernel(const int* __restrict__ list, int n_active, int d,
                                                                       int n_chunks, const double* __restrict__ part,
                                                                       double* __restrict__ beta, double* __restrict__ last_dev,
                                                                       int* __restrict__ iter, int* __restrict__ next_list,
                                                                       int* __restrict__ next_count, int* __restrict__ ok,
                                                                       int* __restrict__ rounds, double* __restrict__ ob,
                                                                       double* __restrict__ os, double* __restrict__ op) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_active) return;
  const int h = list[q];
  const int P = d + 1, E = wald_entries(P);
  double L[kWaldMaxP * kWaldMaxP], rhs[kWaldMaxP], ll = 0.0;
  // sums in chunk order, straight into D (lower triangle of L, row-major P x P) and the right-hand side
  {
    int e = 0;
    for (int a = 0; a <= P; ++a)
      for (int b = a; b <= P; ++b, ++e) {
        const double* src = part + (long long)q * n_chunks * E + e;
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += src[(long long)c * E];
        if (b < P)
          L[b * kWaldMaxP + a] = s;
        else if (a < P)
          rhs[a] = s;
        else
          ll = s;
      }
  }
  const int it = iter[h];
  bool pd = true;
  for (int j = 0; j < P && pd; ++j) {
    double s = L[j * kWaldMaxP + j];
    for (int k = 0; k < j; ++k) s -= L[j * kWaldMaxP + k] * L[j * kWaldMaxP + k];
    if (!(s > 0.0) || !isfinite(s)) {
      pd = false;
      break;
    }
    const double ljj = sqrt(s);
    L[j * kWaldMaxP + j] = ljj;
    for (int i = j + 1; i < P; ++i) {
      double x = L[i * kWaldMaxP + j];
      for (int k = 0; k < j; ++k) x -= L[i * kWaldMaxP + k] * L[j * kWaldMaxP + k];
      L[i * kWaldMaxP + j] = x / ljj;
    }
  }
  auto finish = [&](int status, int nr) {
    ok[h] = status;
    rounds[h] = nr;
  };
  if (!pd) {
    finish(-1, it + 1);
    return;
  }
  // step = D^-1 rhs: L z = rhs, L' step = z
  double z[kWaldMaxP];
  for (int i = 0; i < P; ++i) {
    double x = rhs[i];
    for (int k = 0; k < i; ++k) x -= L[i * kWaldMaxP + k] * z[k];
    z[i] = x / L[i * kWaldMaxP + i];
  }
  for (int i = P - 1; i >= 0; --i) {
    double x = z[i];
    for (int k = i + 1; k < P; ++k) x -= L[k * kWaldMaxP + i] * z[k];
    z[i] = x / L[i * kWaldMaxP + i];
  }
  double* bh = beta + (long long)h * kWaldMaxP;
  for (int a = 0; a < P; ++a) bh[a] += z[a];
  const double dev = -2.0 * ll;
  if (it > 1 && fabs(dev - last_dev[h]) < 1e-3) {
    // converged: covB = D^-1; its diagonal from the columns of L^-1, (D^-1)_kk = sum_i (L^-1)_ik^2
    for (int a = 1; a < P; ++a) {
      double w[kWaldMaxP], s = 0.0;
      for (int i = 0; i < P; ++i) {
        if (i < a) {
          w[i] = 0.0;
          continue;
        }
        double x = (i == a) ? 1.0 : 0.0;
        for (int k = a; k < i; ++k) x -= L[i * kWaldMaxP + k] * w[k];
        w[i] = x / L[i * kWaldMaxP + i];
        s += w[i] * w[i];
      }
      const double b = bh[a];
      ob[(long long)h * d + a - 1] = b;
      os[(long long)h * d + a - 1] = sqrt(s);
      op[(long long)h * d + a - 1] = chisq_Q(b * b / s, 1.0);
    }
    finish(1, it + 1);
    return;
  }
  if (!isfinite(dev) || fabs(dev) < 2.2250738585072014e-308) {  // fpclassify(dev) != FP_NORMAL
    finish(-1, it + 1);
    return;
  }
  last_dev[h] = dev;
  if (it + 1 == kWaldRounds) {
    finish(-1, kWaldRounds);
    return;
  }
  iter[h] = it + 1;
  next_list[atomicAdd(next_count, 1)] = h;
}

}  // namespace rvt_wald
