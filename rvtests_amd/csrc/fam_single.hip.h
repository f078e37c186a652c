// rvtests_amd — single-variant tests for related samples: famLRT and famGrammarGamma (famScore is rvt_score_block_fam).
//
// famLRT (FastLMM(LRT, MLE), regression/FastLMM.cpp:150-212) fits, per variant, the GLS of uy on [ux | ug] at the null's
// delta, W = 1/(|lambda| + delta).  With the null constants A = ux'W ux, beta* = A^-1 ux'W uy and the W-residual
// r* = uy - ux beta* (formed once per null, SSR* = sum W r*^2 by a reduction over the samples), the alternative fit is
// the Schur complement of the bordered system:
//     s = ug'W ug - b'A^-1 b  (b = ux'W ug),   t = ug'W r*  (= ug'W uy - b'beta*, since ux'W r* = 0),
//     altSSR = SSR* - t^2 / s.
//   fam_lrt_kernel     grid (ceil(V / VT)): every thread holds one sample's ux row, W, r* and u1/|lambda| of a 256-sample tile
//                      in registers and reuses them for the VT variants of its workgroup; per variant it accumulates
//                      ug'W ug, b, t and the GetAF numerator sum u1 ug / |lambda|.  The tile loop, the wave shuffles and the
//                      cross-wave sum have a fixed order, so a variant's numbers do not depend on the block it is in.  Threads
//                      0 .. VT-1 finish one variant each.
//
// famGrammarGamma (GrammarGamma, regression/GrammarGamma.cpp:29-152) needs, per variant, only sums over the RAW genotype:
//   grammar_stream_kernel  grid (V): shifted sums of every column (shift = its first entry) — sum (g - K),
//                      sum (g - K)^2, sum (g - K) ty — kGgUnroll samples' loads in flight per thread; with af=kinship also
//                      sum (lambda + delta) u1 ug over the rotated column.  8 N bytes per variant otherwise.
//   grammar_sums_kernel    the null fit's reductions for one delta (mode 0: ux'(lambda + delta)ux, ux'(lambda + delta)uy,
//                      sum log|lambda + delta|; mode 1: sum (uy - ux beta)^2 / (lambda + delta)), kLmmBlocks partial records.
//   apply_u_kernel     U v from the digit planes of U (rot_gemm.hip.h), the panels outside a sample's family skipped as the
//                      rotation GEMM skips them; sample-parallel, the eigenvector axis cut into slices summed in order.
#pragma once
#include <hip/hip_runtime.h>
#include "rvt_special.h"

namespace rvt_fs {

constexpr int kFsThreads = 256;
constexpr int kGgUnroll = 4;      // samples per thread whose loads the GrammarGamma pass issues together
constexpr int kApplySlices = 32;  // eigenvector slices of apply_u_kernel
constexpr double kRefPi = 3.1415926535897;  // FastLMM.cpp:18, GrammarGamma.cpp:22

struct LrtConsts {
  double n;         // N
  double ssr0;      // SSR* = sum W r*^2
  double sigma2;    // sigma2_g of the null fit (its last evaluation)
  double slog;      // sum log(|lambda| + delta)
  double afden;     // u1' |lambda|^-1 u1 (GetAF's denominator)
  int d;
};

struct GgConsts {
  double n, gamma, ysy, sumty, afden;
};

// sum of x over the 64 lanes of a wave in a fixed butterfly order (the callers add the waves in order through LDS)
__device__ __forceinline__ double fs_wave_sum(double x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// out: VT x (DMAX + 3) LDS sums.  ux: N x d column-major (ld N); vec: [W | r* | u1/|lambda|], leading dimension vld.
template <int DMAX, int VT>
__global__ __launch_bounds__(kFsThreads) void fam_lrt_kernel(const double* __restrict__ Gt, long long ld, long long N, int V,
                                                             const double* __restrict__ ux, const double* __restrict__ vec,
                                                             long long vld, const double* __restrict__ Ainv,
                                                             const int* __restrict__ poly, LrtConsts k, int* __restrict__ ok,
                                                             double* __restrict__ af, double* __restrict__ null_ll,
                                                             double* __restrict__ alt_ll, double* __restrict__ pval) {
  constexpr int Q = DMAX + 3;  // [gg, t, afnum, b_0 .. b_{d-1}]
  __shared__ double red[kFsThreads / 64][VT * Q];
  __shared__ double sums[VT * Q];
  const int d = k.d;
  const int h0 = blockIdx.x * VT;
  const double* W = vec;
  const double* R = vec + vld;
  const double* U1 = vec + 2 * vld;
  double acc[VT][Q];
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[v][q] = 0.0;
  for (long long i = threadIdx.x; i < N; i += kFsThreads) {
    const double w = W[i], r = R[i], u = U1[i];
    double x[DMAX];
#pragma unroll
    for (int a = 0; a < DMAX; ++a) x[a] = a < d ? ux[i + a * N] : 0.0;
#pragma unroll
    for (int v = 0; v < VT; ++v) {
      const int h = h0 + v;
      const double g = h < V ? Gt[i + (long long)h * ld] : 0.0;
      const double wg = w * g;
      acc[v][0] = fma(wg, g, acc[v][0]);
      acc[v][1] = fma(wg, r, acc[v][1]);
      acc[v][2] = fma(u, g, acc[v][2]);
#pragma unroll
      for (int a = 0; a < DMAX; ++a) acc[v][3 + a] = fma(wg, x[a], acc[v][3 + a]);
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const double s = fs_wave_sum(acc[v][q]);
      if (lane == 0) red[wave][v * Q + q] = s;
    }
  __syncthreads();
  for (int e = threadIdx.x; e < VT * Q; e += kFsThreads) {
    double s = 0.0;
    for (int w = 0; w < kFsThreads / 64; ++w) s += red[w][e];
    sums[e] = s;
  }
  __syncthreads();
  if (threadIdx.x >= VT) return;
  const int h = h0 + threadIdx.x;
  if (h >= V) return;
  const double* S = sums + threadIdx.x * Q;
  const double sgg = S[0], t = S[1];
  af[h] = k.afden == 0.0 ? 0.0 : 0.5 * S[2] / k.afden;  // GetAFFromUg (FastLMM.cpp:372-400: 0 when denom == 0)
  null_ll[h] = -0.5 * (k.n * log(2.0 * kRefPi) + k.slog + k.n + k.n * log(k.sigma2));
  if (!poly[h]) {
    ok[h] = 0;
    alt_ll[h] = pval[h] = NAN;
    return;
  }
  double bAb = 0.0;
  for (int a = 0; a < d; ++a) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += Ainv[a * d + c] * S[3 + c];
    bAb += S[3 + a] * s;
  }
  const double s = sgg - bAb;
  if (!(sgg > 0.0) || !(s > 1e-12 * sgg)) {  // g in the span of X: reported as a failed fit
    ok[h] = -1;
    alt_ll[h] = pval[h] = NAN;
    return;
  }
  const double alt_s2 = (k.ssr0 - t * t / s) / k.n;
  alt_ll[h] = -0.5 * (k.n * log(2.0 * kRefPi) + k.slog + k.n + k.n * log(alt_s2));
  const double stat = k.n * log(k.sigma2 / alt_s2);  // = 2 (AltLogLik - NullLogLik)
  pval[h] = rvt::chisq_Q(stat, 1.0);
  ok[h] = 1;
}

// GrammarGamma::TestCovariate (GrammarGamma.cpp:122-152): one workgroup per raw column.  KIN = false: af=mean (Gt, wu1 unused).  Every
// thread issues the loads of kGgUnroll samples (column and ty) before it adds them, so that enough loads are in flight to
// stream the column; the summation order depends on N only.
template <bool KIN>
__global__ __launch_bounds__(kFsThreads) void grammar_stream_kernel(const double* __restrict__ G, long long ld, long long N,
                                                                    int V, const double* __restrict__ ty,
                                                                    const double* __restrict__ Gt,
                                                                    const double* __restrict__ wu1, GgConsts k,
                                                                    int* __restrict__ ok, double* __restrict__ af,
                                                                    double* __restrict__ beta, double* __restrict__ beta_var,
                                                                    double* __restrict__ pval) {
  constexpr int Q = 4;  // sum (g-K), sum (g-K)^2, sum (g-K) ty, sum wu1 ug
  constexpr int R = kGgUnroll;
  __shared__ double red[kFsThreads / 64][Q];
  __shared__ double sums[Q];
  const int h = blockIdx.x;
  if (h >= V) return;
  const double* col = G + (long long)h * ld;
  const double* colt = KIN ? Gt + (long long)h * ld : nullptr;
  constexpr bool kin = KIN;
  const double K = col[0];
  double acc[Q] = {0.0, 0.0, 0.0, 0.0};
  long long i = threadIdx.x;
  for (; i + (R - 1) * (long long)kFsThreads < N; i += R * (long long)kFsThreads) {
    double x[R], t[R], gt[R], wu[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      x[u] = col[i + u * kFsThreads];
      t[u] = ty[i + u * kFsThreads];
      if (kin) {
        gt[u] = colt[i + u * kFsThreads];
        wu[u] = wu1[i + u * kFsThreads];
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const double xc = x[u] - K;
      acc[0] += xc;
      acc[1] = fma(xc, xc, acc[1]);
      acc[2] = fma(xc, t[u], acc[2]);
      if (kin) acc[3] = fma(wu[u], gt[u], acc[3]);
    }
  }
  for (; i < N; i += kFsThreads) {
    const double xc = col[i] - K;
    acc[0] += xc;
    acc[1] = fma(xc, xc, acc[1]);
    acc[2] = fma(xc, ty[i], acc[2]);
    if (kin) acc[3] = fma(wu1[i], colt[i], acc[3]);
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const double s = fs_wave_sum(acc[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < Q) {
    double s = 0.0;
    for (int w = 0; w < kFsThreads / 64; ++w) s += red[w][threadIdx.x];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double* S = sums;
  const double mk = S[0] / k.n;                 // mean - K
  const double gg = S[1] - S[0] * mk;           // centred g'g
  const double gty = S[2] - mk * k.sumty;       // (g - mean)' ty
  // af=kinship: (x'x)^-1 x'y of GetAF (GrammarGamma.cpp:199-213), a plain division as there (x'x = 0: inf or NaN)
  af[h] = kin ? 0.5 * S[3] / k.afden : 0.5 * (K + mk);
  if (!(S[1] > 0.0)) {  // every entry equals the first: monomorphic
    ok[h] = 0;
    beta[h] = beta_var[h] = pval[h] = NAN;
    return;
  }
  beta[h] = gty / gg / k.gamma;
  beta_var[h] = k.ysy / gg / k.gamma;
  pval[h] = rvt::chisq_Q(gty * gty / gg / k.gamma, 1.0);
  ok[h] = 1;
}

// mode 0: record [A (d x d row-major) | b (d) | slog] with weights (lam + delta) (GrammarGamma.cpp:167-171: it multiplies by
// sqrt(lambda + delta)); mode 1: record [sum (uy - ux beta)^2 / (lam + delta)].  uxy: N x (d+1), ld N.
__global__ __launch_bounds__(kFsThreads) void grammar_sums_kernel(const double* __restrict__ uxy, const double* __restrict__ lam,
                                                                  long long N, int d, double delta, int mode,
                                                                  const double* __restrict__ beta,
                                                                  double* __restrict__ partial) {
  __shared__ double sm[kFsThreads];
  const int rec = mode == 0 ? d * d + d + 1 : 1;
  double* out = partial + (long long)blockIdx.x * rec;
  for (int q = 0; q < rec; ++q) {
    int a = 0, b = 0, kind;
    if (mode == 1) {
      kind = 3;
    } else if (q < d * d) {
      kind = 0;
      a = q / d;
      b = q % d;
    } else if (q < d * d + d) {
      kind = 1;
      a = q - d * d;
    } else {
      kind = 2;
    }
    double s = 0.0;
    for (long long i = blockIdx.x * (long long)kFsThreads + threadIdx.x; i < N; i += (long long)kFsThreads * gridDim.x) {
      const double w = lam[i] + delta;
      double v;
      if (kind == 0)
        v = uxy[i + a * N] * w * uxy[i + b * N];
      else if (kind == 1)
        v = uxy[i + a * N] * w * uxy[i + (long long)d * N];
      else if (kind == 2)
        v = log(fabs(w));
      else {
        double r = uxy[i + (long long)d * N];
        for (int c = 0; c < d; ++c) r -= uxy[i + c * N] * beta[c];
        v = r * r / w;
      }
      s += v;
    }
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int off = kFsThreads / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = sm[0];
    __syncthreads();
  }
}

// Null vectors of famLRT: vec = [W | r* | u1/|lambda|] (leading dimension vld), W = 1/(absS + delta), r* = uy - ux beta*.
__global__ void fam_lrt_null_kernel(const double* __restrict__ uxy, const double* __restrict__ absS,
                                    const double* __restrict__ u1, long long N, int d, double delta,
                                    const double* __restrict__ beta, double* __restrict__ vec, long long vld) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= N) return;
  double r = uxy[i + (long long)d * N];
  for (int c = 0; c < d; ++c) r -= uxy[i + c * N] * beta[c];
  vec[i] = 1.0 / (absS[i] + delta);
  vec[i + vld] = r;
  vec[i + 2 * vld] = u1[i] / absS[i];
}

// out[i] = v[i] * scale / (S[i] + delta)  (raw S: GrammarGamma.cpp:110-112) and wu1[i] = (S[i] + delta) u1[i]
__global__ void grammar_scale_kernel(const double* __restrict__ S, const double* __restrict__ u1, long long N, double delta,
                                     double scale, double* __restrict__ v, double* __restrict__ wu1) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double t = S[i] + delta;
  v[i] = v[i] * scale / t;
  wu1[i] = t * u1[i];
}

// part[s * ldp + i] = sum over the eigenvectors k of slice s: U[i, k] v[k], from the digit planes: plane p holds, at
// k * ldk + i, digit p of round(U[i, k] 2^sexp).  range (may be null): per 256-row panel of the planes, the K chunks
// (kRotKC samples) that hold its non-zeros; a panel whose chunks miss sample i contributes nothing and is not read.
__global__ __launch_bounds__(kFsThreads) void apply_u_kernel(const signed char* __restrict__ Uq, long long plane, int planes,
                                                             long long ldk, const int2* __restrict__ range, int panel_rows,
                                                             int chunk, long long N, long long npanels,
                                                             const double* __restrict__ v, double* __restrict__ part,
                                                             long long ldp) {
  const long long i = blockIdx.x * (long long)kFsThreads + threadIdx.x;
  const int s = blockIdx.y, ns = gridDim.y;
  const long long p0 = npanels * s / ns, p1 = npanels * (s + 1) / ns;
  double acc = 0.0;
  if (i < N) {
    const int ci = (int)(i / chunk);
    for (long long rp = p0; rp < p1; ++rp) {
      if (range) {
        const int2 r = range[rp];
        if (ci < r.x || ci >= r.y) continue;
      }
      const long long k1 = min((rp + 1) * (long long)panel_rows, N);
      for (long long k = rp * (long long)panel_rows; k < k1; ++k) {
        long long q = 0;
        for (int p = planes - 1; p >= 0; --p) q = q * 128 + (long long)Uq[p * plane + k * ldk + i];
        acc = fma((double)q, v[k], acc);
      }
    }
  }
  if (i < N) part[s * ldp + i] = acc;
}

// out[i] = sum over the non-zeros e of row i of a sparse U (row-compressed, columns ascending): vals[e] * v[cols[e]]
__global__ __launch_bounds__(256) void apply_u_sparse_kernel(const long long* __restrict__ ptr, const int* __restrict__ cols,
                                                             const double* __restrict__ vals, long long N,
                                                             const double* __restrict__ v, double* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= N) return;
  double s = 0.0;
  for (long long e = ptr[i]; e < ptr[i + 1]; ++e) s = fma(vals[e], v[cols[e]], s);
  out[i] = s;
}

// out[i] = 2^-sexp * sum over the slices in order of part[s * ldp + i]
__global__ void apply_u_reduce_kernel(const double* __restrict__ part, long long ldp, int slices, long long N, int sexp,
                                      double* __restrict__ out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= N) return;
  double s = 0.0;
  for (int k = 0; k < slices; ++k) s += part[k * ldp + i];
  out[i] = ldexp(s, -sexp);
}

}  // namespace rvt_fs
