// rvtests_amd — Price's variable-threshold permutation test (--vt price[nPerm:alpha]; VariableThresholdPrice,
// src/Model.h:1745-1882 over makeVariableThreshodlGenotype / zegginiCollapse, src/Model.cpp:132-148,301-382).
//
// The collapsed genotype at threshold t counts, per sample, the carried variants ((int)g > 0) of the frequency groups
// 0 .. t, so the numerator of z_t under a shuffle pi is
//     B_t . y_pi = sum_{groups u <= t}  sum_{(i, j): j in group u, i carries j}  y[pi(i)]
// — a prefix sum over per-group sums taken over the SPARSE carrier list; the row variance below it does not depend on the
// shuffle.  Per gene, once: the carrier list ordered by group (vtp_count_kernel, vtp_fill_kernel: sample order inside a
// column, columns in group order — the same list whatever context builds it) and the exact integers sum b_t, sum b_t^2
// (vtp_rowstat_kernel).  Per chunk of shuffles: vtp_segsum_kernel (a wave = one segment of the list x 64 shuffles, a lane =
// one shuffle, sums in list order in a register) and vtp_finish_kernel (a thread = one shuffle: segments in order, prefix
// over the groups, 1 / sd_t, max |.|).  No atomics on doubles anywhere: every sum has one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "perm_counter.h"

namespace rvt {

constexpr int kVtpMaxGroups = 1024;  // = RVT_MAX_VARIANTS: a group holds at least one column

// cnt[j] = samples that carry column j of the flipped, polymorphic block: (int)g > 0 (src/Model.cpp:142-145 — a mean-imputed
// value below 1 truncates to 0).  One workgroup per column.
#if !defined(RVT_K_SPLIT) || defined(RVT_K_PERM)
static __global__ __launch_bounds__(256) void vtp_count_kernel(const double* __restrict__ G, long long N, long long ld,
                                                               int* __restrict__ cnt) {
  __shared__ int part[4];
  const double* g = G + (long long)blockIdx.x * ld;
  int n = 0;
  for (long long i = threadIdx.x; i < N; i += 256) n += (int)g[i] > 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
#endif  // RVT_K_PERM

// ent[off[j] + k] = the k-th carrier (ascending sample index) of column j.  One workgroup per column walks it in steps of
// 256 samples; the position of a carrier inside a step comes from the waves' ballots.
#if !defined(RVT_K_SPLIT) || defined(RVT_K_PERM)
static __global__ __launch_bounds__(256) void vtp_fill_kernel(const double* __restrict__ G, long long N, long long ld,
                                                              const long long* __restrict__ off, const int* __restrict__ cnt,
                                                              uint32_t* __restrict__ ent) {
  __shared__ int wcount[4];
  const int j = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* g = G + (long long)j * ld;
  uint32_t* out = ent + off[j];
  const int limit = cnt[j];  // (what vtp_count_kernel saw: nothing is written past it)
  int base = 0;
  for (long long i0 = 0; i0 < N; i0 += 256) {
    const long long i = i0 + threadIdx.x;
    const bool carries = i < N && (int)g[i] > 0;
    const unsigned long long mask = __ballot(carries);
    if (lane == 0) wcount[w] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < 4; ++q) {
      before += q < w ? wcount[q] : 0;
      total += wcount[q];
    }
    const int pos = base + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (carries && pos < limit) out[pos] = (uint32_t)i;
    base += total;
    __syncthreads();
  }
}
#endif  // RVT_K_PERM

// The exact integers behind the row variances.  order: the columns in group order, gend[k] = 1 where column order[k] is the
// last of its group, grp[k] its group.  A thread = one sample; b = its collapsed count so far.  b_t(i) is a step function of
// t, so the thread adds the STEPS (c, b_new^2 - b_old^2) at the groups where it carries something: stat[t] and stat[T + t]
// hold the differences of sum_i b_t and sum_i b_t^2 over t, the host takes the prefix sums.  Integer atomics: exact, any order.
#if !defined(RVT_K_SPLIT) || defined(RVT_K_PERM)
static __global__ __launch_bounds__(256) void vtp_rowstat_kernel(const double* __restrict__ G, long long N, long long ld, int m,
                                                                 const int* __restrict__ order, const int* __restrict__ grp,
                                                                 const int* __restrict__ gend, int T,
                                                                 unsigned long long* __restrict__ stat) {
  __shared__ unsigned long long s[2 * kVtpMaxGroups];
  for (int t = threadIdx.x; t < 2 * T; t += 256) s[t] = 0ull;
  __syncthreads();
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < N) {
    unsigned long long b = 0, c = 0;
    for (int k = 0; k < m; ++k) {
      c += (int)G[(long long)order[k] * ld + i] > 0;
      if (gend[k] && c) {
        const unsigned long long nb = b + c;
        atomicAdd(&s[grp[k]], c);
        atomicAdd(&s[T + grp[k]], nb * nb - b * b);
        b = nb;
        c = 0;
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * T; t += 256)
    if (s[t]) atomicAdd(&stat[t], s[t]);
}
#endif  // RVT_K_PERM

// part[seg * n_shuffles + s] = sum over the entries e of segment seg (in list order) of the phenotype of sample ent[e] under
// shuffle s.  A segment lies inside one frequency group.  grid (segments, ceil(n_shuffles / 64)), one wave per workgroup,
// lane = shuffle: the entry index is uniform over the wave (one scalar load per entry), every lane evaluates ITS permutation
// at that sample and gathers one value from the N-vector, which stays in the L2.
//   kCounter : src = y (N), shuffle = the keyed bijection of (seed, gene, shuffle0 + s)           (perm_counter.h)
//   kMatrix  : src = the chunk's permuted-phenotype matrix (N x B column-major, perm_apply_kernel), column s
//   kIdentity: src = y, no shuffle (the observed statistic; n_shuffles = 1: all 64 lanes form the same sum and lane 0 stores it —
//              once per gene, so the observed value comes from the very code and order the permuted ones come from)
enum VtpSource : int { kVtpCounter = 0, kVtpMatrix = 1, kVtpIdentity = 2 };

#if !defined(RVT_K_SPLIT) || defined(RVT_K_PERM)
template <int SRC>
static __global__ __launch_bounds__(64) void vtp_segsum_kernel(const uint32_t* __restrict__ ent, const int2* __restrict__ segs,
                                                               const double* __restrict__ src, long long N,
                                                               unsigned long long seed, unsigned long long gene,
                                                               unsigned shuffle0, int n_shuffles, double* __restrict__ part) {
  const int seg = blockIdx.x;
  const int s = blockIdx.y * 64 + threadIdx.x;
  const bool active = s < n_shuffles;
  const int sc = active ? s : n_shuffles - 1;  // (idle lanes repeat the last shuffle: every address stays inside)
  const int2 se = segs[seg];
  double acc = 0.0;
  if (SRC == kVtpCounter) {
    const int bits = perm_bits((unsigned long long)N);
    const PermKeys pk = perm_keys(seed, gene, shuffle0 + (unsigned)sc);
#pragma unroll 2
    for (int e = se.x; e < se.y; ++e) acc += src[perm_index(ent[e], (uint32_t)N, bits, pk)];
  } else if (SRC == kVtpMatrix) {
    const double* col = src + (long long)sc * N;
#pragma unroll 4
    for (int e = se.x; e < se.y; ++e) acc += col[ent[e]];
  } else {
    for (int e = se.x; e < se.y; ++e) acc += src[ent[e]];
  }
  if (active) part[(long long)seg * n_shuffles + s] = acc;
}
#endif  // RVT_K_PERM

// zmax[s] = max_t |z_t|, z_t = (sum of the segments of groups 0 .. t  -  shift[t]) / sd[t] (undivided where sd[t] = 0), the
// first maximiser kept: strict >, t = 0 always taken (calculateZ, src/Model.h:1841-1848).  shift[t] = 0 for a centred
// quantitative phenotype; for a 0 / 1 phenotype the segments sum the UNCENTRED values — exact integers, the number of cases
// among the carriers — and shift[t] = mean(y) * sum b_t, so that equal configurations give bit-equal z.
#if !defined(RVT_K_SPLIT) || defined(RVT_K_PERM)
static __global__ void vtp_finish_kernel(const double* __restrict__ part, const int* __restrict__ segoff, int T, int n_shuffles,
                                         const double* __restrict__ sd, const double* __restrict__ shift,
                                         double* __restrict__ zmax, int* __restrict__ topt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_shuffles) return;
  double P = 0.0, best = -999.0;
  int bt = 0;
  for (int t = 0; t < T; ++t) {
    for (int q = segoff[t]; q < segoff[t + 1]; ++q) P += part[(long long)q * n_shuffles + s];
    double z = P - shift[t];
    if (sd[t] != 0.0) z = z / sd[t];
    z = fabs(z);
    if (z > best || t == 0) {
      best = z;
      bt = t;
    }
  }
  zmax[s] = best;
  if (topt) topt[s] = bt;
}
#endif  // RVT_K_PERM

}  // namespace rvt
