// rvtests_amd — the dominant / recessive recoding of `--meta dominant` / `--meta recessive`
// (DataConsolidator::codeGenotypeForDominantModel / ...RecessiveModel, src/DataConsolidator.cpp:390-472): one column of raw
// calls x becomes
//     x < 0 (missing)  ->  avg = carriers / nonmissing of the column (0 when nothing is called)
//     x > threshold    ->  1        (threshold 0.5 dominant, 1.5 recessive)
//     otherwise        ->  0        (NaN and -0.0 are NOT missing and code to 0; exactly the threshold codes to 0)
// Two streaming passes, both bound by HBM: a count pass (integers only, so the counts — and the one division the host makes
// of them — are the same numbers in every run) and a write pass.  fp64 columns of a device block: 8 N bytes read by the count
// pass, 8 N read + 8 N written by the write pass (24 N per column; the second read of a 4 MB column is expected to come out
// of L2 / Infinity Cache).  Rows of a resident .bed matrix: N/4 bytes read twice, 8 N written.
// Included by rvt_meta.hip (the unit of rvt_block_upload_columns).
#pragma once
#include <hip/hip_runtime.h>
#include "rvt_bed_codes.h"

namespace rvt {

constexpr int kRecodeThreads = 256;
// blocks of a launch: memory-bound passes are capped at about 2 048 workgroups and stride over the rest
constexpr int kRecodeMaxBlocks = 2048;

// row slices (gridDim.x) of a launch over `cols` columns whose rows are `units` units of work per column
static inline unsigned recode_slices(long long units, int cols) {
  long long want = (units + kRecodeThreads - 1) / kRecodeThreads;
  const long long cap = kRecodeMaxBlocks / (cols < 1 ? 1 : cols);
  if (want > cap) want = cap;
  return (unsigned)(want < 1 ? 1 : want);
}

// sum of `v` over the workgroup's 256 threads (four waves of 64); valid in thread 0
template <int K>
__device__ __forceinline__ void recode_block_sum(int (&v)[K], int (&out)[K]) {
  __shared__ int red[kRecodeThreads / 64][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int a = v[k];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if (lane == 0) red[wave][k] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// counts[col][0] += non-missing calls, counts[col][1] += carriers of column (col0 + col) of G.  grid (row slices, columns),
// 256 threads; a lane reads 16 bytes per step, the odd last row is one scalar read.  counts must be zero before the launch.
__global__ __launch_bounds__(kRecodeThreads) void recode_count_kernel(const double* __restrict__ G, long long N, long long ld,
                                                                      double threshold, unsigned long long* __restrict__ counts) {
  const double* g = G + (long long)blockIdx.y * ld;
  const long long pairs = N >> 1;
  int v[2] = {0, 0};
  for (long long p = (long long)blockIdx.x * kRecodeThreads + threadIdx.x; p < pairs; p += (long long)gridDim.x * kRecodeThreads) {
    const double2 x = *reinterpret_cast<const double2*>(g + 2 * p);
    const bool c0 = !(x.x < 0.0), c1 = !(x.y < 0.0);
    v[0] += (int)c0 + (int)c1;
    v[1] += (int)(c0 && x.x > threshold) + (int)(c1 && x.y > threshold);
  }
  if ((N & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double x = g[N - 1];
    const bool c = !(x < 0.0);
    v[0] += (int)c;
    v[1] += (int)(c && x > threshold);
  }
  int s[2];
  recode_block_sum<2>(v, s);
  if (threadIdx.x == 0) {
    if (s[0]) atomicAdd(counts + 2 * (long long)blockIdx.y, (unsigned long long)s[0]);
    if (s[1]) atomicAdd(counts + 2 * (long long)blockIdx.y + 1, (unsigned long long)s[1]);
  }
}

// column j of dst = the recoding of column j of src with avg[j] where the call is missing; rows [N, ld) stay as they were.
// Same tiling as the count pass.  Correct in place (src == dst, same column): every lane reads its own elements before it
// writes them, and no other lane touches them.
__global__ __launch_bounds__(kRecodeThreads) void recode_write_kernel(const double* src, double* dst, long long N, long long ld,
                                                                      double threshold, const double* __restrict__ avg) {
  const double* s = src + (long long)blockIdx.y * ld;
  double* d = dst + (long long)blockIdx.y * ld;
  const double a = avg[blockIdx.y];
  const long long pairs = N >> 1;
  for (long long p = (long long)blockIdx.x * kRecodeThreads + threadIdx.x; p < pairs; p += (long long)gridDim.x * kRecodeThreads) {
    const double2 x = *reinterpret_cast<const double2*>(s + 2 * p);
    double2 r;
    r.x = x.x < 0.0 ? a : (x.x > threshold ? 1.0 : 0.0);
    r.y = x.y < 0.0 ? a : (x.y > threshold ? 1.0 : 0.0);
    *reinterpret_cast<double2*>(d + 2 * p) = r;
  }
  if ((N & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double x = s[N - 1];
    d[N - 1] = x < 0.0 ? a : (x > threshold ? 1.0 : 0.0);
  }
}

// ---- rows of a resident .bed matrix, cb = ceil(N / 4) bytes apart (the format: rvt_bed_codes.h) -----------------------------------
// counts[row][0..3] += calls of 0 / 1 / 2 / missing of row blockIdx.y, from the codes by population counts: a lane takes four
// bytes (16 samples) per step; the bits of the last byte beyond sample N - 1 are masked out.  counts must be zero before.
__global__ __launch_bounds__(kRecodeThreads) void recode_bed_count_kernel(const unsigned char* __restrict__ rows, long long cb,
                                                                          long long N, unsigned long long* __restrict__ counts) {
  const unsigned char* r = rows + (long long)blockIdx.y * cb;
  const long long words = (cb + 3) >> 2;
  int v[4] = {0, 0, 0, 0};
  for (long long w = (long long)blockIdx.x * kRecodeThreads + threadIdx.x; w < words; w += (long long)gridDim.x * kRecodeThreads) {
    const long long b0 = 4 * w;
    unsigned code = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (b0 + e < cb) code |= (unsigned)r[b0 + e] << (8 * e);
    bed_counts16(code, bed_live_pairs(N - 4 * b0), v);  // (the samples of this word that exist: 16 from sample 4 b0 on)
  }
  int s[4];
  recode_block_sum<4>(v, s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k]) atomicAdd(counts + 4 * (long long)blockIdx.y + k, (unsigned long long)s[k]);
  }
}

// column blockIdx.y of G = the recoding of row blockIdx.y: four samples (one byte) per thread and step, two 16-byte stores, the
// last N mod 4 samples one by one.  two_only: recessive (only the code of 2 is a carrier), else dominant (1 and 2 are).
__global__ __launch_bounds__(kRecodeThreads) void recode_bed_expand_kernel(const unsigned char* __restrict__ rows, long long cb,
                                                                           long long N, long long ld, int two_only,
                                                                           const double* __restrict__ avg, double* __restrict__ G) {
  const unsigned char* r = rows + (long long)blockIdx.y * cb;
  double* g = G + (long long)blockIdx.y * ld;
  const double a = avg[blockIdx.y];
  for (long long b = (long long)blockIdx.x * kRecodeThreads + threadIdx.x; b < cb; b += (long long)gridDim.x * kRecodeThreads) {
    const unsigned code = r[b];
    const long long i = 4 * b;
    double v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned q = (code >> (2 * e)) & 3u;
      v[e] = q == 1u ? a : (q == 3u ? 1.0 : (q == 2u && !two_only ? 1.0 : 0.0));
    }
    if (i + 4 <= N) {
      *reinterpret_cast<double2*>(g + i) = double2{v[0], v[1]};
      *reinterpret_cast<double2*>(g + i + 2) = double2{v[2], v[3]};
    } else {
      for (int e = 0; e < 4 && i + e < N; ++e) g[i + e] = v[e];
    }
  }
}

}  // namespace rvt
