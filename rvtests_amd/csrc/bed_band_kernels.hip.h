// rvtests_amd — MetaCov's band from rows of a resident .bed matrix (rvt_cov_band_bed_dev): the front stage that turns W
// consecutive 2-bit rows into what the MXFP4 band reads of their mean-imputed columns g = h + mu m — the E2M1 nibble rows of
// the calls h and of the missing mask m (band_gemm.hip.h), and per row the column sum, the polymorphic flag, mu and the row of
// T = G'X (band_rows.hip.h, cov_rect_xz_kernel).  No fp64 column exists: a row costs N/4 bytes read and N bytes written
// (two nibble rows of N/2), against 8 N + N + N/2 + N/2 for a column of the ring with its cache.
//
// bed_band_prep_kernel   grid (ceil(W / ROWS), slices), 256 threads.  A lane takes 16 samples (four .bed bytes: bed_load4 of
//                        rvt_bed_codes.h, where the format is stated) of ROWS rows per step and writes 8 bytes of each
//                        nibble row; the ROWS rows share the loads of X.  The sums over X are fp64 FMAs with h in {0, 1, 2} and
//                        m in {0, 1}: per slice and row 2 DMAX partial sums and four integer counts, written — not added — to
//                        part_t / part_c.  The slice partition is a function of N alone (bed_band_slices), so a row's numbers
//                        do not depend on the window it is called in.
// bed_band_finish_kernel one thread per row: the slices in order 0, 1, ...; mu, the column sum, T, the flag and the counts.
// Included by rvt_meta.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rvt_bed_codes.h"
#include "rvt_bed_nibbles.h"

namespace rvt {

constexpr int kBedBandStep = 4096;  // samples a workgroup takes per step: 256 lanes x 16

// rows per workgroup of the instantiation for DMAX covariates: the accumulators are 2 ROWS DMAX doubles per lane
template <int DMAX>
struct BedBandRows {
  static constexpr int value = DMAX <= 8 ? 4 : 2;
};

// samples per slice: whole steps, so that every slice starts on a 16-sample (8-byte nibble) boundary
__host__ __device__ inline long long bed_band_slice_len(long long N, int slices) {
  return ((N + slices - 1) / slices + kBedBandStep - 1) / kBedBandStep * kBedBandStep;
}

// rows: W rows of cb = ceil(N / 4) bytes at any byte address.  outH / outM: [row][ldk4] nibble rows (ldk4 a multiple of 128, at
// least ceil(N / 16) * 8); bytes [0, ceil(N / 16) * 8) of every row are written here, the pad behind them is the caller's.
// part_t: [slice][row][2 DMAX] (sum h X_k for k < DMAX, then sum m X_k), part_c: [slice][row][4] (calls of 0 / 1 / 2 / missing).
template <int DMAX>
__global__ __launch_bounds__(256) void bed_band_prep_kernel(const unsigned char* __restrict__ rows, long long cb, long long N,
                                                            int W, const double* __restrict__ X, long long ldx, int d,
                                                            unsigned char* __restrict__ outH, unsigned char* __restrict__ outM,
                                                            long long ldk4, double* __restrict__ part_t,
                                                            int* __restrict__ part_c) {
  constexpr int ROWS = BedBandRows<DMAX>::value;
  const int row0 = blockIdx.x * ROWS;
  const int nr = min(ROWS, W - row0);
  const long long per = bed_band_slice_len(N, (int)gridDim.y);
  const long long i0 = (long long)blockIdx.y * per, i1 = (i0 + per < N) ? i0 + per : N;
  const unsigned char* rows_end = rows + (long long)W * cb;
  double th[ROWS][DMAX], tm[ROWS][DMAX];
  int cnt[ROWS][4];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int k = 0; k < DMAX; ++k) th[r][k] = tm[r][k] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt[r][q] = 0;
  }
  for (long long i = i0 + 16 * (long long)threadIdx.x; i < i1; i += kBedBandStep) {
    const long long b0 = i >> 2;  // (a multiple of 4: i0 and the step are multiples of 16)
    // (a dword may cover bytes of the next row: samples at or beyond i1 <= N, which `live` below discards)
    unsigned code[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      code[r] = r < nr ? bed_load4(rows + (long long)(row0 + r) * cb + b0, rows, rows_end) : 0u;
    unsigned long long hq[ROWS], mq[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) hq[r] = mq[r] = 0ull;
    // (one .bed byte = four samples at a time, not unrolled: the four bytes unrolled cost registers up to scratch)
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const long long ig = i + 4 * g;
      const long long left = i1 - ig;
      const int live = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
      const unsigned lmask = bed_live_mask(live);
      double hv[ROWS][4], mv[ROWS][4];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const BedNibbles nb = bed_byte_nibbles(code[r] >> (8 * g), lmask);
        hq[r] |= (unsigned long long)nb.h << (16 * g);
        mq[r] |= (unsigned long long)nb.m << (16 * g);
        cnt[r][0] += __popc(nb.zero);
        cnt[r][1] += __popc(nb.one);
        cnt[r][2] += __popc(nb.two);
        cnt[r][3] += __popc(nb.miss);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hv[r][e] = (double)(int)((nb.h >> (4 * e + 1)) & 3u);
          mv[r][e] = (double)(int)((nb.miss >> (4 * e)) & 1u);
        }
      }
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        if (k < d && live > 0) {
          // (ig < N here and ldx is a multiple of 4 at least N: the four doubles exist; those of samples beyond N do not count)
          const double2 a = *reinterpret_cast<const double2*>(X + (long long)k * ldx + ig);
          const double2 b = *reinterpret_cast<const double2*>(X + (long long)k * ldx + ig + 2);
          const double x[4] = {a.x, live > 1 ? a.y : 0.0, live > 2 ? b.x : 0.0, live > 3 ? b.y : 0.0};
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              th[r][k] = fma(hv[r][e], x[e], th[r][k]);
              tm[r][k] = fma(mv[r][e], x[e], tm[r][k]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (r < nr) {
        *reinterpret_cast<unsigned long long*>(outH + (long long)(row0 + r) * ldk4 + 2 * b0) = hq[r];
        *reinterpret_cast<unsigned long long*>(outM + (long long)(row0 + r) * ldk4 + 2 * b0) = mq[r];
      }
    }
  }
  __shared__ double red_t[4][ROWS][2 * DMAX];
  __shared__ int red_c[4][ROWS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
      double u = th[r][k], v = tm[r][k];
      for (int o = 32; o > 0; o >>= 1) {
        u += __shfl_down(u, o);
        v += __shfl_down(v, o);
      }
      if (lane == 0) {
        red_t[wave][r][k] = u;
        red_t[wave][r][DMAX + k] = v;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int a = cnt[r][q];
      for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
      if (lane == 0) red_c[wave][r][q] = a;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < ROWS * (2 * DMAX + 4); idx += 256) {
    const int r = idx / (2 * DMAX + 4), f = idx % (2 * DMAX + 4);
    if (r >= nr) continue;
    const long long o = (long long)blockIdx.y * W + row0 + r;
    if (f < 2 * DMAX)
      part_t[o * (2 * DMAX) + f] = red_t[0][r][f] + red_t[1][r][f] + red_t[2][r][f] + red_t[3][r][f];
    else
      part_c[o * 4 + (f - 2 * DMAX)] = red_c[0][r][f - 2 * DMAX] + red_c[1][r][f - 2 * DMAX] + red_c[2][r][f - 2 * DMAX] +
                                       red_c[3][r][f - 2 * DMAX];
  }
}

// One thread per row: the slices added in order; from the integer counts (bed_site) mu = the mean of the called samples, 0 for a
// row with no missing call (the column is its calls), the column sum (n1 + 2 n2) + mu n_missing and the flag; T_k = sum h X_k +
// mu sum m X_k.  T is W x d column-major; counts (optional): 4 per row; *any_missing is set when some row has a missing call.
__global__ void bed_band_finish_kernel(const double* __restrict__ part_t, const int* __restrict__ part_c, int slices, int W,
                                       int d, int dmax, double* __restrict__ colsum, int* __restrict__ poly,
                                       double* __restrict__ T, double* __restrict__ mu_out, long long* __restrict__ counts,
                                       int* __restrict__ any_missing) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= W) return;
  long long n[4] = {0, 0, 0, 0};
  for (int s = 0; s < slices; ++s)
    for (int q = 0; q < 4; ++q) n[q] += part_c[((long long)s * W + j) * 4 + q];
  const BedSite s = bed_site(n[0], n[1], n[2], n[3]);
  const double mu = n[3] > 0 ? s.mean : 0.0;
  colsum[j] = (double)s.ac + mu * (double)n[3];
  poly[j] = s.poly ? 1 : 0;
  mu_out[j] = mu;
  for (int k = 0; k < d; ++k) {
    double a = 0.0, b = 0.0;
    for (int s = 0; s < slices; ++s) {
      a += part_t[((long long)s * W + j) * (2 * dmax) + k];
      b += part_t[((long long)s * W + j) * (2 * dmax) + dmax + k];
    }
    T[j + (long long)k * W] = a + mu * b;
  }
  if (counts)
    for (int q = 0; q < 4; ++q) counts[4 * (long long)j + q] = n[q];
  if (n[3] > 0) atomicOr(any_missing, 1);
}

}  // namespace rvt
