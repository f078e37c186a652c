// rvtests_amd — kernels of famGrammarGamma over rows of a resident .bed matrix (rvt_grammar_bed_dev, rvt_fam.hip); the arithmetic
// they share with the host test harness is rvt_grammar_bed.h's.
//
//   grammar_ty_planes_kernel   once per null fit: max |ty|, the common exponent, the eight int8 digit planes of ty (zero from
//                              sample N to the planes' leading dimension) and their totals.  One workgroup, fixed order.
//   grammar_bed_kernel         grid (row-tile groups, sample slices), 512 threads = 8 waves.  The workgroup stages its slice of
//                              the B operand [8 planes | ones] in LDS once (9 bytes per sample: the seven padding columns of the
//                              16 are constant zero and come from registers) and every wave walks row tiles of 16 rows over it:
//                              per step of 256 samples a lane loads the 16 bytes of codes of ITS row and quarter (bed_load16
//                              of rvt_bed_codes.h, where the format is stated: no byte outside the V rows is touched), builds the
//                              three 0 / 1 int8 operands H = hi bits, L = lo bits, HL = hi & lo in registers and issues
//                              3 x 4 v_mfma_i32_16x16x64_i8.  The rows of B for samples >= N are zero, ones column included:
//                              that makes the padding pairs of a row's last byte, and whatever lies behind it, harmless.  The
//                              ones column gives sum H = n1 + n2, sum L = missing + n2, sum HL = n2: no separate count pass.
//                              Partial sums go to part[slice][row][27] as int32: no atomics, nothing to clear.
//   grammar_bed_finish_kernel  one thread per row: the slices summed in int64 in slice order (exact: the result does not depend on
//                              the plan), the counts, grammar_bed_finish.
//   grammar_af_kin_kernel      af=kinship only: 1/2 sum wu1 (U'g) / afden per rotated column (GrammarGamma.cpp:199-213).
//
// The matrix instruction: 16x16x64, not 32x32x32.  B has 9 live columns, so a 32-wide tile would spend 23 of 32 columns on zeros
// where the 16-wide one spends 7 of 16, and the 16-row A tile keeps a row's 64 samples of one instruction in FOUR lanes' 4-byte
// groups: a lane's 16-byte load is four instructions' worth of ITS OWN operand, no lane exchange.  The k index of the instruction
// is (lane >> 4, byte): A and B use the same map, so any assignment of samples to it that both sides share is a correct sum.
// Here instruction t (0 .. 3) of a step takes, from lane group g, samples 64 g + 16 t .. + 15 of the step's 256.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rvt_grammar_bed.h"

namespace rvt {

constexpr int kGgThreads = 512;
constexpr int kGgWaves = kGgThreads / 64;
constexpr int kGgStep = 4 * kGgKstep;  // samples of one load step of a wave: 16 bytes of codes per lane, four lane groups
constexpr int kGgPart = 3 * kGgCols;   // int32 partial sums per row and slice

typedef int gg_i4_t __attribute__((ext_vector_type(4)));

static __global__ __launch_bounds__(1024) void grammar_ty_planes_kernel(const double* __restrict__ ty, long long N,
                                                                        signed char* __restrict__ planes, long long ld,
                                                                        int* __restrict__ exp_ok, long long* __restrict__ totals) {
  __shared__ double redm[16];
  __shared__ int redf[16];
  __shared__ long long redt[16][kGgPlanes];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double mx = 0.0;
  int bad = 0;
  for (long long i = threadIdx.x; i < N; i += blockDim.x) {
    const double a = fabs(ty[i]);
    bad |= !(a <= DBL_MAX);
    mx = fmax(mx, a);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, o, 64));
    bad |= __shfl_xor(bad, o, 64);
  }
  if (lane == 0) redm[wave] = mx, redf[wave] = bad;
  __syncthreads();
  for (int w = 0; w < 16; ++w) mx = fmax(mx, redm[w]), bad |= redf[w];
  const int e = grammar_ty_exp(mx);
  if (threadIdx.x == 0) exp_ok[0] = e, exp_ok[1] = bad ? 0 : 1;
  if (bad) return;  // (uniform)
  long long t[kGgPlanes];
#pragma unroll
  for (int p = 0; p < kGgPlanes; ++p) t[p] = 0;
  for (long long i = threadIdx.x; i < ld; i += blockDim.x) {
    signed char d[kGgPlanes];
    (void)grammar_ty_digits(i < N ? ty[i] : 0.0, e, d);
#pragma unroll
    for (int p = 0; p < kGgPlanes; ++p) {
      planes[p * ld + i] = d[p];
      t[p] += d[p];
    }
  }
#pragma unroll
  for (int p = 0; p < kGgPlanes; ++p) {
    long long s = t[p];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) redt[wave][p] = s;
  }
  __syncthreads();
  if (threadIdx.x < kGgPlanes) {
    long long s = 0;
    for (int w = 0; w < 16; ++w) s += redt[w][threadIdx.x];
    totals[threadIdx.x] = s;
  }
}

// part: [slices][V][kGgPart] int32, row-major.  bytes = V * pitch, the extent of the rows.  Dynamic LDS: 9 * slice bytes.
static __global__ __launch_bounds__(kGgThreads) void grammar_bed_kernel(const unsigned char* __restrict__ rows, long long pitch,
                                                                        long long N, int V, long long bytes,
                                                                        const signed char* __restrict__ planes, long long ldp,
                                                                        long long npad, long long slice, int tiles,
                                                                        int* __restrict__ part) {
  extern __shared__ uint4 gg_lds[];  // [group of 16 samples][column 0 .. 8]: the 16 bytes of a B fragment
  const long long s0 = (long long)blockIdx.y * slice;
  const int len = (int)((s0 + slice < npad ? s0 + slice : npad) - s0);  // (a multiple of the K-step)
  const int ngroups = len / 16;
  for (int idx = threadIdx.x; idx < ngroups * kGgCols; idx += kGgThreads) {
    const int col = idx / ngroups, grp = idx - col * ngroups;
    const long long s = s0 + 16LL * grp;
    uint4 v;
    if (col < kGgPlanes) {
      v = *reinterpret_cast<const uint4*>(planes + col * ldp + s);  // (ldp >= npad, a multiple of 64; zero from sample N on)
    } else {
      v = make_uint4(bed_live_lanes(N - s), bed_live_lanes(N - (s + 4)), bed_live_lanes(N - (s + 8)),
                     bed_live_lanes(N - (s + 12)));  // the ones column: 1 for the samples that exist
    }
    gg_lds[grp * kGgCols + col] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;  // A: row r of the tile; B and D: column r; k group g
  const unsigned char* end = rows + bytes;
  for (int t = wave; t < tiles; t += kGgWaves) {
    const long long row0 = ((long long)blockIdx.x * tiles + t) * kGgTileRows;
    if (row0 >= V) break;  // (uniform in the wave)
    const bool live = row0 + r < V;
    const unsigned char* rp = rows + (row0 + r) * pitch + (s0 >> 2) + 16 * g;
    gg_i4_t accH = {0, 0, 0, 0}, accL = {0, 0, 0, 0}, accHL = {0, 0, 0, 0};
    uint32_t cur[4] = {0u, 0u, 0u, 0u}, nxt[4];
    if (live && 64 * g < len) bed_load16(rp, rows, end, cur);
    for (int c0 = 0; c0 < len; c0 += kGgStep) {
      nxt[0] = nxt[1] = nxt[2] = nxt[3] = 0u;
      if (live && c0 + kGgStep + 64 * g < len) bed_load16(rp + ((c0 + kGgStep) >> 2), rows, end, nxt);
      const bool inb = (r < kGgCols) && (c0 + 64 * g < len);
      const uint4* bp = gg_lds + ((c0 >> 4) + 4 * g) * kGgCols + r;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t lo = cur[u] & 0x55555555u, hi = (cur[u] >> 1) & 0x55555555u;
        gg_i4_t H, L, HL, B = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          H[k] = (int)bed_spread(hi, k);
          L[k] = (int)bed_spread(lo, k);
          HL[k] = H[k] & L[k];
        }
        if (inb) {
          const uint4 b = bp[u * kGgCols];
          B = gg_i4_t{(int)b.x, (int)b.y, (int)b.z, (int)b.w};
        }
        accH = __builtin_amdgcn_mfma_i32_16x16x64_i8(H, B, accH, 0, 0, 0);
        accL = __builtin_amdgcn_mfma_i32_16x16x64_i8(L, B, accL, 0, 0, 0);
        accHL = __builtin_amdgcn_mfma_i32_16x16x64_i8(HL, B, accHL, 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
    }
    // D: column = lane & 15 (the plane), row = 4 (lane >> 4) + register
    if (r < kGgCols) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long row = row0 + 4 * g + i;
        if (row < V) {
          int* o = part + ((long long)blockIdx.y * V + row) * kGgPart + r;
          o[0] = accH[i];
          o[kGgCols] = accL[i];
          o[2 * kGgCols] = accHL[i];
        }
      }
    }
  }
}

struct GgBedConsts {
  double gamma, ysy;
  long long T[kGgPlanes];
  int e;
};

// counts (4 V, optional): n0 n1 n2 missing; sums (27 V, optional): the int64 sums as part holds them per row
static __global__ __launch_bounds__(256) void grammar_bed_finish_kernel(const int* __restrict__ part, int slices, int V, long long N,
                                                                        GgBedConsts k, int* __restrict__ ok,
                                                                        double* __restrict__ af, double* __restrict__ beta,
                                                                        double* __restrict__ beta_var, double* __restrict__ pval,
                                                                        long long* __restrict__ counts,
                                                                        long long* __restrict__ sums) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= V) return;
  int64_t S[kGgPart];
#pragma unroll
  for (int j = 0; j < kGgPart; ++j) S[j] = 0;
  for (int s = 0; s < slices; ++s) {
    const int* p = part + ((long long)s * V + h) * kGgPart;
#pragma unroll
    for (int j = 0; j < kGgPart; ++j) S[j] += p[j];
  }
  if (sums)
    for (int j = 0; j < kGgPart; ++j) sums[(long long)h * kGgPart + j] = S[j];
  const long long sH = S[kGgPlanes], sL = S[kGgCols + kGgPlanes], sHL = S[2 * kGgCols + kGgPlanes];
  const long long n2 = sHL, n1 = sH - sHL, nm = sL - sHL, n0 = N - n1 - n2 - nm;
  if (counts) {
    counts[4LL * h] = n0;
    counts[4LL * h + 1] = n1;
    counts[4LL * h + 2] = n2;
    counts[4LL * h + 3] = nm;
  }
  int64_t P[3 * kGgPlanes];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int q = 0; q < kGgPlanes; ++q) P[o * kGgPlanes + q] = S[o * kGgCols + q];
  int okv;
  double a, b, bv, pv;
  grammar_bed_finish(n0, n1, n2, nm, P, k.T, k.e, k.gamma, k.ysy, &okv, &a, &b, &bv, &pv);
  ok[h] = okv;
  if (af) af[h] = a;
  beta[h] = b;
  beta_var[h] = bv;
  pval[h] = pv;
}

// af[h] = 1/2 sum_i wu1_i Gt[i, h] / afden: a plain division as in grammar_stream_kernel; grid = columns, 256 threads, fixed order
static __global__ __launch_bounds__(256) void grammar_af_kin_kernel(const double* __restrict__ Gt, long long ld, long long N,
                                                                    const double* __restrict__ wu1, double afden,
                                                                    double* __restrict__ af) {
  __shared__ double red[4];
  const double* g = Gt + (long long)blockIdx.x * ld;
  double s = 0.0;
  for (long long i = threadIdx.x; i < N; i += 256) s = fma(wu1[i], g[i], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) af[blockIdx.x] = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]) / afden;
}

}  // namespace rvt
