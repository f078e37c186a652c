// rvtests_amd — the empirical kinship of `vcf2kinship --ibs` / `--bn` (IBSKinship and BaldingNicolsKinship,
// vcfUtils/vcf2kinship.cpp:138-266, behind the site filters of :943-960) from rows of a resident .bed matrix
// (rows cb = ceil(N / 4) bytes apart; the format: rvt_bed_codes.h).  Both methods are Gram products over the sites, N x N x V:
//
//   IBS   2 - |g_i - g_j| = n_i n_j + u_i u_j + h_i h_j   with n = [called], u = g - 1, h = [g == 1], all three 0 for a
//         missing call (0/0: 1+1+0, 0/1: 1+0+0, 0/2: 1-1+0, 1/1: 1+0+1, 1/2: 1+0+0, 2/2: 1+1+0).  The pair count is
//         c = sum n n', the numerator k = c + sum (u u' + h h'): three int8 planes, exact int32 sums on
//         v_mfma_i32_32x32x32_i8, one division per entry at the end.
//   BN    z = (g - mean) scale per site, 0 for a missing call: a table of four doubles per site, indexed by the code; the
//         product runs on v_mfma_f64_16x16x4_f64.
//
// Nothing is expanded in HBM: a workgroup owns a 128 x 128 tile of the lower triangle, stages the raw 2-bit bytes of a slab
// of 128 sites for its two sample blocks (2 x 32 bytes per site) in LDS, TRANSPOSED — byte b of the block, sites along the
// row — so that a lane's one LDS read holds the codes of ITS sample at 16 (IBS) or 4 (BN) consecutive sites, and builds its
// fragments from them in registers: bit operations on four packed bytes at a time for the int8 planes, a table lookup per
// site for BN.  The staging is where every edge is dealt with, once: a row is read as aligned words from whatever byte it
// starts at, and a dropped site, a site past V, a sample past N and the padding pairs of a row's last byte all become the
// code 01 (missing), which contributes nothing to any plane or table.
// Included by rvt_kinship.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rvt_bed_codes.h"

namespace rvt {

constexpr int kKinTile = 128;            // samples per side of a workgroup tile (32 bytes of a row)
constexpr int kKinSlab = 128;            // sites staged per step
constexpr int kKinLd = kKinSlab + 32;    // bytes between the rows of the LDS image (40 words: the 16 rows a read meets differ in bank)
constexpr int kKinThreads = 256;         // four waves as 2 x 2, 64 x 64 outputs each
constexpr int kKinBlockBytes = kKinTile / 4;

typedef int kin_i16_t __attribute__((ext_vector_type(16)));
typedef int kin_i4_t __attribute__((ext_vector_type(4)));
typedef double kin_d4_t __attribute__((ext_vector_type(4)));

// what the site pass leaves for the host, summed over all sites of a call
struct KinTotals {
  unsigned long long used, filtered_missing, filtered_maf, monomorphic;
};

// The site loop of vcf2kinship.cpp:943-960 on the counts of one row (n0 n1 n2 missing, recode_bed_count_kernel), in its order —
// missing rate, allele frequency, "no non-zero call" — then what the method adds: BaldingNicolsKinship::addGenotype's
// sum == 0 is the third filter again, and a site whose calls are all 2 (scale = inf there) is skipped as monomorphic.
// drop[v] = 1 for a site that is not used; z[4 v + code] = BN's standardised genotype (0 for code 01 and for a dropped site).
static __global__ __launch_bounds__(256) void kin_site_kernel(const unsigned long long* __restrict__ counts, long long V,
                                                              long long N, int bn, double min_maf, double max_missing,
                                                              unsigned char* __restrict__ drop, double* __restrict__ z,
                                                              KinTotals* __restrict__ totals) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const BedSite site = bed_site((long long)counts[4 * v], (long long)counts[4 * v + 1], (long long)counts[4 * v + 2],
                                (long long)counts[4 * v + 3]);
  const long long called = site.called, ac = site.ac;
  int cat = 0;
  if ((double)site.missing > max_missing * (double)N) {
    cat = 1;
  } else {
    const double af = called > 0 ? (double)ac / (double)(2 * called) : 0.0;
    if (af < min_maf || af > 1.0 - min_maf)
      cat = 2;
    else if (ac == 0 || (bn && ac == 2 * called))
      cat = 3;
  }
  drop[v] = cat != 0;
  if (bn) {
    double z0 = 0.0, z1 = 0.0, z2 = 0.0;
    if (cat == 0) {
      const double mean = site.mean;  // (ac > 0 here: a sample is called)
      const double scale = sqrt(1.0 / (1.0 - mean / 2.0) / mean);
      z0 = (0.0 - mean) * scale, z1 = (1.0 - mean) * scale, z2 = (2.0 - mean) * scale;
    }
    z[4 * v] = z0, z[4 * v + 1] = 0.0, z[4 * v + 2] = z1, z[4 * v + 3] = z2;
  }
  unsigned long long* t = reinterpret_cast<unsigned long long*>(totals);
  atomicAdd(t + cat, 1ull);
}

// tile t of the lower triangle, row block by row block: (rb, ct), ct <= rb
__device__ __forceinline__ void kin_tile(long long t, int* rb, int* ct) {
  long long r = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  *rb = (int)r, *ct = (int)(t - r * (r + 1) / 2);
}

// The slab of sites [s0, s0 + kKinSlab) of the workgroup's two sample blocks into raw[block][byte][site]: thread t takes the 32
// bytes of site t & 127 of block t >> 7 (0: the row block rb, 1: the column block ct).  The bytes start anywhere, so they are
// read as nine aligned words and shifted into place; a word is read only when it starts below `end` = the end of the V rows
// (it then ends at most 3 bytes behind them — rvt_bed_alloc leaves 16), and never below the first row's word (an allocation
// starts aligned).  Bits from sample N on, and everything of a dropped site or of a site >= V, are set to 01 = missing.
__device__ __forceinline__ void kin_stage(const unsigned char* __restrict__ rows, long long cb, long long N, long long V,
                                          const unsigned char* __restrict__ drop, long long s0, int rb, int ct,
                                          unsigned char (*raw)[kKinBlockBytes][kKinLd]) {
  const int t = threadIdx.x, blk = t >> 7, s = t & (kKinSlab - 1);
  const long long site = s0 + s;
  const long long sample0 = (long long)(blk ? ct : rb) * kKinTile;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0x55555555u;
  if (site < V && !drop[site]) {
    const unsigned char* p = rows + site * cb + (sample0 >> 2);
    const unsigned char* end = rows + V * cb;
    const int sh = 8 * (int)((uintptr_t)p & 3);
    const unsigned char* a = p - ((uintptr_t)p & 3);
    uint32_t d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = (a + 4 * i < end) ? *reinterpret_cast<const uint32_t*>(a + 4 * i) : 0u;
    const long long nbits = 2 * (N - sample0);  // > 0: the block exists
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint32_t x = (uint32_t)((((uint64_t)d[i + 1] << 32) | (uint64_t)d[i]) >> sh);
      const long long nb = nbits - 32 * i;
      if (nb <= 0) {
        x = 0x55555555u;
      } else if (nb < 32) {
        const uint32_t m = (1u << (int)nb) - 1u;
        x = (x & m) | (0x55555555u & ~m);
      }
      w[i] = x;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) raw[blk][4 * i + e][s] = (unsigned char)(w[i] >> (8 * e));
}

// the three int8 planes of one sample at 16 sites: x = 16 bytes (one per site) that hold the sample's code at bits sh2, sh2 + 1
__device__ __forceinline__ void kin_planes(kin_i4_t x, int sh2, kin_i4_t* n, kin_i4_t* u, kin_i4_t* h) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t c = ((uint32_t)x[e] >> sh2) & 0x03030303u;
    const uint32_t lo = c & 0x01010101u, hi = (c >> 1) & 0x01010101u;
    (*n)[e] = (int)((lo & ~hi) ^ 0x01010101u);                      // called: not 01
    (*h)[e] = (int)(hi & ~lo);                                      // 10: g == 1
    (*u)[e] = (int)((hi & lo) | (((hi | lo) ^ 0x01010101u) * 0xFFu));  // 11: +1, 00: -1 (0xFF)
  }
}

// IBS: Cc[m ld + j] (+)= sum n_m n_j, Ce[m ld + j] (+)= sum (u_m u_j + h_m h_j) over the V rows, for the tiles of the lower
// triangle (grid = their number, kin_tile); row m of C is sample m, the entries j <= m are the ones that are used.
// accumulate = 0: the first chunk of sites writes, the later ones add.
static __global__ __launch_bounds__(kKinThreads, 2) void kin_ibs_kernel(const unsigned char* __restrict__ rows, long long cb,
                                                                     long long N, long long V,
                                                                     const unsigned char* __restrict__ drop, int* __restrict__ Cc,
                                                                     int* __restrict__ Ce, long long ld, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[2][kKinBlockBytes][kKinLd];
  int rb, ct;
  kin_tile(blockIdx.x, &rb, &ct);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 31, lk = lane >> 5;
  kin_i16_t acc_c[2][2], acc_e[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc_c[a][b][e] = 0, acc_e[a][b][e] = 0;
  for (long long s0 = 0; s0 < V; s0 += kKinSlab) {
    __syncthreads();  // every wave has left the previous slab
    kin_stage(rows, cb, N, V, drop, s0, rb, ct, raw);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kKinSlab / 32; ++ks) {
      kin_i4_t an[2], au[2], ah[2], bn[2], bu[2], bh[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int sl = wm * 64 + a * 32 + lrow;
        kin_planes(*reinterpret_cast<const kin_i4_t*>(&raw[0][sl >> 2][ks * 32 + 16 * lk]), 2 * (sl & 3), &an[a], &au[a], &ah[a]);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int sl = wn * 64 + b * 32 + lrow;
        kin_planes(*reinterpret_cast<const kin_i4_t*>(&raw[1][sl >> 2][ks * 32 + 16 * lk]), 2 * (sl & 3), &bn[b], &bu[b], &bh[b]);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          acc_c[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(an[a], bn[b], acc_c[a][b], 0, 0, 0);
          acc_e[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(au[a], bu[b], acc_e[a][b], 0, 0, 0);
          acc_e[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah[a], bh[b], acc_e[a][b], 0, 0, 0);
        }
    }
  }
  // element 4 g + e of a lane's tile: row 8 g + 4 (lane >> 5) + e of the A side, column lane & 31 of the B side
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const long long j = (long long)ct * kKinTile + wn * 64 + b * 32 + lrow;
    if (j >= N) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long m = (long long)rb * kKinTile + wm * 64 + a * 32 + 8 * g + 4 * lk + e;
          if (m >= N) continue;
          const long long o = m * ld + j;
          if (accumulate) {
            Cc[o] += acc_c[a][b][4 * g + e];
            Ce[o] += acc_e[a][b][4 * g + e];
          } else {
            Cc[o] = acc_c[a][b][4 * g + e];
            Ce[o] = acc_e[a][b][4 * g + e];
          }
        }
  }
}

// BN: C[m ld + j] (+)= sum z_m z_j over the V rows, same tiles.  A k-step of the matrix instruction is four sites; lane group
// lg = lane >> 4 takes the sites 4 lg .. 4 lg + 3 of a run of 16 in its four steps (both operands agree, so the order of the
// contraction is free), which are the four bytes of ONE LDS word.  The sums of entry (m, j) run over the sites in one fixed
// order, whatever the tile.
static __global__ __launch_bounds__(kKinThreads, 2) void kin_bn_kernel(const unsigned char* __restrict__ rows, long long cb,
                                                                    long long N, long long V,
                                                                    const unsigned char* __restrict__ drop,
                                                                    const double* __restrict__ z, double* __restrict__ C,
                                                                    long long ld, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[2][kKinBlockBytes][kKinLd];
  __shared__ double zl[kKinSlab][4];
  int rb, ct;
  kin_tile(blockIdx.x, &rb, &ct);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lg = lane >> 4;
  kin_d4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = kin_d4_t{0.0, 0.0, 0.0, 0.0};
  for (long long s0 = 0; s0 < V; s0 += kKinSlab) {
    __syncthreads();
    kin_stage(rows, cb, N, V, drop, s0, rb, ct, raw);
    for (int q = threadIdx.x; q < 4 * kKinSlab; q += kKinThreads)
      zl[q >> 2][q & 3] = (s0 + (q >> 2) < V) ? z[4 * s0 + q] : 0.0;
    __syncthreads();
#pragma unroll 2
    for (int ch = 0; ch < kKinSlab / 16; ++ch) {
      uint32_t ca[4], cbv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int sl = wm * 64 + a * 16 + lrow;
        ca[a] = (*reinterpret_cast<const uint32_t*>(&raw[0][sl >> 2][ch * 16 + 4 * lg]) >> (2 * (sl & 3))) & 0x03030303u;
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int sl = wn * 64 + b * 16 + lrow;
        cbv[b] = (*reinterpret_cast<const uint32_t*>(&raw[1][sl >> 2][ch * 16 + 4 * lg]) >> (2 * (sl & 3))) & 0x03030303u;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double* zs = zl[ch * 16 + 4 * lg + j];
        double fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = zs[(ca[a] >> (8 * j)) & 3u];
#pragma unroll
        for (int b = 0; b < 4; ++b) fb[b] = zs[(cbv[b] >> (8 * j)) & 3u];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
    }
  }
  // element r of a lane's tile: row 4 r + (lane >> 4) of the A side, column lane & 15 of the B side
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long long j = (long long)ct * kKinTile + wn * 64 + b * 16 + lrow;
    if (j >= N) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long m = (long long)rb * kKinTile + wm * 64 + a * 16 + 4 * r + lg;
        if (m >= N) continue;
        const long long o = m * ld + j;
        C[o] = accumulate ? C[o] + acc[a][b][r] : acc[a][b][r];
      }
  }
}

// K[i N + j] for every (i, j) from the entry (max, min) of the lower triangle: both halves are the SAME number.
// IBS: k / c with k = c + e, 0 where the pair was never called together (IBSKinship::calculate leaves the 0 it started from).
static __global__ __launch_bounds__(256) void kin_finish_ibs_kernel(const int* __restrict__ Cc, const int* __restrict__ Ce,
                                                                    long long N, long long ld, double* __restrict__ K) {
  const long long total = N * N;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
    const long long i = q / N, j = q - i * N;
    const long long o = i >= j ? i * ld + j : j * ld + i;
    const int c = Cc[o];
    K[q] = c > 0 ? (double)((long long)c + (long long)Ce[o]) / (double)c : 0.0;
  }
}

// BN: sum / n, n = the sites that were used (BaldingNicolsKinship::calculate; n == 0 leaves K zero)
static __global__ __launch_bounds__(256) void kin_finish_bn_kernel(const double* __restrict__ C, long long N, long long ld,
                                                                   const KinTotals* __restrict__ totals, double* __restrict__ K) {
  const long long total = N * N;
  const unsigned long long n = totals->used;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
    const long long i = q / N, j = q - i * N;
    const long long o = i >= j ? i * ld + j : j * ld + i;
    K[q] = n > 0 ? C[o] / (double)n : 0.0;
  }
}

}  // namespace rvt
