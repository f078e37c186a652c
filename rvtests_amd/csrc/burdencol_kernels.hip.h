// rvtests_amd — the collapsed columns of a batch of genes (rvt_burden_blocks: --burden cmcWald, zegginiWald, fp, exactCMC) and
// Fisher's exact test of a batch of 2 x 2 tables.
//
//  burden_columns_kernel   cmcCollapse / zegginiCollapse / fpCollapse (src/Model.cpp:73-89,115-130,177-197) of every gene of a
//                          batch in ONE stream over the gene's original N x M block: the flip 2 - g and the column filter of
//                          getFlippedToMinorPolymorphicGenotype (decided before, by fam_colstat_kernel) are applied in registers,
//                          no flipped copy goes to memory.  Per gene it also counts CMCWaldTest::totalNonRefSite and the 2 x 2
//                          table of CMCFisherExactTest::fit (src/Model.h:1123-1130) — integers, exact in any order.
//  fisher_2x2_kernel       Table2by2::FullFastFisherExactTest (regression/Table2by2.cpp:316-357), one workgroup per table.
//
// Layout of the stream: grid (sample-parts x genes), 256 threads; a thread owns two adjacent samples, so a wave reads 1 KB of a
// column with 16-byte loads (columns start on 128-byte lines: ld is a multiple of 16 doubles).  The kept-column list of the gene is
// wave-uniform and comes through the scalar cache.  Registers: two accumulators per test, no LDS in the loop — the kernel is bound
// by the read of the genes.
#pragma once

namespace rvt {

// one gene of the batch: its block, where its kept columns start in the batch-wide lists, how many there are
struct BurdenColGene {
  const double* G;
  int kept0;
  int m;
};

constexpr int kBurdenColCounters = 8;  // per gene: NonRefSite, N00, N01, N10, N11 (three spare)

#if !defined(RVT_K_SPLIT) || defined(RVT_K_META)
// kept_col[k]: column index within the gene's block, bit 30 set when the column is flipped; kept_w[k]: the Fp weight
// 1 / sqrt(f (1 - f)), 0 for a column fpCollapse skips.  cmc / zeg / fp: N x n blocks (ld apart), column = gene index; a null
// pointer leaves that block alone.  y: the phenotype for the 2 x 2 table (may be null: no table).
static __global__ __launch_bounds__(256) void burden_columns_kernel(const BurdenColGene* __restrict__ genes,
                                                                    const int* __restrict__ kept_col,
                                                                    const double* __restrict__ kept_w, long long N, long long ld,
                                                                    const double* __restrict__ y, double* __restrict__ cmc,
                                                                    double* __restrict__ zeg, double* __restrict__ fp,
                                                                    int* __restrict__ counters) {
  const int gi = blockIdx.y;
  const BurdenColGene gd = genes[gi];
  const int* kc = kept_col + gd.kept0;
  const double* kw = kept_w + gd.kept0;
  const bool want_fp = fp != nullptr;
  int nonref = 0, n00 = 0, n01 = 0, n10 = 0, n11 = 0;
  const long long pairs = ld / 2;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < pairs; t += (long long)gridDim.x * blockDim.x) {
    const long long i = 2 * t;
    int c0 = 0, c1 = 0;
    double s0 = 0.0, s1 = 0.0;
    if (i < N) {
      const bool two = i + 1 < N;
#pragma unroll 4
      for (int k = 0; k < gd.m; ++k) {
        const int cj = kc[k];
        const double2 g = *reinterpret_cast<const double2*>(gd.G + (long long)(cj & 0x3fffffff) * ld + i);
        const bool fl = (cj & 0x40000000) != 0;
        const double a = fl ? 2.0 - g.x : g.x, b = fl ? 2.0 - g.y : g.y;
        c0 += ((int)a > 0) ? 1 : 0;
        c1 += ((int)b > 0) ? 1 : 0;
        if (want_fp) {
          const double w = kw[k];
          if (w > 0.0) {
            s0 += a * w;
            s1 += b * w;
          }
        }
      }
      if (!two) c1 = 0, s1 = 0.0;
      nonref += (c0 > 0) + (c1 > 0);
      if (y) {
        const int p0 = (int)y[i], p1 = two ? (int)y[i + 1] : -1;
        const int q0 = c0 > 0, q1 = c1 > 0;
        n00 += (p0 == 0 && !q0) + (p1 == 0 && !q1);
        n01 += (p0 == 1 && !q0) + (p1 == 1 && !q1);
        n10 += (p0 == 0 && q0) + (p1 == 0 && q1);
        n11 += (p0 == 1 && q0) + (p1 == 1 && q1);
      }
    }
    // (rows N .. ld - 1 are written as zeros)
    if (cmc) *reinterpret_cast<double2*>(cmc + (long long)gi * ld + i) = make_double2(c0 > 0 ? 1.0 : 0.0, c1 > 0 ? 1.0 : 0.0);
    if (zeg) *reinterpret_cast<double2*>(zeg + (long long)gi * ld + i) = make_double2((double)c0, (double)c1);
    if (fp) *reinterpret_cast<double2*>(fp + (long long)gi * ld + i) = make_double2(s0, s1);
  }
  // the five integers: wave sums, then one vector atomic per wave and counter
  int v[5] = {nonref, n00, n01, n10, n11};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    int n = v[q];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n != 0) atomicAdd(counters + (long long)gi * kBurdenColCounters + q, n);
  }
}

// log of the hypergeometric probability of the table (a, b; c, d): Table2by2::logHypergeometricProb with lgamma(n + 1) in the
// place of the table of cumulative log sums.  margins = the five terms that depend on the margins alone.
static __device__ inline double fisher_margins(int row0, int row1, int col0, int col1, int sum) {
  return lgamma((double)row0 + 1.0) + lgamma((double)row1 + 1.0) + lgamma((double)col0 + 1.0) + lgamma((double)col1 + 1.0) -
         lgamma((double)sum + 1.0);
}
static __device__ inline double fisher_logp(double margins, int a, int b, int c, int d) {
  return margins - lgamma((double)a + 1.0) - lgamma((double)b + 1.0) - lgamma((double)c + 1.0) - lgamma((double)d + 1.0);
}

// One workgroup per table.  tables: kBurdenColCounters ints per table, N00 N01 N10 N11 at 1 .. 4 (the counters of
// burden_columns_kernel); out: three doubles per table — PvalueTwoSide, PvalueLess, PvalueGreater.  The admissible n00 are strided
// over the 256 threads; every thread adds its terms in ascending i, the 256 partial sums are added by a fixed tree: two runs give
// the same bits.
static __global__ __launch_bounds__(256) void fisher_2x2_kernel(const int* __restrict__ tables, int n_tables,
                                                                double* __restrict__ out) {
  __shared__ double sm[3][256];
  const int t = blockIdx.x;
  if (t >= n_tables) return;
  const int* tb = tables + (long long)t * kBurdenColCounters;
  const int a = tb[1], b = tb[2], c = tb[3], d = tb[4];
  const int row0 = a + b, row1 = c + d, col0 = a + c, sum = a + b + c + d;
  // CalculateBoundsIn00ForFisher
  int upper = row0 < col0 ? row0 : col0;
  int lower = row0 + col0 - sum;
  if (lower < 0) lower = 0;
  const double margins = fisher_margins(row0, row1, col0, b + d, sum);
  const double cutoff = fisher_logp(margins, a, b, c, d);  // (the term i = n00 below is this number, bit for bit)
  double two = 0.0, less = 0.0, greater = 0.0;
  for (int i = lower + (int)threadIdx.x; i <= upper; i += 256) {
    const double lp = fisher_logp(margins, i, row0 - i, col0 - i, row1 + i - col0);
    const double e = exp(lp - cutoff);
    if (lp <= cutoff) two += e;
    if (i <= a) less += e;
    if (i >= a) greater += e;
  }
  sm[0][threadIdx.x] = two;
  sm[1][threadIdx.x] = less;
  sm[2][threadIdx.x] = greater;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sm[0][threadIdx.x] += sm[0][threadIdx.x + off];
      sm[1][threadIdx.x] += sm[1][threadIdx.x + off];
      sm[2][threadIdx.x] += sm[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[(long long)t * 3 + threadIdx.x] = exp(cutoff + log(sm[threadIdx.x][0]));
}
#endif  // RVT_K_META

}  // namespace rvt
