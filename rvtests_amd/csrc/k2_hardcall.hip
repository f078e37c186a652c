// rvtests_amd — hard-call sufficient-statistics kernels (suffstat_hc.hip.h), one instantiation per tile class and launch
// shape; a translation unit of its own so that the engine's objects compile in parallel.
#include "suffstat_hc.hip.h"

namespace rvt {

// (ring depth x waves per SIMD) per tile class.  Without masked entries every instantiated shape streams at the HBM rate
// when it has the chip to itself (tools/k2hc_bench.hip), so that rate alone does not choose between them.  What chooses is
// the room a class leaves on a SIMD that holds its full complement of waves: the per-gene tail kernels of the previous batch
// (63 - 127 registers; the p-value kernel 248) run beside the streaming launches, and where fewer than 128 of the 512
// registers stay free a tail wave gets onto the SIMD only in place of a streaming wave and its loads in flight.  THE RULE: a
// class takes the shape whose waves at full occupancy leave at least 128 registers per SIMD free, provided its isolated rate
// is not lower — judged without and with 0.1 % masked entries, where the one-wave shapes of MT 4 fall 12 % behind, so MT 4
// keeps two waves.  Registers and rates of every shape: DESIGN 3.1a.  The engine's defaults (rvt_engine_int.h: hc_shape)
// follow the rule; RVT_HC_CFG overrides them per class.
typedef void (*hc_kernel_t)(const GeneDesc*, NullTile, long long, long long, int);
static hc_kernel_t hc_kernel(int MT, int depth, int waves) {
  if (MT < 1 || MT > kHcMaxMT || depth < 1 || depth > 9 || waves < 1 || waves > 9) return nullptr;  // (one digit each below)
  switch (MT * 100 + depth * 10 + waves) {
    case 124: return gene_suffstat_hc<1, 2, 4, false>;
    case 223: return gene_suffstat_hc<2, 2, 3, false>;
    case 242: return gene_suffstat_hc<2, 4, 2, false>;
    case 241: return gene_suffstat_hc_one<2, 4, false>;
    case 322: return gene_suffstat_hc<3, 2, 2, false>;
    case 331: return gene_suffstat_hc_one<3, 3, false>;
    case 422: return gene_suffstat_hc<4, 2, 2, false>;
    case 421: return gene_suffstat_hc_one<4, 2, false>;
    case 431: return gene_suffstat_hc_one<4, 3, false>;
    case 511: return gene_suffstat_hc<5, 1, 1, false>;  // rolling refill: one step buffer
    case 611: return gene_suffstat_hc<6, 1, 1, false>;
    default: return nullptr;  // no such shape compiled in
  }
}

bool k2_hc_has_shape(int MT, int depth, int waves) { return hc_kernel(MT, depth, waves) != nullptr; }

bool k2_launch_hc(int MT, int depth, int waves, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, long long N,
                  long long ld, int d) {
  const hc_kernel_t k = hc_kernel(MT, depth, waves);
  if (!k) return false;
  hipLaunchKernelGGL(k, grid, dim3(64), 0, st, d_desc, nt, N, ld, d);
  return true;
}

// the one-wave shape of a class, i.e. its body in gene_suffstat_hc_any (0: the class has none)
int k2_hc_any_depth(int MT) { return hc_any_depth(MT); }

void k2_launch_hc_any(unsigned classes, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, long long N,
                      long long ld, int d) {
  hipLaunchKernelGGL((gene_suffstat_hc_any<false>), grid, dim3(64), 0, st, d_desc, nt, N, ld, d, classes);
}

void k2_launch_classify(dim3 grid, hipStream_t st, const double* G, long long N, long long ld, int M, int* flag) {
  hipLaunchKernelGGL(block_classify_kernel<0>, grid, dim3(256), 0, st, G, N, ld, M, flag);
}

}  // namespace rvt
