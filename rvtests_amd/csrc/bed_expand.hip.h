// rvtests_amd — rows of 2-bit codes back to fp64 columns (the format and the row sources: rvt_bed_codes.h).  One kernel for the
// columns that crossed PCIe as codes (rvt_meta.hip: expand_packed_rows), for consecutive rows of a resident .bed matrix
// (bed_rows_expand) and for the listed, flipped kept rows of a gene batch (rvt_fam.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "rvt_bed_codes.h"

namespace rvt {

// Column j of G (leading dimension ld, 16-byte aligned columns) = the doubles of row j of src: 00 -> 0, 10 -> 1, 11 -> 2, 01 -> the
// column's one other value mu[j] (host_stage.h pack_column_f64; e.g. an imputed mean), and 2.0 - that where the row source flips
// the row — what fam_flip_compact_kernel writes for the imputed column.  grid (ceil(N / 1024), rows), 256 threads, four samples
// (one byte) per thread, two 16-byte stores, the last N mod 4 samples one by one.
template <class Rows>
static __global__ __launch_bounds__(256) void bed_expand_columns_kernel(const Rows src, const double* __restrict__ mu, long long N,
                                                                        long long ld, double* __restrict__ G) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x, i = 4 * b;
  if (i >= N) return;
  const int j = blockIdx.y;
  const unsigned code = src.row(j)[b];
  const double m = mu[j];
  const bool fl = src.flip(j);
  double* g = G + (long long)j * ld + i;
  double v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double x = bed_value((code >> (2 * e)) & 3u, m);
    v[e] = fl ? 2.0 - x : x;
  }
  if (i + 4 <= N) {
    *reinterpret_cast<double2*>(g) = double2{v[0], v[1]};
    *reinterpret_cast<double2*>(g + 2) = double2{v[2], v[3]};
  } else {
    for (int e = 0; e < 4 && i + e < N; ++e) g[e] = v[e];
  }
}

}  // namespace rvt
