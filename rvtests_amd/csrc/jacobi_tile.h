// rvtests_amd — the tile of the Jacobi kernels (jacobi_kernels.hip.h).  Apart from them because the family form of the kinship
// (rvt_fam.hip) is bounded by it — a family is at most one tile — without launching any of those kernels.
#pragma once

namespace rvt {
constexpr int kJacB = 32;        // columns per block
constexpr int kJacP = 2 * kJacB; // columns per pair
}  // namespace rvt
