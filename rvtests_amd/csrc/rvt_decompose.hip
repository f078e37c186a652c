// rvtests_amd — KinshipHolder::decompose on the device: the eigendecomposition K = U S U' of a kinship matrix, solver by solver.
// Three routes, tried in this order (rvt_kinship_decompose): family by family when the sparsity pattern of K splits the samples
// into groups of at most 64 (decompose_by_family; rvt_kinship_decompose_families is handed the groups and their blocks),
// tridiagonalisation + bisection + inverse iteration for a dense K (decompose_dense_tridiag, tridiag_kernels.hip.h), and the
// one-sided block Jacobi iteration for whatever is left (decompose_dense_jacobi, jacobi_kernels.hip.h).  A route answers with an
// Outcome: done, not mine (the next route takes the matrix) or failed.  Installing the result is rvt_fam.hip's.
// Part of librvtests_amd.so.  This unit compiles (and ships) the jac_* and td_* kernels only: see "kernel families" in
// rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_DECOMPOSE
#include "rvt_engine_int.h"
#include "jacobi_kernels.hip.h"
#include "tridiag_kernels.hip.h"

namespace {
// connected components of a list of pairs over n items (union by size, path halving).  cap > 0: stop as soon as a
// component outgrows it (false).  Components in the order of their first member, members ascending.
struct Components {
  std::vector<int> parent, csize;
  explicit Components(int64_t n) : parent((size_t)n), csize((size_t)n, 1) {
    for (int64_t i = 0; i < n; ++i) parent[i] = (int)i;
  }
  int find(int x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  }
  bool join(int p, int q, int cap) {
    int a = find(p), b = find(q);
    if (a == b) return true;
    if (csize[a] < csize[b]) std::swap(a, b);
    parent[b] = a;
    csize[a] += csize[b];
    return cap <= 0 || csize[a] <= cap;
  }
  void list(std::vector<int64_t>* fam_ptr, std::vector<int>* members) {
    const int64_t n = (int64_t)parent.size();
    std::vector<int> first_of((size_t)n, -1), fam_of((size_t)n);
    std::vector<int64_t> count;
    for (int64_t i = 0; i < n; ++i) {
      const int r = find((int)i);
      if (first_of[r] < 0) {
        first_of[r] = (int)count.size();
        count.push_back(0);
      }
      fam_of[i] = first_of[r];
      ++count[first_of[r]];
    }
    fam_ptr->assign(count.size() + 1, 0);
    for (size_t f = 0; f < count.size(); ++f) (*fam_ptr)[f + 1] = (*fam_ptr)[f] + count[f];
    std::vector<int64_t> fill(fam_ptr->begin(), fam_ptr->end() - 1);
    members->resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) (*members)[fill[fam_of[i]]++] = (int)i;  // i ascending: members ascending per family
  }
};

// What a step of the decomposition — a whole route, or one stage of the tridiagonal route — answers: done (a route: U and S
// are with the caller, rc is the installation's), not mine (the next route takes the matrix), or failed (the call fails with
// rc).  An int (HIP_TRY, fail(), another entry point's result) converts to done or failed.
struct Outcome {
  enum Kind { kDone, kNotMine, kFailed } kind;
  int rc;
  Outcome(int rc_, Kind k) : kind(k), rc(rc_) {}
  Outcome(int rc_) : Outcome(rc_, rc_ ? kFailed : kDone) {}
};
Outcome not_mine() { return Outcome(RVT_OK, Outcome::kNotMine); }
#define ROUTE_TRY(step)                       \
  do {                                        \
    const Outcome o_ = (step);                \
    if (o_.kind != Outcome::kDone) return o_; \
  } while (0)

// a gemm_tn_f64 call that found no room for its K-slice buffer: not an error of the decomposition, Jacobi takes over
Outcome gemm_or_not_mine(rvt_ctx* c, int rc) {
  if (rc != RVT_E_HIP || !strstr(rvt_last_error(c), "out of memory")) return rc;
  (void)hipGetLastError();
  return not_mine();
}

// |lambda| <= the largest absolute row sum of K (Gershgorin).  mu = 4 x that bound scales the pads of the Jacobi tiles (they sit
// well outside the spectrum) and every route's residual bar.
double mu_from_row_sum(double max_row_sum) { return 4.0 * std::max(max_row_sum, 1e-300); }

int64_t jac_padded_order(int64_t N) { return (N + kJacP - 1) / kJacP * kJacP; }  // an even number of 32-column blocks

// What the three routes over a dense K end with: U (on the device) and S to the caller, the five numbers of the info, the
// installation when asked for.
int hand_over(rvt_ctx* c, int64_t N, const float* dU, const std::vector<float>& S, const rvt_decompose_info& values, float* U_out,
              float* S_out, rvt_decompose_info* info, int install) {
  if (U_out) HIP_TRY(c, hipMemcpy(U_out, dU, sizeof(float) * (size_t)N * (size_t)N, hipMemcpyDeviceToHost));
  if (S_out) std::memcpy(S_out, S.data(), sizeof(float) * (size_t)N);
  if (info) *info = values;
  if (install) return rvt_set_kinship(c, N, dU, S.data());
  return RVT_OK;
}

// ---- one pass over the N^2 floats on the host (40 GB at N = 100 000): column ranges dealt to a few threads -----------------
struct KinshipScan {
  double mu = 0.0;                                       // mu_from_row_sum of K
  std::vector<std::vector<std::pair<int, int>>> edges;   // off-diagonal non-zeros (j, i), i > j, per scanning thread
  bool sparse_pattern = true;                            // false: more non-zeros than families of <= 64 could have
};

int scan_kinship(rvt_ctx* c, int64_t N, const float* K, KinshipScan* s) {
  const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)16, (int64_t)std::thread::hardware_concurrency(),
                                                               N / 512}));
  std::vector<std::vector<double>> part((size_t)nthr, std::vector<double>((size_t)N, 0.0));
  std::vector<int> bad((size_t)nthr, 0);
  s->edges.assign((size_t)nthr, {});
  std::vector<std::thread> pool;
  for (int t = 0; t < nthr; ++t)
    pool.emplace_back([&, t]() {
      std::vector<double>& rows = part[t];
      std::vector<std::pair<int, int>>& ed = s->edges[t];
      const int64_t j0 = N * t / nthr, j1 = N * (t + 1) / nthr;
      const size_t cap = (size_t)(j1 - j0) * kJacP;  // more non-zeros than families of 64 could have: a dense matrix
      bool dense_here = false;
      for (int64_t j = j0; j < j1; ++j) {
        const float* col = K + (size_t)j * N;
        for (int64_t i = 0; i < N; ++i) {
          if (!std::isfinite(col[i])) bad[t] = 1;
          rows[i] += std::fabs((double)col[i]);
          if (col[i] != 0.0f && i != j && !dense_here) {
            // edges come from the lower triangle; every off-diagonal non-zero of either triangle must have its mirror
            // image (an asymmetric matrix would silently lose cross-family entries otherwise)
            if (col[i] != K[(size_t)i * N + j]) bad[t] |= 4;
            if (i > j) {
              if (ed.size() >= cap)
                dense_here = true;
              else
                ed.emplace_back((int)j, (int)i);
            }
          }
        }
      }
      if (dense_here) bad[t] |= 2;
    });
  for (auto& th : pool) th.join();
  for (int t = 0; t < nthr; ++t) {
    if (bad[t] & 1) return fail(c, RVT_E_INVALID, "kinship matrix holds a non-finite entry");
    if (bad[t] & 4) return fail(c, RVT_E_INVALID, "kinship matrix is not symmetric");
    if (bad[t] & 2) s->sparse_pattern = false;
  }
  double max_row_sum = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    double r = 0.0;
    for (int t = 0; t < nthr; ++t) r += part[t][i];
    max_row_sum = std::max(max_row_sum, r);
  }
  s->mu = mu_from_row_sum(max_row_sum);
  return RVT_OK;
}

// ---- family by family --------------------------------------------------------------------------------------------------------
// When the sparsity pattern of K splits the samples into groups that do not interact (the connected components of its
// non-zeros: families, in whatever order the samples are listed) and none is larger than 64, the eigenproblem is that of its
// blocks: families are packed into 64 x 64 tiles (block diagonal inside a tile, distinct negative pads on the rest of the
// diagonal: zero off-diagonals are never rotated, so nothing mixes), every tile is diagonalised by the two-sided cyclic Jacobi
// kernel of the dense iteration (jac_small_eig_kernel) and the eigenpairs are merged in ascending order.
//
// The part both entries share — rvt_kinship_decompose, which finds the families in a dense K, and
// rvt_kinship_decompose_families, which is handed them with their blocks: FamTiles packs consecutive families into tiles,
// run() diagonalises the tiles [t0, t1) and checks the residual of every eigenpair.  kval(f, r, q): the entry of K between
// members r and q of family f.
struct FamTiles {
  const std::vector<int64_t>& fam_ptr;
  std::vector<int64_t> tile_fam;  // first family of every tile, nt + 1 entries
  struct Bufs {
    DevBuf<double> A, R, lam;
    DevBuf<unsigned long long> maxcos;
  } b;
  std::vector<double> A, R, lam;  // host copies of the tiles of the last run(): input, eigenvectors (row-major), eigenvalues
  double worst = 0.0;             // largest || K u - lambda u || so far

  explicit FamTiles(const std::vector<int64_t>& fp) : fam_ptr(fp) {
    int64_t rows = 0;
    for (size_t f = 0; f + 1 < fp.size(); ++f) {
      const int64_t k = fp[f + 1] - fp[f];
      if (tile_fam.empty() || rows + k > kJacP) {
        tile_fam.push_back((int64_t)f);
        rows = 0;
      }
      rows += k;
    }
    tile_fam.push_back((int64_t)fp.size() - 1);
  }
  size_t tiles() const { return tile_fam.size() - 1; }
  int64_t first_row(size_t t) const { return fam_ptr[tile_fam[t]]; }  // position in `members` of the tile's first row
  int len(size_t t) const { return (int)(fam_ptr[tile_fam[t + 1]] - fam_ptr[tile_fam[t]]); }

  int run(rvt_ctx* c, size_t t0, size_t t1, const std::function<double(int64_t, int, int)>& kval, double mu) {
    hipStream_t st = c->stream;
    const size_t n = t1 - t0, tile = (size_t)kJacP * kJacP, tile_bytes = sizeof(double) * tile;
    A.assign(n * tile, 0.0);
    for (size_t t = t0; t < t1; ++t) {
      double* a = A.data() + (t - t0) * tile;
      for (int64_t f = tile_fam[t]; f < tile_fam[t + 1]; ++f) {  // block diagonal inside the tile: K is zero between families
        const int k = (int)(fam_ptr[f + 1] - fam_ptr[f]), o = (int)(fam_ptr[f] - first_row(t));
        for (int q = 0; q < k; ++q)
          for (int r = 0; r < k; ++r) a[(size_t)(o + r) * kJacP + o + q] = kval(f, r, q);
      }
      for (int r = len(t); r < kJacP; ++r) a[(size_t)r * kJacP + r] = -mu * (1.0 + (double)r / kJacP);  // pads: last, apart
    }
    HIP_TRY(c, b.A.grow(tile_bytes * n, tile_bytes * n));
    HIP_TRY(c, b.R.grow(tile_bytes * n, tile_bytes * n));
    HIP_TRY(c, b.lam.grow(sizeof(double) * kJacP * n, sizeof(double) * kJacP * n));
    HIP_TRY(c, b.maxcos.grow(sizeof(unsigned long long), sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(b.maxcos, 0, sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemcpyAsync(b.A, A.data(), tile_bytes * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(jac_small_eig_kernel, dim3((unsigned)n), dim3(256), 0, st, b.A, 1, 1e-14, b.R, b.maxcos, 1, b.lam);
    HIP_TRY(c, hipGetLastError());
    R.resize(n * tile);
    lam.resize(n * (size_t)kJacP);
    HIP_TRY(c, hipMemcpyAsync(R.data(), b.R, tile_bytes * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(lam.data(), b.lam, sizeof(double) * kJacP * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    // the first len(t) output columns of a tile are its own eigenpairs (decreasing; the pads are below all of them)
    for (size_t t = t0; t < t1; ++t) {
      const double* a = A.data() + (t - t0) * tile;
      const double* r = R.data() + (t - t0) * tile;
      const int tl = len(t);
      for (int q = 0; q < tl; ++q) {
        const double l = lam[(t - t0) * kJacP + q];
        double res2 = 0.0;  // || K u - lambda u || inside the tile (K is zero outside)
        for (int i = 0; i < tl; ++i) {
          double s = 0.0;
          for (int k = 0; k < tl; ++k) s += a[(size_t)i * kJacP + k] * r[(size_t)k * kJacP + q];
          s -= l * r[(size_t)i * kJacP + q];
          res2 += s * s;
        }
        worst = std::max(worst, std::sqrt(res2));
      }
    }
    return RVT_OK;
  }
};

// Not mine: K is not of that form (a family larger than a tile, one family only), or a tile did not converge.
Outcome decompose_by_family(rvt_ctx* c, int64_t N, const float* K, const KinshipScan& scan, float* U_out, float* S_out, int install,
                            rvt_decompose_info* info) {
  // families = connected components of the sparsity pattern (union-find over the off-diagonal non-zeros)
  Components cc(N);
  for (const auto& ed : scan.edges)
    for (const auto& e : ed)
      if (!cc.join(e.first, e.second, kJacP)) return not_mine();  // a family larger than a tile
  // members of every family in ascending order; families in the order of their first member
  std::vector<int64_t> fam_ptr;
  std::vector<int> members;
  cc.list(&fam_ptr, &members);
  if (fam_ptr.size() < 3) return not_mine();
  // tiles of consecutive families: the sample index behind row r of tile t is members[first_row(t) + r]
  FamTiles ft(fam_ptr);
  const size_t nt = ft.tiles();
  std::vector<int> tlen;
  for (size_t t = 0; t < nt; ++t) tlen.push_back(ft.len(t));
  int rc = ft.run(c, 0, nt, [&](int64_t f, int r, int q) {
    const int* m = members.data() + fam_ptr[f];
    return (double)K[(size_t)m[r] + (size_t)m[q] * N];
  }, scan.mu);
  if (rc) return rc;
  hipStream_t st = c->stream;
  struct Bufs {
    DevBuf<float> dU;
    DevBuf<int> meta;
  } b;
  struct Pair {
    double lam;
    int tile, col;
  };
  std::vector<Pair> pairs;
  pairs.reserve((size_t)N);
  for (size_t t = 0; t < nt; ++t)
    for (int q = 0; q < tlen[t]; ++q) pairs.push_back({ft.lam[t * kJacP + q], (int)t, q});
  if ((int64_t)pairs.size() != N) return fail(c, RVT_E_STATE, "family-wise decomposition lost eigenpairs");
  // the 30 cyclic sweeps of jac_small_eig_kernel converge for every family tile seen so far; should one not have, the
  // dense routes (which check their own convergence and residuals) take the matrix instead
  if (ft.worst > 1e-9 * scan.mu) return not_mine();
  std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& x, const Pair& y) { return x.lam < y.lam; });  // ascending
  std::vector<float> S((size_t)N);
  std::vector<int> meta(3 * (size_t)N + nt * (size_t)kJacP, 0);  // tile | column | length per eigenpair, rows per tile
  for (int64_t k = 0; k < N; ++k) {
    S[k] = (float)pairs[k].lam;
    meta[k] = pairs[k].tile;
    meta[(size_t)N + k] = pairs[k].col;
    meta[2 * (size_t)N + k] = tlen[pairs[k].tile];
  }
  for (size_t t = 0; t < nt; ++t)
    for (int r = 0; r < tlen[t]; ++r) meta[3 * (size_t)N + t * kJacP + r] = members[ft.first_row(t) + r];
  if (U_out || install) {
    HIP_TRY(c, b.dU.alloc(sizeof(float) * (size_t)N * (size_t)N));
    HIP_TRY(c, hipMemsetAsync(b.dU, 0, sizeof(float) * (size_t)N * (size_t)N, st));
    HIP_TRY(c, b.meta.alloc(sizeof(int) * meta.size()));
    HIP_TRY(c, hipMemcpyAsync(b.meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(jac_scatter_blocks_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, ft.b.R, b.meta,
                       b.meta + N, b.meta + 2 * N, b.meta + 3 * N, (long long)N, b.dU);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
  }
  // (no block sweeps: every family is an eigenproblem of its own)
  return hand_over(c, N, b.dU, S, {0, 0.0, jac_padded_order(N), 0.0, ft.worst}, U_out, S_out, info, install);
}

// ---- dense kinship: tridiagonalisation + bisection + inverse iteration (tridiag_kernels.hip.h) ------------------------------
// Done when U and S were produced AND passed the closing check (residual, orthogonality); not mine when the matrix has
// eigenvalues closer than the inverse iteration separates, the check failed, or the device has no room for the work areas:
// the caller then runs the Jacobi iteration.
//
// The work areas of the route and its five stages.  Peak: the matrix with its reflectors (A), the eigenvectors (Z) and the float
// matrix for the closing check — 20 N^2 bytes (the inverse iteration's factors are kept for a batch of eigenvectors at a time
// and the check's fp64 copy of K re-uses A).  The order of the allocations and releases is what holds it there:
//   buffer  holds                                                  born in         freed in
//   dK      the caller's K in float                                reduce, check   the same stage, behind its conversion
//   A       K in fp64, then the reflectors; K again for the check  reduce          emit (before dU is born)
//   W, P    the panel's W; partial products of a column step       reduce          check
//   vec     the vectors named below                                reduce          (the end)
//   Z       eigenvectors of T, then of K                           eigenvectors    emit (behind the conversion to float)
//   fac     the inverse iteration's factors of one batch           eigenvectors    eigenvectors
//   cz, yy  V'Z; Y', V' and the panel's Gram matrix                back-transform  check
//   worst   largest residual | largest |U'U - I| (bits)            check           (the end)
//   kz      K Z and Z'Z of a batch of columns                      check           (the end)
//   dU      U in float                                             emit            (the end)
struct Tridiag {
  rvt_ctx* const c;
  const hipStream_t st;
  const int64_t N;
  const float* const K;
  const double mu;
  const bool trace = getenv("RVT_TRIDIAG_TRACE") != nullptr;
  const int n = (int)N;
  const int64_t ld = (N + 63) / 64 * 64;
  const size_t mat = sizeof(double) * (size_t)ld * (size_t)N;
  DevBuf<float> dK, dU;
  DevBuf<double> A, fac, Z, kz, W, vec, cz, yy, P;
  DevBuf<unsigned long long> worst;
  // vec: d | e | tau | y | t12 (2 kTdNb) | partial dots | scaled d | scaled e^2 | lambda
  const int64_t vs = std::max<int64_t>(ld, 1024);  // (y doubles as the panel's Gram matrix later)
  const int comb_blocks = (int)((N + 63) / 64);    // workgroups of td_w_comb_kernel = partial dots per column
  const int64_t n_part = std::max<int64_t>(1024, comb_blocks);
  const size_t nv = 7 * (size_t)vs + 2 * kTdNb + (size_t)n_part;
  double *d_d, *d_e, *d_tau, *d_y, *d_t12, *d_part, *d_ss, *d_ds, *d_e2s, *d_lam;  // (named once vec is born)
  std::vector<double> hd, he, lam;  // T's diagonal and off-diagonal, its eigenvalues (ascending)
  double span0 = 0.0, resid = 0.0;  // the Gershgorin span of T; the closing check's largest |K u - lambda u|
  double t_start = now_s(), t_tri = 0.0, t_eig = 0.0, t_vec = 0.0, t_back = 0.0;
  Tridiag(rvt_ctx* c_, int64_t N_, const float* K_, double mu_) : c(c_), st(c_->stream), N(N_), K(K_), mu(mu_) {}

  // an allocation the device cannot serve (fragmentation, another context) is not an error of the call: the gemms' K slices
  // go, and the matrix is left to the Jacobi iteration, as the size check of reduce() promises
  Outcome alloc_failed() {
    (void)hipGetLastError();
    c->d_rot_part.reset();
    if (trace) fprintf(stderr, "[rvt] tridiag: device allocation failed: left to the Jacobi iteration\n");
    return not_mine();
  }

  // 1. K = Q T Q'
  Outcome reduce() {
    {
      // When the device cannot hold the peak (other contexts, a large block pool) the Jacobi iteration (16 N^2 bytes) gets the
      // matrix instead of an allocation failure.  (Nothing of the route's is held yet: the gemms' K slices stay.)
      size_t free_b = 0, total_b = 0;
      const size_t need = 2 * mat + sizeof(float) * (size_t)N * (size_t)N + sizeof(double) * (size_t)ld * (4 * kTdNbb + kTdNb + 16 * 1024) +
                          ((size_t)2 << 30);
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need) {
        (void)hipGetLastError();
        if (trace) fprintf(stderr, "[rvt] tridiag: %zu MB needed, %zu MB free: left to the Jacobi iteration\n", need >> 20, free_b >> 20);
        return not_mine();
      }
    }
    if (dK.alloc(sizeof(float) * (size_t)N * (size_t)N) != hipSuccess) return alloc_failed();
    if (A.alloc(mat) != hipSuccess) return alloc_failed();
    if (W.alloc(sizeof(double) * (size_t)ld * kTdNb) != hipSuccess) return alloc_failed();
    if (vec.alloc(sizeof(double) * nv) != hipSuccess) return alloc_failed();
    HIP_TRY(c, hipMemsetAsync(vec, 0, sizeof(double) * nv, st));
    HIP_TRY(c, hipMemsetAsync(W, 0, sizeof(double) * (size_t)ld * kTdNb, st));
    d_d = vec, d_e = d_d + vs, d_tau = d_e + vs, d_y = d_tau + vs, d_t12 = d_y + vs, d_part = d_t12 + 2 * kTdNb, d_ss = d_y;
    d_ds = d_part + n_part, d_e2s = d_ds + vs, d_lam = d_e2s + vs;
    HIP_TRY(c, hipMemcpyAsync(dK, K, sizeof(float) * (size_t)N * (size_t)N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(td_init_kernel, dim3(4096), dim3(256), 0, st, dK, (long long)N, (long long)ld, A);
    const int nblk = (int)((N + kSyT - 1) / kSyT);  // 64-row blocks of the matrix; P: the (nblk + 1) x ld partial products of a column step
    if (P.alloc(sizeof(double) * (size_t)(nblk + 1) * (size_t)ld) != hipSuccess) return alloc_failed();
    for (int j0 = 0; j0 < n; j0 += kTdNb) {
      const int j1 = std::min(n, j0 + kTdNb);
      for (int j = j0; j < j1; ++j) {
        const int n_ss = (n - j + 255) / 256;
        hipLaunchKernelGGL(td_col_update_kernel, dim3((unsigned)n_ss), dim3(256), 0, st, A, (long long)N, (long long)ld, j, j0, W, d_ss);
        hipLaunchKernelGGL(td_col_house_kernel, dim3(1), dim3(1024), 0, st, A, (long long)N, (long long)ld, j, d_ss, n_ss, d_d, d_e,
                           d_tau);
        if (j + 1 >= n) continue;
        const int i = j - j0;
        const int nbt = nblk - (j + 1) / kSyT, groups = (nbt + kSyRun - 1) / kSyRun;
        hipLaunchKernelGGL(td_symv_kernel, dim3((unsigned)groups, (unsigned)(nbt + (2 * i + groups - 1) / groups)), dim3(256), 0, st, A,
                           (long long)N, (long long)ld, j, j0, nbt, W, P, d_t12);
        hipLaunchKernelGGL(td_w_comb_kernel, dim3((unsigned)comb_blocks), dim3(256), 0, st, A, (long long)N, (long long)ld, j, j0, W, P,
                           nblk, d_t12, d_tau, d_part);
        hipLaunchKernelGGL(td_w_final_kernel, dim3(1), dim3(1024), 0, st, A, (long long)N, (long long)ld, j, j0, W, d_tau, d_part,
                           comb_blocks);
      }
      if (j1 < n) {
        const unsigned tiles = (unsigned)((n - j1 + 63) / 64);
        hipLaunchKernelGGL(td_rank2k_kernel, dim3(tiles, tiles), dim3(256), 0, st, A, (long long)N, (long long)ld, j0, j1, W);
      }
    }
    HIP_TRY(c, hipGetLastError());
    hd.assign((size_t)N, 0.0);
    he.assign((size_t)N, 0.0);
    HIP_TRY(c, hipMemcpyAsync(hd.data(), d_d, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(he.data(), d_e, sizeof(double) * (size_t)(N - 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    dK.reset();
    t_tri = now_s();
    return RVT_OK;
  }

  // 2. eigenvalues of T (scaled as coop_tridiag_eigvals scales: Gershgorin span into [1/2, 1), squares floored)
  Outcome eigenvalues() {
    double lo = hd[0], hi = hd[0];
    for (int64_t j = 0; j < N; ++j) {
      if (!std::isfinite(hd[j]) || !std::isfinite(he[j])) return not_mine();  // (the Jacobi iteration reports what is wrong)
      const double r = (j > 0 ? std::fabs(he[j - 1]) : 0.0) + (j < N - 1 ? std::fabs(he[j]) : 0.0);
      lo = std::min(lo, hd[j] - r);
      hi = std::max(hi, hd[j] + r);
    }
    span0 = std::max(std::fabs(lo), std::fabs(hi));
    if (!(span0 > 0.0)) return not_mine();
    int sh = 0;
    (void)std::frexp(span0, &sh);
    {
      std::vector<double> ds((size_t)N), e2s((size_t)N, 0.0);
      for (int64_t j = 0; j < N; ++j) {
        ds[j] = std::ldexp(hd[j], -sh);
        if (j < N - 1) {
          const double es = std::ldexp(he[j], -sh);
          e2s[j] = std::max(es * es, 0x1p-200);
        }
      }
      HIP_TRY(c, hipMemcpyAsync(d_ds, ds.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(d_e2s, e2s.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
      HIP_TRY(c, sync_stream(st));
    }
    const double slo = std::ldexp(lo, -sh), shi = std::ldexp(hi, -sh), span = std::max(std::fabs(slo), std::fabs(shi));
    const double pivmin = DBL_MIN * 1024.0, slack = 2.0 * kDblEps * span * (double)N + 2.0 * pivmin;
    hipLaunchKernelGGL(td_eigvals_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, d_ds, d_e2s, n, slo - slack, shi + slack,
                       span, sh, d_lam);
    lam.resize((size_t)N);
    HIP_TRY(c, hipMemcpyAsync(lam.data(), d_lam, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    t_eig = now_s();
    // gaps: the inverse iteration is not reorthogonalised
    double min_gap = span0;
    for (int64_t j = 1; j < N; ++j) min_gap = std::min(min_gap, lam[j] - lam[j - 1]);
    if (trace) fprintf(stderr, "[rvt] tridiag: N %lld, reduction %.3f s, eigenvalues %.3f s, smallest gap %.3g of %.3g\n", (long long)N,
                       t_tri - t_start, t_eig - t_tri, min_gap, span0);
    // neighbours a gap g apart come out orthogonal to ~ eps |T| / g: 4e-9 of the norm promises 6e-8, float rounding of the U the
    // boundary stores (the closing check holds the result to 1e-7 whatever this predicts)
    if (!(min_gap > 4e-9 * span0)) return not_mine();
    return RVT_OK;
  }

  // 3. eigenvectors of T, a batch of columns at a time (the factors of a batch: three [row][eigenvector] arrays + the vectors)
  Outcome eigenvectors() {
    if (Z.alloc(mat) != hipSuccess) return alloc_failed();
    HIP_TRY(c, hipMemsetAsync(Z, 0, mat, st));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
    int64_t nkb = (int64_t)((free_b / 2) / (4 * sizeof(double) * (size_t)ld)) / 64 * 64;  // half of what is free
    if (const char* e = getenv("RVT_TRIDIAG_BATCH")) nkb = std::max(64, atoi(e) / 64 * 64);  // (tests: several batches on a small matrix)
    nkb = std::max<int64_t>(64, std::min<int64_t>(nkb, ld));
    const size_t arr = sizeof(double) * (size_t)ld * (size_t)nkb;
    if (fac.alloc(4 * arr) != hipSuccess) return alloc_failed();
    double *zt = fac, *ud = zt + (size_t)ld * nkb, *uu = ud + (size_t)ld * nkb, *uw = uu + (size_t)ld * nkb;
    for (int64_t k0 = 0; k0 < N; k0 += nkb) {
      const int nk = (int)std::min<int64_t>(nkb, N - k0);
      hipLaunchKernelGGL(td_invit_kernel, dim3((unsigned)((nk + 63) / 64)), dim3(64), 0, st, d_d, d_e, n, d_lam + k0, nk, (long long)k0, (long long)nkb,
                         kDblEps * span0, ud, uu, uw, zt);
      hipLaunchKernelGGL(td_transpose_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((nk + 31) / 32)), dim3(256), 0, st, zt,
                         (long long)nkb, n, nk, (long long)ld, Z + (size_t)k0 * ld);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    fac.reset();
    t_vec = now_s();
    return RVT_OK;
  }

  // 4. U = Q Z, the reflectors kTdNbb at a time in reverse order: G = V'V and V'Z (K = N), the back substitution with
  //    T^-1 = triu(G, 1) + diag(1 / tau), and Z -= V Y' (K = kTdNbb) — all three products on the matrix cores
  Outcome back_transform() {
    if (cz.alloc(sizeof(double) * (size_t)ld * kTdNbb) != hipSuccess) return alloc_failed();
    if (yy.alloc(sizeof(double) * (size_t)ld * kTdNbb * 2 + sizeof(double) * kTdNbb * kTdNbb) != hipSuccess) return alloc_failed();
    double *d_yt = yy, *d_vt = yy + (size_t)ld * kTdNbb, *d_gram = d_vt + (size_t)ld * kTdNbb;
    HIP_TRY(c, hipMemsetAsync(d_gram, 0, sizeof(double) * kTdNbb * kTdNbb, st));
    for (int j0 = ((n - 1) / kTdNbb) * kTdNbb; j0 >= 0; j0 -= kTdNbb) {
      const int nbp = std::min(n, j0 + kTdNbb) - j0;
      const double* Vp = A + (size_t)j0 * ld;
      ROUTE_TRY(gemm_or_not_mine(c, gemm_tn_f64(c, Vp, ld, nbp, Vp, ld, nbp, nullptr, 0, 0, nullptr, ld, d_gram, kTdNbb, true, st)));
      ROUTE_TRY(gemm_or_not_mine(c, gemm_tn_f64(c, Z, ld, n, Vp, ld, nbp, nullptr, 0, 0, nullptr, ld, cz, ld, false, st)));
      hipLaunchKernelGGL(td_rsolve_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, cz, (long long)ld, n, nbp, d_gram,
                         d_tau + j0, d_yt);
      hipLaunchKernelGGL(td_panel_transpose_kernel, dim3((unsigned)((N + 31) / 32), kTdNbb / 32), dim3(256), 0, st, A, (long long)N,
                         (long long)ld, j0, nbp, d_vt);
      ROUTE_TRY(gemm_or_not_mine(c, gemm_tn_f64(c, d_vt, kTdNbb, n, d_yt, kTdNbb, n, nullptr, 0, 0, nullptr, kTdNbb, Z, ld, false, st, true)));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    t_back = now_s();
    return RVT_OK;
  }

  // 5. the closing check: max |K u - lambda u|, max |U'U - I|, in column batches (the product's K slices need room)
  Outcome closing_check() {
    if (worst.alloc(2 * sizeof(unsigned long long)) != hipSuccess) return alloc_failed();
    HIP_TRY(c, hipMemsetAsync(worst, 0, 2 * sizeof(unsigned long long), st));
    for (DevBuf<double>* q : {&cz, &yy, &W, &P}) q->reset();
    if (dK.alloc(sizeof(float) * (size_t)N * (size_t)N) != hipSuccess) return alloc_failed();
    HIP_TRY(c, hipMemcpyAsync(dK, K, sizeof(float) * (size_t)N * (size_t)N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(td_init_kernel, dim3(4096), dim3(256), 0, st, dK, (long long)N, (long long)ld, A);
    HIP_TRY(c, sync_stream(st));
    dK.reset();
    constexpr int kBatch = 1024;
    if (kz.alloc(sizeof(double) * (size_t)ld * kBatch) != hipSuccess) return alloc_failed();
    for (int k0 = 0; k0 < n; k0 += kBatch) {
      const int nk = std::min(kBatch, n - k0);
      const double* Zk = Z + (size_t)k0 * ld;
      ROUTE_TRY(gemm_or_not_mine(c, gemm_tn_f64(c, A, ld, n, Zk, ld, nk, nullptr, 0, 0, nullptr, ld, kz, ld, false, st)));
      hipLaunchKernelGGL(td_residual_kernel, dim3((unsigned)nk), dim3(256), 0, st, kz, (long long)ld, Zk, (long long)ld, n, d_lam + k0,
                         worst);
      ROUTE_TRY(gemm_or_not_mine(c, gemm_tn_f64(c, Z, ld, n, Zk, ld, nk, nullptr, 0, 0, nullptr, ld, kz, ld, false, st)));
      hipLaunchKernelGGL(td_orth_kernel, dim3((unsigned)nk), dim3(256), 0, st, kz, (long long)ld, n, k0, worst);
    }
    unsigned long long bits[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(bits, worst, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    double orth;
    std::memcpy(&resid, &bits[0], 8);
    std::memcpy(&orth, &bits[1], 8);
    const double t_chk = now_s();
    if (trace)
      fprintf(stderr, "[rvt] tridiag: vectors %.3f s, back-transformation %.3f s, check %.3f s: residual %.3g (scale %.3g), |U'U - I| %.3g\n",
              t_vec - t_eig, t_back - t_vec, t_chk - t_back, resid, span0, orth);
    if (!(resid <= 1e-9 * mu) || !(orth <= 1e-7)) {  // (mu = 4 x a bound on the spectral radius; Jacobi's own bar)
      c->d_rot_part.reset();  // (the products' K slices: the Jacobi iteration that takes over needs the room)
      return not_mine();
    }
    return RVT_OK;
  }

  // U in float in place of A; Z and the K slices of the check's products (GBs at this size) go before the installation, which
  // needs room for the digit planes of U
  Outcome emit(float* U_out, float* S_out, int install, rvt_decompose_info* info) {
    std::vector<float> S((size_t)N);
    for (int64_t j = 0; j < N; ++j) S[j] = (float)lam[j];
    A.reset();
    if (dU.alloc(sizeof(float) * (size_t)N * (size_t)N) != hipSuccess) return alloc_failed();
    hipLaunchKernelGGL(td_to_float_kernel, dim3(4096), dim3(256), 0, st, Z, (long long)ld, (long long)N, dU);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    Z.reset();
    c->d_rot_part.reset();
    return hand_over(c, N, dU, S, {0, 0.0, ld, 0.0, resid}, U_out, S_out, info, install);  // (no Jacobi sweeps)
  }
};

Outcome decompose_dense_tridiag(rvt_ctx* c, int64_t N, const float* K, double mu, float* U_out, float* S_out, int install,
                                rvt_decompose_info* info) {
  Tridiag t(c, N, K, mu);
  ROUTE_TRY(t.reduce());
  ROUTE_TRY(t.eigenvalues());
  ROUTE_TRY(t.eigenvectors());
  ROUTE_TRY(t.back_transform());
  ROUTE_TRY(t.closing_check());
  return t.emit(U_out, S_out, install, info);
}

// ---- dense kinship: the one-sided block Jacobi iteration (jacobi_kernels.hip.h) ---------------------------------------------
// The last route: what it cannot allocate, or does not converge on, is an error of the call.
struct Jacobi {
  rvt_ctx* const c;
  const hipStream_t st;
  const int64_t N;
  const float* const K;
  const double mu;
  const int64_t np = jac_padded_order(N);
  const int nb = (int)(np / kJacB), pairs = nb / 2;
  // row splits of the Gram pass / row slabs of the update: enough waves to fill the chip when there are few pairs
  const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(np / 64, (1024 + pairs - 1) / pairs / 4));
  const int nparts = splits * 4, slabs = splits;
  DevBuf<float> dK;
  DevBuf<double> W, V, part, R, lam;
  DevBuf<unsigned long long> maxcos;
  DevBuf<float> dU;
  DevBuf<int> dsrc;
  int total_sweeps = 0;
  double last = 0.0, shift = 0.0, worst_resid = 0.0;  // the last sweep's largest cosine, the second attempt's shift, max |K u - lambda u|
  std::vector<double> h_lam;                          // lambda of the np columns, the shift taken off
  Jacobi(rvt_ctx* c_, int64_t N_, const float* K_, double mu_) : c(c_), st(c_->stream), N(N_), K(K_), mu(mu_) {}

  // sweeps until every cross-block cosine is below 1e-10; a large residual at the end (nearly opposite eigenvalues) sends
  // K + shift I through a second time
  int iterate() {
    const size_t nn = (size_t)np * (size_t)np;
    HIP_TRY(c, V.alloc(sizeof(double) * nn));
    HIP_TRY(c, part.alloc(sizeof(double) * (size_t)pairs * nparts * kJacP * kJacP));
    HIP_TRY(c, R.alloc(sizeof(double) * (size_t)pairs * kJacP * kJacP));
    HIP_TRY(c, lam.alloc(sizeof(double) * 2 * (size_t)np));
    HIP_TRY(c, maxcos.alloc(sizeof(unsigned long long)));
    const double tol = 1e-10;
    const int max_sweeps = 40;
    const int sort_mode = getenv("RVT_JACOBI_NOSORT") ? 0 : 1;
    std::vector<double> resid((size_t)np);
    h_lam.resize((size_t)np);
    for (int attempt = 0; attempt < 2; ++attempt) {
      HIP_TRY(c, W.grow(sizeof(double) * nn, sizeof(double) * nn));
      HIP_TRY(c, dK.alloc(sizeof(float) * (size_t)N * (size_t)N));
      HIP_TRY(c, hipMemcpyAsync(dK, K, sizeof(float) * (size_t)N * (size_t)N, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(jac_init_kernel, dim3(4096), dim3(256), 0, st, dK, (long long)N, (long long)np, mu + shift, shift, W, V);
      HIP_TRY(c, sync_stream(st));
      dK.reset();
      int sweeps = 0;
      while (sweeps < max_sweeps) {
        HIP_TRY(c, hipMemsetAsync(maxcos, 0, sizeof(unsigned long long), st));
        for (int r = 0; r < nb - 1; ++r) {
          hipLaunchKernelGGL(jac_gram_kernel, dim3((unsigned)pairs, (unsigned)splits), dim3(256), 0, st, W, (long long)np, nb, r, splits,
                             part);
          hipLaunchKernelGGL(jac_small_eig_kernel, dim3((unsigned)pairs), dim3(256), 0, st, part, nparts, 1e-15, R, maxcos, sort_mode);
          hipLaunchKernelGGL(jac_apply_kernel, dim3((unsigned)pairs, (unsigned)slabs, 2), dim3(256), 0, st, W, V, (long long)np, nb, r, R);
        }
        HIP_TRY(c, hipGetLastError());
        unsigned long long bits = 0;
        HIP_TRY(c, hipMemcpyAsync(&bits, maxcos, sizeof(bits), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, sync_stream(st));
        std::memcpy(&last, &bits, sizeof(last));
        ++sweeps;
        if (getenv("RVT_JACOBI_TRACE")) fprintf(stderr, "[rvt] jacobi sweep %d: max cosine %.3e\n", sweeps, last);
        if (last < tol) break;
      }
      total_sweeps += sweeps;
      if (!(last < tol))
        return fail(c, RVT_E_INVALID, "kinship decomposition did not converge (cosine %.3g after %d sweeps)", last, sweeps);
      hipLaunchKernelGGL(jac_lambda_kernel, dim3((unsigned)np), dim3(256), 0, st, W, V, (long long)np, lam, lam + np);
      HIP_TRY(c, hipMemcpyAsync(h_lam.data(), lam, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(resid.data(), lam + np, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      worst_resid = 0.0;
      for (int64_t j = 0; j < np; ++j) worst_resid = std::max(worst_resid, resid[j]);
      if (worst_resid <= 1e-9 * mu || attempt == 1) break;
      shift = 0.26 * mu;  // mu = 4 x (bound on the spectral radius): K + shift I is positive definite
    }
    for (int64_t j = 0; j < np; ++j) h_lam[j] -= shift;
    W.reset();  // (80 GB at N = 100 000)
    return RVT_OK;
  }

  // the N columns that are not pads, in ascending order of lambda (as Eigen returns them), gathered from V as floats
  int emit(float* U_out, float* S_out, int install, rvt_decompose_info* info) {
    std::vector<int> src;
    src.reserve((size_t)N);
    for (int64_t j = 0; j < np; ++j)
      if (h_lam[j] > -0.5 * mu - shift) src.push_back((int)j);
    if ((int64_t)src.size() != N) return fail(c, RVT_E_INVALID, "kinship decomposition: %zu of %lld eigenpairs separated", src.size(), (long long)N);
    std::stable_sort(src.begin(), src.end(), [&](int x, int y) { return h_lam[x] < h_lam[y]; });
    std::vector<float> S((size_t)N);
    for (int64_t j = 0; j < N; ++j) S[j] = (float)h_lam[src[j]];
    HIP_TRY(c, dsrc.alloc(sizeof(int) * (size_t)N));
    HIP_TRY(c, hipMemcpyAsync(dsrc, src.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(c, dU.alloc(sizeof(float) * (size_t)N * (size_t)N));
    hipLaunchKernelGGL(jac_gather_kernel, dim3((unsigned)N), dim3(256), 0, st, V, (long long)np, (long long)N, dsrc, dU);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    V.reset();
    return hand_over(c, N, dU, S, {total_sweeps, last, np, shift, worst_resid}, U_out, S_out, info, install);
  }
};

int decompose_dense_jacobi(rvt_ctx* c, int64_t N, const float* K, double mu, float* U_out, float* S_out, int install,
                           rvt_decompose_info* info) {
  Jacobi j(c, N, K, mu);
  const int rc = j.iterate();
  return rc ? rc : j.emit(U_out, S_out, install, info);
}

// symmetry of every family's kinship block and mu_from_row_sum over them, as rvt_kinship_decompose scales its pads and its
// residual bar
int scan_kinship_blocks(rvt_ctx* c, int64_t n_fam, const int64_t* fam_ptr, const std::vector<long long>& blk_off,
                        const float* K_blocks, double* mu) {
  double max_row_sum = 0.0;
  for (int64_t f = 0; f < n_fam; ++f) {
    const int k = (int)(fam_ptr[f + 1] - fam_ptr[f]);
    const float* b = K_blocks + blk_off[f];
    for (int r = 0; r < k; ++r) {
      double s = 0.0;
      for (int q = 0; q < k; ++q) {
        if (b[r + (size_t)q * k] != b[q + (size_t)r * k])
          return fail(c, RVT_E_INVALID, "kinship families: the kinship block of family %lld is not symmetric", (long long)f);
        s += std::fabs((double)b[r + (size_t)q * k]);
      }
      max_row_sum = std::max(max_row_sum, s);
    }
  }
  *mu = mu_from_row_sum(max_row_sum);
  return RVT_OK;
}
}  // namespace

extern "C" {

int rvt_kinship_components(int64_t N, int64_t n_pairs, const int32_t* pi, const int32_t* pj, int64_t* n_fam,
                           int64_t* fam_ptr, int32_t* members) {
  if (N < 1 || N > INT32_MAX || n_pairs < 0 || (n_pairs && (!pi || !pj)) || !n_fam || !fam_ptr || !members) return RVT_E_INVALID;
  for (int64_t e = 0; e < n_pairs; ++e)
    if (pi[e] < 0 || pi[e] >= N || pj[e] < 0 || pj[e] >= N) return RVT_E_INVALID;
  Components cc(N);
  for (int64_t e = 0; e < n_pairs; ++e) cc.join(pi[e], pj[e], 0);
  std::vector<int64_t> fp;
  std::vector<int> mem;
  cc.list(&fp, &mem);
  *n_fam = (int64_t)fp.size() - 1;
  std::copy(fp.begin(), fp.end(), fam_ptr);
  std::copy(mem.begin(), mem.end(), members);
  return RVT_OK;
}

int rvt_kinship_decompose(rvt_ctx* c, int64_t N, const float* K, float* U_out, float* S_out, int install,
                          rvt_decompose_info* info) {
  if (!c || !K || N < 2) return fail(c, RVT_E_INVALID, "bad kinship matrix");
  if (N > (int64_t)1 << 20) return fail(c, RVT_E_TOO_LARGE, "kinship of %lld samples", (long long)N);
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  KinshipScan scan;
  rc = scan_kinship(c, N, K, &scan);
  if (rc) return rc;
  // a block-diagonal (pedigree) kinship is decomposed family by family
  if (!getenv("RVT_KINSHIP_DENSE") && scan.sparse_pattern) {
    const Outcome o = decompose_by_family(c, N, K, scan, U_out, S_out, install, info);
    if (o.kind != Outcome::kNotMine) return o.rc;
  }
  // a dense matrix whose work areas fit (20 N^2 bytes at the peak): tridiagonalisation + bisection + inverse iteration;
  // repeated eigenvalues (and anything that fails its closing check) fall through to the Jacobi iteration
  if (!getenv("RVT_KINSHIP_JACOBI") && N >= 128) {
    const Outcome o = decompose_dense_tridiag(c, N, K, scan.mu, U_out, S_out, install, info);
    if (o.kind != Outcome::kNotMine) return o.rc;
  }
  return decompose_dense_jacobi(c, N, K, scan.mu, U_out, S_out, install, info);
}

// The family-wise decomposition fed from blocks: the tiles of decompose_by_family (FamTiles), a bounded number at a time, the
// eigenvectors written back as blocks and installed through the family form.  Nothing of order N^2 exists at any point.
int rvt_kinship_decompose_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                                   const float* K_blocks, float* U_blocks_out, float* S_out, int install,
                                   rvt_decompose_info* info) {
  if (!c || !K_blocks) return fail(c, RVT_E_INVALID, "bad kinship families");
  std::vector<long long> blk_off;
  int rc = check_families(c, N, n_fam, fam_ptr, members, &blk_off);
  if (rc) return rc;
  rc = check_blocks_finite(c, n_fam, fam_ptr, blk_off, K_blocks, "the kinship block");
  if (rc) return rc;
  double mu = 0.0;
  rc = scan_kinship_blocks(c, n_fam, fam_ptr, blk_off, K_blocks, &mu);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  const std::vector<int64_t> fp(fam_ptr, fam_ptr + n_fam + 1);
  FamTiles ft(fp);
  const bool want_u = U_blocks_out || install;
  std::vector<float> Ub(want_u && !U_blocks_out ? (size_t)blk_off[n_fam] : 0), Sb(S_out ? 0 : (size_t)N);
  float* U = U_blocks_out ? U_blocks_out : Ub.data();
  float* S = S_out ? S_out : Sb.data();
  const auto kval = [&](int64_t f, int r, int q) {
    return (double)K_blocks[blk_off[f] + r + (size_t)q * (size_t)(fp[f + 1] - fp[f])];
  };
  constexpr size_t kChunk = 2048;  // tiles per pass: 64 MB of tiles each way
  std::vector<int> cols;
  for (size_t t0 = 0; t0 < ft.tiles(); t0 += kChunk) {
    const size_t t1 = std::min(ft.tiles(), t0 + kChunk);
    rc = ft.run(c, t0, t1, kval, mu);
    if (rc) return rc;
    for (size_t t = t0; t < t1; ++t) {
      const double* r = ft.R.data() + (t - t0) * (size_t)kJacP * kJacP;
      const double* lam = ft.lam.data() + (t - t0) * (size_t)kJacP;
      const int tl = ft.len(t);
      for (int64_t f = ft.tile_fam[t]; f < ft.tile_fam[t + 1]; ++f) {
        // the family's eigenpairs among the tile's: the columns whose largest entry lies in the family's rows (zero
        // off-diagonals are never rotated, so a column is non-zero inside one family only)
        const int k = (int)(fp[f + 1] - fp[f]), o = (int)(fp[f] - ft.first_row(t));
        cols.clear();
        for (int q = 0; q < tl; ++q) {
          int best = 0;
          for (int i = 1; i < tl; ++i)
            if (std::fabs(r[(size_t)i * kJacP + q]) > std::fabs(r[(size_t)best * kJacP + q])) best = i;
          if (best >= o && best < o + k) cols.push_back(q);
        }
        if ((int)cols.size() != k)
          return fail(c, RVT_E_STATE, "family-wise decomposition: family %lld got %zu of its %d eigenpairs", (long long)f,
                      cols.size(), k);
        std::stable_sort(cols.begin(), cols.end(), [&](int x, int y) { return lam[x] < lam[y]; });  // ascending
        for (int j = 0; j < k; ++j) {
          S[fp[f] + j] = (float)lam[cols[j]];
          if (want_u)
            for (int i = 0; i < k; ++i) U[blk_off[f] + i + (size_t)j * k] = (float)r[(size_t)(o + i) * kJacP + cols[j]];
        }
      }
    }
  }
  if (ft.worst > 1e-9 * mu)
    return fail(c, RVT_E_INVALID, "family-wise kinship decomposition did not converge: residual %.3g against %.3g", ft.worst,
                1e-9 * mu);
  if (info) *info = {0, 0.0, jac_padded_order(N), 0.0, ft.worst};  // (no block sweeps: every family is an eigenproblem of its own)
  if (!install) return RVT_OK;
  ft.b = FamTiles::Bufs();  // (the tiles' device buffers go before the installation)
  return install_families(c, N, n_fam, fam_ptr, members, blk_off, U, S);
}

}  // extern "C"
