// rvtests_amd — related samples: the kinship (installation from dense U or from family blocks, family structure; its
// eigendecomposition is rvt_decompose.hip's), the exact integer rotation G~ = U'G (rot_gemm.hip.h), the FastLMM null model,
// FamSKAT / the family burden tests / the family forms of MetaCov and MetaScore.  Part of librvtests_amd.so; the per-gene
// pipeline behind it is rvt_engine.hip's.
// this unit compiles (and ships) the FAM kernel family only: see "kernel families" in rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_FAM
#include "rvt_engine_int.h"
#include "fam_single.hip.h"
#include "fam_bed_kernels.hip.h"
#include "grammar_bed_kernels.hip.h"

static void free_csc(rvt_ctx* c) {  // the column-compressed form of U
  c->d_csc_ptr.reset();
  c->d_csc_rows.reset();
  c->d_csc_vals.reset();
}

static void clear_kinship(rvt_ctx* c) {  // what both forms of the installation start from
  c->d_S.reset();
  c->d_u1.reset();
  c->d_Uq.reset();
  c->d_uq_range.reset();
  free_csc(c);
  c->d_csr_ptr.reset();
  c->d_csr_cols.reset();
  c->d_csr_vals.reset();
  c->d_fam_ptr.reset();
  c->d_fam_members.reset();
  c->d_fam_of.reset();
  c->d_fam_run.reset();
  c->fam_count = 0;
  c->fam_runs = 0;
  c->uq_visit = 1.0;
  c->have_kin = c->have_fam = c->have_grammar = false;
}

extern "C" {

int ensure_fam_cols(rvt_ctx* c, size_t T, int64_t ld) {
  // (the capacity is columns OF THIS LEADING DIMENSION: a context whose null model was replaced by one with more samples
  //  otherwise kept buffers of the old column length — a memory fault in the permutation stage, found in round 6)
  const size_t cols = c->fam_cols_ld ? c->d_Gp.cap / (sizeof(double) * (size_t)c->fam_cols_ld) : 0;  // columns held
  // Both are work spaces of the call that asks — every caller asks before it writes them, and runs on the context's stream —, so
  // they take DevBuf::grow's test fills (RVT_POISON on allocation, RVT_SCRIBBLE on a block that is large enough) on that stream.
  if (T <= cols && ld <= c->fam_cols_ld) {
    HIP_TRY(c, c->d_Gp.scribble(c->stream, "d_Gp"));
    HIP_TRY(c, c->d_Gt.scribble(c->stream, "d_Gt"));
    return RVT_OK;
  }
  c->d_Gp.reset();
  c->d_Gt.reset();
  const size_t want = std::max(T + T / 4, cols);
  c->fam_cols_ld = 0;
  const size_t bytes = sizeof(double) * (size_t)ld * want;
  HIP_TRY(c, c->d_Gp.grow(bytes, bytes, c->stream, true));
  HIP_TRY(c, c->d_Gt.grow(bytes, bytes, c->stream, true));
  c->fam_cols_ld = ld;
  return RVT_OK;
}


// ---- related samples: kinship, FastLMM null model, FamSKAT ----------------------------------------------------
int rvt_set_kinship(rvt_ctx* c, int64_t N, const float* U, const float* S) {
  if (!c || !U || !S || N < 2) return fail(c, RVT_E_INVALID, "bad kinship");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  clear_kinship(c);
  HIP_TRY(c, c->d_S.alloc(sizeof(double) * N));
  HIP_TRY(c, c->d_u1.alloc(sizeof(double) * N));
  // U -> fixed-point digit planes (rot_gemm.hip.h): 40 fractional bits.  Eigenvectors have |u| <= 1; six digits in [-64, 63]
  // hold every |u| < 1.98.
  c->uq_ldk = (N + 127) / 128 * 128;
  c->uq_rows_pad = (N + kRotBM - 1) / kRotBM * kRotBM;
  c->uq_plane = (size_t)c->uq_rows_pad * (size_t)c->uq_ldk;
  c->uq_sexp = 7 * kRotPlanesU - 2;
  HIP_TRY(c, c->d_Uq.alloc(c->uq_plane * kRotPlanesU));
  HIP_TRY(c, hipMemsetAsync(c->d_Uq, 0, c->uq_plane * kRotPlanesU, c->stream));
  const long long csc_cap = 64ll * N;  // non-zeros the sparse form may hold
  std::vector<long long> csc_ptr((size_t)N + 1, 0);
  bool csc_ok = !getenv("RVT_KINSHIP_DENSE");
  DevBuf<int> d_span;  // first / last non-zero row of every column of U
  {  // whole columns at a time through a bounded staging buffer (the caller's U can be tens of GB): digits + column sums
    const int64_t cols_per = std::max<int64_t>(1, std::min<int64_t>(N, ((int64_t)256 << 20) / N));
    DevBuf<int> d_cnt, d_flag;
    DevBuf<double> d_tmp64;
    DevBuf<float> d_tmp;
    HIP_TRY(c, d_span.alloc(sizeof(int) * 2 * (size_t)N));
    HIP_TRY(c, d_cnt.alloc(sizeof(int) * (size_t)cols_per));
    HIP_TRY(c, c->d_csc_ptr.alloc(sizeof(long long) * (size_t)(N + 1)));
    HIP_TRY(c, c->d_csc_rows.alloc(sizeof(int) * (size_t)csc_cap));
    HIP_TRY(c, c->d_csc_vals.alloc(sizeof(double) * (size_t)csc_cap));
    HIP_TRY(c, d_tmp.alloc(sizeof(float) * (size_t)cols_per * N));
    HIP_TRY(c, d_tmp64.alloc(sizeof(double) * (size_t)cols_per * N));
    HIP_TRY(c, d_flag.alloc(sizeof(int)));
    HIP_TRY(c, hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    for (int64_t k0 = 0; k0 < N; k0 += cols_per) {
      const int64_t nc = std::min(cols_per, N - k0);
      const size_t n = (size_t)nc * N;
      // (hipMemcpyDefault: rvt_kinship_decompose hands over eigenvectors that are already on the device)
      HIP_TRY(c, hipMemcpyAsync(d_tmp, U + (size_t)k0 * N, sizeof(float) * n, hipMemcpyDefault, c->stream));
      hipLaunchKernelGGL(rot_quantize_f32_kernel, dim3(2048), dim3(256), 0, c->stream, d_tmp, (long long)N, (long long)nc,
                         (long long)N, c->uq_sexp, kRotPlanesU, c->d_Uq, (long long)c->uq_ldk, (long long)c->uq_plane,
                         (long long)k0, d_flag);
      hipLaunchKernelGGL(rot_span_kernel, dim3((unsigned)nc), dim3(256), 0, c->stream, d_tmp, (long long)N, (long long)N,
                         d_span + k0, d_span + N + k0);
      if (csc_ok) {  // column-compressed copy of the chunk while it fits the budget of 64 non-zeros per column
        hipLaunchKernelGGL(rot_nnz_count_kernel, dim3((unsigned)nc), dim3(256), 0, c->stream, d_tmp, (long long)N,
                           (long long)N, d_cnt);
        std::vector<int> cnt((size_t)nc);
        HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, sync_stream(c->stream));
        for (int64_t j = 0; j < nc; ++j) csc_ptr[k0 + j + 1] = csc_ptr[k0 + j] + cnt[j];
        if (csc_ptr[k0 + nc] > csc_cap) {
          csc_ok = false;
        } else {
          HIP_TRY(c, hipMemcpyAsync(c->d_csc_ptr + k0, csc_ptr.data() + k0, sizeof(long long) * (size_t)(nc + 1),
                                    hipMemcpyHostToDevice, c->stream));
          hipLaunchKernelGGL(rot_nnz_fill_kernel, dim3((unsigned)nc), dim3(256), 0, c->stream, d_tmp, (long long)N,
                             (long long)N, c->d_csc_ptr + k0, c->d_csc_rows, c->d_csc_vals);
        }
      }
      hipLaunchKernelGGL(cvt_f32_f64_kernel, dim3(1024), dim3(256), 0, c->stream, d_tmp, d_tmp64, n);
      hipLaunchKernelGGL(column_sums_kernel, dim3((unsigned)nc), dim3(256), 0, c->stream, d_tmp64, (long long)N,
                         (long long)N, c->d_u1 + k0);
      HIP_TRY(c, sync_stream(c->stream));
    }
    int bad = 0;
    HIP_TRY(c, hipMemcpy(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost));
    if (!csc_ok) free_csc(c);
    if (bad) return fail(c, RVT_E_INVALID, "kinship eigenvectors have entries >= 1.98 in magnitude (not unit vectors)");
  }
  c->h_S.resize(N);
  for (int64_t i = 0; i < N; ++i) c->h_S[i] = (double)S[i];
  c->h_u1.resize(N);
  HIP_TRY(c, hipMemcpy(c->h_u1.data(), c->d_u1, sizeof(double) * N, hipMemcpyDeviceToHost));
  {
    // Structure of U.  A kinship matrix of unrelated families is block diagonal and so are its eigenvectors: column k
    // of U is non-zero on the rows [lo_k, hi_k] of one family only.  The statistics do not depend on the ORDER of the
    // eigenpairs, so they are re-ordered by lo_k (stable; a dense U keeps its order): a 256-row panel of the planes
    // then holds eigenvectors of neighbouring families, its non-zeros fall into a few K chunks, and the rotation GEMM
    // visits only those (rot_gemm.hip.h: a_krange).  Exact — the skipped chunks are exact zeros.
    std::vector<int> span(2 * (size_t)N);
    HIP_TRY(c, hipMemcpy(span.data(), d_span, sizeof(int) * 2 * (size_t)N, hipMemcpyDeviceToHost));
    d_span.reset();
    const int* lo = span.data();
    const int* hi = span.data() + N;
    std::vector<int> order((size_t)N);
    for (int64_t k = 0; k < N; ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lo[a] < lo[b]; });
    const int64_t nrp = c->uq_rows_pad / kRotBM, nchunk = c->uq_ldk / kRotKC;
    std::vector<int2> range((size_t)nrp);
    double visited = 0.0;
    for (int64_t rp = 0; rp < nrp; ++rp) {
      int l = (int)N, h = -1;
      for (int64_t r = rp * kRotBM; r < std::min<int64_t>(N, (rp + 1) * kRotBM); ++r) {
        l = std::min(l, lo[order[r]]);
        h = std::max(h, hi[order[r]]);
      }
      range[rp] = (h < l) ? int2{0, 0} : int2{l / kRotKC, h / kRotKC + 1};
      visited += range[rp].y - range[rp].x;
    }
    const double frac = visited / ((double)nrp * (double)nchunk);
    if (frac < 0.5 && !getenv("RVT_KINSHIP_DENSE")) {
      bool identity = true;
      for (int64_t k = 0; k < N && identity; ++k) identity = order[k] == (int)k;
      if (!identity) {  // re-order the rows of every plane (one plane-sized scratch buffer) and S, U'1 with them
        DevBuf<signed char> d_scratch;
        DevBuf<int> d_order;
        HIP_TRY(c, d_scratch.alloc(c->uq_plane));
        HIP_TRY(c, d_order.alloc(sizeof(int) * (size_t)N));
        HIP_TRY(c, hipMemcpy(d_order, order.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice));
        for (int p = 0; p < kRotPlanesU; ++p) {
          signed char* plane = c->d_Uq + (size_t)p * c->uq_plane;
          HIP_TRY(c, hipMemcpyAsync(d_scratch, plane, (size_t)N * c->uq_ldk, hipMemcpyDeviceToDevice, c->stream));
          hipLaunchKernelGGL(rot_gather_rows_kernel, dim3((unsigned)N), dim3(256), 0, c->stream, d_scratch, d_order,
                             (long long)c->uq_ldk, plane);
        }
        HIP_TRY(c, sync_stream(c->stream));
        d_scratch.reset();
        d_order.reset();
        std::vector<double> s2((size_t)N), u2((size_t)N);
        for (int64_t r = 0; r < N; ++r) {
          s2[r] = c->h_S[order[r]];
          u2[r] = c->h_u1[order[r]];
        }
        c->h_S.swap(s2);
        c->h_u1.swap(u2);
        HIP_TRY(c, hipMemcpy(c->d_u1, c->h_u1.data(), sizeof(double) * N, hipMemcpyHostToDevice));
      }
      HIP_TRY(c, c->d_uq_range.alloc(sizeof(int2) * (size_t)nrp));
      HIP_TRY(c, hipMemcpy(c->d_uq_range, range.data(), sizeof(int2) * (size_t)nrp, hipMemcpyHostToDevice));
      c->uq_visit = frac;
      free_csc(c);  // not needed then
    } else if (c->d_csc_ptr) {
      // sparse eigenvectors whose supports are scattered over the samples (families interleaved in the sample order):
      // the rotation gathers (rot_sparse_kernel); eigenpairs stay in the caller's order.  The digit planes (6 N^2 bytes)
      // are never read in this mode: give them back.
      c->uq_visit = (double)csc_ptr[N] / ((double)N * (double)N);
      c->d_Uq.reset();
    }
  }
  HIP_TRY(c, hipMemcpy(c->d_S, c->h_S.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  c->kin_N = N;
  c->have_kin = true;
  return RVT_OK;
}

int rvt_kinship_structure(rvt_ctx* c, double* visited_fraction) {
  if (!c || !visited_fraction) return RVT_E_INVALID;
  if (!c->have_kin) return fail(c, RVT_E_STATE, "no kinship decomposition installed");
  *visited_fraction = c->uq_visit;
  return RVT_OK;
}

// ---- the family form: U as one k x k block per family, never N x N ----------------------------------------------------------
// The descriptors of the family form as the caller hands them over; blk_off[f] = where family f's block starts in `blocks`.
// (this and the two functions below are rvt_decompose.hip's too: rvt_kinship_decompose_families)
int check_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                          std::vector<long long>* blk_off) {
  if (!fam_ptr || !members || N < 2 || N > INT32_MAX || n_fam < 1 || n_fam > N) return fail(c, RVT_E_INVALID, "bad kinship families");
  if (fam_ptr[0] != 0) return fail(c, RVT_E_INVALID, "kinship families: fam_ptr[0] is %lld, not 0", (long long)fam_ptr[0]);
  blk_off->assign((size_t)n_fam + 1, 0);
  for (int64_t f = 0; f < n_fam; ++f) {
    const int64_t k = fam_ptr[f + 1] - fam_ptr[f];
    if (k < 1) return fail(c, RVT_E_INVALID, "kinship families: family %lld is empty (fam_ptr must increase)", (long long)f);
    if (k > kJacP)
      return fail(c, RVT_E_INVALID, "kinship families: family %lld has %lld members (at most %d)", (long long)f, (long long)k, kJacP);
    if (fam_ptr[f + 1] > N)
      return fail(c, RVT_E_INVALID, "kinship families: family %lld ends at %lld, past N = %lld", (long long)f,
                  (long long)fam_ptr[f + 1], (long long)N);
    (*blk_off)[f + 1] = (*blk_off)[f] + k * k;
  }
  if (fam_ptr[n_fam] != N)
    return fail(c, RVT_E_INVALID, "kinship families: fam_ptr[n_fam] is %lld, not N = %lld", (long long)fam_ptr[n_fam], (long long)N);
  std::vector<bool> seen((size_t)N, false);
  for (int64_t i = 0; i < N; ++i) {
    const int32_t m = members[i];
    if (m < 0 || m >= N) return fail(c, RVT_E_INVALID, "kinship families: members[%lld] = %d is not a sample index", (long long)i, m);
    if (seen[m]) return fail(c, RVT_E_INVALID, "kinship families: members[%lld] = %d is listed twice", (long long)i, m);
    seen[m] = true;
  }
  return RVT_OK;
}

// first non-finite entry of the blocks: RVT_E_INVALID naming its family
int check_blocks_finite(rvt_ctx* c, int64_t n_fam, const int64_t* fam_ptr, const std::vector<long long>& blk_off,
                               const float* blocks, const char* what) {
  for (int64_t f = 0; f < n_fam; ++f) {
    const int k = (int)(fam_ptr[f + 1] - fam_ptr[f]);
    const float* b = blocks + blk_off[f];
    for (int e = 0; e < k * k; ++e)
      if (!std::isfinite(b[e]))
        return fail(c, RVT_E_INVALID, "kinship families: %s of family %lld holds a non-finite entry (row %d, column %d)", what,
                    (long long)f, e % k, e / k);
  }
  return RVT_OK;
}

// the installation itself, arguments checked: column-compressed U straight from the blocks (every entry kept, zeros too),
// U'1 from them in fp64 on the device, the descriptors and the runs of rot_fam_kernel
int install_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                            const std::vector<long long>& blk_off, const float* blocks, const float* S) {
  hipStream_t st = c->stream;
  clear_kinship(c);
  const size_t total = (size_t)blk_off[n_fam];
  std::vector<long long> csc_ptr((size_t)N + 1), fp(fam_ptr, fam_ptr + n_fam + 1);
  std::vector<int> rows(total), fam_of((size_t)N), run, sorted((size_t)N);
  std::vector<float> vals(total);
  for (int64_t f = 0; f < n_fam; ++f) {
    const int64_t fs = fam_ptr[f];
    const int k = (int)(fam_ptr[f + 1] - fs);
    if (run.empty() || fam_ptr[f + 1] - run.back() > kRotFamRows) run.push_back((int)fs);
    // the rows of a block go to ascending sample order: every sum over a family then runs in the order in which the dense
    // installation's column-compressed form (rot_nnz_fill_kernel) would run it
    int perm[kJacP];
    for (int r = 0; r < k; ++r) perm[r] = r;
    std::sort(perm, perm + k, [&](int a, int b) { return members[fs + a] < members[fs + b]; });
    for (int r = 0; r < k; ++r) sorted[fs + r] = members[fs + perm[r]];
    for (int j = 0; j < k; ++j) {
      csc_ptr[fs + j] = blk_off[f] + (long long)j * k;
      fam_of[fs + j] = (int)f;
      int* rw = rows.data() + blk_off[f] + (size_t)j * k;
      float* vw = vals.data() + blk_off[f] + (size_t)j * k;
      const float* bw = blocks + blk_off[f] + (size_t)j * k;
      for (int r = 0; r < k; ++r) {
        rw[r] = sorted[fs + r];
        vw[r] = bw[perm[r]];
      }
    }
  }
  csc_ptr[N] = (long long)total;
  run.push_back((int)N);
  DevBuf<float> d_tmp;
  HIP_TRY(c, c->d_S.alloc(sizeof(double) * N));
  HIP_TRY(c, c->d_u1.alloc(sizeof(double) * N));
  HIP_TRY(c, c->d_csc_ptr.alloc(sizeof(long long) * ((size_t)N + 1)));
  HIP_TRY(c, c->d_csc_rows.alloc(sizeof(int) * total));
  HIP_TRY(c, c->d_csc_vals.alloc(sizeof(double) * total));
  HIP_TRY(c, c->d_fam_ptr.alloc(sizeof(long long) * fp.size()));
  HIP_TRY(c, c->d_fam_members.alloc(sizeof(int) * (size_t)N));
  HIP_TRY(c, c->d_fam_of.alloc(sizeof(int) * (size_t)N));
  HIP_TRY(c, c->d_fam_run.alloc(sizeof(int) * run.size()));
  HIP_TRY(c, d_tmp.alloc(sizeof(float) * total));
  HIP_TRY(c, hipMemcpyAsync(c->d_csc_ptr, csc_ptr.data(), sizeof(long long) * csc_ptr.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_csc_rows, rows.data(), sizeof(int) * total, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_fam_ptr, fp.data(), sizeof(long long) * fp.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_fam_members, sorted.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_fam_of, fam_of.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_fam_run, run.data(), sizeof(int) * run.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_tmp, vals.data(), sizeof(float) * total, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(cvt_f32_f64_kernel, dim3(1024), dim3(256), 0, st, d_tmp, c->d_csc_vals, total);
  hipLaunchKernelGGL(rot_fam_colsum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_csc_ptr, c->d_csc_vals,
                     (long long)N, c->d_u1);
  HIP_TRY(c, hipGetLastError());
  c->h_S.resize(N);
  for (int64_t i = 0; i < N; ++i) c->h_S[i] = (double)S[i];
  c->h_u1.resize(N);
  HIP_TRY(c, hipMemcpyAsync(c->d_S, c->h_S.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->h_u1.data(), c->d_u1, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));  // (the host vectors above go out of scope)
  c->uq_plane = 0;
  c->uq_ldk = c->uq_rows_pad = 0;
  c->uq_visit = (double)total / ((double)N * (double)N);
  c->fam_count = n_fam;
  c->fam_runs = (int)run.size() - 1;
  c->kin_N = N;
  c->have_kin = true;
  return RVT_OK;
}

int rvt_set_kinship_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                             const float* U_blocks, const float* S) {
  if (!c || !U_blocks || !S) return fail(c, RVT_E_INVALID, "bad kinship families");
  std::vector<long long> blk_off;
  int rc = check_families(c, N, n_fam, fam_ptr, members, &blk_off);
  if (rc) return rc;
  rc = check_blocks_finite(c, n_fam, fam_ptr, blk_off, U_blocks, "the eigenvector block");
  if (rc) return rc;
  for (int64_t i = 0; i < N; ++i)
    if (!std::isfinite(S[i])) return fail(c, RVT_E_INVALID, "kinship families: eigenvalue S[%lld] is not finite", (long long)i);
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  return install_families(c, N, n_fam, fam_ptr, members, blk_off, U_blocks, S);
}

// ---- integer-plane GEMMs (rot_gemm.hip.h) ---------------------------------------------------------------------------
namespace {
constexpr int kRotMaxCols = 1 << 15;

struct QuantCols {       // digit planes of a set of columns, in a context-owned buffer
  signed char* d = nullptr;
  size_t plane_stride = 0;
  int planes = 0;
  std::vector<int> sexp;  // per column: entries were scaled by 2^sexp
};

// (work spaces of the call that asks, on its stream: both callers write what they read — scales, maxima, exponents — behind this
//  and keep nothing here between calls, so the blocks take grow's test fills)
int ensure_rot_scratch(rvt_ctx* c, hipStream_t st) {
  HIP_TRY(c, c->d_rot_scale.grow(sizeof(double) * 4 * kRotMaxCols, sizeof(double) * 4 * kRotMaxCols, st, true, 0, "d_rot_scale"));  // col | max | row | spare
  HIP_TRY(c, c->d_rot_sexp.grow(sizeof(int) * kRotMaxCols, sizeof(int) * kRotMaxCols, st, true, 0, "d_rot_sexp"));
  return RVT_OK;
}

// Quantise ncols <= kRotMaxCols columns of n_rows doubles (column-major, leading dimension ld_src) into planes laid out
// [plane][column (padded to `pad`)][ldk].  One plane when every column holds integers in [-127, 127], else kRotPlanesG.
int quantize_columns(rvt_ctx* c, const double* d_src, int64_t n_rows, int64_t ld_src, int ncols, int pad, int64_t ldk,
                     DevBuf<signed char>& buf, hipStream_t st, QuantCols* out, bool known_hard_calls = false) {
  int rc = ensure_rot_scratch(c, st);
  if (rc) return rc;
  double* d_max = c->d_rot_scale + kRotMaxCols;
  std::vector<double> cmax(ncols, 2.0);  // (hard calls: 0 / 1 / 2, no scan needed)
  if (!known_hard_calls) {
    hipLaunchKernelGGL(rot_colmax_kernel, dim3((unsigned)ncols), dim3(256), 0, st, d_src, (long long)n_rows,
                       (long long)ld_src, d_max);
    HIP_TRY(c, hipMemcpyAsync(cmax.data(), d_max, sizeof(double) * ncols, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  bool small = true;
  for (int j = 0; j < ncols; ++j) small = small && cmax[j] >= 0.0 && cmax[j] <= 127.0;
  const int PG = small ? 1 : kRotPlanesG;
  out->planes = PG;
  out->sexp.assign(ncols, 0);
  for (int j = 0; j < ncols; ++j) {
    const double mx = cmax[j] < 0.0 ? -cmax[j] - 1.0 : cmax[j];
    if (!std::isfinite(mx)) return fail(c, RVT_E_INVALID, "non-finite value in a column of an integer-plane product");
    out->sexp[j] = (PG == 1 || mx == 0.0) ? 0 : 7 * PG - 3 - std::ilogb(mx);
  }
  const int64_t cols_pad = ((int64_t)ncols + pad - 1) / pad * pad;
  out->plane_stride = (size_t)cols_pad * (size_t)ldk;
  const size_t need = out->plane_stride * PG;
  HIP_TRY(c, buf.grow(need, need + need / 4, st, true));
  out->d = buf;
  HIP_TRY(c, hipMemsetAsync(out->d, 0, need, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_rot_sexp, out->sexp.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(rot_quantize_f64_kernel, dim3(2048), dim3(256), 0, st, d_src, (long long)n_rows, (long long)ncols,
                     (long long)ld_src, c->d_rot_sexp, PG, out->d, (long long)ldk, (long long)out->plane_stride);
  HIP_TRY(c, sync_stream(st));  // d_rot_sexp / the host vectors are reused by the next call
  return RVT_OK;
}

// C[a + b * ldc] = sum_i A[i, a] B[i, b] from digit planes: nA rows (A columns), nB columns, K = n_rows samples.
// row_exp (host, may be null: uniform a_exp) / col_exp: binary scale exponents of the two sides.
int planes_gemm(rvt_ctx* c, const signed char* A, size_t a_stride, int PA, int nA, const int* row_exp, int a_exp,
                const signed char* B, size_t b_stride, int PB, int nB, const int* col_exp, int64_t n_rows, int64_t ldk,
                double* C, int64_t ldc, hipStream_t st, const int2* a_krange = nullptr) {
  int rc = ensure_rot_scratch(c, st);
  if (rc) return rc;
  std::vector<double> cs(nB), rs;
  for (int j = 0; j < nB; ++j) cs[j] = std::ldexp(1.0, -((row_exp ? 0 : a_exp) + (col_exp ? col_exp[j] : 0)));
  HIP_TRY(c, hipMemcpyAsync(c->d_rot_scale, cs.data(), sizeof(double) * nB, hipMemcpyHostToDevice, st));
  const double* d_rs = nullptr;
  if (row_exp) {
    rs.resize(nA);
    for (int a = 0; a < nA; ++a) rs[a] = std::ldexp(1.0, -row_exp[a]);
    HIP_TRY(c, hipMemcpyAsync(c->d_rot_scale + 2 * kRotMaxCols, rs.data(), sizeof(double) * nA, hipMemcpyHostToDevice, st));
    d_rs = c->d_rot_scale + 2 * kRotMaxCols;
  }
  const int nrp = (nA + kRotBM - 1) / kRotBM, nct = (nB + kRotBN - 1) / kRotBN;
  const long long sets = (long long)((nrp + 31) / 32) * ((nct + 7) / 8);
  const long long kbytes = (n_rows + kRotKC - 1) / kRotKC * kRotKC;
  // the kernel accumulates a whole K range in int32: |digit| <= 64 (several planes) or <= 127 (one plane of small
  // integers), so ranges longer than 2^31 / (bound_A bound_B) samples are cut and added in fp64
  const long long bound = (long long)(PA == 1 ? 127 : 64) * (PB == 1 ? 127 : 64);
  long long kmax = std::max<long long>(kRotKC, ((1LL << 31) - 1) / bound / kRotKC * kRotKC);
  if (const char* e = getenv("RVT_ROT_KMAX"))  // tests: force the cut on small problems
    kmax = std::max<long long>(kRotKC, std::min<long long>(kmax, atoll(e) / kRotKC * kRotKC));
  // Few output tiles (a short, wide product such as G'G of one MetaCov block: 16 tiles for 1024 x 1024) cannot fill
  // 256 CUs: K is then also split across workgroups (grid.y), every slice writes its own partial result and a
  // fixed-order reduction adds them.  Also used for the int32 range cut above.
  const long long tiles = (long long)nrp * nct;
  long long slices = 1;
  if (tiles < 256) slices = std::min<long long>((512 + tiles - 1) / tiles, std::max<long long>(1, kbytes / (16 * kRotKC)));
  slices = std::max(slices, (kbytes + kmax - 1) / kmax);
  if (const char* e = getenv("RVT_ROT_SLICES")) slices = std::max<long long>(1, atoll(e));
  long long kslice = ((kbytes + slices - 1) / slices + kRotKC - 1) / kRotKC * kRotKC;
  kslice = std::min(kslice, kmax);
  slices = (kbytes + kslice - 1) / kslice;
  double* d_part = nullptr;
  long long c_slice = 0;
  if (slices > 1) {
    c_slice = (long long)ldc * nB;
    const size_t need = sizeof(double) * (size_t)c_slice * (size_t)slices;
    HIP_TRY(c, c->d_rot_part.grow(need, need, st, true));
    d_part = c->d_rot_part;
  }
  if (a_krange && !row_exp) {
    // structured A: every plane of A inside one launch per plane of B, C written once (rot_gemm_i8_short_kernel)
    const int nct_s = (nB + kRotShortBN - 1) / kRotShortBN;
    const long long sets_s = (long long)((nrp + 31) / 32) * ((nct_s + 7) / 8);
    for (int q = 0; q < PB; ++q)
      hipLaunchKernelGGL(rot_gemm_i8_short, dim3((unsigned)(sets_s * 256)), dim3(512), 0, st, (const int8_t*)A,
                         (long long)a_stride, PA, (const int8_t*)(B + (size_t)q * b_stride), (long long)ldk, kbytes, C,
                         (long long)ldc, nA, nB, nrp, nct_s, c->d_rot_scale, std::ldexp(1.0, 7 * q), q > 0 ? 1 : 0, a_krange);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    return RVT_OK;
  }
  int first = 1;
  for (int sdeg = 0; sdeg <= (PA - 1) + (PB - 1); ++sdeg)  // least significant digit pairs first
    for (int p = 0; p < PA; ++p) {
      const int q = sdeg - p;
      if (q < 0 || q >= PB) continue;
      const dim3 grid((unsigned)(sets * 256), (unsigned)slices);
      if (slices == 1) {
        hipLaunchKernelGGL(rot_gemm_i8_kernel, grid, dim3(kRotThreads), 0, st, (const int8_t*)(A + (size_t)p * a_stride),
                           (const int8_t*)(B + (size_t)q * b_stride), (long long)ldk, kbytes, C, (long long)ldc, nA, nB, nrp,
                           nct, c->d_rot_scale, d_rs, std::ldexp(1.0, 7 * (p + q)), first ? 0 : 1, kbytes, 0LL);
      } else {
        hipLaunchKernelGGL(rot_gemm_i8_kernel, grid, dim3(kRotThreads), 0, st, (const int8_t*)(A + (size_t)p * a_stride),
                           (const int8_t*)(B + (size_t)q * b_stride), (long long)ldk, kbytes, d_part, (long long)ldc, nA, nB,
                           nrp, nct, c->d_rot_scale, d_rs, std::ldexp(1.0, 7 * (p + q)), 0, kslice, c_slice);
        hipLaunchKernelGGL(rot_reduce_slices_kernel, dim3(1024), dim3(256), 0, st, d_part, (long long)ldc, (long long)nA,
                           (long long)nB, c_slice, (int)slices, C, first ? 0 : 1);
      }
      first = 0;
    }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sync_stream(st));  // (the scale arrays are reused by the next call)
  return RVT_OK;
}
}  // namespace

// dst (N x ncols doubles, leading dimension ld_dst) = U' src (src: N x ncols doubles, leading dimension ld_src), exactly
// as the integer products of the digit planes.  Columns of small integers (hard calls after the flip, collapsed burden
// columns) are one digit plane; any other batch is quantised to kRotPlanesG digits per column.
// (planes_gemm for the other translation units: MetaCov's hard-call band)
int rvt_planes_gemm(rvt_ctx* c, const signed char* A, size_t a_stride, int PA, int nA, const int* row_exp, int a_exp,
                    const signed char* B, size_t b_stride, int PB, int nB, const int* col_exp, int64_t n_rows, int64_t ldk,
                    double* C, int64_t ldc, hipStream_t st, const int2* a_krange) {
  return planes_gemm(c, A, a_stride, PA, nA, row_exp, a_exp, B, b_stride, PB, nB, col_exp, n_rows, ldk, C, ldc, st, a_krange);
}
// (quantize_columns for rvt_mtscore.hip: the B operand of a piece of dosage columns, in the context's d_mt_B)
int quantize_columns_mt(rvt_ctx* c, const double* d_src, int64_t n_rows, int64_t ld_src, int ncols, int pad, int64_t ldk,
                        hipStream_t st, signed char** planes, size_t* plane_stride, int* n_planes, int* col_exp) {
  if (ncols > kRotMaxCols) return fail(c, RVT_E_TOO_LARGE, "integer-plane product: too many columns");
  QuantCols q;
  int rc = quantize_columns(c, d_src, n_rows, ld_src, ncols, pad, ldk, c->d_mt_B, st, &q);
  if (rc) return rc;
  *planes = q.d;
  *plane_stride = q.plane_stride;
  *n_planes = q.planes;
  std::copy(q.sexp.begin(), q.sexp.end(), col_exp);
  return RVT_OK;
}
int rotate_columns(rvt_ctx* c, const double* d_src, int64_t ld_src, int ncols, double* d_dst, int64_t ld_dst,
                          hipStream_t st) {
  const int64_t N = c->kin_N;
  if (c->d_fam_run) {  // the family form: one workgroup per run of families and tile of columns (rot_fam_kernel)
    const int per = 65535 * kRotFamCols;  // (gridDim.y holds at most 65535 column tiles)
    for (int c0 = 0; c0 < ncols; c0 += per) {
      const int nc = std::min(per, ncols - c0);
      hipLaunchKernelGGL(rot_fam_kernel, dim3((unsigned)c->fam_runs, (unsigned)((nc + kRotFamCols - 1) / kRotFamCols)),
                         dim3(kRotFamRows), 0, st, c->d_fam_run, c->d_fam_of, c->d_fam_ptr, c->d_fam_members, c->d_csc_ptr,
                         c->d_csc_vals, d_src + (size_t)c0 * ld_src, (long long)ld_src, nc, d_dst + (size_t)c0 * ld_dst,
                         (long long)ld_dst);
      HIP_TRY(c, hipGetLastError());
    }
    return RVT_OK;
  }
  if (c->d_csc_ptr && !c->d_uq_range) {  // sparse U, scattered supports: a gather per output (fp64 products and sums)
    for (int c0 = 0; c0 < ncols; c0 += 65535) {  // (gridDim.y holds at most 65535 columns)
      const int nc = std::min(65535, ncols - c0);
      hipLaunchKernelGGL(rot_sparse_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)nc), dim3(256), 0, st,
                         c->d_csc_ptr, c->d_csc_rows, c->d_csc_vals, (long long)N, d_src + (size_t)c0 * ld_src,
                         (long long)ld_src, d_dst + (size_t)c0 * ld_dst, (long long)ld_dst);
      HIP_TRY(c, hipGetLastError());
    }
    return RVT_OK;
  }
  for (int c0 = 0; c0 < ncols; c0 += kRotMaxCols) {  // long lists in pieces
    const int nc = std::min(kRotMaxCols, ncols - c0);
    QuantCols qb;
    int rc = quantize_columns(c, d_src + (size_t)c0 * ld_src, N, ld_src, nc, kRotBN, c->uq_ldk, c->d_rotB, st,
                              &qb);
    if (rc) return rc;
    rc = planes_gemm(c, c->d_Uq, c->uq_plane, kRotPlanesU, (int)N, nullptr, c->uq_sexp, qb.d, qb.plane_stride, qb.planes,
                     nc, qb.sexp.data(), N, c->uq_ldk, d_dst + (size_t)c0 * ld_dst, ld_dst, st, c->d_uq_range);
    if (rc) return rc;
  }
  return RVT_OK;
}

// Test hook: the first ncols columns of a device block through rotate_columns, N x ncols to the host (column-major, no padding).
int rvt_debug_rotate(rvt_ctx* c, const double* dG, int ncols, double* out) {
  if (!c || !dG || !out || ncols < 1) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_kin) return fail(c, RVT_E_STATE, "rvt_set_kinship first");
  if (!c->have_null && !c->have_fam) return fail(c, RVT_E_STATE, "set the null model first (defines the block layout)");
  const int64_t N = c->kin_N, ld = block_dims(c).ld;  // (the layout rvt_block_alloc gave dG)
  if (block_dims(c).N != N) return fail(c, RVT_E_STATE, "the kinship and the null model differ in N");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  rc = ensure_fam_cols(c, (size_t)ncols, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * ncols, st));
  rc = rotate_columns(c, dG, ld, ncols, c->d_Gt, ld, st);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy2DAsync(out, sizeof(double) * (size_t)N, c->d_Gt, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)N,
                              (size_t)ncols, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  return RVT_OK;
}

// Measurement hook: the same rotation without the copy to the host, between two HIP events recorded directly around it
int rvt_debug_rotate_timed(rvt_ctx* c, const double* dG, int ncols, double* ms) {
  if (!c || !dG || !ms || ncols < 1) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_kin) return fail(c, RVT_E_STATE, "rvt_set_kinship first");
  if (!c->have_null && !c->have_fam) return fail(c, RVT_E_STATE, "set the null model first (defines the block layout)");
  const int64_t N = c->kin_N, ld = block_dims(c).ld;
  if (block_dims(c).N != N) return fail(c, RVT_E_STATE, "the kinship and the null model differ in N");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  rc = ensure_fam_cols(c, (size_t)ncols, ld);
  if (rc) return rc;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(c, hipEventCreate(&ev[0]));
  hipError_t e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) {
    rc = rotate_columns(c, dG, ld, ncols, c->d_Gt, ld, st);
    if (!rc) e = hipEventRecord(ev[1], st);
    if (!rc && e == hipSuccess) e = sync_stream(st);
    float t = 0.0f;
    if (!rc && e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    *ms = t;
  }
  hipEventDestroy(ev[0]);
  if (ev[1]) hipEventDestroy(ev[1]);
  if (rc) return rc;
  HIP_TRY(c, e);
  return RVT_OK;
}

// C (nA x nB, column-major, leading dimension ldc) = A' B for two double matrices with n_rows rows (column-major) through
// the integer planes: exact when both hold small integers, else to ~2^-40 relative of each column's largest entry.
int gemm_tn_planes(rvt_ctx* c, const double* dA, int64_t ldA, int nA, const double* dB, int64_t ldB, int nB,
                          int64_t n_rows, double* C, int64_t ldc, hipStream_t st) {
  if (nA > kRotMaxCols || nB > kRotMaxCols) return fail(c, RVT_E_TOO_LARGE, "integer-plane product: too many columns");
  const int64_t ldk = (n_rows + 127) / 128 * 128;
  QuantCols qa, qb;
  int rc = quantize_columns(c, dA, n_rows, ldA, nA, kRotBM, ldk, c->d_rotA, st, &qa);
  if (rc) return rc;
  rc = quantize_columns(c, dB, n_rows, ldB, nB, kRotBN, ldk, c->d_rotB, st, &qb);
  if (rc) return rc;
  return planes_gemm(c, qa.d, qa.plane_stride, qa.planes, nA, qa.sexp.data(), 0, qb.d, qb.plane_stride, qb.planes, nB,
                     qb.sexp.data(), n_rows, ldk, C, ldc, st);
}

namespace {
// GSL 1.16 Brent minimiser exactly as Minimizer::minimize drives it (regression/GSLMinimizer.cpp:18-66: set, then
// iterate until the bracket is narrower than epsabs = 1e-3 or 100 iterations).  The evaluation SEQUENCE matters:
// the reference's beta / sigma2 are side effects of the last evaluation (regression/FastLMM.cpp:812-817).
int brent_like_gsl(const std::function<double(double)>& f, double start, double lb, double ub, double* xmin) {
  const double golden = 0.3819660, sqrt_eps = 1.4901161193847656e-08;
  double xl = lb, xu = ub, xm = start;
  const double fl = f(xl);
  if (!std::isfinite(fl)) return -1;
  const double fu = f(xu);
  if (!std::isfinite(fu)) return -1;
  double fm = f(xm);
  if (!std::isfinite(fm)) return -1;
  if (xl > xu || xm >= xu || xm <= xl || fm >= fl || fm >= fu) return -1;
  double v = xl + golden * (xu - xl), w = v, st_d = 0, st_e = 0;
  double fv = f(v);
  if (!std::isfinite(fv)) return -1;
  double fw = fv;
  for (int iter = 1;; ++iter) {
    const double z = xm, fz = fm;
    double d = st_e, e = st_d;  // the roles of the two saved steps are exchanged on entry, as in GSL
    const double w_lower = z - xl, w_upper = xu - z, tol = sqrt_eps * std::fabs(z), mid = 0.5 * (xl + xu);
    double p = 0, q = 0, r = 0;
    if (std::fabs(e) > tol) {  // parabola through (v, w, z)
      r = (z - w) * (fz - fv);
      q = (z - v) * (fz - fw);
      p = (z - v) * q - (z - w) * r;
      q = 2 * (q - r);
      if (q > 0)
        p = -p;
      else
        q = -q;
      r = e;
      e = d;
    }
    double u;
    if (std::fabs(p) < std::fabs(0.5 * q * r) && p < q * w_lower && p < q * w_upper) {
      d = p / q;
      u = z + d;
      if ((u - xl) < 2 * tol || (xu - u) < 2 * tol) d = (z < mid) ? tol : -tol;
    } else {  // golden section into the larger part
      e = (z < mid) ? xu - z : -(z - xl);
      d = golden * e;
    }
    u = (std::fabs(d) >= tol) ? z + d : z + ((d > 0) ? tol : -tol);
    st_e = e;
    st_d = d;
    const double fuu = f(u);
    if (!std::isfinite(fuu)) return -1;
    if (fuu <= fz) {
      if (u < z)
        xu = z;
      else
        xl = z;
      v = w;
      fv = fw;
      w = z;
      fw = fz;
      xm = u;
      fm = fuu;
    } else {
      if (u < z)
        xl = u;
      else
        xu = u;
      if (fuu <= fw || w == z) {
        v = w;
        fv = fw;
        w = u;
        fw = fuu;
      } else if (fuu <= fv || v == z || v == w) {
        v = u;
        fv = fuu;
      }
    }
    *xmin = xm;
    if (std::fabs(xu - xl) < 0.001 || iter >= 100) return 0;
  }
}
}  // namespace

int rvt_fit_fam_null(rvt_ctx* c, int64_t N, int d, const double* X, const double* y, rvt_fam_null* out) {
  if (!c || !X || !y || !out || d < 1 || d + 2 > RVT_MAX_COV) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_kin || c->kin_N != N) return fail(c, RVT_E_STATE, "rvt_set_kinship with the same N first");
  if (c->have_null && c->nc.N != N) return fail(c, RVT_E_STATE, "sample count differs from the installed null model");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t ld = rvt_padded_ld(N);
  for (DevBuf<double>* p : {&c->d_uxy, &c->d_lmm_part, &c->d_fX, &c->d_frr, &c->d_fv, &c->d_fzeros, &c->d_fbeta}) p->reset();
  c->have_fam = false;
  ++c->fam_gen;
  c->famcov_b2 = 1.0;
  const int dx = d + 1;
  DevBuf<double> d_xy;  // N x (d+1): X | y
  HIP_TRY(c, d_xy.alloc(sizeof(double) * (size_t)N * dx));
  HIP_TRY(c, c->d_uxy.alloc(sizeof(double) * (size_t)N * dx));
  HIP_TRY(c, hipMemcpy(d_xy, X, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_xy + (size_t)N * d, y, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
  {  // ux = U'X, uy = U'y  (FastLMM.cpp:55-57)
    int rcr = rotate_columns(c, d_xy, N, dx, c->d_uxy, N, st);
    if (rcr) return rcr;
    HIP_TRY(c, sync_stream(st));
  }
  d_xy.reset();
  // |lambda| for the likelihood (FastLMM.cpp:50); the raw S stays in d_S for FamSkat's Sigma
  std::vector<double> absS(N);
  for (int64_t i = 0; i < N; ++i) absS[i] = std::fabs(c->h_S[i]);
  DevBuf<double> d_abs;
  HIP_TRY(c, d_abs.alloc(sizeof(double) * N));
  HIP_TRY(c, hipMemcpy(d_abs, absS.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  const int rec = lmm_rec_len(d);
  // (reset above: a fresh block per fit, with grow's poison fill)
  HIP_TRY(c, c->d_lmm_part.grow(sizeof(double) * (size_t)kLmmBlocks * rec, sizeof(double) * (size_t)kLmmBlocks * rec, st, true));
  std::vector<double> part((size_t)kLmmBlocks * rec), sums(rec);
  std::vector<double> beta(d, 0.0);
  double sigma2 = 0.0;
  bool hip_failed = false;
  // device sums for one delta: A, b, yy, sum log|lambda + delta|
  auto device_sums = [&](const double* lam, double delta, int take_abs) {
    hipLaunchKernelGGL(lmm_sums_kernel, dim3(kLmmBlocks), dim3(256), sizeof(double) * 256, st, c->d_uxy, lam,
                       (long long)N, d, delta, take_abs, c->d_lmm_part);
    if (hipMemcpyAsync(part.data(), c->d_lmm_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st) !=
            hipSuccess ||
        sync_stream(st) != hipSuccess)
      hip_failed = true;
    for (int q = 0; q < rec; ++q) {
      double s = 0.0;
      for (int b = 0; b < kLmmBlocks; ++b) s += part[(size_t)b * rec + q];  // fixed order
      sums[q] = s;
    }
  };
  // getBetaSigma2 + getLogLikelihood for one delta (FastLMM.cpp:297-346, model MLE); returns the log-likelihood
  auto evaluate = [&](double delta) {
    device_sums(d_abs, delta, 1);
    const double* A = sums.data();
    const double* b = A + d * d;
    const double yy = sums[d * d + d], slog = sums[d * d + d + 1];
    double Ai[RVT_MAX_COV * RVT_MAX_COV];
    if (!invert_spd(A, d, Ai)) return (double)NAN;
    for (int a = 0; a < d; ++a) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s += Ai[a * d + k] * b[k];
      beta[a] = s;
    }
    // sum (uy - ux beta)^2 / (lambda + delta) = yy - 2 beta'b + beta'A beta
    double bb = 0.0, bAb = 0.0;
    for (int a = 0; a < d; ++a) {
      bb += beta[a] * b[a];
      for (int k = 0; k < d; ++k) bAb += beta[a] * A[a * d + k] * beta[k];
    }
    sigma2 = (yy - 2.0 * bb + bAb) / (double)N;
    const double n = (double)N;
    return -0.5 * (n * std::log(2.0 * 3.14159265358979323846) + slog + n + n * std::log(sigma2));
  };
  int maxIndex = -1;
  double maxLL = 0.0, delta = 0.0;
  for (int i = 0; i <= 100; ++i) {
    delta = std::exp(-10. + i * 0.2);
    const double ll = evaluate(delta);
    if (std::isnan(ll)) continue;
    if (maxIndex < 0 || ll > maxLL) {
      maxIndex = i;
      maxLL = ll;
    }
  }
  int evals = 0;
  if (maxIndex > 0 && maxIndex < 100) {
    const double lb = std::exp(-10. + (maxIndex - 1) * 0.2), ub = std::exp(-10. + (maxIndex + 1) * 0.2);
    const double start = std::exp(-10. + maxIndex * 0.2);
    double xmin = start;
    auto goal = [&](double x) {
      ++evals;
      return -evaluate(x);
    };
    delta = brent_like_gsl(goal, start, lb, ub, &xmin) ? start : xmin;
  }  // else: on the boundary delta (and beta, sigma2) stay at the LAST grid point, as in the reference
  if (hip_failed) return fail(c, RVT_E_HIP, "device evaluation of the FastLMM likelihood failed");
  out->delta = delta;
  out->sigma2_g = sigma2;
  c->fam_delta = delta;
  c->fam_sigma2 = sigma2;
  std::memset(out->beta, 0, sizeof(out->beta));
  for (int a = 0; a < d; ++a) out->beta[a] = beta[a];
  out->max_index = maxIndex;
  out->brent_evals = evals;
  // ---- what FamSkat::FitNullModel prepares (FamSkat.cpp:34-64), in rotated / folded form --------------------
  NullConsts& fn = c->fam_nc;
  std::memset(&fn, 0, sizeof(fn));
  fn.N = N;
  fn.ld = ld;
  fn.d = dx;
  fn.binary = 1;  // the sufficient statistics are weighted by V = sigma2 (S + delta)
  fn.sigma2 = 1.0;
  {  // C = X' Sigma^-1 X = sum ux ux' / (sigma2 (S + delta)) with the RAW S (FamSkat.cpp:48-56)
    device_sums(c->d_S, delta, 0);
    double C[RVT_MAX_COV * RVT_MAX_COV], Ci[RVT_MAX_COV * RVT_MAX_COV];
    for (int a = 0; a < d * d; ++a) C[a] = sums[a] / sigma2;
    if (hip_failed || !invert_spd(C, d, Ci)) return fail(c, RVT_E_INVALID, "X' Sigma^-1 X is singular");
    for (int a = 0; a < dx; ++a)
      for (int b = 0; b < dx; ++b) {
        const bool in = a < d && b < d;
        fn.C[a * dx + b] = in ? C[a * d + b] : (a == b ? 1.0 : 0.0);
        fn.Cinv[a * dx + b] = in ? Ci[a * d + b] : (a == b ? 1.0 : 0.0);
      }
  }
  d_abs.reset();
  {  // denom of FastGetAF: u1' |S|^-1 u1 (FastLMM.cpp:414-420), kept in the otherwise unused rss slot
    double den = 0.0;
    for (int64_t i = 0; i < N; ++i) den += c->h_u1[i] / std::fabs(c->h_S[i]) * c->h_u1[i];
    fn.rss = den;
  }
  const size_t vb = sizeof(double) * (size_t)ld;
  HIP_TRY(c, c->d_fX.alloc(vb * dx));
  HIP_TRY(c, c->d_frr.alloc(vb));
  HIP_TRY(c, c->d_fv.alloc(vb));
  HIP_TRY(c, c->d_fzeros.alloc(vb));
  HIP_TRY(c, c->d_fbeta.alloc(sizeof(double) * RVT_MAX_COV));
  HIP_TRY(c, hipMemsetAsync(c->d_fX, 0, vb * dx, st));
  HIP_TRY(c, hipMemsetAsync(c->d_frr, 0, vb, st));
  HIP_TRY(c, hipMemsetAsync(c->d_fv, 0, vb, st));
  HIP_TRY(c, hipMemsetAsync(c->d_fzeros, 0, vb, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_fbeta, out->beta, sizeof(double) * RVT_MAX_COV, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fam_build_null_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_uxy, c->d_S,
                     c->d_u1, (long long)N, (long long)ld, d, sigma2, delta, c->d_fbeta, c->d_fX, c->d_frr, c->d_fv);
  HIP_TRY(c, c->d_fam_nc.grow(sizeof(NullConsts), sizeof(NullConsts)));
  HIP_TRY(c, hipMemcpyAsync(c->d_fam_nc, &fn, sizeof(NullConsts), hipMemcpyHostToDevice, st));
  // ---- the family MetaCov's constants and null set (MetaCovFamQtl over FastLMM::GetCov*, FastLMM.cpp:510-625) ----
  {
    // [U'X | u1] with weights 1/|lambda + delta|: A = ux'W ux, b = ux'W u1, yy = u1'W u1
    DevBuf<double> d_xu;
    HIP_TRY(c, d_xu.alloc(sizeof(double) * (size_t)N * dx));
    HIP_TRY(c, hipMemcpyAsync(d_xu, c->d_uxy, sizeof(double) * (size_t)N * d, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_xu + (size_t)N * d, c->d_u1, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
    DevBuf<double> d_abs2;
    HIP_TRY(c, d_abs2.alloc(sizeof(double) * N));
    HIP_TRY(c, hipMemcpyAsync(d_abs2, absS.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lmm_sums_kernel, dim3(kLmmBlocks), dim3(256), sizeof(double) * 256, st, d_xu, d_abs2,
                       (long long)N, d, delta, 1, c->d_lmm_part);
    HIP_TRY(c, hipMemcpyAsync(part.data(), c->d_lmm_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    d_xu.reset();
    d_abs2.reset();
    for (int q = 0; q < rec; ++q) {
      double s2 = 0.0;
      for (int b = 0; b < kLmmBlocks; ++b) s2 += part[(size_t)b * rec + q];
      sums[q] = s2;
    }
    for (int a = 0; a < d * d; ++a) c->famcov_zz[a] = sums[a] / sigma2;
    for (int a = 0; a < d; ++a) c->famcov_c1x[a] = sums[d * d + a] / sigma2;
    c->famcov_c11 = sums[d * d + d] / sigma2;
    if (!invert_spd(c->famcov_zz, d, c->famcov_zzinv)) return fail(c, RVT_E_INVALID, "covZZ is singular");
    {  // k1r = u1' D uResid = (u1'W uy - (ux'W u1)' beta) / sigma2 : one more reduction over [u1 | uy]
      DevBuf<double> d_uy2;
      HIP_TRY(c, d_uy2.alloc(sizeof(double) * (size_t)N * 2));
      HIP_TRY(c, hipMemcpyAsync(d_uy2, c->d_u1, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(d_uy2 + (size_t)N, c->d_uxy + (size_t)N * d, sizeof(double) * (size_t)N,
                                hipMemcpyDeviceToDevice, st));
      DevBuf<double> d_abs3;
      HIP_TRY(c, d_abs3.alloc(sizeof(double) * N));
      HIP_TRY(c, hipMemcpyAsync(d_abs3, absS.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(lmm_sums_kernel, dim3(kLmmBlocks), dim3(256), sizeof(double) * 256, st, d_uy2, d_abs3,
                         (long long)N, 1, delta, 1, c->d_lmm_part);
      const int rec1 = lmm_rec_len(1);
      std::vector<double> p1((size_t)kLmmBlocks * rec1);
      HIP_TRY(c, hipMemcpyAsync(p1.data(), c->d_lmm_part, sizeof(double) * p1.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      d_uy2.reset();
      d_abs3.reset();
      double u1Wy = 0.0;
      for (int b = 0; b < kLmmBlocks; ++b) u1Wy += p1[(size_t)b * rec1 + 1];  // b[0] = u1' W uy
      double k = u1Wy;
      for (int a = 0; a < d; ++a) k -= sums[d * d + a] * beta[a];
      c->famcov_k1r = k / sigma2;
    }
    for (DevBuf<double>* pp : {&c->d_cX, &c->d_cv, &c->d_cr}) pp->reset();
    const int dc = d + 2;  // U'X | u1 | allele-frequency column
    HIP_TRY(c, c->d_cX.alloc(vb * dc));
    HIP_TRY(c, c->d_cv.alloc(vb));
    HIP_TRY(c, c->d_cr.alloc(vb));
    HIP_TRY(c, hipMemsetAsync(c->d_cX, 0, vb * dc, st));
    HIP_TRY(c, hipMemsetAsync(c->d_cv, 0, vb, st));
    HIP_TRY(c, hipMemsetAsync(c->d_cr, 0, vb, st));
    hipLaunchKernelGGL(famcov_build_null_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_uxy,
                       c->d_S, c->d_u1, (long long)N, (long long)ld, d, sigma2, delta, c->d_fbeta, c->d_cX, c->d_cr,
                       c->d_cv);
    NullConsts& cn = c->famcov_nc;
    std::memset(&cn, 0, sizeof(cn));
    cn.N = N;
    cn.ld = ld;
    cn.d = dc;
    cn.binary = 1;
    cn.sigma2 = 1.0;
    for (int a = 0; a < dc; ++a) cn.C[a * dc + a] = cn.Cinv[a * dc + a] = 1.0;  // unused by the covariance kernels
    HIP_TRY(c, c->d_famcov_nc.grow(sizeof(NullConsts), sizeof(NullConsts)));
    HIP_TRY(c, hipMemcpyAsync(c->d_famcov_nc, &cn, sizeof(NullConsts), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, sync_stream(st));
  c->have_fam = true;
  return RVT_OK;
}

// Run V already ROTATED columns (d_rot, leading dimension ld) through the sufficient statistics with the family
// covariance null set and finish with the covariance kernels in family mode.  d_cs / d_poly: raw (unrotated) column
// sums and polymorphic flags on the device.
namespace {
int famcov_run(rvt_ctx* c, const double* d_rot, int V, const double* d_cs, const int* d_poly, CovOut* co) {
  const int64_t ld = c->fam_nc.ld;
  std::vector<double> af(V, 0.01);
  rvt_gene_result r;
  co->fam = true;
  co->d_raw_colsum = d_cs;
  co->d_raw_poly = d_poly;
  const double* p = d_rot;
  // the batch code reads the null set from the context: install the family-covariance set for this call
  NullConsts keep_nc = c->nc;
  NullConsts* keep_dnc = c->d_nc;
  double *kX = c->d_X, *kres = c->d_res, *krr = c->d_rr, *kv = c->d_v, *kz = c->d_zeros;
  const bool khave = c->have_null;
  const int64_t kld = c->null_ld;
  c->nc = c->famcov_nc;
  c->d_nc = c->d_famcov_nc;
  c->d_X = c->d_cX;
  c->d_res = c->d_fzeros;
  c->d_rr = c->d_cr;
  c->d_v = c->d_cv;
  c->d_zeros = c->d_fzeros;
  c->have_null = true;
  c->null_ld = ld;
  int rc = run_batch(c, 1, &p, &V, af.data(), nullptr, 0u, nullptr, &r, nullptr, co);
  c->nc = keep_nc;
  c->d_nc = keep_dnc;
  c->d_X = kX;
  c->d_res = kres;
  c->d_rr = krr;
  c->d_v = kv;
  c->d_zeros = kz;
  c->have_null = khave;
  c->null_ld = kld;
  for (auto& sl : c->slots)
    if (sl.pending_out == &r) {
      sl.pending_out = nullptr;
      sl.pending_n = 0;
    }
  return rc;
}
}  // namespace

// Raw column statistics + rotation by U' of one block of <= RVT_MAX_VARIANTS raw columns, then famcov_run.
static int fam_block_run(rvt_ctx* c, const double* dG, int V, CovOut* cop) {
  if (V > RVT_MAX_VARIANTS) return fail(c, RVT_E_TOO_LARGE, "block of %d variants exceeds RVT_MAX_VARIANTS", V);
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  rc = ensure_fam_cols(c, (size_t)V, ld);
  if (rc) return rc;
  DevBuf<double> d_cs;
  DevBuf<int> d_poly;
  HIP_TRY(c, d_cs.alloc(sizeof(double) * (size_t)V));
  HIP_TRY(c, d_poly.alloc(sizeof(int) * (size_t)V));
  hipLaunchKernelGGL(raw_colstat_kernel, dim3((unsigned)V), dim3(256), 0, st, dG, (long long)N, (long long)ld, d_cs,
                     d_poly);
  HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * V, st));
  {
    int rcr = rotate_columns(c, dG, ld, V, c->d_Gt, ld, st);
    if (rcr) return rcr;
  }
  HIP_TRY(c, sync_stream(st));
  return famcov_run(c, c->d_Gt, V, d_cs, d_poly, cop);
}

// MetaCov with kinship (quantitative): rotate the block, then famcov_run.
int rvt_cov_block_fam(rvt_ctx* c, const double* dG, int V, double* cov, double* xz, double* zz, int* polymorphic) {
  if (!c || !dG || V < 1 || !cov || !xz || !polymorphic) return fail(c, RVT_E_INVALID, "bad arguments");
  CovOut co;
  co.cov = cov;
  co.xz = xz;
  co.zz = zz;
  co.poly = polymorphic;
  int rc = fam_block_run(c, dG, V, &co);
  if (!rc && c->famcov_b2 != 1.0) {  // MetaCovFamBinary: covXX, covXZ, covZZ each carry b^2 (Model.cpp:651-668)
    const double b2 = c->famcov_b2;
    const int du = c->famcov_nc.d - 2;
    for (int h = 0; h < V; ++h)
      for (int j = h; j < V; ++j) cov[(size_t)h + (size_t)j * V] *= b2;
    for (size_t i = 0; i < (size_t)V * du; ++i) xz[i] *= b2;
    if (zz)
      for (int i = 0; i < du * du; ++i) zz[i] *= b2;
  }
  return rc;
}

// FamAnalyticVT (AnalyticVT(RELATED), src/Model.h:2189-2214): af_i = FastLMM::FastGetAF of column i of the flipped,
// polymorphic genotype, (u, v) = FastLMM::CalculateUandV (regression/FastLMM.cpp:259-291: u = (U'g_c)' (lambda + delta)^-1
// uResid / sigma2, v = (U'g_c)' scaledK (U'g_c) / sigma2), then MultivariateVT::compute.  u, v and af of the RAW columns
// come from the family-covariance machinery (ustat / band / GLS frequency of fam_block_run); flipping a column to its
// minor allele (g -> 2 - g) changes the sign of its centred genotype and maps af to 1 - af, monomorphic columns drop out.
int rvt_fam_analytic_vt(rvt_ctx* c, int n, const double* const* dG, const int* Ms, rvt_gene_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !Ms || !out))) return fail(c, RVT_E_INVALID, "bad batch arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  hipSetDevice(c->device);
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  for (int g = 0; g < n; ++g) {
    const int M = Ms[g];
    rvt_gene_result& r = out[g];
    std::memset(&r, 0, sizeof(r));
    r.gene_id = g;
    r.n_variants = M;
    if (M < 1 || M > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M);
    int rc = rvt_sync(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    // flip / polymorphic decisions on the raw columns (DataConsolidator.cpp:46-69,94-116)
    std::vector<const double*> cols(M);
    for (int j = 0; j < M; ++j) cols[j] = dG[g] + (size_t)j * ld;
    DevBuf<const double*> d_cols;
    DevBuf<int> d_flags;
    DevBuf<double> d_buf;
    DevBuf<rvt_gene_result> d_res;
    HIP_TRY(c, d_cols.alloc(sizeof(double*) * (size_t)M));
    HIP_TRY(c, d_flags.alloc(sizeof(int) * (size_t)M));
    HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fam_colstat_kernel, dim3((unsigned)M), dim3(256), 0, st, d_cols, (long long)N, d_flags);
    std::vector<int> flags(M);
    HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * M, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    std::vector<double> cov((size_t)M * M), xz((size_t)M * RVT_MAX_COV), ustat(M), vstat(M), af(M), pval(M);
    std::vector<int> poly(M);
    CovOut co;
    co.cov = cov.data();
    co.xz = xz.data();
    co.poly = poly.data();
    co.ustat = ustat.data();
    co.vstat = vstat.data();
    co.af = af.data();
    co.pval = pval.data();
    rc = fam_block_run(c, dG[g], M, &co);
    if (rc) return rc;
    std::vector<int> kept;
    for (int j = 0; j < M; ++j)
      if (flags[j] & 2) kept.push_back(j);
    const int m = (int)kept.size();
    r.n_poly = m;
    if (m == 0) continue;  // genotype.cols == 0 -> NA row
    const int Mp = (m + 15) / 16 * 16;
    const size_t nbuf = 2 * (size_t)m + (size_t)m * m + gene_vt_doubles(Mp);
    std::vector<double> host(2 * (size_t)m + (size_t)m * m);
    for (int a = 0; a < m; ++a) {
      const int j = kept[a];
      const double sa = (flags[j] & 1) ? -1.0 : 1.0;
      host[a] = (flags[j] & 1) ? 1.0 - af[j] : af[j];
      host[m + a] = sa * ustat[j];
      for (int b = 0; b < m; ++b) {
        const int k = kept[b];
        const double sb = (flags[k] & 1) ? -1.0 : 1.0;
        const double v = j <= k ? cov[(size_t)j + (size_t)k * M] : cov[(size_t)k + (size_t)j * M];
        host[2 * (size_t)m + (size_t)b * m + a] = sa * sb * v;
      }
    }
    HIP_TRY(c, d_buf.alloc(sizeof(double) * nbuf));
    HIP_TRY(c, d_res.alloc(sizeof(rvt_gene_result)));
    HIP_TRY(c, hipMemcpyAsync(d_buf, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_res, &r, sizeof(r), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(vt_direct_kernel, dim3(1), dim3(256), 0, st, m, Mp, d_buf, d_res);
    {
      GeneDesc gdv;
      std::memset(&gdv, 0, sizeof(gdv));
      gdv.Mp = Mp;
      gdv.vt_mem = d_buf + 2 * (size_t)m + (size_t)m * m;
      gdv.result = d_res;
      DevBuf<GeneDesc> d_gdv;
      HIP_TRY(c, d_gdv.alloc(sizeof(GeneDesc)));
      hipError_t e = hipMemcpyAsync(d_gdv, &gdv, sizeof(gdv), hipMemcpyHostToDevice, st);
      for (int stage = 0; stage < 2 && e == hipSuccess; ++stage) {
        k_vt_integrate(dim3(1, kMvnShifts), st, d_gdv, stage);
        k_vt_finish(dim3(1), st, d_gdv, 1, stage);
      }
      if (e == hipSuccess) e = sync_stream(st);
      d_gdv.reset();
      HIP_TRY(c, e);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&r, d_res, sizeof(r), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  return RVT_OK;
}

// MetaScore with kinship: FastLMM score test of every raw column, the block in pieces of RVT_MAX_VARIANTS.
// binary = 0: MetaFamQtl; binary = 1: MetaFamBinary (genotype not centred; U b, V b^2 with the b of rvt_fam_binary_scale).
int rvt_score_block_fam(rvt_ctx* c, const double* dG, int V, int binary, int* ok, double* ustat, double* vstat,
                        double* af, double* pvalue) {
  if (!c || !dG || V < 1 || !ok || !ustat || !vstat || !af || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  const int64_t ld = c->fam_nc.ld;
  for (int c0 = 0; c0 < V; c0 += RVT_MAX_VARIANTS) {
    const int n = std::min(RVT_MAX_VARIANTS, V - c0);
    CovOut co;
    co.poly = ok + c0;
    co.ustat = ustat + c0;
    co.vstat = vstat + c0;
    co.af = af + c0;
    co.pval = pvalue + c0;
    co.uncentred = binary != 0;
    int rc = fam_block_run(c, dG + (size_t)c0 * ld, n, &co);
    if (rc) return rc;
  }
  if (binary) {  // MetaFamBinary::GetU / GetV (src/Model.h:3647-3648); the p-value is the unscaled statistic's
    const double b2 = c->famcov_b2, b = std::sqrt(b2);
    for (int h = 0; h < V; ++h) {
      ustat[h] *= b;
      vstat[h] *= b2;
    }
  }
  return RVT_OK;
}

// FastLMM::GetNullCovB (regression/FastLMM.cpp:473-483) as MetaFamQtl::PrintNullModel prints it: the diagonal of
// (ux' diag(lambda + delta) ux)^-1 — literally the reference's expression (it multiplies by lambda + delta where its
// own comment derives the inverse weights).
int rvt_fam_null_summary(rvt_ctx* c, double* covb_diag) {
  if (!c || !covb_diag) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  const int64_t N = c->fam_nc.N;
  const int d = c->fam_nc.d - 1;
  std::vector<double> ux((size_t)N * d);
  HIP_TRY(c, hipMemcpy(ux.data(), c->d_uxy, sizeof(double) * (size_t)N * d, hipMemcpyDeviceToHost));
  double A[RVT_MAX_COV * RVT_MAX_COV] = {}, Ai[RVT_MAX_COV * RVT_MAX_COV];
  for (int a = 0; a < d; ++a)
    for (int b = a; b < d; ++b) {
      double t = 0.0;
      for (int64_t i = 0; i < N; ++i)
        t += ux[(size_t)a * N + i] * (std::fabs(c->h_S[i]) + c->fam_delta) * ux[(size_t)b * N + i];
      A[a * d + b] = A[b * d + a] = t;
    }
  if (!invert_spd(A, d, Ai)) return fail(c, RVT_E_INVALID, "ux' (lambda + delta) ux is singular");
  for (int a = 0; a < d; ++a) covb_diag[a] = Ai[a * d + a];
  return RVT_OK;
}

int rvt_fam_binary_scale(rvt_ctx* c, int64_t n_case, int64_t n_ctrl, double* alpha_out, double* b_out) {
  if (!c || n_case < 0 || n_ctrl < 0) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_fit_fam_null first");
  const float alpha = (n_ctrl > 0) ? (float)std::log(1.0 * (double)n_case / (double)n_ctrl) : 500.f;
  // b = int logistic'(alpha + x) phi(x) dx.  The integrand is analytic and decays like exp(-x^2/2), for which the
  // trapezoidal rule converges geometrically: h = 1/64 over [-40, 40] is exact to rounding (the reference's QAGI
  // stops at 1e-7 relative).  A scalar constant of the null model, evaluated once.
  const double a = (double)alpha, h = 1.0 / 64.0;
  double sum = 0.0;
  for (int i = -40 * 64; i <= 40 * 64; ++i) {
    const double x = i * h;
    const double t = std::exp(a + x);
    const double k = 1.0 / std::sqrt(2.0 * 3.1415926535897);  // the reference's constant (src/Model.cpp:343)
    const double f = std::isfinite(t) ? t / (1. + t) / (1. + t) * k * std::exp(-x * x * 0.5) : 0.0;
    sum += f;
  }
  const float b = (float)(sum * h);  // `float b` member (src/Model.cpp:680)
  c->famcov_b2 = (double)b * (double)b;
  if (alpha_out) *alpha_out = alpha;
  if (b_out) *b_out = b;
  return RVT_OK;
}

static int fam_tests_tail(rvt_ctx* c, int n, uint32_t tests, const std::vector<int>& Mk, const std::vector<int>& off,
                          const std::vector<int>& kgene, size_t T, const double* d_bcs, const int* d_bpoly,
                          rvt_gene_result* out);

int rvt_run_fam_blocks(rvt_ctx* c, int n, const double* const* dG, const int* Ms, const int64_t* ids,
                       rvt_gene_result* out) {
  return rvt_run_fam_tests(c, n, dG, Ms, ids, RVT_TEST_FAMSKAT, out);
}

int rvt_run_fam_tests(rvt_ctx* c, int n, const double* const* dG, const int* Ms, const int64_t* ids, uint32_t tests,
                      rvt_gene_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !Ms || !out))) return fail(c, RVT_E_INVALID, "bad batch arguments");
  if (!(tests & (RVT_TEST_FAMSKAT | RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)) ||
      (tests & ~(RVT_TEST_FAMSKAT | RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)))
    return fail(c, RVT_E_INVALID, "rvt_run_fam_tests takes the FAMSKAT / FAMCMC / FAMZEGGINI bits");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  if (n == 0) return RVT_OK;
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  // ---- 1. flip / monomorphic flags of every column (DataConsolidator.cpp:46-69,94-142) ------------------------
  size_t tot = 0;
  for (int g = 0; g < n; ++g) {
    if (Ms[g] < 1 || Ms[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_TOO_LARGE, "gene %d: M=%d", g, Ms[g]);
    tot += (size_t)Ms[g];
  }
  std::vector<const double*> cols(tot);
  {
    size_t k = 0;
    for (int g = 0; g < n; ++g)
      for (int j = 0; j < Ms[g]; ++j) cols[k++] = dG[g] + (size_t)j * ld;
  }
  // column pointer / flag lists of the batch: one grow-only allocation of the context (no hipMalloc / hipFree per batch)
  {
    const size_t need = (sizeof(double*) + sizeof(int)) * tot * 2 + 64;
    HIP_TRY(c, c->d_fam_list.grow(need, need + need / 2, st, true));
  }
  const double** d_cols = reinterpret_cast<const double**>(c->d_fam_list.get());
  int* d_flags = reinterpret_cast<int*>(c->d_fam_list + sizeof(double*) * tot * 2);
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * tot, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fam_colstat_kernel, dim3((unsigned)tot), dim3(256), 0, st, d_cols, (long long)N, d_flags);
  std::vector<int> flags(tot);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * tot, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  // ---- 2. compact the kept columns (flipped where needed) and rotate them by U' --------------------------------
  std::vector<const double*> kept_cols;
  std::vector<int> kept_flip, Mk(n), off(n);
  bool all_hard = true;  // every kept column holds hard calls only
  {
    size_t k = 0;
    for (int g = 0; g < n; ++g) {
      off[g] = (int)kept_cols.size();
      for (int j = 0; j < Ms[g]; ++j, ++k)
        if (flags[k] & 2) {
          kept_cols.push_back(cols[k]);
          kept_flip.push_back(flags[k] & 1);
          all_hard = all_hard && (flags[k] & 4);
        }
      Mk[g] = (int)kept_cols.size() - off[g];
    }
  }
  const size_t T = kept_cols.size();
  for (int g = 0; g < n; ++g) {
    rvt_gene_result& r = out[g];
    std::memset(&r, 0, sizeof(r));
    r.gene_id = ids ? ids[g] : g;
    r.n_variants = Ms[g];
    r.n_poly = Mk[g];
  }
  if (T == 0) return RVT_OK;  // genotype.cols == 0 everywhere: all NA (src/Model.h:3066-3069)
  // genes with a polymorphic column, and — for the burden tests — two collapsed columns each after the T genotype ones
  const bool burden = (tests & (RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)) != 0;
  std::vector<int> kgene, koff, km;
  for (int g = 0; g < n; ++g)
    if (Mk[g] > 0) {
      kgene.push_back(g);
      koff.push_back(off[g]);
      km.push_back(Mk[g]);
    }
  const size_t nk = kgene.size(), TB = burden ? 2 * nk : 0;
  rc = ensure_fam_cols(c, T + TB, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_cols + tot, kept_cols.data(), sizeof(double*) * T, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags + tot, kept_flip.data(), sizeof(int) * T, hipMemcpyHostToDevice, st));
  if (ld != N)  // pad rows must be zero (the rotation writes rows 0 .. N-1 of every column)
    HIP_TRY(c, hipMemset2DAsync(c->d_Gt + N, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)(ld - N), T + TB, st));
  // FamSKAT alone on hard calls: the flipped columns go straight to the int8 plane of the rotation (no fp64 copy, no
  // column scan, no separate quantiser pass)
  const bool direct = !burden && all_hard && c->hc_enabled && !(c->d_csc_ptr && !c->d_uq_range) &&
                      !getenv("RVT_FAM_NO_DIRECT");
  if (!direct) {
    for (size_t t0 = 0; t0 < T; t0 += 65535) {  // (gridDim.y holds at most 65535 columns)
      const unsigned nt = (unsigned)std::min<size_t>(65535, T - t0);
      hipLaunchKernelGGL(fam_flip_compact_kernel, dim3(64, nt), dim3(256), 0, st, d_cols + tot + t0, d_flags + tot + t0,
                         (long long)N, (long long)ld, c->d_Gp + t0 * (size_t)ld);
    }
    HIP_TRY(c, hipGetLastError());
  }
  DevBuf<int> d_koff;
  DevBuf<double> d_bcs;
  DevBuf<int> d_bpoly;
  if (burden) {
    // cmcCollapse / zegginiCollapse of the flipped, filtered blocks into columns T .. T + 2 nk - 1, then their raw
    // sums (the score test centres the collapsed genotype, FastLMM.cpp:218-220)
    HIP_TRY(c, d_koff.alloc(sizeof(int) * 2 * nk));
    HIP_TRY(c, d_bcs.alloc(sizeof(double) * TB));
    HIP_TRY(c, d_bpoly.alloc(sizeof(int) * TB));
    HIP_TRY(c, hipMemcpyAsync(d_koff, koff.data(), sizeof(int) * nk, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_koff + nk, km.data(), sizeof(int) * nk, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->d_Gp + (size_t)T * ld, 0, sizeof(double) * (size_t)ld * TB, st));
    hipLaunchKernelGGL(fam_collapse_kernel, dim3(64, (unsigned)nk), dim3(256), 0, st, c->d_Gp, d_koff, d_koff + nk,
                       (long long)N, (long long)ld, c->d_Gp + (size_t)T * ld);
    hipLaunchKernelGGL(raw_colstat_kernel, dim3((unsigned)TB), dim3(256), 0, st, c->d_Gp + (size_t)T * ld,
                       (long long)N, (long long)ld, d_bcs, d_bpoly);
  }
  if (direct) {
    const int64_t ldk = c->uq_ldk;
    for (size_t c0 = 0; c0 < T; c0 += kRotMaxCols) {  // long lists in pieces, as rotate_columns
      const int ncp = (int)std::min<size_t>(kRotMaxCols, T - c0);
      const int64_t cols_pad = ((int64_t)ncp + kRotBN - 1) / kRotBN * kRotBN;
      const size_t need = (size_t)cols_pad * (size_t)ldk;
      HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
      HIP_TRY(c, hipMemsetAsync(c->d_rotB, 0, need, st));
      hipLaunchKernelGGL(fam_flip_quant_kernel, dim3(64, (unsigned)ncp), dim3(256), 0, st, d_cols + tot + c0,
                         d_flags + tot + c0, (long long)N, (long long)ldk, c->d_rotB);
      std::vector<int> zero_exp((size_t)ncp, 0);
      int rcr = planes_gemm(c, c->d_Uq, c->uq_plane, kRotPlanesU, (int)N, nullptr, c->uq_sexp, c->d_rotB, need, 1, ncp,
                            zero_exp.data(), N, ldk, c->d_Gt + c0 * (size_t)ld, ld, st, c->d_uq_range);
      if (rcr) return rcr;
    }
  } else {  // the rotation of the whole batch: genotype columns + collapsed burden columns (exact int8 products, rot_gemm.hip.h)
    int rcr = rotate_columns(c, c->d_Gp, ld, (int)(T + TB), c->d_Gt, ld, st);
    if (rcr) return rcr;
  }
  HIP_TRY(c, sync_stream(st));
  return fam_tests_tail(c, n, tests, Mk, off, kgene, T, d_bcs, d_bpoly, out);
}

// The tail of rvt_run_fam_tests and rvt_run_fam_tests_bed_dev, behind either front stage.  The front has initialised the n
// records (gene_id, n_variants, n_poly) and left in c->d_Gt, leading dimension fam_nc.ld, the T rotated kept columns — gene g
// owns Mk[g] of them from column off[g] on — and, for the burden tests, behind them the rotated CMC / Zeggini columns of the genes
// with a kept column (kgene, two each) with their raw sums d_bcs and polymorphic flags d_bpoly on the device.
static int fam_tests_tail(rvt_ctx* c, int n, uint32_t tests, const std::vector<int>& Mk, const std::vector<int>& off,
                          const std::vector<int>& kgene, size_t T, const double* d_bcs, const int* d_bpoly,
                          rvt_gene_result* out) {
  int rc;
  const int64_t ld = c->fam_nc.ld;
  const bool burden = (tests & (RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)) != 0;
  const size_t nk = kgene.size(), TB = burden ? 2 * nk : 0;
  if (burden) {
    // FamCMC / FamZeggini: the 2 nk rotated collapsed columns as blocks of the family covariance machinery
    // (V = cov(h,h), U from the uResid column, AF from the allele-frequency column)
    std::vector<double> us(TB), vs(TB), afs(TB), ps(TB);
    for (size_t b0 = 0; b0 < TB; b0 += RVT_MAX_VARIANTS) {
      const int V = (int)std::min<size_t>(RVT_MAX_VARIANTS, TB - b0);
      CovOut co;
      co.ustat = us.data() + b0;
      co.vstat = vs.data() + b0;
      co.af = afs.data() + b0;
      co.pval = ps.data() + b0;
      rc = famcov_run(c, c->d_Gt + (T + b0) * (size_t)ld, V, d_bcs + b0, d_bpoly + b0, &co);
      if (rc) return rc;
    }
    for (size_t k = 0; k < nk; ++k) {
      rvt_gene_result& r = out[kgene[k]];
      if (tests & RVT_TEST_FAMCMC) {
        r.famcmc_ok = 1;
        r.famcmc_af = afs[2 * k];
        r.famcmc_U = us[2 * k];
        r.famcmc_V = vs[2 * k];
        r.famcmc_p = ps[2 * k];
      }
      if (tests & RVT_TEST_FAMZEGGINI) {
        r.famzeg_ok = 1;
        r.famzeg_af = afs[2 * k + 1];
        r.famzeg_U = us[2 * k + 1];
        r.famzeg_V = vs[2 * k + 1];
        r.famzeg_p = ps[2 * k + 1];
      }
    }
  }
  if (!(tests & RVT_TEST_FAMSKAT)) return RVT_OK;
  // ---- 3. the rotated blocks go through the ordinary batch machinery with the FamSKAT null set ---------------
  std::vector<const double*> ptr;
  std::vector<int> mm, which;
  std::vector<int64_t> gid;
  size_t af_total = 0;
  for (int g = 0; g < n; ++g)
    if (Mk[g] > 0) {
      ptr.push_back(c->d_Gt + (size_t)off[g] * ld);
      mm.push_back(Mk[g]);
      which.push_back(g);
      gid.push_back(out[g].gene_id);
      af_total += (size_t)Mk[g];
    }
  std::vector<double> af(af_total, 0.0);  // unused: FamSKAT derives its allele frequencies on the device
  std::vector<rvt_gene_result> rec(ptr.size());
  struct Swap {  // the batch code reads the null set from the context
    rvt_ctx* c;
    NullConsts nc;
    NullConsts* d_nc;
    double *X, *res, *rr, *v, *zeros;
    bool have;
    int64_t nld;
    explicit Swap(rvt_ctx* c_) : c(c_), nc(c_->nc), d_nc(c_->d_nc), X(c_->d_X), res(c_->d_res), rr(c_->d_rr),
                                 v(c_->d_v), zeros(c_->d_zeros), have(c_->have_null), nld(c_->null_ld) {
      c->nc = c->fam_nc;
      c->d_nc = c->d_fam_nc;
      c->d_X = c->d_fX;
      c->d_res = c->d_fzeros;
      c->d_rr = c->d_frr;
      c->d_v = c->d_fv;
      c->d_zeros = c->d_fzeros;
      c->have_null = true;
      c->null_ld = c->fam_nc.ld;
    }
    ~Swap() {
      c->nc = nc;
      c->d_nc = d_nc;
      c->d_X = X;
      c->d_res = res;
      c->d_rr = rr;
      c->d_v = v;
      c->d_zeros = zeros;
      c->have_null = have;
      c->null_ld = nld;
    }
  };
  {
    Swap sw(c);
    // batches of <= 256 genes keep the per-batch arena bounded
    for (size_t b0 = 0; b0 < ptr.size(); b0 += 256) {
      const int nb = (int)std::min<size_t>(256, ptr.size() - b0);
      size_t afo = 0;
      for (size_t k = 0; k < b0; ++k) afo += (size_t)mm[k];
      rc = run_batch(c, nb, ptr.data() + b0, mm.data() + b0, af.data() + afo, gid.data() + b0, RVT_TEST_FAMSKAT,
                     nullptr, rec.data() + b0, nullptr);
      if (!rc) rc = rvt_sync(c);
      if (rc) return rc;
    }
  }
  for (size_t k = 0; k < which.size(); ++k) {
    rvt_gene_result& r = out[which[k]];
    r.status = rec[k].status;
    r.famskat_ok = rec[k].famskat_ok;
    r.famskat_Q = rec[k].famskat_Q;
    r.famskat_p = rec[k].famskat_p;
    r.skat_nlambda = rec[k].skat_nlambda;
    r.davies_terms = rec[k].davies_terms;
  }
  return RVT_OK;
}

// ---- single-variant tests for related samples: famLRT and famGrammarGamma (fam_single.hip.h) ------------------------------
namespace {
using namespace rvt_fs;

// the kLmmBlocks partial records of a reduction, summed in block order
int fs_records(rvt_ctx* c, const double* d_part, int rec, hipStream_t st, std::vector<double>* sums) {
  std::vector<double> part((size_t)kLmmBlocks * rec);
  HIP_TRY(c, hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  sums->assign(rec, 0.0);
  for (int q = 0; q < rec; ++q) {
    double s = 0.0;
    for (int b = 0; b < kLmmBlocks; ++b) s += part[(size_t)b * rec + q];
    (*sums)[q] = s;
  }
  return RVT_OK;
}

// d_out = U d_v (N doubles each, eigenpairs in the installed order).  The digit planes with the family panels of the
// rotation (apply_u_kernel), or, for a sparse U whose supports are scattered, a gather over its row-compressed copy
// (apply_u_sparse_kernel; the copy is made once per installed kinship).
int fs_apply_u(rvt_ctx* c, const double* d_v, double* d_out, double* d_part, int64_t ldp, hipStream_t st) {
  const int64_t N = c->kin_N;
  if (c->d_Uq) {
    const long long npanels = (long long)(c->uq_rows_pad / kRotBM);
    const int slices = (int)std::max<long long>(1, std::min<long long>(kApplySlices, npanels));
    hipLaunchKernelGGL(apply_u_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)slices), dim3(kFsThreads), 0, st, c->d_Uq,
                       (long long)c->uq_plane, kRotPlanesU, (long long)c->uq_ldk, c->d_uq_range, kRotBM, kRotKC,
                       (long long)N, npanels, d_v, d_part, (long long)ldp);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(apply_u_reduce_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_part, (long long)ldp,
                       slices, (long long)N, c->uq_sexp, d_out);
    HIP_TRY(c, hipGetLastError());
    return RVT_OK;
  }
  if (!c->d_csc_ptr) return fail(c, RVT_E_STATE, "no kinship eigenvectors installed");
  if (!c->d_csr_ptr) {  // once per installed kinship: the column-compressed U transposed (rows in order, columns ascending)
    std::vector<long long> ptr((size_t)N + 1);
    HIP_TRY(c, hipMemcpyAsync(ptr.data(), c->d_csc_ptr, sizeof(long long) * ptr.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    const size_t nnz = (size_t)ptr[N];
    std::vector<int> rows(nnz), cols(nnz);
    std::vector<double> vals(nnz), tvals(nnz);
    HIP_TRY(c, hipMemcpyAsync(rows.data(), c->d_csc_rows, sizeof(int) * nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(vals.data(), c->d_csc_vals, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    std::vector<long long> rp((size_t)N + 1, 0), fill;
    for (size_t e = 0; e < nnz; ++e) ++rp[(size_t)rows[e] + 1];
    for (int64_t i = 0; i < N; ++i) rp[i + 1] += rp[i];
    fill.assign(rp.begin(), rp.end() - 1);
    for (int64_t k = 0; k < N; ++k)
      for (long long e = ptr[k]; e < ptr[k + 1]; ++e) {
        const long long o = fill[rows[e]]++;
        cols[o] = (int)k;
        tvals[o] = vals[e];
      }
    HIP_TRY(c, c->d_csr_ptr.alloc(sizeof(long long) * ((size_t)N + 1)));
    HIP_TRY(c, c->d_csr_cols.alloc(sizeof(int) * std::max<size_t>(nnz, 1)));
    HIP_TRY(c, c->d_csr_vals.alloc(sizeof(double) * std::max<size_t>(nnz, 1)));
    HIP_TRY(c, hipMemcpyAsync(c->d_csr_ptr, rp.data(), sizeof(long long) * rp.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_csr_cols, cols.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_csr_vals, tvals.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(c, sync_stream(st));
  }
  hipLaunchKernelGGL(apply_u_sparse_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_csr_ptr, c->d_csr_cols,
                     c->d_csr_vals, (long long)N, d_v, d_out);
  HIP_TRY(c, hipGetLastError());
  return RVT_OK;
}

extern "C++" {
template <int DMAX, int VT>
void fs_launch_lrt(hipStream_t st, int n, const double* Gt, long long ld, long long N, const double* ux, const double* vec,
                   long long vld, const double* Ainv, const int* poly, const LrtConsts& k, int* ok, double* af, double* nll,
                   double* all, double* pv) {
  hipLaunchKernelGGL((fam_lrt_kernel<DMAX, VT>), dim3((unsigned)((n + VT - 1) / VT)), dim3(kFsThreads), 0, st, Gt, ld, N, n,
                     ux, vec, vld, Ainv, poly, k, ok, af, nll, all, pv);
}
}  // extern "C++"
}  // namespace

namespace {
// famLRT's work space (d_lrt_ws) as a piece of columns uses it, and the constants of the null fit
struct LrtWs {
  double *vec, *ainv, *cs, *af, *nll, *all, *pv;
  int *poly, *ok;
  LrtConsts k;
};

// The work space and, once per null fit, its constants (lrt_gen).  Shared by rvt_lrt_block_fam and rvt_lrt_bed_dev_fam.
int lrt_prepare(rvt_ctx* c, hipStream_t st, LrtWs* w) {
  int rc = RVT_OK;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  const int d = c->fam_nc.d - 1;
  const int MV = RVT_MAX_VARIANTS;
  Layout L;
  const size_t o_vec = L.take(sizeof(double) * 3 * (size_t)ld), o_abs = L.take(sizeof(double) * (size_t)ld),
               o_ainv = L.take(sizeof(double) * RVT_MAX_COV * RVT_MAX_COV), o_beta = L.take(sizeof(double) * RVT_MAX_COV),
               o_part = L.take(sizeof(double) * (size_t)kLmmBlocks * lmm_rec_len(RVT_MAX_COV)),
               o_cs = L.take(sizeof(double) * MV), o_poly = L.take(sizeof(int) * MV), o_ok = L.take(sizeof(int) * MV),
               o_af = L.take(sizeof(double) * MV), o_nll = L.take(sizeof(double) * MV), o_all = L.take(sizeof(double) * MV),
               o_pv = L.take(sizeof(double) * MV);
  // the constants live in the work space: a new block has lost them, and so has one that RVT_SCRIBBLE refills
  if (c->d_lrt_ws.cap < L.total || getenv("RVT_SCRIBBLE")) c->lrt_gen = 0;
  HIP_TRY(c, c->d_lrt_ws.grow(L.total, L.total, st, true));  // (grow-only, outside every loop; RVT_POISON fills it)
  char* ws = c->d_lrt_ws;
  double* d_vec = reinterpret_cast<double*>(ws + o_vec);
  double* d_abs = reinterpret_cast<double*>(ws + o_abs);
  double* d_ainv = reinterpret_cast<double*>(ws + o_ainv);
  double* d_beta = reinterpret_cast<double*>(ws + o_beta);
  double* d_part = reinterpret_cast<double*>(ws + o_part);
  double* d_cs = reinterpret_cast<double*>(ws + o_cs);
  int* d_poly = reinterpret_cast<int*>(ws + o_poly);
  int* d_ok = reinterpret_cast<int*>(ws + o_ok);
  double* d_af = reinterpret_cast<double*>(ws + o_af);
  double* d_nll = reinterpret_cast<double*>(ws + o_nll);
  double* d_all = reinterpret_cast<double*>(ws + o_all);
  double* d_pv = reinterpret_cast<double*>(ws + o_pv);
  const double delta = c->fam_delta;
  if (c->lrt_gen != c->fam_gen) {  // constants of the null fit, once per null (FastLMM.cpp:150-180 at the null's delta)
    std::vector<double> absS((size_t)N);
    for (int64_t i = 0; i < N; ++i) absS[i] = std::fabs(c->h_S[i]);
    HIP_TRY(c, hipMemcpyAsync(d_abs, absS.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lmm_sums_kernel, dim3(kLmmBlocks), dim3(256), sizeof(double) * 256, st, c->d_uxy, d_abs,
                       (long long)N, d, delta, 1, d_part);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> sums;
    rc = fs_records(c, d_part, lmm_rec_len(d), st, &sums);
    if (rc) return rc;
    double Ai[RVT_MAX_COV * RVT_MAX_COV] = {}, beta[RVT_MAX_COV] = {};
    if (!invert_spd(sums.data(), d, Ai)) return fail(c, RVT_E_INVALID, "ux' W ux is singular");
    for (int a = 0; a < d; ++a)
      for (int k = 0; k < d; ++k) beta[a] += Ai[a * d + k] * sums[d * d + k];
    c->lrt_slog = sums[d * d + d + 1];
    HIP_TRY(c, hipMemcpyAsync(d_ainv, Ai, sizeof(Ai), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_beta, beta, sizeof(beta), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fam_lrt_null_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_uxy, d_abs, c->d_u1,
                       (long long)N, d, delta, d_beta, d_vec, (long long)ld);
    hipLaunchKernelGGL(grammar_sums_kernel, dim3(kLmmBlocks), dim3(kFsThreads), 0, st, c->d_uxy, d_abs, (long long)N, d,
                       delta, 1, d_beta, d_part);
    HIP_TRY(c, hipGetLastError());
    rc = fs_records(c, d_part, 1, st, &sums);
    if (rc) return rc;
    c->lrt_ssr0 = sums[0];
    c->lrt_gen = c->fam_gen;
  }
  LrtConsts& k = w->k;
  k.n = (double)N;
  k.ssr0 = c->lrt_ssr0;
  k.sigma2 = c->fam_sigma2;
  k.slog = c->lrt_slog;
  k.afden = c->fam_nc.rss;  // u1' |S|^-1 u1 (rvt_fit_fam_null)
  k.d = d;
  w->vec = d_vec, w->ainv = d_ainv, w->cs = d_cs, w->poly = d_poly, w->ok = d_ok;
  w->af = d_af, w->nll = d_nll, w->all = d_all, w->pv = d_pv;
  return RVT_OK;
}

// n <= RVT_MAX_VARIANTS rotated columns in c->d_Gt with their polymorphic flags on the device -> the outputs on the host
int lrt_piece(rvt_ctx* c, hipStream_t st, const LrtWs& w, int n, const int* d_poly, int* ok, double* af, double* null_loglik,
              double* alt_loglik, double* pvalue) {
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  const int d = c->fam_nc.d - 1;
  if (d <= 4)
    fs_launch_lrt<4, 4>(st, n, c->d_Gt, ld, N, c->d_uxy, w.vec, ld, w.ainv, d_poly, w.k, w.ok, w.af, w.nll, w.all, w.pv);
  else if (d <= 8)
    fs_launch_lrt<8, 2>(st, n, c->d_Gt, ld, N, c->d_uxy, w.vec, ld, w.ainv, d_poly, w.k, w.ok, w.af, w.nll, w.all, w.pv);
  else
    fs_launch_lrt<RVT_MAX_COV, 1>(st, n, c->d_Gt, ld, N, c->d_uxy, w.vec, ld, w.ainv, d_poly, w.k, w.ok, w.af, w.nll, w.all,
                                  w.pv);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(ok, w.ok, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(af, w.af, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(null_loglik, w.nll, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(alt_loglik, w.all, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(pvalue, w.pv, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  return RVT_OK;
}
}  // namespace

int rvt_lrt_block_fam(rvt_ctx* c, const double* dG, int V, int* ok, double* af, double* null_loglik, double* alt_loglik,
                      double* pvalue) {
  if (!c || !dG || V < 1 || !ok || !af || !null_loglik || !alt_loglik || !pvalue)
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  const int MV = RVT_MAX_VARIANTS;
  LrtWs w;
  rc = lrt_prepare(c, st, &w);
  if (rc) return rc;
  for (int c0 = 0; c0 < V; c0 += MV) {
    const int n = std::min(MV, V - c0);
    const double* g = dG + (size_t)c0 * ld;
    rc = ensure_fam_cols(c, (size_t)n, ld);
    if (rc) return rc;
    hipLaunchKernelGGL(raw_colstat_kernel, dim3((unsigned)n), dim3(256), 0, st, g, (long long)N, (long long)ld, w.cs, w.poly);
    HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * n, st));
    rc = rotate_columns(c, g, ld, n, c->d_Gt, ld, st);
    if (rc) return rc;
    rc = lrt_piece(c, st, w, n, w.poly, ok + c0, af + c0, null_loglik + c0, alt_loglik + c0, pvalue + c0);
    if (rc) return rc;
  }
  return RVT_OK;
}

// ---- famScore / famLRT over rows of a resident .bed matrix (fam_bed_kernels.hip.h) ----------------------------------------------
namespace {
// what the front stage leaves on the device for a consumer (in d_fam_bed_ws), per row of the piece
struct FamBedPiece {
  unsigned long long* cnt;  // n0 n1 n2 missing
  double *mu, *muq, *cs;    // the fill value of a missing call, the same in the digit planes' fixed point; the column sum
  int* poly;
};

// the state every call here needs, and its V rows at d_rows (bed_rows_span): *cb = their pitch
int fam_bed_check(rvt_ctx* c, const char* who, const unsigned char* d_rows, int64_t V, int64_t* cb) {
  if (!c->have_fam) return fail(c, RVT_E_STATE, "%s: rvt_set_kinship + rvt_fit_fam_null first", who);
  return bed_rows_span(c, who, d_rows, V, BedModel::kFam, cb);
}

int fam_bed_ws(rvt_ctx* c, hipStream_t st, FamBedPiece* p) {
  const int MV = RVT_MAX_VARIANTS;
  Layout L;
  const size_t o_cnt = L.take(sizeof(unsigned long long) * 4 * MV), o_mu = L.take(sizeof(double) * MV),
               o_muq = L.take(sizeof(double) * MV), o_cs = L.take(sizeof(double) * MV), o_poly = L.take(sizeof(int) * MV);
  HIP_TRY(c, c->d_fam_bed_ws.grow(L.total, L.total, st, true));
  char* ws = c->d_fam_bed_ws;
  p->cnt = reinterpret_cast<unsigned long long*>(ws + o_cnt);
  p->mu = reinterpret_cast<double*>(ws + o_mu);
  p->muq = reinterpret_cast<double*>(ws + o_muq);
  p->cs = reinterpret_cast<double*>(ws + o_cs);
  p->poly = reinterpret_cast<int*>(ws + o_poly);
  return RVT_OK;
}

// The front stage of both calls: n <= RVT_MAX_VARIANTS consecutive rows, cb bytes apart -> what raw_colstat_kernel + rotate_columns give for
// the imputed fp64 columns of the same calls: the rotated columns in c->d_Gt (leading dimension fam_nc.ld, rows N .. ld - 1
// zero), their raw sums in p.cs and polymorphic flags in p.poly.  counts (host, 4 n entries, optional): n0 n1 n2 missing per row.
// The rotation goes by the installed form of U (fam_bed_kernels.hip.h); enqueued on st, which is synchronised on the way (the
// counts decide on the host whether the piece has a missing call at all).
int fam_bed_front(rvt_ctx* c, hipStream_t st, const unsigned char* d_rows, int64_t cb, int n, const FamBedPiece& p,
                  long long* counts) {
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  // 1. the site pass over the codes
  int rc = bed_piece_counts(c, st, d_rows, cb, N, n, p.cnt, nullptr, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(fam_bed_site_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.cnt, n, p.mu, p.muq,
                     p.cs, p.poly);
  HIP_TRY(c, hipGetLastError());
  std::vector<unsigned long long> cnt;
  rc = bed_counts_host(c, st, p.cnt, n, &cnt, counts);
  if (rc) return rc;
  bool any_missing = false;
  for (int h = 0; h < n; ++h) any_missing = any_missing || cnt[4 * (size_t)h + 3] != 0;
  // 2. the rotation, by the installed form
  const bool dense = !c->d_fam_run && !(c->d_csc_ptr && !c->d_uq_range);
  rc = ensure_fam_cols(c, (size_t)(dense && any_missing ? 2 * n : n), ld);  // (d_Gp holds [U'c | U'm] of a dense piece)
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * n, st));
  if (c->d_fam_run) {  // the family form
    hipLaunchKernelGGL(rot_fam_bed_kernel<BedRowsAt>, dim3((unsigned)c->fam_runs, (unsigned)((n + kRotFamCols - 1) / kRotFamCols)),
                       dim3(kRotFamRows), 0, st, c->d_fam_run, c->d_fam_of, c->d_fam_ptr, c->d_fam_members, c->d_csc_ptr,
                       c->d_csc_vals, BedRowsAt{d_rows, (long long)cb}, p.mu, n, c->d_Gt, (long long)ld);
    HIP_TRY(c, hipGetLastError());
    return RVT_OK;
  }
  if (!dense) {  // column-compressed U, scattered supports: fp64 columns on the device, then the gather of rotate_columns
    bed_rows_expand(st, d_rows, cb, p.mu, N, ld, n, c->d_Gp);
    HIP_TRY(c, hipGetLastError());
    return rotate_columns(c, c->d_Gp, ld, n, c->d_Gt, ld, st);
  }
  // dense U on digit planes: B = [c | m], one plane each (the m half only when the piece has a missing call); the operands are
  // 0 / 1 / 2, inside the 127 x 127 bound planes_gemm cuts its int32 ranges by
  const int64_t ldk = c->uq_ldk;
  const int nB = any_missing ? 2 * n : n;
  const size_t need = (size_t)(((int64_t)nB + kRotBN - 1) / kRotBN * kRotBN) * (size_t)ldk;
  HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
  HIP_TRY(c, hipMemsetAsync(c->d_rotB, 0, need, st));
  hipLaunchKernelGGL(fam_bed_unpack_kernel<BedRowsAt>, dim3((unsigned)((cb + 255) / 256), (unsigned)n), dim3(256), 0, st,
                     BedRowsAt{d_rows, (long long)cb}, (long long)cb, (long long)N, n, any_missing ? 1 : 0, c->d_rotB.get(),
                     (long long)ldk);
  HIP_TRY(c, hipGetLastError());
  const std::vector<int> zero_exp((size_t)nB, 0);
  double* C = any_missing ? c->d_Gp.get() : c->d_Gt.get();
  rc = planes_gemm(c, c->d_Uq, c->uq_plane, kRotPlanesU, (int)N, nullptr, c->uq_sexp, c->d_rotB, need, 1, nB, zero_exp.data(), N,
                   ldk, C, ld, st, c->d_uq_range);
  if (rc) return rc;
  if (any_missing) {
    hipLaunchKernelGGL(fam_bed_combine_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)n), dim3(256), 0, st, C,
                       (long long)ld, (long long)N, n, p.muq, c->d_Gt.get(), (long long)ld);
    HIP_TRY(c, hipGetLastError());
  }
  return RVT_OK;
}
}  // namespace

// MetaScore with kinship from resident rows: rvt_score_block_fam's loop with the front stage in place of the fp64 prefix.
int rvt_score_bed_dev_fam(rvt_ctx* c, const unsigned char* d_rows, int64_t V, int binary, int* ok, double* ustat, double* vstat,
                          double* af, double* pvalue, long long* counts) {
  if (!c || !d_rows || V < 1 || !ok || !ustat || !vstat || !af || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = fam_bed_check(c, "rvt_score_bed_dev_fam", d_rows, V, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  FamBedPiece p;
  rc = fam_bed_ws(c, st, &p);
  if (rc) return rc;
  for (int64_t v0 = 0; v0 < V; v0 += RVT_MAX_VARIANTS) {
    const int n = (int)std::min<int64_t>(RVT_MAX_VARIANTS, V - v0);
    rc = fam_bed_front(c, st, d_rows + (size_t)cb * (size_t)v0, cb, n, p, counts ? counts + 4 * v0 : nullptr);
    if (rc) return rc;
    HIP_TRY(c, sync_stream(st));
    CovOut co;
    co.poly = ok + v0;
    co.ustat = ustat + v0;
    co.vstat = vstat + v0;
    co.af = af + v0;
    co.pval = pvalue + v0;
    co.uncentred = binary != 0;
    rc = famcov_run(c, c->d_Gt, n, p.cs, p.poly, &co);
    if (rc) return rc;
  }
  if (binary) {  // MetaFamBinary::GetU / GetV (src/Model.h:3647-3648), as rvt_score_block_fam
    const double b2 = c->famcov_b2, b = std::sqrt(b2);
    for (int64_t h = 0; h < V; ++h) {
      ustat[h] *= b;
      vstat[h] *= b2;
    }
  }
  return RVT_OK;
}

// famLRT from resident rows: rvt_lrt_block_fam's loop from the rotated piece onward, behind the front stage.
int rvt_lrt_bed_dev_fam(rvt_ctx* c, const unsigned char* d_rows, int64_t V, int* ok, double* af, double* null_loglik,
                        double* alt_loglik, double* pvalue, long long* counts) {
  if (!c || !d_rows || V < 1 || !ok || !af || !null_loglik || !alt_loglik || !pvalue)
    return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = fam_bed_check(c, "rvt_lrt_bed_dev_fam", d_rows, V, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  FamBedPiece p;
  LrtWs w;
  rc = fam_bed_ws(c, st, &p);
  if (!rc) rc = lrt_prepare(c, st, &w);
  if (rc) return rc;
  for (int64_t v0 = 0; v0 < V; v0 += RVT_MAX_VARIANTS) {
    const int n = (int)std::min<int64_t>(RVT_MAX_VARIANTS, V - v0);
    rc = fam_bed_front(c, st, d_rows + (size_t)cb * (size_t)v0, cb, n, p, counts ? counts + 4 * v0 : nullptr);
    if (!rc) rc = lrt_piece(c, st, w, n, p.poly, ok + v0, af + v0, null_loglik + v0, alt_loglik + v0, pvalue + v0);
    if (rc) return rc;
  }
  return RVT_OK;
}

// FamSKAT / FamCMC / FamZeggini from resident rows: steps 1-2 of rvt_run_fam_tests formed from the 2-bit codes (the gene-side
// kernels of fam_bed_kernels.hip.h), then its tail.  Work spaces: counts and flags of every row, flip / fill values of the kept
// ones and the burden columns' sums and flags in d_fam_bed_ws; the kept rows' addresses, their site indices and the genes' ranges
// in d_fam_list; each is sized once per call, in front of its first write.
namespace {
struct FamGenesFront {        // what steps 1-2 leave for fam_tests_tail
  std::vector<int> Mk, off, kgene;
  size_t T = 0;
  const double* d_bcs = nullptr;
  const int* d_bpoly = nullptr;
};
}  // namespace

// The checks of a list call, all of them before any device work: the arguments, the state, the rows of EVERY gene (a refused
// call starts nothing); *cb = the rows' pitch.
static int fam_genes_bed_check(rvt_ctx* c, int n, const unsigned char* const* d_rows, const int* Ms, uint32_t tests,
                               rvt_gene_result* out, int64_t* cb) {
  if (!c || n < 0 || (n > 0 && (!d_rows || !Ms || !out))) return fail(c, RVT_E_INVALID, "bad batch arguments");
  if (!(tests & (RVT_TEST_FAMSKAT | RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)) ||
      (tests & ~(RVT_TEST_FAMSKAT | RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)))
    return fail(c, RVT_E_INVALID, "rvt_run_fam_tests_bed_dev takes the FAMSKAT / FAMCMC / FAMZEGGINI bits");
  for (int g = 0; g < n; ++g)
    if (!d_rows[g]) return fail(c, RVT_E_INVALID, "gene %d: null row address", g);
  if (int rc = fam_bed_check(c, "rvt_run_fam_tests_bed_dev", nullptr, 0, cb)) return rc;
  size_t tot = 0;
  for (int g = 0; g < n; ++g) {
    if (Ms[g] < 1 || Ms[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_TOO_LARGE, "gene %d: M=%d", g, Ms[g]);
    tot += (size_t)Ms[g];
  }
  if (tot > (size_t)INT32_MAX) return fail(c, RVT_E_TOO_LARGE, "%zu rows in one call", tot);
  for (int g = 0; g < n; ++g)
    if (int rc = fam_bed_check(c, "rvt_run_fam_tests_bed_dev", d_rows[g], Ms[g], cb)) return rc;
  return RVT_OK;
}

// steps 1-2 of a checked call: the records' initialisation and the front stage proper; *run = whether a tail is left to run
// (n > 0 and a kept row somewhere)
static int fam_genes_bed_front(rvt_ctx* c, int n, const unsigned char* const* d_rows, int64_t cb, const int* Ms, const int64_t* ids,
                               uint32_t tests, rvt_gene_result* out, FamGenesFront* F, bool* run) {
  *run = false;
  if (n == 0) return RVT_OK;
  size_t tot = 0;
  std::vector<size_t> row0(n);
  for (int g = 0; g < n; ++g) {
    row0[g] = tot;
    tot += (size_t)Ms[g];
  }
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  const bool burden = (tests & (RVT_TEST_FAMCMC | RVT_TEST_FAMZEGGINI)) != 0;
  // ---- 1. the site pass over the codes: counts, then flip / keep / no-missing flags of every row ---------------------------------
  Layout W, Lst;  // (sized by the rows of the batch: T <= tot kept rows, at most n genes with one)
  const size_t o_cnt = W.take(sizeof(unsigned long long) * 4 * tot), o_flags = W.take(sizeof(int) * tot),
               o_flip = W.take(sizeof(int) * tot), o_mu = W.take(sizeof(double) * tot), o_fq = W.take(sizeof(double) * tot),
               o_bcs = W.take(sizeof(double) * 2 * (size_t)n), o_bpoly = W.take(sizeof(int) * 2 * (size_t)n);
  const size_t o_rows = Lst.take(sizeof(unsigned char*) * tot), o_src = Lst.take(sizeof(int) * tot),
               o_koff = Lst.take(sizeof(int) * 2 * (size_t)n);
  HIP_TRY(c, c->d_fam_bed_ws.grow(W.total, W.total + W.total / 2, st, true));
  HIP_TRY(c, c->d_fam_list.grow(Lst.total, Lst.total + Lst.total / 2, st, true));
  char *ws = c->d_fam_bed_ws, *lst = c->d_fam_list;
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(ws + o_cnt);
  int *d_flags = reinterpret_cast<int*>(ws + o_flags), *d_flip = reinterpret_cast<int*>(ws + o_flip);
  double *d_mu = reinterpret_cast<double*>(ws + o_mu), *d_fq = reinterpret_cast<double*>(ws + o_fq);
  double* d_bcs = reinterpret_cast<double*>(ws + o_bcs);
  int* d_bpoly = reinterpret_cast<int*>(ws + o_bpoly);
  const unsigned char** d_krow = reinterpret_cast<const unsigned char**>(lst + o_rows);
  int *d_ksrc = reinterpret_cast<int*>(lst + o_src), *d_koff = reinterpret_cast<int*>(lst + o_koff);
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 4 * tot, st));
  for (int g = 0; g < n; ++g)  // (the rows of one gene are consecutive, the genes are not)
    bed_row_counts(st, d_rows[g], cb, N, Ms[g], d_cnt + 4 * row0[g]);
  hipLaunchKernelGGL(fam_bed_gene_site_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, d_cnt, (long long)tot,
                     d_flags);
  HIP_TRY(c, hipGetLastError());
  std::vector<int> flags(tot);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * tot, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  // ---- 2. the kept rows, flipped where flagged, rotated by U' -----------------------------------------------------------------
  std::vector<const unsigned char*> krow;
  std::vector<int> ksrc;
  std::vector<int>&Mk = F->Mk, &off = F->off, &kgene = F->kgene;
  Mk.assign(n, 0), off.assign(n, 0);
  bool any_missing = false;  // a kept row with a missing call (the block route's "not every kept column is a hard call")
  for (int g = 0; g < n; ++g) {
    off[g] = (int)krow.size();
    for (int j = 0; j < Ms[g]; ++j) {
      const size_t k = row0[g] + (size_t)j;
      if (!(flags[k] & 2)) continue;
      krow.push_back(d_rows[g] + (size_t)cb * (size_t)j);
      ksrc.push_back((int)k);
      any_missing = any_missing || !(flags[k] & 4);
    }
    Mk[g] = (int)krow.size() - off[g];
  }
  const size_t T = krow.size();
  for (int g = 0; g < n; ++g) {
    rvt_gene_result& r = out[g];
    std::memset(&r, 0, sizeof(r));
    r.gene_id = ids ? ids[g] : g;
    r.n_variants = Ms[g];
    r.n_poly = Mk[g];
  }
  if (T == 0) return RVT_OK;  // genotype.cols == 0 everywhere: all NA (src/Model.h:3066-3069)
  std::vector<int> kom;  // (kgene: the genes with a kept row) their first kept row, then their numbers of kept rows
  for (int g = 0; g < n; ++g)
    if (Mk[g] > 0) kgene.push_back(g);
  const size_t nk = kgene.size(), TB = burden ? 2 * nk : 0;
  kom.resize(2 * nk);
  for (size_t k = 0; k < nk; ++k) kom[k] = off[kgene[k]], kom[nk + k] = Mk[kgene[k]];
  HIP_TRY(c, hipMemcpyAsync(d_krow, krow.data(), sizeof(unsigned char*) * T, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_ksrc, ksrc.data(), sizeof(int) * T, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_koff, kom.data(), sizeof(int) * 2 * nk, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fam_bed_kept_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, d_cnt, d_ksrc, (long long)T, d_flip,
                     d_mu, d_fq);
  HIP_TRY(c, hipGetLastError());
  const bool dense = !c->d_fam_run && !(c->d_csc_ptr && !c->d_uq_range);
  // a dense piece with a missing call is the product [U'c' | U'm] (in d_Gp) of at most kRotMaxCols columns
  const size_t piece = dense && any_missing ? kRotMaxCols / 2 : kRotMaxCols;
  rc = ensure_fam_cols(c, std::max(T + TB, dense && any_missing ? 2 * std::min(T, piece) : (size_t)0), ld);
  if (rc) return rc;
  if (ld != N)  // pad rows must be zero (the rotation writes rows 0 .. N-1 of every column)
    HIP_TRY(c, hipMemset2DAsync(c->d_Gt + N, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)(ld - N), T + TB, st));
  if (c->d_fam_run) {  // the family form: the tile filled from the codes
    const size_t per = (size_t)65535 * kRotFamCols;  // (gridDim.y holds at most 65535 column tiles)
    for (size_t t0 = 0; t0 < T; t0 += per) {
      const int nc = (int)std::min(per, T - t0);
      hipLaunchKernelGGL(rot_fam_bed_kernel<BedRowList>, dim3((unsigned)c->fam_runs, (unsigned)((nc + kRotFamCols - 1) / kRotFamCols)),
                         dim3(kRotFamRows), 0, st, c->d_fam_run, c->d_fam_of, c->d_fam_ptr, c->d_fam_members, c->d_csc_ptr,
                         c->d_csc_vals, BedRowList{d_krow + t0, d_flip + t0}, d_mu + t0, nc, c->d_Gt + t0 * (size_t)ld,
                         (long long)ld);
      HIP_TRY(c, hipGetLastError());
    }
  } else if (!dense) {  // column-compressed U, scattered supports: the flipped fp64 columns on the device, then the gather
    for (size_t t0 = 0; t0 < T; t0 += 65535) {  // (gridDim.y holds at most 65535 columns)
      const unsigned nt = (unsigned)std::min<size_t>(65535, T - t0);
      hipLaunchKernelGGL(bed_expand_columns_kernel<BedRowList>, dim3((unsigned)((cb + 255) / 256), nt), dim3(256), 0, st,
                         BedRowList{d_krow + t0, d_flip + t0}, d_mu + t0, (long long)N, (long long)ld, c->d_Gp + t0 * (size_t)ld);
      HIP_TRY(c, hipGetLastError());
    }
    rc = rotate_columns(c, c->d_Gp, ld, (int)T, c->d_Gt, ld, st);
    if (rc) return rc;
  } else {  // dense U on digit planes: B = [c' | m], one plane each; without a missing call c' alone, straight into d_Gt
    const int64_t ldk = c->uq_ldk;
    for (size_t c0 = 0; c0 < T; c0 += piece) {
      const int ncp = (int)std::min(piece, T - c0), nB = any_missing ? 2 * ncp : ncp;
      const size_t need = (size_t)(((int64_t)nB + kRotBN - 1) / kRotBN * kRotBN) * (size_t)ldk;
      HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
      HIP_TRY(c, hipMemsetAsync(c->d_rotB, 0, need, st));
      hipLaunchKernelGGL(fam_bed_unpack_kernel<BedRowList>, dim3((unsigned)((cb + 255) / 256), (unsigned)ncp), dim3(256), 0, st,
                         BedRowList{d_krow + c0, d_flip + c0}, (long long)cb, (long long)N, ncp, any_missing ? 1 : 0,
                         c->d_rotB.get(), (long long)ldk);
      HIP_TRY(c, hipGetLastError());
      const std::vector<int> zero_exp((size_t)nB, 0);
      double* dst = c->d_Gt + c0 * (size_t)ld;
      double* C = any_missing ? c->d_Gp.get() : dst;
      rc = planes_gemm(c, c->d_Uq, c->uq_plane, kRotPlanesU, (int)N, nullptr, c->uq_sexp, c->d_rotB, need, 1, nB, zero_exp.data(),
                       N, ldk, C, ld, st, c->d_uq_range);
      if (rc) return rc;
      if (any_missing) {
        hipLaunchKernelGGL(fam_bed_combine_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)ncp), dim3(256), 0, st, C,
                           (long long)ld, (long long)N, ncp, d_fq + c0, dst, (long long)ld);
        HIP_TRY(c, hipGetLastError());
      }
    }
  }
  if (burden) {
    // cmcCollapse / zegginiCollapse from the codes into columns 0 .. 2 nk - 1 of d_Gp (the rotation above is done with it), their
    // raw sums and flags (the score test centres the collapsed genotype, FastLMM.cpp:218-220), rotated behind the T columns
    if (ld != N)
      HIP_TRY(c, hipMemset2DAsync(c->d_Gp + N, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)(ld - N), TB, st));
    for (size_t k0 = 0; k0 < nk; k0 += 65535) {  // (gridDim.y)
      const unsigned nkp = (unsigned)std::min<size_t>(65535, nk - k0);
      hipLaunchKernelGGL(fam_bed_collapse_kernel, dim3((unsigned)((cb + 255) / 256), nkp), dim3(256), 0, st, d_krow, d_flip, d_mu,
                         d_koff + k0, d_koff + nk + k0, (long long)cb, (long long)N, (long long)ld,
                         c->d_Gp + 2 * k0 * (size_t)ld);
    }
    hipLaunchKernelGGL(raw_colstat_kernel, dim3((unsigned)TB), dim3(256), 0, st, c->d_Gp.get(), (long long)N, (long long)ld,
                       d_bcs, d_bpoly);
    HIP_TRY(c, hipGetLastError());
    rc = rotate_columns(c, c->d_Gp, ld, (int)TB, c->d_Gt + T * (size_t)ld, ld, st);
    if (rc) return rc;
  }
  HIP_TRY(c, sync_stream(st));
  F->T = T, F->d_bcs = d_bcs, F->d_bpoly = d_bpoly;
  *run = true;
  return RVT_OK;
}

int rvt_run_fam_tests_bed_dev(rvt_ctx* c, int n, const unsigned char* const* d_rows, const int* Ms, const int64_t* ids,
                              uint32_t tests, rvt_gene_result* out) {
  FamGenesFront F;
  bool run = false;
  int64_t cb = 0;
  int rc = fam_genes_bed_check(c, n, d_rows, Ms, tests, out, &cb);
  if (!rc) rc = fam_genes_bed_front(c, n, d_rows, cb, Ms, ids, tests, out, &F, &run);
  if (rc || !run) return rc;
  return fam_tests_tail(c, n, tests, F.Mk, F.off, F.kgene, F.T, F.d_bcs, F.d_bpoly, out);
}

// Measurement hook: the front stage of rvt_run_fam_tests_bed_dev alone (site pass, lists, rotation, burden collapse and its
// rotation; the records are initialised, no test runs) between two HIP events — the events also enclose the copy of the flags to
// the host and the host's pass over them (cf. rvt_debug_rotate_bed_timed)
int rvt_debug_fam_genes_bed_front_timed(rvt_ctx* c, int n, const unsigned char* const* d_rows, const int* Ms, uint32_t tests,
                                        rvt_gene_result* out, double* ms) {
  if (!c || !ms) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = fam_genes_bed_check(c, n, d_rows, Ms, tests, out, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(c, hipEventCreate(&ev[0]));
  hipError_t e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) {
    FamGenesFront F;
    bool run = false;
    rc = fam_genes_bed_front(c, n, d_rows, cb, Ms, nullptr, tests, out, &F, &run);
    if (!rc) e = hipEventRecord(ev[1], st);
    if (!rc && e == hipSuccess) e = sync_stream(st);
    float t = 0.0f;
    if (!rc && e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    *ms = t;
  }
  hipEventDestroy(ev[0]);
  if (ev[1]) hipEventDestroy(ev[1]);
  if (rc) return rc;
  HIP_TRY(c, e);
  return RVT_OK;
}

namespace {
// the front stage of the first ncols rows, piece by piece; out (host, N x ncols, optional) takes the rotated columns
int fam_bed_rotate_all(rvt_ctx* c, hipStream_t st, const unsigned char* d_rows, int64_t cb, int ncols, double* out) {
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  FamBedPiece p;
  int rc = fam_bed_ws(c, st, &p);
  for (int v0 = 0; v0 < ncols && !rc; v0 += RVT_MAX_VARIANTS) {
    const int n = std::min(RVT_MAX_VARIANTS, ncols - v0);
    rc = fam_bed_front(c, st, d_rows + (size_t)cb * (size_t)v0, cb, n, p, nullptr);
    if (rc || !out) continue;
    HIP_TRY(c, hipMemcpy2DAsync(out + (size_t)N * v0, sizeof(double) * (size_t)N, c->d_Gt, sizeof(double) * (size_t)ld,
                                sizeof(double) * (size_t)N, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  return rc;
}
}  // namespace

// Test hook: the first ncols rows through the front stage, the rotated columns N x ncols to the host (cf. rvt_debug_rotate)
int rvt_debug_rotate_bed(rvt_ctx* c, const unsigned char* d_rows, int ncols, double* out) {
  if (!c || !d_rows || !out || ncols < 1) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = fam_bed_check(c, "rvt_debug_rotate_bed", d_rows, ncols, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  return fam_bed_rotate_all(c, c->stream, d_rows, cb, ncols, out);
}

// Measurement hook: the same front stage without the copy to the host, between two HIP events (cf. rvt_debug_rotate_timed)
int rvt_debug_rotate_bed_timed(rvt_ctx* c, const unsigned char* d_rows, int ncols, double* ms) {
  if (!c || !d_rows || !ms || ncols < 1) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = fam_bed_check(c, "rvt_debug_rotate_bed_timed", d_rows, ncols, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(c, hipEventCreate(&ev[0]));
  hipError_t e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) {
    rc = fam_bed_rotate_all(c, st, d_rows, cb, ncols, nullptr);
    if (!rc) e = hipEventRecord(ev[1], st);
    if (!rc && e == hipSuccess) e = sync_stream(st);
    float t = 0.0f;
    if (!rc && e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    *ms = t;
  }
  hipEventDestroy(ev[0]);
  if (ev[1]) hipEventDestroy(ev[1]);
  if (rc) return rc;
  HIP_TRY(c, e);
  return RVT_OK;
}

namespace {
struct GgLayout {
  size_t o_ty, o_wu1, o_xy, o_uxy, o_r, o_ur, o_upart, o_part, o_beta, o_ok, o_af, o_b, o_bv, o_pv, total;
};
GgLayout gg_layout(int64_t ld, int64_t N, int d) {
  GgLayout L;
  Layout lay;
  const int MV = RVT_MAX_VARIANTS;
  L.o_ty = lay.take(sizeof(double) * (size_t)ld);
  L.o_wu1 = lay.take(sizeof(double) * (size_t)ld);
  L.o_xy = lay.take(sizeof(double) * (size_t)N * (d + 1));
  L.o_uxy = lay.take(sizeof(double) * (size_t)N * (d + 1));
  L.o_r = lay.take(sizeof(double) * (size_t)ld);
  L.o_ur = lay.take(sizeof(double) * (size_t)ld);
  L.o_upart = lay.take(sizeof(double) * (size_t)kApplySlices * ld);
  L.o_part = lay.take(sizeof(double) * (size_t)kLmmBlocks * (d * d + d + 1));
  L.o_beta = lay.take(sizeof(double) * RVT_MAX_COV);
  L.o_ok = lay.take(sizeof(int) * MV);
  L.o_af = lay.take(sizeof(double) * MV);
  L.o_b = lay.take(sizeof(double) * MV);
  L.o_bv = lay.take(sizeof(double) * MV);
  L.o_pv = lay.take(sizeof(double) * MV);
  L.total = lay.total;
  return L;
}
}  // namespace

int rvt_fit_grammar_null(rvt_ctx* c, int64_t N, int d, const double* X, const double* y, rvt_grammar_null* out) {
  if (!c || !X || !y || !out || d < 1 || d > RVT_MAX_COV || N < 2) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_kin || c->kin_N != N) return fail(c, RVT_E_STATE, "rvt_set_kinship with the same N first");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  c->have_grammar = false;
  const int64_t ld = rvt_padded_ld(N);
  const GgLayout L = gg_layout(ld, N, d);
  HIP_TRY(c, c->d_gg_ws.grow(L.total, L.total, st, true));
  char* ws = c->d_gg_ws;
  double* d_ty = reinterpret_cast<double*>(ws + L.o_ty);
  double* d_wu1 = reinterpret_cast<double*>(ws + L.o_wu1);
  double* d_xy = reinterpret_cast<double*>(ws + L.o_xy);
  double* d_uxy = reinterpret_cast<double*>(ws + L.o_uxy);
  double* d_r = reinterpret_cast<double*>(ws + L.o_r);
  double* d_ur = reinterpret_cast<double*>(ws + L.o_ur);
  double* d_upart = reinterpret_cast<double*>(ws + L.o_upart);
  double* d_part = reinterpret_cast<double*>(ws + L.o_part);
  double* d_beta = reinterpret_cast<double*>(ws + L.o_beta);
  // ux = U'X, uy = U'y (GrammarGamma.cpp:38-40)
  HIP_TRY(c, hipMemcpyAsync(d_xy, X, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_xy + (size_t)N * d, y, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
  rc = rotate_columns(c, d_xy, N, d + 1, d_uxy, N, st);
  if (rc) return rc;
  double minS = c->h_S[0];
  for (int64_t i = 1; i < N; ++i) minS = std::min(minS, c->h_S[i]);
  const double n = (double)N;
  double sigma2_g = NAN;
  bool hip_failed = false;
  std::vector<double> sums;
  // getBetaSigma2 + getLogLikelihood (GrammarGamma.cpp:159-197): beta by the least squares weighted with (lambda + delta),
  // SSR with 1 / (lambda + delta), raw lambda; the objective takes log SSR (not log sigma2)
  auto evaluate = [&](double delta) -> double {
    if (minS + delta < 0.0) {  // sqrt(lambda + delta) of a negative number: NaN throughout
      sigma2_g = NAN;
      return NAN;
    }
    const int rec = d * d + d + 1;
    hipLaunchKernelGGL(grammar_sums_kernel, dim3(kLmmBlocks), dim3(kFsThreads), 0, st, d_uxy, c->d_S, (long long)N, d, delta,
                       0, d_beta, d_part);
    if (hipGetLastError() != hipSuccess || fs_records(c, d_part, rec, st, &sums)) {
      hip_failed = true;
      return NAN;
    }
    const double slog = sums[d * d + d];
    double Ai[RVT_MAX_COV * RVT_MAX_COV], beta[RVT_MAX_COV] = {};
    if (!invert_spd(sums.data(), d, Ai)) {
      sigma2_g = NAN;
      return NAN;
    }
    for (int a = 0; a < d; ++a)
      for (int k = 0; k < d; ++k) beta[a] += Ai[a * d + k] * sums[d * d + k];
    if (hipMemcpyAsync(d_beta, beta, sizeof(double) * d, hipMemcpyHostToDevice, st) != hipSuccess) hip_failed = true;
    hipLaunchKernelGGL(grammar_sums_kernel, dim3(kLmmBlocks), dim3(kFsThreads), 0, st, d_uxy, c->d_S, (long long)N, d, delta,
                       1, d_beta, d_part);
    if (hipGetLastError() != hipSuccess || fs_records(c, d_part, 1, st, &sums)) {
      hip_failed = true;
      return NAN;
    }
    const double ssr = sums[0];
    sigma2_g = ssr / n;
    return -0.5 * (n * std::log(2.0 * kRefPi) + slog + n + n * std::log(ssr));
  };
  int maxIndex = -1;
  double maxLL = 0.0;
  for (int i = 0; i <= 100; ++i) {
    const double ll = evaluate(std::exp(-10. + i * 0.2));
    if (std::isnan(ll)) continue;
    if (maxIndex < 0 || ll > maxLL) {
      maxIndex = i;
      maxLL = ll;
    }
  }
  if (hip_failed) return fail(c, RVT_E_HIP, "device evaluation of the GrammarGamma likelihood failed");
  if (maxIndex < 0) return fail(c, RVT_E_INVALID, "GrammarGamma: the likelihood is NaN at every grid point");
  // at a boundary maximum the reference leaves delta as it was (uninitialised on the first fit): here the grid point
  double delta = std::exp(-10. + maxIndex * 0.2);
  int evals = 0;
  if (maxIndex > 0 && maxIndex < 100) {
    const double lb = std::exp(-10. + (maxIndex - 1) * 0.2), ub = std::exp(-10. + (maxIndex + 1) * 0.2);
    const double start = delta;
    double xmin = start;
    auto goal = [&](double x) {
      ++evals;
      return -evaluate(x);
    };
    delta = brent_like_gsl(goal, start, lb, ub, &xmin) ? start : xmin;
    if (hip_failed) return fail(c, RVT_E_HIP, "device evaluation of the GrammarGamma likelihood failed");
  }  // sigma2_g stays that of the LAST evaluation (the last Brent call, or grid point 100)
  // gamma (GrammarGamma.cpp:100-102)
  double glam = 0.0;
  for (int64_t i = 0; i < N; ++i) glam += c->h_S[i] / (c->h_S[i] + delta);
  const double gamma = glam / sigma2_g / (n - 1.0);
  // resid = y - X (X'X)^-1 X'y in the original space (GrammarGamma.cpp:113-120)
  std::vector<double> resid((size_t)N);
  {
    double XtX[RVT_MAX_COV * RVT_MAX_COV], XtXi[RVT_MAX_COV * RVT_MAX_COV], Xty[RVT_MAX_COV] = {}, b[RVT_MAX_COV] = {};
    for (int a = 0; a < d; ++a) {
      for (int k = a; k < d; ++k) {
        double s = 0.0;
        for (int64_t i = 0; i < N; ++i) s += X[(size_t)a * N + i] * X[(size_t)k * N + i];
        XtX[a * d + k] = XtX[k * d + a] = s;
      }
      for (int64_t i = 0; i < N; ++i) Xty[a] += X[(size_t)a * N + i] * y[i];
    }
    if (!invert_spd(XtX, d, XtXi)) return fail(c, RVT_E_INVALID, "X'X is singular");
    for (int a = 0; a < d; ++a)
      for (int k = 0; k < d; ++k) b[a] += XtXi[a * d + k] * Xty[k];
    for (int64_t i = 0; i < N; ++i) {
      double p = 0.0;
      for (int a = 0; a < d; ++a) p += X[(size_t)a * N + i] * b[a];
      resid[i] = y[i] - p;
    }
  }
  // ty = U (lambda + delta)^-1 U' resid / sigma2_g (GrammarGamma.cpp:122-128); wu1 = (lambda + delta) u1 for af=kinship
  HIP_TRY(c, hipMemcpyAsync(d_r, resid.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
  rc = rotate_columns(c, d_r, ld, 1, d_ur, ld, st);
  if (rc) return rc;
  hipLaunchKernelGGL(grammar_scale_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_S, c->d_u1, (long long)N,
                     delta, 1.0 / sigma2_g, d_ur, d_wu1);
  HIP_TRY(c, hipGetLastError());
  rc = fs_apply_u(c, d_ur, d_ty, d_upart, ld, st);
  if (rc) return rc;
  std::vector<double> ty((size_t)N);
  HIP_TRY(c, hipMemcpyAsync(ty.data(), d_ty, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  double ysy = 0.0, sumty = 0.0, afden = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    ysy += resid[i] * ty[i];
    sumty += ty[i];
    afden += (c->h_S[i] + delta) * c->h_u1[i] * c->h_u1[i];
  }
  c->gg_N = N;
  c->gg_d = d;
  c->gg_delta = delta;
  c->gg_gamma = gamma;
  c->gg_ysy = ysy;
  c->gg_sumty = sumty;
  c->gg_afden = afden;
  c->have_grammar = true;
  ++c->gg_gen;  // (rvt_grammar_bed_dev forms the digit planes of ty once per fit)
  out->delta = delta;
  out->sigma2_g = sigma2_g;
  out->gamma = gamma;
  out->ySigmaY = ysy;
  out->max_index = maxIndex;
  out->brent_evals = evals;
  return RVT_OK;
}

int rvt_grammar_block(rvt_ctx* c, const double* dG, int V, int af_kinship, int* ok, double* af, double* beta,
                      double* beta_var, double* pvalue) {
  if (!c || !dG || V < 1 || !ok || !af || !beta || !beta_var || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_grammar) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_grammar_null first");
  if (!c->have_fam || c->fam_nc.N != c->gg_N)
    return fail(c, RVT_E_STATE, "rvt_fit_fam_null with the same samples first (it defines the block layout)");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->gg_N, ld = c->fam_nc.ld;
  const GgLayout L = gg_layout(rvt_padded_ld(N), N, c->gg_d);
  char* ws = c->d_gg_ws;
  const double* d_ty = reinterpret_cast<const double*>(ws + L.o_ty);
  const double* d_wu1 = reinterpret_cast<const double*>(ws + L.o_wu1);
  int* d_ok = reinterpret_cast<int*>(ws + L.o_ok);
  double* d_af = reinterpret_cast<double*>(ws + L.o_af);
  double* d_b = reinterpret_cast<double*>(ws + L.o_b);
  double* d_bv = reinterpret_cast<double*>(ws + L.o_bv);
  double* d_pv = reinterpret_cast<double*>(ws + L.o_pv);
  const int MV = RVT_MAX_VARIANTS;
  GgConsts k;
  k.n = (double)N;
  k.gamma = c->gg_gamma;
  k.ysy = c->gg_ysy;
  k.sumty = c->gg_sumty;
  k.afden = c->gg_afden;
  for (int c0 = 0; c0 < V; c0 += MV) {
    const int n = std::min(MV, V - c0);
    const double* g = dG + (size_t)c0 * ld;
    const double* gt = nullptr;
    if (af_kinship) {  // U'g for the kinship-weighted frequency (GrammarGamma.cpp:129-134, 199-213)
      rc = ensure_fam_cols(c, (size_t)n, ld);
      if (rc) return rc;
      HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * n, st));
      rc = rotate_columns(c, g, ld, n, c->d_Gt, ld, st);
      if (rc) return rc;
      gt = c->d_Gt;
    }
    if (af_kinship)
      hipLaunchKernelGGL(grammar_stream_kernel<true>, dim3((unsigned)n), dim3(kFsThreads), 0, st, g, (long long)ld, (long long)N,
                         n, d_ty, gt, d_wu1, k, d_ok, d_af, d_b, d_bv, d_pv);
    else
      hipLaunchKernelGGL(grammar_stream_kernel<false>, dim3((unsigned)n), dim3(kFsThreads), 0, st, g, (long long)ld, (long long)N,
                         n, d_ty, nullptr, nullptr, k, d_ok, d_af, d_b, d_bv, d_pv);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(ok + c0, d_ok, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(af + c0, d_af, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(beta + c0, d_b, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(beta_var + c0, d_bv, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(pvalue + c0, d_pv, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  return RVT_OK;
}

// ---- famGrammarGamma over rows of a resident .bed matrix (grammar_bed_kernels.hip.h, rvt_grammar_bed.h) ---------------------------
namespace {
constexpr int kGgBedPiece = 8192;  // rows of one launch of the product; af=kinship walks the front stage's RVT_MAX_VARIANTS

// what a call may be refused for, before anything is written; *cb = the pitch of its V rows at d_rows
int gg_bed_check(rvt_ctx* c, int af_kinship, const char* who, const unsigned char* d_rows, int64_t V, int64_t* cb) {
  if (!c->have_grammar) return fail(c, RVT_E_STATE, "%s: rvt_set_kinship + rvt_fit_grammar_null first", who);
  if (int rc = bed_rows_span(c, who, d_rows, V, BedModel::kGrammar, cb)) return rc;
  if (af_kinship && (!c->have_fam || c->fam_nc.N != c->gg_N))
    return fail(c, RVT_E_STATE, "%s: af=kinship needs rvt_fit_fam_null on the same samples (the rotation takes its layout)", who);
  if (c->gg_N > kGgMaxN) return fail(c, RVT_E_TOO_LARGE, "%s: N = %lld (at most %lld)", who, (long long)c->gg_N, (long long)kGgMaxN);
  return RVT_OK;
}

// The digit planes of ty, formed once per rvt_fit_grammar_null (gg_planes_gen) in a buffer of their own; a new block has lost
// them, and so has one that RVT_SCRIBBLE refills.  ty not finite: RVT_E_STATE.
int gg_bed_planes(rvt_ctx* c, hipStream_t st, const signed char** planes, int64_t* ldp_out) {
  const int64_t N = c->gg_N, ldp = (N + kGgKstep - 1) / kGgKstep * kGgKstep;
  Layout L;
  const size_t o_pl = L.take((size_t)kGgPlanes * (size_t)ldp), o_e = L.take(sizeof(int) * 2),
               o_t = L.take(sizeof(long long) * kGgPlanes);
  if (c->d_gg_planes.cap < L.total || getenv("RVT_SCRIBBLE")) c->gg_planes_gen = 0;
  HIP_TRY(c, c->d_gg_planes.grow(L.total, L.total, st, true));
  char* ws = c->d_gg_planes;
  if (c->gg_planes_gen != c->gg_gen) {
    const GgLayout G = gg_layout(rvt_padded_ld(N), N, c->gg_d);
    const double* d_ty = reinterpret_cast<const double*>(c->d_gg_ws.get() + G.o_ty);
    hipLaunchKernelGGL(grammar_ty_planes_kernel, dim3(1), dim3(1024), 0, st, d_ty, (long long)N,
                       reinterpret_cast<signed char*>(ws + o_pl), (long long)ldp, reinterpret_cast<int*>(ws + o_e),
                       reinterpret_cast<long long*>(ws + o_t));
    HIP_TRY(c, hipGetLastError());
    int eo[2] = {0, 0};
    long long tot[kGgPlanes] = {};
    HIP_TRY(c, hipMemcpyAsync(eo, ws + o_e, sizeof(eo), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    if (!eo[1]) return fail(c, RVT_E_STATE, "the GrammarGamma null model's ty is not finite");
    HIP_TRY(c, hipMemcpyAsync(tot, ws + o_t, sizeof(tot), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    c->gg_exp = eo[0];
    for (int p = 0; p < kGgPlanes; ++p) c->gg_totals[p] = tot[p];
    c->gg_planes_gen = c->gg_gen;
  }
  *planes = reinterpret_cast<const signed char*>(ws + o_pl);
  *ldp_out = ldp;
  return RVT_OK;
}

GgBedPlan gg_bed_plan_of(rvt_ctx* c, int n) {  // (the overrides are read at every call: the tests change them)
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) cus = 0;
  const char* es = getenv("RVT_GG_BED_SLICE");
  const char* et = getenv("RVT_GG_BED_TILES");
  return grammar_bed_plan(c->gg_N, n, cus, es ? atoll(es) : 0, et ? atoi(et) : 0);
}

struct GgBedOut {  // host arrays of a call (any may be null), V entries each (counts 4 V, sums 27 V)
  int* ok = nullptr;
  double *af = nullptr, *beta = nullptr, *beta_var = nullptr, *pvalue = nullptr;
  long long *counts = nullptr, *sums = nullptr;
  double* product_ms = nullptr;  // the product kernels alone between two events; nothing else runs
};

// The call proper, the state checked: pieces of rows through the product, the finish and, with af=kinship, the front stage.
int gg_bed_run(rvt_ctx* c, hipStream_t st, const unsigned char* d_rows, size_t cb, int64_t V, int af_kinship, const GgBedOut& out) {
  const int64_t N = c->gg_N;
  const signed char* planes = nullptr;
  int64_t ldp = 0;
  int rc = gg_bed_planes(c, st, &planes, &ldp);
  if (rc) return rc;
  const int piece = af_kinship ? RVT_MAX_VARIANTS : kGgBedPiece;
  const int nmax = (int)std::min<int64_t>(piece, V), nlast = (int)(V % piece);
  size_t part_ints = 0;
  for (int n : {nmax, nlast}) {
    if (n < 1) continue;
    const GgBedPlan P = gg_bed_plan_of(c, n);
    if (P.slices > 65535) return fail(c, RVT_E_INVALID, "RVT_GG_BED_SLICE: %d slices (at most 65535)", P.slices);
    part_ints = std::max(part_ints, (size_t)P.slices * (size_t)n * kGgPart);
  }
  // the work space, sized once per call in front of its first write
  Layout L;
  const size_t o_part = L.take(sizeof(int) * part_ints), o_ok = L.take(sizeof(int) * nmax), o_af = L.take(sizeof(double) * nmax),
               o_b = L.take(sizeof(double) * nmax), o_bv = L.take(sizeof(double) * nmax), o_pv = L.take(sizeof(double) * nmax),
               o_cnt = L.take(sizeof(long long) * 4 * nmax), o_sums = L.take(out.sums ? sizeof(long long) * kGgPart * nmax : 0);
  HIP_TRY(c, c->d_gg_bed_ws.grow(L.total, L.total, st, true));
  char* ws = c->d_gg_bed_ws;
  int* d_part = reinterpret_cast<int*>(ws + o_part);
  int* d_ok = reinterpret_cast<int*>(ws + o_ok);
  double* d_af = reinterpret_cast<double*>(ws + o_af);
  double* d_b = reinterpret_cast<double*>(ws + o_b);
  double* d_bv = reinterpret_cast<double*>(ws + o_bv);
  double* d_pv = reinterpret_cast<double*>(ws + o_pv);
  long long* d_cnt = reinterpret_cast<long long*>(ws + o_cnt);
  long long* d_sums = out.sums ? reinterpret_cast<long long*>(ws + o_sums) : nullptr;
  FamBedPiece fp;
  const double* d_wu1 = nullptr;
  if (af_kinship) {
    rc = fam_bed_ws(c, st, &fp);
    if (rc) return rc;
    const GgLayout G = gg_layout(rvt_padded_ld(N), N, c->gg_d);
    d_wu1 = reinterpret_cast<const double*>(c->d_gg_ws.get() + G.o_wu1);
  }
  GgBedConsts k;
  k.gamma = c->gg_gamma;
  k.ysy = c->gg_ysy;
  k.e = c->gg_exp;
  for (int p = 0; p < kGgPlanes; ++p) k.T[p] = c->gg_totals[p];
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (out.product_ms) {
    HIP_TRY(c, hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e != hipSuccess) {
      hipEventDestroy(ev[0]);
      if (ev[1]) hipEventDestroy(ev[1]);
      HIP_TRY(c, e);
    }
  }
  hipError_t herr = hipSuccess;
  std::vector<char> stage;
  for (int64_t v0 = 0; v0 < V && !rc && herr == hipSuccess; v0 += piece) {
    const int n = (int)std::min<int64_t>(piece, V - v0);
    const unsigned char* rows = d_rows + cb * (size_t)v0;
    const GgBedPlan P = gg_bed_plan_of(c, n);
    hipLaunchKernelGGL(grammar_bed_kernel, dim3((unsigned)P.groups, (unsigned)P.slices), dim3(kGgThreads),
                       (size_t)kGgCols * (size_t)P.slice, st, rows, (long long)cb, (long long)N, n, (long long)(cb * (size_t)n),
                       planes, (long long)ldp, P.npad, P.slice, P.tiles, d_part);
    herr = hipGetLastError();
    if (out.product_ms || herr != hipSuccess) continue;
    hipLaunchKernelGGL(grammar_bed_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_part, P.slices, n,
                       (long long)N, k, d_ok, d_af, d_b, d_bv, d_pv, d_cnt, d_sums);
    herr = hipGetLastError();
    if (herr != hipSuccess) break;
    if (af_kinship) {  // U'g of the piece by the installed form of U, then GetAF's AF_KINSHIP form over it
      rc = fam_bed_front(c, st, rows, (int64_t)cb, n, fp, nullptr);
      if (rc) break;
      hipLaunchKernelGGL(grammar_af_kin_kernel, dim3((unsigned)n), dim3(256), 0, st, c->d_Gt.get(), (long long)c->fam_nc.ld,
                         (long long)N, d_wu1, c->gg_afden, d_af);
      herr = hipGetLastError();
      if (herr != hipSuccess) break;
    }
    // one copy of the piece's outputs (they lie behind one another in the work space), handed out on the host
    const size_t o_end = out.sums ? o_sums + sizeof(long long) * kGgPart * n : out.counts ? o_cnt + sizeof(long long) * 4 * n
                                                                                          : o_pv + sizeof(double) * n;
    stage.resize(o_end - o_ok);
    herr = hipMemcpyAsync(stage.data(), ws + o_ok, stage.size(), hipMemcpyDeviceToHost, st);
    if (herr == hipSuccess) herr = sync_stream(st);  // (the next piece writes the same work space)
    if (herr != hipSuccess) break;
    auto back = [&](void* dst, size_t off, size_t bytes) {
      if (dst) std::memcpy(dst, stage.data() + (off - o_ok), bytes);
    };
    back(out.ok ? out.ok + v0 : nullptr, o_ok, sizeof(int) * n);
    back(out.af ? out.af + v0 : nullptr, o_af, sizeof(double) * n);
    back(out.beta ? out.beta + v0 : nullptr, o_b, sizeof(double) * n);
    back(out.beta_var ? out.beta_var + v0 : nullptr, o_bv, sizeof(double) * n);
    back(out.pvalue ? out.pvalue + v0 : nullptr, o_pv, sizeof(double) * n);
    back(out.counts ? out.counts + 4 * v0 : nullptr, o_cnt, sizeof(long long) * 4 * n);
    back(out.sums ? out.sums + (int64_t)kGgPart * v0 : nullptr, o_sums, sizeof(long long) * kGgPart * n);
  }
  if (out.product_ms) {
    float t = 0.0f;
    if (!rc && herr == hipSuccess) herr = hipEventRecord(ev[1], st);
    if (!rc && herr == hipSuccess) herr = sync_stream(st);
    if (!rc && herr == hipSuccess) herr = hipEventElapsedTime(&t, ev[0], ev[1]);
    *out.product_ms = t;
    hipEventDestroy(ev[0]);
    hipEventDestroy(ev[1]);
  }
  if (rc) return rc;
  HIP_TRY(c, herr);
  return RVT_OK;
}
}  // namespace

int rvt_grammar_bed_dev(rvt_ctx* c, const unsigned char* d_rows, int64_t V, int af_kinship, int* ok, double* af, double* beta,
                        double* beta_var, double* pvalue, long long* counts) {
  if (!c || !d_rows || V < 1 || !ok || !af || !beta || !beta_var || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = gg_bed_check(c, af_kinship, "rvt_grammar_bed_dev", d_rows, V, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  GgBedOut out;
  out.ok = ok, out.af = af, out.beta = beta, out.beta_var = beta_var, out.pvalue = pvalue, out.counts = counts;
  return gg_bed_run(c, c->stream, d_rows, (size_t)cb, V, af_kinship, out);
}

// Test hook: what rvt_grammar_bed_dev multiplies with and what the product returns.  planes (8 N, plane p at planes + p N, may be
// null), *exp2 and totals (8) describe ty; sums (V x 3 x 9, may be null): per row the int64 sums of H, L and HL against the eight
// planes and the ones column.
int rvt_debug_grammar_bed(rvt_ctx* c, const unsigned char* d_rows, int64_t V, signed char* planes, int* exp2, long long* totals,
                          long long* sums) {
  if (!c || !exp2 || !totals || (sums && (!d_rows || V < 1))) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;  // (without sums no row is read: the state alone)
  int rc = gg_bed_check(c, 0, "rvt_debug_grammar_bed", sums ? d_rows : nullptr, sums ? V : 0, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const signed char* d_planes = nullptr;
  int64_t ldp = 0;
  rc = gg_bed_planes(c, st, &d_planes, &ldp);
  if (rc) return rc;
  if (sums) {
    std::vector<int> ok((size_t)V);
    std::vector<double> v((size_t)V);
    GgBedOut out;
    out.ok = ok.data(), out.beta = out.beta_var = out.pvalue = v.data(), out.sums = sums;
    rc = gg_bed_run(c, st, d_rows, (size_t)cb, V, 0, out);
    if (rc) return rc;
  }
  if (planes) {
    HIP_TRY(c, hipMemcpy2DAsync(planes, (size_t)c->gg_N, d_planes, (size_t)ldp, (size_t)c->gg_N, kGgPlanes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  *exp2 = c->gg_exp;
  for (int p = 0; p < kGgPlanes; ++p) totals[p] = c->gg_totals[p];
  return RVT_OK;
}

// Measurement hook: the product kernels of rvt_grammar_bed_dev over the V rows alone, between two HIP events
int rvt_debug_grammar_bed_timed(rvt_ctx* c, const unsigned char* d_rows, int64_t V, double* ms) {
  if (!c || !d_rows || V < 1 || !ms) return fail(c, RVT_E_INVALID, "bad arguments");
  int64_t cb = 0;
  int rc = gg_bed_check(c, 0, "rvt_debug_grammar_bed_timed", d_rows, V, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  GgBedOut out;
  out.product_ms = ms;
  return gg_bed_run(c, c->stream, d_rows, (size_t)cb, V, 0, out);
}

}  // extern "C"

// ---- launchers of this unit's kernels for the other units (rvt_engine_int.h, "kernel families") -----------------------------
void k_lmm_sums(dim3 grid, hipStream_t st, const double* uxy, const double* lam, long long N, int d, double delta, int take_abs,
                double* partial) {
  hipLaunchKernelGGL(lmm_sums_kernel, grid, dim3(256), sizeof(double) * 256, st, uxy, lam, N, d, delta, take_abs, partial);
}
void k_fam_colstat(dim3 grid, hipStream_t st, const double* const* cols, long long N, int* flags) {
  hipLaunchKernelGGL(fam_colstat_kernel, grid, dim3(256), 0, st, cols, N, flags);
}
void k_fam_flip_compact(dim3 grid, hipStream_t st, const double* const* src_cols, const int* src_flip, long long N, long long ld,
                        double* dst) {
  hipLaunchKernelGGL(fam_flip_compact_kernel, grid, dim3(256), 0, st, src_cols, src_flip, N, ld, dst);
}
void k_raw_colstat(dim3 grid, hipStream_t st, const double* G, long long N, long long ld, double* colsum, int* poly) {
  hipLaunchKernelGGL(raw_colstat_kernel, grid, dim3(256), 0, st, G, N, ld, colsum, poly);
}
void k_rot_reduce_slices(hipStream_t st, const double* part, long long ldc, long long M, long long N, long long stride, int slices,
                         double* C, int accumulate) {
  hipLaunchKernelGGL(rot_reduce_slices_kernel, dim3(1024), dim3(256), 0, st, part, ldc, M, N, stride, slices, C, accumulate);
}
