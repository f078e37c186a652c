// rvtests_amd — the multiple-trait score test (`--single fastmtscore`): every variant of a block against T (phenotype,
// covariate list) tests, each with its own missing values (FastMultipleTraitScoreTest src/Model.h:4935-5125 on
// regression/FastMultipleTraitLinearRegressionScoreTest.cpp).  Part of librvtests_amd.so.
// A block of N x V genotypes against the traits is one tall-skinny product G'[Yc | Zc | indModel]: the centred traits and
// covariates stay resident as digit planes (the A operand of rot_gemm.hip.h), hard calls are one exact plane of B.
// this unit compiles (and ships) the multiple-trait kernels only: see "kernel families" in rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_MT
#include "rvt_engine_int.h"
#include "mtscore_kernels.hip.h"

static_assert(kMtMaxCov == RVT_MAX_COV - 1, "a test holds at most RVT_MAX_COV - 1 covariates");

namespace {
constexpr int kMtMaxRows = 1 << 15;  // resident rows: what one integer-plane product takes (kRotMaxCols, rvt_fam.hip)
constexpr int kMtPiece = 1024;       // variants per piece of a block

// lower Cholesky factor of the symmetric n x n matrix A (row-major) and A^-1 from it; false when A is not positive definite
bool mt_spd_inverse(const std::vector<double>& A, int n, std::vector<double>* inv) {
  std::vector<double> L((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[(size_t)i * n + j];
      if (!std::isfinite(s)) return false;
      for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        L[(size_t)i * n + i] = std::sqrt(s);
      } else {
        L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
      }
    }
  // W = L^-1 (lower), A^-1 = W' W
  std::vector<double> W((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    W[(size_t)j * n + j] = 1.0 / L[(size_t)j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= L[(size_t)i * n + k] * W[(size_t)k * n + j];
      W[(size_t)i * n + j] = s / L[(size_t)i * n + i];
    }
  }
  inv->assign((size_t)n * n, 0.0);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = 0.0;
      for (int k = a; k < n; ++k) s += W[(size_t)k * n + a] * W[(size_t)k * n + b];
      (*inv)[(size_t)a * n + b] = (*inv)[(size_t)b * n + a] = s;
    }
  return true;
}

uint64_t mt_hash(const signed char* p, size_t n) {  // FNV-1a: a bucket key only, patterns are compared by content
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
  return h;
}

void mt_reset(rvt_ctx* c) {
  c->have_mt = false;
  c->d_mt_planes.reset();
  c->d_mt_pat.reset();
  c->d_mt_B.reset();
  c->d_mt_rowsum.reset();
  c->d_mt_tests.reset();
  c->d_mt_ws.reset();
  c->mt_row_exp.clear();
  c->mt_N = c->mt_ld = c->mt_ldk = 0;
  c->mt_R = c->mt_K = c->mt_T = 0;
}
}  // namespace

extern "C" {

int rvt_mt_clear(rvt_ctx* c) {
  if (!c) return RVT_E_INVALID;
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  HIP_TRY(c, sync_stream(c->stream));
  mt_reset(c);
  return RVT_OK;
}

// FitNullModel (:233-377): observed indicators, centring, the per-test scales, zz_inv, zy and sigma2
int rvt_mt_fit_null(rvt_ctx* c, int64_t N, int P, const double* Y, int Q, const double* Z, int T, const int* test_pheno,
                    const int* test_cov_ptr, const int* test_cov, int* ok_out, double* obs_out, double* sigma2_out) {
  if (!c || N < 1 || P < 1 || !Y || Q < 0 || (Q > 0 && !Z) || T < 1 || !test_pheno || !test_cov_ptr)
    return fail(c, RVT_E_INVALID, "bad arguments");
  for (int t = 0; t < T; ++t) {
    const int nc = test_cov_ptr[t + 1] - test_cov_ptr[t];
    if (test_pheno[t] < 0 || test_pheno[t] >= P) return fail(c, RVT_E_INVALID, "test %d: phenotype index %d outside [0, %d)", t, test_pheno[t], P);
    if (nc < 0 || nc > kMtMaxCov) return fail(c, RVT_E_INVALID, "test %d: %d covariates (at most %d)", t, nc, kMtMaxCov);
    if (nc > 0 && !test_cov) return fail(c, RVT_E_INVALID, "bad arguments");
    for (int k = 0; k < nc; ++k) {
      const int z = test_cov[test_cov_ptr[t] + k];
      if (z < 0 || z >= Q) return fail(c, RVT_E_INVALID, "test %d: covariate index %d outside [0, %d)", t, z, Q);
    }
  }
  const int R = P + Q;
  if (R > kMtMaxRows) return fail(c, RVT_E_TOO_LARGE, "%d traits and covariates exceed the %d resident rows", R, kMtMaxRows);
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  HIP_TRY(c, sync_stream(st));
  mt_reset(c);  // replaces an earlier multiple-trait null
  const size_t n = (size_t)N;
  auto column = [&](int r) { return r < P ? Y + (size_t)r * n : Z + (size_t)(r - P) * n; };
  // ---- observed indicators of [Y | Z] and the distinct indModel patterns (createObsInd :78-88, indModel :336) ------------------
  std::vector<signed char> ind((size_t)R * n);
  std::vector<double> cnt((size_t)R, 0.0);
  for (int r = 0; r < R; ++r) {
    const double* s = column(r);
    signed char* o = ind.data() + (size_t)r * n;
    int64_t k = 0;
    for (size_t i = 0; i < n; ++i) {
      o[i] = s[i] == s[i] ? 1 : 0;
      k += o[i];
    }
    cnt[r] = (double)k;
  }
  std::vector<std::vector<signed char>> pats;
  std::vector<double> pat_obs;
  std::vector<int> test_pat((size_t)T);
  {
    std::unordered_map<uint64_t, std::vector<int>> buckets;
    std::map<std::vector<int>, int> by_formula;  // (y, sorted covariates): the same columns give the same pattern
    std::vector<signed char> cur(n);
    for (int t = 0; t < T; ++t) {
      std::vector<int> key;
      for (int k = test_cov_ptr[t]; k < test_cov_ptr[t + 1]; ++k) key.push_back(test_cov[k]);
      std::sort(key.begin(), key.end());
      key.erase(std::unique(key.begin(), key.end()), key.end());
      key.insert(key.begin(), -1 - test_pheno[t]);
      auto itf = by_formula.find(key);
      if (itf != by_formula.end()) {
        test_pat[t] = itf->second;
        continue;
      }
      std::memcpy(cur.data(), ind.data() + (size_t)test_pheno[t] * n, n);
      for (size_t k = 1; k < key.size(); ++k) {
        const signed char* z = ind.data() + (size_t)(P + key[k]) * n;
        for (size_t i = 0; i < n; ++i) cur[i] &= z[i];
      }
      const uint64_t h = mt_hash(cur.data(), n);
      int id = -1;
      for (int cand : buckets[h])
        if (std::memcmp(pats[(size_t)cand].data(), cur.data(), n) == 0) id = cand;
      if (id < 0) {
        id = (int)pats.size();
        int64_t k = 0;
        for (size_t i = 0; i < n; ++i) k += cur[i];
        pats.push_back(cur);
        pat_obs.push_back((double)k);
        buckets[h].push_back(id);
      }
      by_formula[key] = id;
      test_pat[t] = id;
    }
  }
  const int K = (int)pats.size();
  if (R + K > kMtMaxRows) return fail(c, RVT_E_TOO_LARGE, "%d resident rows (traits, covariates and %d patterns) exceed %d", R + K, K, kMtMaxRows);
  // ---- resident planes -------------------------------------------------------------------------------------------------------------
  const int64_t ldk = (N + kRotKC - 1) / kRotKC * kRotKC;
  const int64_t rows_pad = ((int64_t)R + kRotBM - 1) / kRotBM * kRotBM + kRotBM;  // (+ a panel: a product may start at row P)
  const int64_t pat_pad = ((int64_t)K + kRotBM - 1) / kRotBM * kRotBM;
  const size_t plane = (size_t)rows_pad * (size_t)ldk;
  HIP_TRY(c, c->d_mt_planes.alloc(plane * kMtPlanes));
  HIP_TRY(c, hipMemsetAsync(c->d_mt_planes, 0, plane * kMtPlanes, st));
  HIP_TRY(c, c->d_mt_pat.alloc((size_t)pat_pad * (size_t)ldk));
  HIP_TRY(c, hipMemsetAsync(c->d_mt_pat, 0, (size_t)pat_pad * (size_t)ldk, st));
  HIP_TRY(c, sync_stream(st));
  for (int k = 0; k < K; ++k)
    HIP_TRY(c, hipMemcpy(c->d_mt_pat + (size_t)k * (size_t)ldk, pats[(size_t)k].data(), n, hipMemcpyHostToDevice));
  pats.clear();
  pats.shrink_to_fit();
  // ---- counts, means, centring and digits, a chunk of columns at a time ----------------------------------------------------------
  std::vector<int> row_exp((size_t)R, 0);
  std::vector<double> rowsum((size_t)R, 0.0), sumsq((size_t)R, 0.0);
  {
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(R, ((int64_t)512 << 20) / (int64_t)(sizeof(double) * n)));
    DevBuf<double> d_src, d_stat, d_sumsq;
    DevBuf<int> d_sexp;
    DevBuf<long long> d_rowq;
    HIP_TRY(c, d_src.alloc(sizeof(double) * n * (size_t)chunk));
    HIP_TRY(c, d_stat.alloc(sizeof(double) * 4 * (size_t)chunk));
    HIP_TRY(c, d_sumsq.alloc(sizeof(double) * (size_t)chunk));
    HIP_TRY(c, d_sexp.alloc(sizeof(int) * (size_t)chunk));
    HIP_TRY(c, d_rowq.alloc(sizeof(long long) * (size_t)chunk));
    std::vector<double> stat((size_t)chunk * 4), ssq((size_t)chunk);
    std::vector<int> sexp((size_t)chunk);
    std::vector<long long> rowq((size_t)chunk);
    for (int r0 = 0; r0 < R; r0 += chunk) {
      const int nc = std::min(chunk, R - r0);
      for (int j = 0; j < nc; ++j)  // (Y and Z are two arrays: column by column)
        HIP_TRY(c, hipMemcpyAsync(d_src + (size_t)j * n, column(r0 + j), sizeof(double) * n, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(mt_colstat_kernel, dim3((unsigned)nc), dim3(256), 0, st, d_src.get(), (long long)N, d_stat.get());
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(stat.data(), d_stat, sizeof(double) * 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      for (int j = 0; j < nc; ++j) {
        const double mx = stat[(size_t)4 * j + 2];
        if (!std::isfinite(mx)) return fail(c, RVT_E_INVALID, "non-finite value in column %d of [Y | Z]", r0 + j);
        sexp[j] = mx == 0.0 ? 0 : 7 * kMtPlanes - 3 - std::ilogb(mx);  // |x| 2^sexp < 2^40 (as quantize_columns, rvt_fam.hip)
        row_exp[(size_t)(r0 + j)] = sexp[j];
      }
      HIP_TRY(c, hipMemcpyAsync(d_sexp, sexp.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(mt_quantize_rows_kernel, dim3((unsigned)nc), dim3(256), 0, st, d_src.get(), (long long)N, d_stat.get(),
                         d_sexp.get(), r0, c->d_mt_planes.get(), (long long)ldk, (long long)plane, d_rowq.get(), d_sumsq.get());
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(rowq.data(), d_rowq, sizeof(long long) * (size_t)nc, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(ssq.data(), d_sumsq, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      for (int j = 0; j < nc; ++j) {
        rowsum[(size_t)(r0 + j)] = std::ldexp((double)rowq[j], -sexp[j]);
        sumsq[(size_t)(r0 + j)] = ssq[j];
      }
    }
  }
  HIP_TRY(c, c->d_mt_rowsum.alloc(sizeof(double) * (size_t)R));
  HIP_TRY(c, hipMemcpy(c->d_mt_rowsum, rowsum.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice));
  // ---- Zc'[Yc | Zc] and indZ'[indY | indZ]: exact integer products of the stored digits (:313, :337, :352-353) ---------------------
  std::vector<double> cz, ci;  // Q x R, column-major: entry (a, r) at a + r Q
  if (Q > 0) {
    DevBuf<signed char> d_ind;
    DevBuf<double> d_c;
    HIP_TRY(c, d_ind.alloc((size_t)rows_pad * (size_t)ldk));
    HIP_TRY(c, hipMemset(d_ind, 0, (size_t)rows_pad * (size_t)ldk));
    HIP_TRY(c, hipMemcpy2D(d_ind, (size_t)ldk, ind.data(), n, n, (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(c, d_c.alloc(sizeof(double) * (size_t)Q * (size_t)R));
    cz.resize((size_t)Q * R);
    ci.resize((size_t)Q * R);
    rc = rvt_planes_gemm(c, c->d_mt_planes + (size_t)P * (size_t)ldk, plane, kMtPlanes, Q, row_exp.data() + P, 0, c->d_mt_planes,
                         plane, kMtPlanes, R, row_exp.data(), N, ldk, d_c, Q, st);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(cz.data(), d_c, sizeof(double) * cz.size(), hipMemcpyDeviceToHost));
    std::vector<int> zero_exp((size_t)R, 0);
    rc = rvt_planes_gemm(c, d_ind + (size_t)P * (size_t)ldk, 0, 1, Q, zero_exp.data(), 0, d_ind, 0, 1, R, zero_exp.data(), N, ldk, d_c,
                         Q, st);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(ci.data(), d_c, sizeof(double) * ci.size(), hipMemcpyDeviceToHost));
  }
  ind.clear();
  ind.shrink_to_fit();
  // ---- the constants of every test (:332-368), fp64 on the host -----------------------------------------------------------------------
  std::vector<MtTest> tests((size_t)T);
  for (int t = 0; t < T; ++t) {
    MtTest& m = tests[(size_t)t];
    std::memset(&m, 0, sizeof(m));
    const int y = test_pheno[t], C = test_cov_ptr[t + 1] - test_cov_ptr[t];
    const int* zl = C > 0 ? test_cov + test_cov_ptr[t] : nullptr;
    m.y = y;
    m.ncov = C;
    m.pattern = test_pat[(size_t)t];
    for (int a = 0; a < C; ++a) m.z[a] = P + zl[a];
    const double OBS = pat_obs[(size_t)m.pattern];
    m.obs = OBS;
    bool ok = OBS > 0.0 && cnt[(size_t)y] > 0.0;
    for (int a = 0; a < C; ++a) ok = ok && cnt[(size_t)(P + zl[a])] > 0.0;
    double sigma2 = NAN;
    if (ok) {
      m.scale_xy = OBS / cnt[(size_t)y];
      m.scale_xx = OBS / (double)N;
      for (int a = 0; a < C; ++a) m.scale_xz[a] = OBS / cnt[(size_t)(P + zl[a])];
      sigma2 = sumsq[(size_t)y] * OBS / cnt[(size_t)y];
      if (C > 0) {
        std::vector<double> A((size_t)C * C), inv;
        for (int a = 0; a < C; ++a)
          for (int b = 0; b < C; ++b)
            A[(size_t)a * C + b] = cz[(size_t)zl[a] + (size_t)(P + zl[b]) * Q] * OBS / ci[(size_t)zl[a] + (size_t)(P + zl[b]) * Q];
        ok = mt_spd_inverse(A, C, &inv);
        for (int a = 0; a < C && ok; ++a) {
          m.zy[a] = cz[(size_t)zl[a] + (size_t)y * Q] * OBS / ci[(size_t)zl[a] + (size_t)y * Q];
          ok = std::isfinite(m.zy[a]);
        }
        if (ok) {
          double q = 0.0;
          for (int a = 0; a < C; ++a)
            for (int b = 0; b < C; ++b) {
              m.zz_inv[a * C + b] = inv[(size_t)a * C + b];
              q += m.zy[a] * inv[(size_t)a * C + b] * m.zy[b];
            }
          sigma2 -= q;
        }
      }
      sigma2 /= OBS;
    }
    m.ok = ok ? 1 : 0;
    m.sigma2 = ok ? sigma2 : NAN;
    if (ok_out) ok_out[t] = m.ok;
    if (obs_out) obs_out[t] = OBS;
    if (sigma2_out) sigma2_out[t] = m.sigma2;
  }
  HIP_TRY(c, c->d_mt_tests.alloc(sizeof(MtTest) * (size_t)T));
  HIP_TRY(c, hipMemcpy(c->d_mt_tests, tests.data(), sizeof(MtTest) * (size_t)T, hipMemcpyHostToDevice));
  c->mt_row_exp = std::move(row_exp);
  c->mt_N = N;
  c->mt_ld = rvt_padded_ld(N);
  c->mt_ldk = ldk;
  c->mt_plane = plane;
  c->mt_R = R;
  c->mt_K = K;
  c->mt_T = T;
  c->have_mt = true;
  return RVT_OK;
}

// TestCovariateBlock (:391-470) of the V columns of a device block, V x T row-major outputs
int rvt_mt_score_block(rvt_ctx* c, const double* dG, int V, double* ustat, double* vstat, double* pvalue) {
  if (!c || !dG || V < 1 || !ustat || !vstat || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_mt) return fail(c, RVT_E_STATE, "no multiple-trait null model (rvt_mt_fit_null)");
  // the layout rvt_block_alloc gave the block
  const int64_t N = c->mt_N, ld = block_dims(c).ld;
  if ((c->have_null && c->nc.N != N) || (!c->have_null && c->have_fam && c->fam_nc.N != N))
    return fail(c, RVT_E_STATE, "the multiple-trait null and the context's null model differ in N");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t ldk = c->mt_ldk;
  const int R = c->mt_R, K = c->mt_K, T = c->mt_T;
  const int Vp = kMtPiece;  // (the work space of a whole piece: a piece of dosages is multiplied at that width, see below)
  const int64_t vpad = kMtPiece;
  Layout L;
  const size_t o_isum = L.take(sizeof(unsigned long long) * 2 * (size_t)Vp), o_bad = L.take(sizeof(int)),
               o_gsum = L.take(sizeof(double) * (size_t)Vp), o_gg = L.take(sizeof(double) * (size_t)Vp),
               o_c1 = L.take(sizeof(double) * (size_t)R * (size_t)Vp), o_c2 = L.take(sizeof(double) * (size_t)K * (size_t)Vp),
               o_u = L.take(sizeof(double) * (size_t)Vp * (size_t)T), o_v = L.take(sizeof(double) * (size_t)Vp * (size_t)T),
               o_p = L.take(sizeof(double) * (size_t)Vp * (size_t)T);
  HIP_TRY(c, c->d_mt_ws.grow(L.total, L.total, st, true));
  HIP_TRY(c, c->d_mt_B.grow((size_t)vpad * (size_t)ldk, (size_t)vpad * (size_t)ldk, st, true));
  char* ws = c->d_mt_ws;
  unsigned long long* d_isum = reinterpret_cast<unsigned long long*>(ws + o_isum);
  int* d_bad = reinterpret_cast<int*>(ws + o_bad);
  double* d_gsum = reinterpret_cast<double*>(ws + o_gsum);
  double* d_gg = reinterpret_cast<double*>(ws + o_gg);
  double* d_c1 = reinterpret_cast<double*>(ws + o_c1);
  double* d_c2 = reinterpret_cast<double*>(ws + o_c2);
  double* d_u = reinterpret_cast<double*>(ws + o_u);
  double* d_v = reinterpret_cast<double*>(ws + o_v);
  double* d_p = reinterpret_cast<double*>(ws + o_p);
  std::vector<int> zero_exp((size_t)std::max(K, Vp), 0), col_exp;
  static_assert(kMtPiece % kRotBN == 0, "a piece is whole column tiles");
  c->mt_ms[0] = c->mt_ms[1] = c->mt_ms[2] = 0.0;
  for (int v0 = 0; v0 < V; v0 += kMtPiece) {
    const int nv = std::min(kMtPiece, V - v0);
    const int64_t nvpad = ((int64_t)nv + kRotBN - 1) / kRotBN * kRotBN;
    const double* Gp = dG + (size_t)v0 * (size_t)ld;
    // ---- genotype pass: value test, int8 copy, exact sums (nothing is assumed or remembered about the block's content) --------------
    double t0 = now_s();
    HIP_TRY(c, hipMemsetAsync(d_isum, 0, sizeof(unsigned long long) * 2 * (size_t)nv, st));
    HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(int), st));
    if (nvpad > nv)  // the product reads whole column tiles: the pass writes nv columns of ldk bytes
      HIP_TRY(c, hipMemsetAsync(c->d_mt_B + (size_t)nv * (size_t)ldk, 0, (size_t)(nvpad - nv) * (size_t)ldk, st));
    hipLaunchKernelGGL(mt_geno_pass_kernel, dim3((unsigned)nv, (unsigned)((ldk + kMtPassRows - 1) / kMtPassRows)), dim3(256), 0, st, Gp,
                       (long long)N, (long long)ld, c->d_mt_B.get(), (long long)ldk, d_isum, d_bad);
    HIP_TRY(c, hipGetLastError());
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    const signed char* B = c->d_mt_B;
    size_t b_stride = 0;
    int PB = 1;
    const int* cexp = zero_exp.data();
    int nb = nv;  // columns the products run over
    if (!bad) {
      hipLaunchKernelGGL(mt_int_moments_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, d_isum, nv, (double)N, d_gsum, d_gg);
    } else {  // dosages, mean-imputed columns: kRotPlanesG digits per column (quantize_columns) and fp64 column moments
      // Products of two six-digit operands are rounded when the plane pairs and the K slices are added, and the slices follow
      // the number of column tiles: such a piece is multiplied at the full piece width (zero columns behind nv), so that a
      // column's bits do not depend on where in a block it lies.  (Hard-call pieces are exact sums: any width gives the same.)
      signed char* qd = nullptr;
      col_exp.assign((size_t)kMtPiece, 0);
      nb = kMtPiece;
      rc = quantize_columns_mt(c, Gp, N, ld, nv, kMtPiece, ldk, st, &qd, &b_stride, &PB, col_exp.data());
      if (rc) return rc;
      B = qd;
      cexp = col_exp.data();
      hipLaunchKernelGGL(mt_col_moments_kernel, dim3((unsigned)nv), dim3(256), 0, st, Gp, (long long)N, (long long)ld, d_gsum, d_gg);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));
    double t1 = now_s();
    c->mt_ms[0] += 1e3 * (t1 - t0);
    // ---- GYZ = [Yc | Zc]'G (six planes of A) and nm = indModel'G (one plane): two groups of launches -------------------------------
    rc = rvt_planes_gemm(c, c->d_mt_planes, c->mt_plane, kMtPlanes, R, c->mt_row_exp.data(), 0, B, b_stride, PB, nb, cexp, N, ldk, d_c1,
                         R, st);
    if (rc) return rc;
    rc = rvt_planes_gemm(c, c->d_mt_pat, 0, 1, K, zero_exp.data(), 0, B, b_stride, PB, nb, cexp, N, ldk, d_c2, K, st);
    if (rc) return rc;
    double t2 = now_s();
    c->mt_ms[1] += 1e3 * (t2 - t1);
    // ---- u, v, p of every cell -------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL((mt_finish_kernel<false>), dim3((unsigned)((T + kMtFinTests - 1) / kMtFinTests), (unsigned)((nv + kMtFinVars - 1) / kMtFinVars)),
                       dim3(256), 0, st, d_c1, (long long)R, d_c2, (long long)K, c->d_mt_rowsum.get(), d_gsum, d_gg,
                       reinterpret_cast<const MtTest*>(c->d_mt_tests.get()), T, nv, (double)N, d_u, d_v, d_p);
    HIP_TRY(c, hipGetLastError());
    const size_t cells = (size_t)nv * (size_t)T, off = (size_t)v0 * (size_t)T;
    HIP_TRY(c, hipMemcpyAsync(ustat + off, d_u, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(vstat + off, d_v, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(pvalue + off, d_p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    c->mt_ms[2] += 1e3 * (now_s() - t2);
  }
  return RVT_OK;
}

// TestCovariateBlock (:391-470) of V consecutive rows of a resident .bed matrix: rvt_mt_score_block's loop with the front stage
// over the 2-bit codes in place of the pass over fp64 columns (mtscore_kernels.hip.h, second half).  The imputed column is
// g = c + mu m, so a piece costs the block route's hard-call products of c — launched in that route's shape: one plane, the
// piece's own width — and, for the rows that have a missing call, the same two products of the compact m.
int rvt_mt_score_bed_dev(rvt_ctx* c, const unsigned char* d_rows, int64_t V, double* ustat, double* vstat, double* pvalue,
                         long long* counts) {
  if (!c || !d_rows || V < 1 || !ustat || !vstat || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_mt) return fail(c, RVT_E_STATE, "no multiple-trait null model (rvt_mt_fit_null)");
  const int64_t N = c->mt_N;
  int64_t pitch = 0;
  int rc = bed_rows_span(c, "rvt_mt_score_bed_dev", d_rows, V, BedModel::kMt, &pitch);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t ldk = c->mt_ldk;
  const int R = c->mt_R, K = c->mt_K, T = c->mt_T;
  const int Vp = kMtPiece;
  Layout L;
  const size_t o_cnt = L.take(sizeof(unsigned long long) * 4 * (size_t)Vp), o_mu = L.take(sizeof(double) * (size_t)Vp),
               o_gg = L.take(sizeof(double) * (size_t)Vp), o_slot = L.take(sizeof(int) * (size_t)Vp),
               o_idx = L.take(sizeof(int) * (size_t)Vp), o_c1 = L.take(sizeof(double) * (size_t)R * (size_t)Vp),
               o_c2 = L.take(sizeof(double) * (size_t)K * (size_t)Vp), o_c1m = L.take(sizeof(double) * (size_t)R * (size_t)Vp),
               o_c2m = L.take(sizeof(double) * (size_t)K * (size_t)Vp), o_u = L.take(sizeof(double) * (size_t)Vp * (size_t)T),
               o_v = L.take(sizeof(double) * (size_t)Vp * (size_t)T), o_p = L.take(sizeof(double) * (size_t)Vp * (size_t)T);
  // B = [c | m]: a piece of c columns, behind them as many m columns as a piece can have
  const size_t b_half = (size_t)kMtPiece * (size_t)ldk;
  HIP_TRY(c, c->d_mt_ws.grow(L.total, L.total, st, true));
  HIP_TRY(c, c->d_mt_B.grow(2 * b_half, 2 * b_half, st, true));
  char* ws = c->d_mt_ws;
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(ws + o_cnt);
  double* d_mu = reinterpret_cast<double*>(ws + o_mu);
  double* d_gg = reinterpret_cast<double*>(ws + o_gg);
  int* d_slot = reinterpret_cast<int*>(ws + o_slot);
  int* d_idx = reinterpret_cast<int*>(ws + o_idx);
  double* d_c1 = reinterpret_cast<double*>(ws + o_c1);
  double* d_c2 = reinterpret_cast<double*>(ws + o_c2);
  double* d_c1m = reinterpret_cast<double*>(ws + o_c1m);
  double* d_c2m = reinterpret_cast<double*>(ws + o_c2m);
  double* d_u = reinterpret_cast<double*>(ws + o_u);
  double* d_v = reinterpret_cast<double*>(ws + o_v);
  double* d_p = reinterpret_cast<double*>(ws + o_p);
  signed char* Bc = c->d_mt_B;
  signed char* Bm = c->d_mt_B + b_half;
  const std::vector<int> zero_exp((size_t)std::max(K, Vp), 0);
  std::vector<unsigned long long> cnt;
  std::vector<int> slot((size_t)Vp), idx((size_t)Vp);
  c->mt_ms[0] = c->mt_ms[1] = c->mt_ms[2] = 0.0;
  for (int64_t v0 = 0; v0 < V; v0 += kMtPiece) {
    const int nv = (int)std::min<int64_t>(kMtPiece, V - v0);
    const int64_t nvpad = ((int64_t)nv + kRotBN - 1) / kRotBN * kRotBN;
    const unsigned char* rows = d_rows + (size_t)v0 * (size_t)pitch;
    // ---- front stage: the counts of every row, its moments, the list of the rows with a missing call, c and the compact m --------
    double t0 = now_s();
    rc = bed_piece_counts(c, st, rows, pitch, N, nv, d_cnt, nullptr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(mt_bed_site_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, d_cnt, nv, d_mu, d_gg);
    HIP_TRY(c, hipGetLastError());
    rc = bed_counts_host(c, st, d_cnt, nv, &cnt, counts ? counts + 4 * (size_t)v0 : nullptr);
    if (rc) return rc;
    int nm = 0;  // rows of the piece with a missing call
    for (int h = 0; h < nv; ++h) {
      const bool miss = cnt[4 * (size_t)h + 3] != 0;
      slot[(size_t)h] = miss ? nm : -1;
      if (miss) idx[(size_t)nm++] = h;
    }
    const int64_t nmpad = ((int64_t)nm + kRotBN - 1) / kRotBN * kRotBN;
    HIP_TRY(c, hipMemcpyAsync(d_slot, slot.data(), sizeof(int) * (size_t)nv, hipMemcpyHostToDevice, st));
    if (nm > 0) HIP_TRY(c, hipMemcpyAsync(d_idx, idx.data(), sizeof(int) * (size_t)nm, hipMemcpyHostToDevice, st));
    if (nvpad > nv)  // the products read whole column tiles: the kernel writes nv (nm) columns of ldk bytes
      HIP_TRY(c, hipMemsetAsync(Bc + (size_t)nv * (size_t)ldk, 0, (size_t)(nvpad - nv) * (size_t)ldk, st));
    if (nmpad > nm) HIP_TRY(c, hipMemsetAsync(Bm + (size_t)nm * (size_t)ldk, 0, (size_t)(nmpad - nm) * (size_t)ldk, st));
    hipLaunchKernelGGL(mt_bed_unpack_kernel, dim3((unsigned)nv, (unsigned)((ldk + kMtPassRows - 1) / kMtPassRows)), dim3(256), 0, st,
                       rows, (long long)pitch, (long long)N, (long long)nv * (long long)pitch, d_slot, Bc, Bm, (long long)ldk);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_stream(st));  // (slot and idx are refilled for the next piece)
    double t1 = now_s();
    c->mt_ms[0] += 1e3 * (t1 - t0);
    // ---- [Yc | Zc]'c and indModel'c as a hard-call piece of rvt_mt_score_block, then the same of m and C = Cc + mu Cm ---------------
    rc = rvt_planes_gemm(c, c->d_mt_planes, c->mt_plane, kMtPlanes, R, c->mt_row_exp.data(), 0, Bc, 0, 1, nv, zero_exp.data(), N, ldk,
                         d_c1, R, st);
    if (rc) return rc;
    rc = rvt_planes_gemm(c, c->d_mt_pat, 0, 1, K, zero_exp.data(), 0, Bc, 0, 1, nv, zero_exp.data(), N, ldk, d_c2, K, st);
    if (rc) return rc;
    if (nm > 0) {
      rc = rvt_planes_gemm(c, c->d_mt_planes, c->mt_plane, kMtPlanes, R, c->mt_row_exp.data(), 0, Bm, 0, 1, nm, zero_exp.data(), N, ldk,
                           d_c1m, R, st);
      if (rc) return rc;
      rc = rvt_planes_gemm(c, c->d_mt_pat, 0, 1, K, zero_exp.data(), 0, Bm, 0, 1, nm, zero_exp.data(), N, ldk, d_c2m, K, st);
      if (rc) return rc;
      hipLaunchKernelGGL(mt_bed_combine_kernel, dim3((unsigned)((R + K + 255) / 256), (unsigned)nm), dim3(256), 0, st, d_c1, d_c1m,
                         (long long)R, R, d_c2, d_c2m, (long long)K, K, d_idx, d_mu);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, sync_stream(st));
    }
    double t2 = now_s();
    c->mt_ms[1] += 1e3 * (t2 - t1);
    // ---- u, v, p of every cell (gbar = mu) --------------------------------------------------------------------------------------------
    hipLaunchKernelGGL((mt_finish_kernel<true>), dim3((unsigned)((T + kMtFinTests - 1) / kMtFinTests), (unsigned)((nv + kMtFinVars - 1) / kMtFinVars)),
                       dim3(256), 0, st, d_c1, (long long)R, d_c2, (long long)K, c->d_mt_rowsum.get(), d_mu, d_gg,
                       reinterpret_cast<const MtTest*>(c->d_mt_tests.get()), T, nv, (double)N, d_u, d_v, d_p);
    HIP_TRY(c, hipGetLastError());
    const size_t cells = (size_t)nv * (size_t)T, off = (size_t)v0 * (size_t)T;
    HIP_TRY(c, hipMemcpyAsync(ustat + off, d_u, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(vstat + off, d_v, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(pvalue + off, d_p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    c->mt_ms[2] += 1e3 * (now_s() - t2);
  }
  return RVT_OK;
}

// Measurement (tools/bench_mtscore.py, tools/bench_mtscore_bed.py): host milliseconds the last rvt_mt_score_block or
// rvt_mt_score_bed_dev spent in its three phases — the genotype pass (front stage), the products (with the combine), the
// finishing kernel with its copies (every phase ends with a wait for the stream).
int rvt_mt_last_timing(rvt_ctx* c, double* ms3) {
  if (!c || !ms3) return RVT_E_INVALID;
  for (int k = 0; k < 3; ++k) ms3[k] = c->mt_ms[k];
  return RVT_OK;
}

}  // extern "C"
