// rvtests_amd — the SKAT permutation test (--kernel skat[nPerm=..]): the exact replay of the reference's rand() stream and the
// counter-based shuffles (perm_kernels.hip.h, perm_counter.h).  Part of librvtests_amd.so.
// this unit compiles (and ships) the PERM kernel family only: see "kernel families" in rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_PERM
#include "rvt_engine_int.h"

extern "C" {

// ---- SKAT permutations (exact replay of the reference's rand() stream) ------------------------------------------
namespace {
void mat31_mul(const uint32_t* A, const uint32_t* B, uint32_t* C) {  // C = A B over Z/2^32
  uint32_t T[31 * 31];
  for (int i = 0; i < 31; ++i)
    for (int j = 0; j < 31; ++j) {
      uint32_t s = 0;
      for (int k = 0; k < 31; ++k) s += A[i * 31 + k] * B[k * 31 + j];
      T[i * 31 + j] = s;
    }
  std::memcpy(C, T, sizeof(T));
}
// J = A^e, A the one-draw transition x' = (x[1..30], x[0] + x[28])
void jump_matrix(uint64_t e, uint32_t* J) {
  uint32_t P[31 * 31] = {0}, R[31 * 31] = {0};
  for (int t = 0; t < 30; ++t) P[t * 31 + t + 1] = 1;
  P[30 * 31 + 0] = 1;
  P[30 * 31 + 28] = 1;
  for (int t = 0; t < 31; ++t) R[t * 31 + t] = 1;
  while (e) {
    if (e & 1) mat31_mul(R, P, R);
    mat31_mul(P, P, P);
    e >>= 1;
  }
  std::memcpy(J, R, sizeof(R));
}
void mat31_apply(const uint32_t* J, const uint32_t* x, uint32_t* y) {
  uint32_t t[31];
  for (int i = 0; i < 31; ++i) {
    uint32_t s = 0;
    for (int k = 0; k < 31; ++k) s += J[i * 31 + k] * x[k];
    t[i] = s;
  }
  std::memcpy(y, t, sizeof(t));
}

// the chunk buffers of both permutation stages, freed together before either grows them (perm_cap_B: the shuffles they hold)
static void free_perm(rvt_ctx* c) {
  for (DevBuf<uint32_t>* b : {&c->d_perm_idx, &c->d_perm_states}) b->reset();
  for (DevBuf<double>* b : {&c->d_perm_R, &c->d_perm_C, &c->d_perm_Q, &c->d_perm_cur}) b->reset();
  c->perm_cap_B = 0;
}

// Shuffles per chunk of the exact mode: the chunk's permuted vectors (N x B doubles) stay under 6 GB
static int exact_chunk(int nPerm, int64_t N) {
  return std::max(1, std::min(nPerm, (int)std::min<int64_t>(2048, ((int64_t)6 << 30) / (8 * N))));
}

// rvt_debug_perm_trace: the statistics a SKAT permutation stage hands to the stop rule, in order, into the caller's array
struct PermTrace {
  double* stats = nullptr;
  int cap = 0;
  int* n_written = nullptr;
  void add(int actual, double q) const {  // after ++actual
    if (stats && actual <= cap) stats[actual - 1] = q;
  }
  void done(int actual) const {
    if (n_written) *n_written = std::min(actual, cap);
  }
};
static PermTrace take_perm_trace(rvt_ctx* c) {  // (and disarm: one gene per arming)
  PermTrace t;
  t.stats = c->perm_trace_stats, t.cap = c->perm_trace_cap, t.n_written = c->perm_trace_n;
  c->perm_trace_stats = nullptr, c->perm_trace_cap = 0, c->perm_trace_n = nullptr;
  return t;
}

// The exact-mode permutation test shared by the SKAT and the variable-threshold stage: cumulative Fisher-Yates shuffles of
// the vector d_start (N doubles on the device) on the emulated rand() stream, a chunk of B = exact_chunk() at a time.
// stat(nb, B, &d_out) launches, on the context's stream, what turns the chunk's permuted vectors (columns of d_perm_R,
// N x nb) into its nb statistics and names the device array that holds them; they are compared with obs under
// Permutation's stop rule (src/Permutation.h:69-98).  m: columns of d_perm_C that the caller's statistic needs (0: none).
// On return the stream stands behind the shuffles PERFORMED, whatever the chunk generated beyond them.
// failed_ (optional, Madsen-Browning's loop, src/Model.h:1286-1299): a statistic below zero is a failed TestCovariate — the
// shuffle is drawn but not added; the eleventh ends the test with *failed_ = 11.
// trace (optional): rvt_debug_perm_trace's record of the statistics added.
extern "C++" {  // (this unit's functions sit inside extern "C"; a template cannot)
template <class Stat>
int exact_permutations(rvt_ctx* c, const double* d_start, int nPerm, double alpha, double obs, int m, Stat&& stat, int* actual_,
                       int* numX_, int* numEq_, int* failed_ = nullptr, const PermTrace* trace = nullptr) {
  const int64_t N = c->nc.N;
  hipStream_t st = c->stream;
  // chunk buffers
  const int B = exact_chunk(nPerm, N);
  if (sizeof(uint32_t) * N * B > c->d_perm_idx.cap || B > c->perm_cap_B || sizeof(double) * N * B > c->d_perm_R.cap ||
      sizeof(double) * B * m > c->d_perm_C.cap ||
      sizeof(double) * N * 2 > c->d_perm_cur.cap) {  // (d_perm_cur holds 2 N doubles whatever B is: fewer shuffles of more samples must not keep it)
    free_perm(c);
    const size_t bm = (size_t)B * std::max(m, RVT_MAX_VARIANTS / 4);
    HIP_TRY(c, c->d_perm_idx.alloc(sizeof(uint32_t) * (size_t)N * B));
    HIP_TRY(c, c->d_perm_states.alloc(sizeof(uint32_t) * 31 * (size_t)B));
    HIP_TRY(c, c->d_perm_R.alloc(sizeof(double) * (size_t)N * B));
    HIP_TRY(c, c->d_perm_C.alloc(sizeof(double) * bm));
    HIP_TRY(c, c->d_perm_Q.alloc(sizeof(double) * (size_t)B));
    HIP_TRY(c, c->d_perm_cur.alloc(sizeof(double) * (size_t)N * 2));
    c->perm_cap_B = B;
  }
  if (c->jump_N != N) {
    c->jump.resize(31 * 31);
    jump_matrix((uint64_t)(N - 1), c->jump.data());  // one shuffle draws N-1 numbers (LinearAlgebra.h:12-14)
    c->jump_N = N;
  }
  // the chunk buffers are work spaces of this call (perm_apply_kernel, the caller's statistic and the copy below write what is
  // read); the index arrays and generator states are rewritten per chunk too, but count as state of the generation
  HIP_TRY(c, c->d_perm_R.scribble(st, "d_perm_R"));
  HIP_TRY(c, c->d_perm_C.scribble(st, "d_perm_C"));
  HIP_TRY(c, c->d_perm_Q.scribble(st, "d_perm_Q"));
  HIP_TRY(c, c->d_perm_cur.scribble(st, "d_perm_cur"));
  double* cur = c->d_perm_cur;
  double* nxt = c->d_perm_cur + N;
  HIP_TRY(c, hipMemcpyAsync(cur, d_start, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
  // Permutation::init — `threshold` is an INT member of the reference's class (src/Permutation.h:153): the product is truncated
  // (nPerm = 100, alpha = 0.001 -> 0: the test stops before its first shuffle and reports p = 1; found by running the
  // reference's compiled class beside this rule, tests/test_oracle_ref.py)
  const double threshold = (double)(int)(1.0 * nPerm * alpha * 2);
  int actual = 0, numX = 0, numEq = 0;
  uint32_t s0[31];
  std::memcpy(s0, c->rand_state, sizeof(s0));
  std::vector<uint32_t> states((size_t)31 * (B + 1));
  std::vector<double> Q(B);
  bool more = true;
  while (more) {
    // Permutation::next() before every shuffle
    if (actual >= nPerm || numX + numEq >= threshold) break;
    const int nb = std::min(B, nPerm - actual);
    std::memcpy(states.data(), s0, sizeof(s0));
    for (int p = 0; p < nb; ++p) mat31_apply(c->jump.data(), &states[(size_t)31 * p], &states[(size_t)31 * (p + 1)]);
    HIP_TRY(c, hipMemcpyAsync(c->d_perm_states, states.data(), sizeof(uint32_t) * 31 * (size_t)nb,
                              hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(perm_init_kernel, dim3(2048), dim3(256), 0, st, c->d_perm_idx, (long long)N, B);
    hipLaunchKernelGGL(perm_fisher_yates_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st,
                       c->d_perm_states, c->d_perm_idx, (long long)N, B);
    for (int p = 0; p < nb; ++p) {  // the shuffles are cumulative: apply them in order
      hipLaunchKernelGGL(perm_apply_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_perm_idx, cur,
                         nxt, c->d_perm_R, (long long)N, B, p);
      std::swap(cur, nxt);
    }
    const double* d_out = nullptr;
    const int rcs = stat(nb, B, &d_out);
    if (rcs) return rcs;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Q.data(), d_out, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    int used = 0;
    for (; used < nb; ++used) {
      if (actual >= nPerm || numX + numEq >= threshold) {
        more = false;
        break;
      }
      if (failed_ && Q[used] < 0) {
        if (*failed_ < 10) {
          ++*failed_;
          continue;
        }
        *failed_ = 11;
        ++used;  // (this shuffle was drawn too)
        more = false;
        break;
      }
      ++actual;  // Permutation::add
      if (trace) trace->add(actual, Q[used]);
      if (Q[used] > obs) ++numX;
      if (Q[used] == obs) ++numEq;
    }
    std::memcpy(s0, &states[(size_t)31 * used], sizeof(s0));  // the stream continues after the shuffles performed
    if (used < nb) {
      // the vector of the next gene restarts from its own start anyway; nothing else carries over
      more = false;
    }
  }
  std::memcpy(c->rand_state, s0, sizeof(s0));
  if (trace) trace->done(actual);
  *actual_ = actual, *numX_ = numX, *numEq_ = numEq;
  return RVT_OK;
}
}  // extern "C++"

// The permutation test of one gene whose analytic SKAT result (obs = skat_Q) and weights are already on the device.
//   dG: the gene's block (unflipped), g0: its descriptor of the batch that just finished (weights in its scratch)
int perm_stage(rvt_ctx* c, const double* dG, int M, const GeneDesc& g0, const rvt_params& prm, rvt_gene_result* r) {
  const int64_t N = c->nc.N, ld = c->nc.ld;
  const int nPerm = prm.skat_nperm;
  hipStream_t st = c->stream;
  const PermTrace trace = take_perm_trace(c);
  // flipped, polymorphic genotype block (K_sqrt = diag(w^1/2) G', Skat.cpp:42-47)
  std::vector<const double*> cols(M);
  for (int j = 0; j < M; ++j) cols[j] = dG + (size_t)j * ld;
  DevBuf<const double*> d_cols;
  DevBuf<int> d_flags;
  HIP_TRY(c, d_cols.alloc(sizeof(double*) * (size_t)M * 2));
  HIP_TRY(c, d_flags.alloc(sizeof(int) * (size_t)M * 2));
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * M, hipMemcpyHostToDevice, st));
  k_fam_colstat(dim3((unsigned)M), st, d_cols, (long long)N, d_flags);
  std::vector<int> flags(M);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  std::vector<const double*> kc;
  std::vector<int> kf;
  for (int j = 0; j < M; ++j)
    if (flags[j] & 2) {
      kc.push_back(cols[j]);
      kf.push_back(flags[j] & 1);
    }
  const int m = (int)kc.size();
  if (m != r->n_poly) return fail(c, RVT_E_STATE, "permutation stage: %d polymorphic columns, batch reported %d", m, r->n_poly);
  int rc = ensure_fam_cols(c, (size_t)m, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_cols + M, kc.data(), sizeof(double*) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags + M, kf.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
  k_fam_flip_compact(dim3(64, (unsigned)m), st, d_cols + M, d_flags + M, (long long)N, (long long)ld, c->d_Gp);
  const double* d_bw = gene_scratch_carve(g0.scratch, g0.Mp, g0.Cp).bw;  // sqrt of the SKAT weights, filtered order
  if (!c->perm_exact) {
    // ---- counter-based permutations (perm_counter.h): no stream shared between genes, nothing stored per shuffle ----------
    constexpr int kChunk = 2048;
    const int Mp = (m + 15) / 16 * 16;
    const long long ngroups = (N + 15) / 16;
    HIP_TRY(c, c->d_pc_Q.grow(sizeof(double) * kChunk, sizeof(double) * kChunk, st, true));
    const double obs = r->skat_Q;
    // Permutation::init — `threshold` is an INT member of the reference's class (src/Permutation.h:153): the product is truncated
    // (nPerm = 100, alpha = 0.001 -> 0: the test stops before its first shuffle and reports p = 1; found by running the
    // reference's compiled class beside this rule, tests/test_oracle_ref.py)
    const double threshold = (double)(int)(1.0 * nPerm * prm.skat_alpha * 2);
    int actual = 0, numX = 0, numEq = 0;
    std::vector<double> Q(kChunk);
    bool more = true;
    while (more) {
      if (actual >= nPerm || numX + numEq >= threshold) break;  // Permutation::next() before every shuffle
      // the first chunk is short: a gene far from significance stops after ~2 threshold shuffles
      const int want = actual == 0 ? std::min<int>(kChunk, (int)std::max(64.0, 2.5 * threshold)) : kChunk;
      const int nb = std::min(want, nPerm - actual);
      const int n_bt = (nb + 63) / 64;
      // ~4096 waves per launch; a slice holds at least 64 groups of 16 samples
      int slices = (int)std::max<long long>(1, std::min<long long>(4096 / n_bt, (ngroups + 63) / 64));
      const int gps = (int)((ngroups + slices - 1) / slices);
      slices = (int)((ngroups + gps - 1) / gps);
      const size_t need = (size_t)slices * nb * Mp;
      HIP_TRY(c, c->d_pc_part.grow(sizeof(double) * need, sizeof(double) * (need + need / 4), st, true));
      hipLaunchKernelGGL(perm_counter_partial_kernel, dim3((unsigned)slices, (unsigned)n_bt), dim3(64), 0, st, c->d_Gp,
                         (long long)ld, (long long)N, m, c->d_res, (unsigned long long)c->perm_seed,
                         (unsigned long long)r->gene_id, (unsigned)actual, nb, gps, Mp, c->d_pc_part);
      hipLaunchKernelGGL(perm_counter_q_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, c->d_pc_part, slices,
                         nb, Mp, m, d_bw, c->d_pc_Q);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(Q.data(), c->d_pc_Q, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      for (int u = 0; u < nb; ++u) {
        if (actual >= nPerm || numX + numEq >= threshold) {
          more = false;
          break;
        }
        ++actual;  // Permutation::add
        trace.add(actual, Q[u]);
        if (Q[u] > obs) ++numX;
        if (Q[u] == obs) ++numEq;
      }
    }
    trace.done(actual);
    r->perm_ok = 1;
    r->perm_num_perm = nPerm;
    r->perm_actual_perm = actual;
    r->perm_num_greater = numX;
    r->perm_num_equal = numEq;
    r->perm_pvalue = actual == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEq) / actual;
    return RVT_OK;
  }
  // permutedRes = res (src/Model.h:2708)
  int actual = 0, numX = 0, numEq = 0;
  rc = exact_permutations(
      c, c->d_res, nPerm, prm.skat_alpha, r->skat_Q, m,
      [&](int nb, int B, const double** d_out) -> int {
        if (N <= 2048) {  // few samples: sums in sample order, so that exact ties with the observed Q resolve as in the reference
          hipLaunchKernelGGL(perm_dot_sequential_kernel, dim3((unsigned)(((long long)nb * m + 255) / 256)), dim3(256), 0, st,
                             c->d_perm_R, c->d_Gp, (long long)N, (long long)ld, nb, m, B, c->d_perm_C);
        } else {  // C (nb x m) = Rp' G with Rp = the chunk's permuted residuals as columns (N x nb): integer-plane product
          int rcg = gemm_tn_planes(c, c->d_perm_R, N, nb, c->d_Gp, ld, m, N, c->d_perm_C, B, st);
          if (rcg) return rcg;
        }
        hipLaunchKernelGGL(perm_q_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, c->d_perm_C, d_bw, B, m,
                           c->d_perm_Q);
        *d_out = c->d_perm_Q;
        return RVT_OK;
      },
      &actual, &numX, &numEq, nullptr, &trace);
  if (rc) return rc;
  r->perm_ok = 1;
  r->perm_num_perm = nPerm;
  r->perm_actual_perm = actual;
  r->perm_num_greater = numX;
  r->perm_num_equal = numEq;
  r->perm_pvalue = actual == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEq) / actual;
  return RVT_OK;
}

// KBAC (KBACTest::fit, src/Model.h:2925-2998 over regression/kbac.cpp) of one gene.  y: the 0 / 1 phenotype (host).
int kbac_stage(rvt_ctx* c, const double* dG, int M, const double* af, const std::vector<unsigned char>& y, int nPerm,
               double alpha, rvt_kbac_result* r) {
  std::memset(r, 0, sizeof(*r));
  r->pvalue = 9.0;
  const int64_t N = c->nc.N, ld = c->nc.ld;
  hipStream_t st = c->stream;
  // ---- flipped, polymorphic block (dc->getFlippedToMinorPolymorphicGenotype()) ---------------------------------------
  std::vector<const double*> cols(M);
  for (int j = 0; j < M; ++j) cols[j] = dG + (size_t)j * ld;
  DevBuf<const double*> d_cols;
  DevBuf<int> d_flags;
  DevBuf<double> d_id;
  DevBuf<int> d_carrier;
  DevBuf<unsigned char> d_y, d_sub;
  HIP_TRY(c, d_cols.alloc(sizeof(double*) * (size_t)M * 2));
  HIP_TRY(c, d_flags.alloc(sizeof(int) * (size_t)M * 3));
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * M, hipMemcpyHostToDevice, st));
  k_fam_colstat(dim3((unsigned)M), st, d_cols, (long long)N, d_flags);
  std::vector<int> flags(M);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  std::vector<const double*> kc;
  std::vector<int> kf;
  for (int j = 0; j < M; ++j)
    if (flags[j] & 2) {
      kc.push_back(cols[j]);
      kf.push_back(flags[j] & 1);
    }
  const int m = (int)kc.size();
  r->n_poly = m;
  if (m == 0) {  // genotype.cols == 0: xdat is empty, KbacTest's constructor would reject it; rvtests prints what it got
    r->fit_ok = 0;
    return RVT_OK;
  }
  int rc = ensure_fam_cols(c, (size_t)m, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_cols + M, kc.data(), sizeof(double*) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags + M, kf.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
  k_fam_flip_compact(dim3(64, (unsigned)m), st, d_cols + M, d_flags + M, (long long)N, (long long)ld, c->d_Gp);
  // ---- m_trimXdat: columns with 0 < maf <= 1 (maf of filtered position j = counter of unfiltered column j) --------------
  std::vector<int> use;
  for (int j = 0; j < m; ++j)
    if (!(af[j] <= 0.0 || af[j] > 1.0)) use.push_back(j);
  const int n_used = (int)use.size();
  std::vector<double> id((size_t)N, 0.0);
  if (n_used > 0) {
    std::vector<double> p3((size_t)n_used + 1);
    for (int k = 0; k <= n_used; ++k) p3[k] = std::pow(3.0, 1.0 * k);  // the host's pow, as the reference evaluates it
    double* d_p3 = nullptr;
    HIP_TRY(c, d_id.alloc(sizeof(double) * ((size_t)N + p3.size())));
    d_p3 = d_id + N;
    HIP_TRY(c, hipMemcpyAsync(d_p3, p3.data(), sizeof(double) * p3.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_flags + 2 * M, use.data(), sizeof(int) * n_used, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kbac_pattern_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_Gp, (long long)N,
                       (long long)ld, d_flags + 2 * M, n_used, d_p3, d_id);
    HIP_TRY(c, hipMemcpyAsync(id.data(), d_id, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  // ---- unique patterns (ascending), their counts, the carriers --------------------------------------------------------
  std::vector<double> pat;
  for (int64_t i = 0; i < N; ++i)
    if (id[i] != 0.0) pat.push_back(id[i]);
  if (pat.empty()) {  // "non-wildtype genotype data is empty ... Return p-value 1.0"
    r->fit_ok = 1;
    r->pvalue = 1.0;
    return RVT_OK;
  }
  std::sort(pat.begin(), pat.end());
  pat.erase(std::unique(pat.begin(), pat.end()), pat.end());
  const int P = (int)pat.size();
  std::vector<int> carrier, cpat;
  std::vector<unsigned> cnt(P, 0);
  for (int64_t i = 0; i < N; ++i)
    if (id[i] != 0.0) {
      const int u = (int)(std::lower_bound(pat.begin(), pat.end(), id[i]) - pat.begin());
      carrier.push_back((int)i);
      cpat.push_back(u);
      ++cnt[u];
    }
  const int nc_ = (int)carrier.size();
  r->n_pattern = P;
  r->n_carrier = nc_;
  unsigned nCases = 0;
  for (int64_t i = 0; i < N; ++i) nCases += y[i] == 1;
  const unsigned nCtrls = (unsigned)N - nCases;
  // kernel weights for every possible case count of every pattern
  static const Hypergeometric hyper;
  std::vector<std::vector<double>> W(P);
  for (int u = 0; u < P; ++u) {
    W[u].resize(cnt[u] + 1);
    for (unsigned k = 0; k <= cnt[u]; ++k) W[u][k] = hyper.cdf(k, cnt[u], (unsigned)N - cnt[u], nCases);
  }
  std::vector<unsigned> sub(P);
  auto statistic = [&](const unsigned char* yc) {  // yc: phenotype of the carriers, in carrier order
    std::fill(sub.begin(), sub.end(), 0u);
    for (int q = 0; q < nc_; ++q) sub[cpat[q]] += yc[q] == 1;
    double kbac = 0.0;
    for (int u = 0; u < P; ++u)
      kbac = kbac + ((1.0 * sub[u]) / (1.0 * nCases) - (1.0 * (cnt[u] - sub[u])) / (1.0 * nCtrls)) * W[u][sub[u]];
    return kbac;
  };
  std::vector<unsigned char> yc(nc_);
  for (int q = 0; q < nc_; ++q) yc[q] = y[carrier[q]];
  const double observed = statistic(yc.data());
  r->stat = observed;
  // ---- permutations: cumulative std::random_shuffle of the phenotype, chunks of B shuffles -------------------------------
  const unsigned adaptive = alpha >= 1.0 ? 0u : 5000u;
  const int total = nPerm + 1;  // the loop shuffles once more after the last statistic (kbac.cpp:185,323-324)
  const int B = std::max(1, std::min(total, (int)std::min<int64_t>(2048, ((int64_t)6 << 30) / (4 * N))));
  if (sizeof(uint32_t) * N * B > c->d_perm_idx.cap || B > c->perm_cap_B) {
    free_perm(c);
    HIP_TRY(c, c->d_perm_idx.alloc(sizeof(uint32_t) * (size_t)N * B));
    HIP_TRY(c, c->d_perm_states.alloc(sizeof(uint32_t) * 31 * (size_t)B));
    c->perm_cap_B = B;
  }
  if (c->jump_N != N) {
    c->jump.resize(31 * 31);
    jump_matrix((uint64_t)(N - 1), c->jump.data());  // one shuffle draws N-1 numbers
    c->jump_N = N;
  }
  HIP_TRY(c, d_y.alloc((size_t)N * 2));
  HIP_TRY(c, d_sub.alloc((size_t)B * nc_));
  HIP_TRY(c, d_carrier.alloc(sizeof(int) * (size_t)nc_));
  HIP_TRY(c, hipMemcpyAsync(d_carrier, carrier.data(), sizeof(int) * (size_t)nc_, hipMemcpyHostToDevice, st));
  unsigned char *cur = d_y, *nxt = d_y + N;
  HIP_TRY(c, hipMemcpyAsync(cur, y.data(), (size_t)N, hipMemcpyHostToDevice, st));
  uint32_t s0[31];
  std::memcpy(s0, c->rand_state, sizeof(s0));
  std::vector<uint32_t> states((size_t)31 * (B + 1));
  std::vector<unsigned char> ysub((size_t)B * nc_);
  unsigned pc1 = 0, pc2 = 0;
  int done = 0;  // shuffles performed = statistics evaluated after the observed one
  bool stop = false;
  while (!stop && done < nPerm) {
    const int nb = std::min(B, nPerm - done);
    std::memcpy(states.data(), s0, sizeof(s0));
    for (int p = 0; p < nb; ++p) mat31_apply(c->jump.data(), &states[(size_t)31 * p], &states[(size_t)31 * (p + 1)]);
    HIP_TRY(c, hipMemcpyAsync(c->d_perm_states, states.data(), sizeof(uint32_t) * 31 * (size_t)nb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(perm_init_kernel, dim3(2048), dim3(256), 0, st, c->d_perm_idx, (long long)N, B);
    hipLaunchKernelGGL(perm_random_shuffle_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, c->d_perm_states,
                       c->d_perm_idx, (long long)N, B);
    for (int p = 0; p < nb; ++p) {  // the shuffles are cumulative: apply them in order, keep the carriers' phenotype
      hipLaunchKernelGGL(perm_apply_u8_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_perm_idx, cur, nxt,
                         (long long)N, B, p);
      hipLaunchKernelGGL(perm_gather_u8_kernel, dim3((unsigned)((nc_ + 255) / 256)), dim3(256), 0, st, nxt, d_carrier, nc_,
                         d_sub + (size_t)p * nc_);
      std::swap(cur, nxt);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(ysub.data(), d_sub, (size_t)nb * nc_, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    int used = 0;
    for (; used < nb; ++used) {
      const double s = statistic(&ysub[(size_t)used * nc_]);
      ++done;
      if (s >= observed) ++pc1;
      if (s <= observed) ++pc2;
      if (adaptive != 0 && (unsigned)done % adaptive == 0) {  // m_checkAdaptivePvalue, alternative = 0 (kbac.cpp:338-372)
        const double ap = (1.0 * pc1 + 1.0) / (1.0 * done + 1.0);
        const double sd = std::sqrt(ap * (1.0 - ap) / (1.0 * done));
        if (ap - 6.0 * sd > alpha) {
          r->pvalue = ap;
          stop = true;
          ++used;
          break;
        }
      }
    }
    std::memcpy(s0, &states[(size_t)31 * used], sizeof(s0));
  }
  if (!stop) {  // every statistic evaluated: the reference's loop shuffles once more before it ends
    uint32_t t[31];
    mat31_apply(c->jump.data(), s0, t);
    std::memcpy(s0, t, sizeof(s0));
    r->pvalue = (1.0 * pc1 + 1.0) / (1.0 * nPerm + 1.0);
  }
  std::memcpy(c->rand_state, s0, sizeof(s0));
  r->fit_ok = 1;
  r->actual_perm = done;
  r->num_ge = (int)pc1;
  r->num_le = (int)pc2;
  return RVT_OK;
}

// Price's variable-threshold test (VariableThresholdPrice::fit, src/Model.h:1752-1805) of one gene; kernels and the form of
// the statistic: vtprice_kernels.hip.h.  d_y: the phenotype on the device — centred (centerVector, src/LinearAlgebra.h:43-49)
// for a quantitative trait, the 0 / 1 values themselves for a binary one, ybar then being their mean.
// af[j] is taken as the frequency of column j of the FLIPPED, POLYMORPHIC block, as the reference's groupFrequency pairs
// them (and as rvt_kbac_blocks does).
int vtprice_stage(rvt_ctx* c, const double* dG, int M, const double* af, const double* d_y, double ybar, int nPerm, double alpha,
                  rvt_vtprice_result* r) {
  std::memset(r, 0, sizeof(*r));
  r->num_perm = nPerm;  // what Permutation holds after reset() (src/Permutation.h:99-105)
  r->perm_pvalue = 1.0;
  r->opt_freq = r->zmax = -1.0;
  const int64_t N = c->nc.N, ld = c->nc.ld;
  hipStream_t st = c->stream;
  // ---- flipped, polymorphic block (dc->getFlippedToMinorPolymorphicGenotype()) ---------------------------------------
  std::vector<const double*> cols(M);
  for (int j = 0; j < M; ++j) cols[j] = dG + (size_t)j * ld;
  DevBuf<const double*> d_cols;
  DevBuf<int> d_flags;
  HIP_TRY(c, d_cols.alloc(sizeof(double*) * (size_t)M * 2));
  HIP_TRY(c, d_flags.alloc(sizeof(int) * (size_t)M * 2));
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * M, hipMemcpyHostToDevice, st));
  k_fam_colstat(dim3((unsigned)M), st, d_cols, (long long)N, d_flags);
  std::vector<int> flags(M);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  std::vector<const double*> kc;
  std::vector<int> kf;
  for (int j = 0; j < M; ++j)
    if (flags[j] & 2) {
      kc.push_back(cols[j]);
      kf.push_back(flags[j] & 1);
    }
  const int m = (int)kc.size();
  r->n_poly = m;
  if (m == 0) return RVT_OK;  // genotype.cols == 0: fitOK = false before anything is drawn (src/Model.h:1758-1761)
  int rc = ensure_fam_cols(c, (size_t)m, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_cols + M, kc.data(), sizeof(double*) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags + M, kf.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
  k_fam_flip_compact(dim3(64, (unsigned)m), st, d_cols + M, d_flags + M, (long long)N, (long long)ld, c->d_Gp);
  // ---- frequency groups, ascending and cumulative (groupFrequency, src/Model.cpp:254-261; :311-338) ---------------------
  std::map<double, std::vector<int>> fg;
  for (int j = 0; j < m; ++j) fg[std::ceil(1000000. * af[j]) / 1000000].push_back(j);
  const int T = (int)fg.size();
  std::vector<double> freq;
  std::vector<int> tab((size_t)3 * m);  // order | grp | gend
  int *order = tab.data(), *grp = order + m, *gend = grp + m;
  {
    int k = 0;
    for (const auto& kv : fg) {
      for (int j : kv.second) {
        order[k] = j;
        grp[k] = (int)freq.size();
        gend[k++] = 0;
      }
      gend[k - 1] = 1;
      freq.push_back(kv.first);
    }
  }
  r->n_threshold = T;
  Layout L;
  const size_t o_tab = L.take(sizeof(int) * 3 * (size_t)m), o_cnt = L.take(sizeof(int) * (size_t)m),
               o_stat = L.take(sizeof(unsigned long long) * 2 * (size_t)T), o_off = L.take(sizeof(long long) * (size_t)m),
               o_segoff = L.take(sizeof(int) * ((size_t)T + 1)), o_sd = L.take(sizeof(double) * 2 * (size_t)T),
               o_obs = L.take(sizeof(double) + sizeof(int));
  HIP_TRY(c, c->d_vtp_ws.grow(L.total, L.total + L.total / 2, st, true));
  char* ws = c->d_vtp_ws;
  int* d_tab = (int*)(ws + o_tab);
  int* d_cnt = (int*)(ws + o_cnt);
  unsigned long long* d_stat = (unsigned long long*)(ws + o_stat);
  long long* d_off = (long long*)(ws + o_off);
  int* d_segoff = (int*)(ws + o_segoff);
  double* d_sd = (double*)(ws + o_sd);  // sd | shift
  double* d_obs = (double*)(ws + o_obs);
  HIP_TRY(c, hipMemcpyAsync(d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * 2 * (size_t)T, st));
  hipLaunchKernelGGL(vtp_count_kernel, dim3((unsigned)m), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, d_cnt);
  hipLaunchKernelGGL(vtp_rowstat_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld,
                     m, d_tab, d_tab + m, d_tab + 2 * m, T, d_stat);
  HIP_TRY(c, hipGetLastError());
  std::vector<int> cnt(m);
  std::vector<unsigned long long> stat((size_t)2 * T);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(stat.data(), d_stat, sizeof(unsigned long long) * stat.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  // ---- the carrier list in group order, cut into segments that stay inside one group ------------------------------------
  std::vector<long long> off(m), goff((size_t)T + 1, 0);
  long long nnz = 0;
  for (int k = 0; k < m; ++k) {
    off[order[k]] = nnz;
    nnz += cnt[order[k]];
    goff[grp[k] + 1] = nnz;
  }
  if (nnz > 0x7fffffffLL) return fail(c, RVT_E_INVALID, "variable-threshold test: %lld carrier entries", nnz);
  r->n_carrier_entries = nnz;
  const int seglen = (int)std::min<long long>(4096, std::max<long long>(64, (nnz / 512 + 63) / 64 * 64));  // (a function of the gene alone)
  std::vector<int2> segs;
  std::vector<int> segoff((size_t)T + 1, 0);
  std::vector<double> sds((size_t)2 * T);  // sd | shift
  unsigned long long S1 = 0, S2 = 0;
  for (int t = 0; t < T; ++t) {
    if (goff[t + 1] - goff[t] != (long long)stat[t])
      return fail(c, RVT_E_STATE, "variable-threshold test: group %d holds %lld carriers, the sample pass counted %llu", t,
                  goff[t + 1] - goff[t], stat[t]);
    for (long long e = goff[t]; e < goff[t + 1]; e += seglen)
      segs.push_back(make_int2((int)e, (int)std::min<long long>(e + seglen, goff[t + 1])));
    segoff[t + 1] = (int)segs.size();
    S1 += stat[t];
    S2 += stat[T + t];
    // sum (b - mean)^2 / N = (N sum b^2 - (sum b)^2) / N^2, the numerator an exact integer: zero exactly when the row is
    // constant, where the reference leaves z undivided (src/Model.h:1865-1868)
    const unsigned __int128 num = (unsigned __int128)(unsigned long long)N * S2 - (unsigned __int128)S1 * S1;
    sds[t] = std::sqrt((double)num / ((double)N * (double)N));
    sds[T + t] = ybar * (double)S1;
  }
  const int nseg = (int)segs.size();
  Layout E;
  const size_t o_ent = E.take(sizeof(uint32_t) * (size_t)std::max<long long>(nnz, 1)),
               o_segs = E.take(sizeof(int2) * (size_t)std::max(nseg, 1));
  HIP_TRY(c, c->d_vtp_ent.grow(E.total, E.total + E.total / 2, st, true));
  uint32_t* d_ent = (uint32_t*)(c->d_vtp_ent.get() + o_ent);
  int2* d_segs = (int2*)(c->d_vtp_ent.get() + o_segs);
  HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), sizeof(long long) * m, hipMemcpyHostToDevice, st));
  if (nseg) {
    HIP_TRY(c, hipMemcpyAsync(d_segs, segs.data(), sizeof(int2) * (size_t)nseg, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemcpyAsync(d_segoff, segoff.data(), sizeof(int) * segoff.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_sd, sds.data(), sizeof(double) * sds.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vtp_fill_kernel, dim3((unsigned)m), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, d_off, d_cnt, d_ent);
  // ---- observed statistic: the same two kernels, no shuffle --------------------------------------------------------------
  constexpr int kChunk = 2048;
  const int B = c->perm_exact ? exact_chunk(nPerm, N) : kChunk;  // shuffles whose partial sums d_vtp_part holds
  {
    const size_t need = sizeof(double) * (size_t)std::max(nseg, 1) * (size_t)B;
    HIP_TRY(c, c->d_vtp_part.grow(need, need + need / 4, st, true));
    HIP_TRY(c, c->d_vtp_z.grow(sizeof(double) * kChunk, sizeof(double) * kChunk, st, true));
  }
  if (nseg)
    hipLaunchKernelGGL((vtp_segsum_kernel<kVtpIdentity>), dim3((unsigned)nseg, 1), dim3(64), 0, st, d_ent, d_segs, d_y, (long long)N,
                       0ull, 0ull, 0u, 1, c->d_vtp_part);
  hipLaunchKernelGGL(vtp_finish_kernel, dim3(1), dim3(64), 0, st, c->d_vtp_part, d_segoff, T, 1, d_sd, d_sd + T, d_obs,
                     (int*)(d_obs + 1));
  HIP_TRY(c, hipGetLastError());
  struct {
    double z;
    int t;
  } ob;
  HIP_TRY(c, hipMemcpyAsync(&ob, d_obs, sizeof(double) + sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  const double obs = ob.z;  // perm.init(fabs(zmax)): already an absolute value
  r->zmax = obs;
  r->opt_freq = freq[ob.t];
  // Permutation::init — `threshold` is an INT member of the reference's class (src/Permutation.h:153): the product is truncated
  const double threshold = (double)(int)(1.0 * nPerm * alpha * 2);
  int actual = 0, numX = 0, numEq = 0;
  std::vector<double> Z(kChunk);
  auto launch_statistics = [&](int srcKind, const double* src, unsigned shuffle0, int nb, uint64_t key) {
    if (nseg) {
      const dim3 grid((unsigned)nseg, (unsigned)((nb + 63) / 64));
      if (srcKind == kVtpCounter)
        hipLaunchKernelGGL((vtp_segsum_kernel<kVtpCounter>), grid, dim3(64), 0, st, d_ent, d_segs, src, (long long)N,
                           (unsigned long long)c->perm_seed, (unsigned long long)key, shuffle0, nb, c->d_vtp_part);
      else
        hipLaunchKernelGGL((vtp_segsum_kernel<kVtpMatrix>), grid, dim3(64), 0, st, d_ent, d_segs, src, (long long)N, 0ull, 0ull,
                           0u, nb, c->d_vtp_part);
    }
    hipLaunchKernelGGL(vtp_finish_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, c->d_vtp_part, d_segoff, T, nb, d_sd,
                       d_sd + T, c->d_vtp_z, (int*)nullptr);
  };
  auto statistics = [&](int srcKind, const double* src, unsigned shuffle0, int nb, uint64_t key) -> int {
    launch_statistics(srcKind, src, shuffle0, nb, key);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Z.data(), c->d_vtp_z, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    return RVT_OK;
  };
  auto finish = [&]() {
    r->fit_ok = 1;
    r->actual_perm = actual;
    r->num_greater = numX;
    r->num_equal = numEq;
    r->perm_pvalue = actual == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEq) / actual;
    return RVT_OK;
  };
  if (!c->perm_exact) {
    // ---- counter-based shuffles (perm_counter.h): keyed by a hash of the gene's frequencies, so that a gene draws the same
    // shuffles wherever and whenever it runs (the call carries no gene ids)
    uint64_t key = 0xcbf29ce484222325ull;  // FNV-1a over M and the bytes of af
    auto mix = [&](const void* p, size_t n) {
      for (size_t i = 0; i < n; ++i) key = (key ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
    };
    mix(&M, sizeof(M));
    mix(af, sizeof(double) * (size_t)M);
    bool more = true;
    while (more) {
      if (actual >= nPerm || numX + numEq >= threshold) break;  // Permutation::next() before every shuffle
      // the first chunk is short: a gene far from significance stops after ~2 threshold shuffles
      const int want = actual == 0 ? std::min<int>(kChunk, (int)std::max(64.0, 2.5 * threshold)) : kChunk;
      const int nb = std::min(want, nPerm - actual);
      rc = statistics(kVtpCounter, d_y, (unsigned)actual, nb, key);
      if (rc) return rc;
      for (int u = 0; u < nb; ++u) {
        if (actual >= nPerm || numX + numEq >= threshold) {
          more = false;
          break;
        }
        ++actual;  // Permutation::add
        if (Z[u] > obs) ++numX;
        if (Z[u] == obs) ++numEq;
      }
    }
    return finish();
  }
  // ---- exact mode: the reference's rand() stream, N - 1 draws per shuffle, cumulative shuffles of the phenotype -------------
  rc = exact_permutations(
      c, d_y, nPerm, alpha, obs, 0,
      [&](int nb, int, const double** d_out) -> int {
        launch_statistics(kVtpMatrix, c->d_perm_R, 0u, nb, 0);
        *d_out = c->d_vtp_z;
        return RVT_OK;
      },
      &actual, &numX, &numEq);
  if (rc) return rc;
  return finish();
}


// ---- the permutation burden tests for a 0 / 1 phenotype (burdenperm_kernels.hip.h) -----------------------------------------------
// dc->getFlippedToMinorPolymorphicGenotype() of one gene into c->d_Gp (ld x *m_)
static int flipped_poly_block(rvt_ctx* c, const double* dG, int M, int* m_) {
  const int64_t N = c->nc.N, ld = c->nc.ld;
  hipStream_t st = c->stream;
  std::vector<const double*> cols(M);
  for (int j = 0; j < M; ++j) cols[j] = dG + (size_t)j * ld;
  DevBuf<const double*> d_cols;
  DevBuf<int> d_flags;
  HIP_TRY(c, d_cols.alloc(sizeof(double*) * (size_t)M * 2));
  HIP_TRY(c, d_flags.alloc(sizeof(int) * (size_t)M * 2));
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * M, hipMemcpyHostToDevice, st));
  k_fam_colstat(dim3((unsigned)M), st, d_cols, (long long)N, d_flags);
  std::vector<int> flags(M);
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  std::vector<const double*> kc;
  std::vector<int> kf;
  for (int j = 0; j < M; ++j)
    if (flags[j] & 2) {
      kc.push_back(cols[j]);
      kf.push_back(flags[j] & 1);
    }
  const int m = (int)kc.size();
  *m_ = m;
  if (m == 0) return RVT_OK;
  int rc = ensure_fam_cols(c, (size_t)m, ld);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_cols + M, kc.data(), sizeof(double*) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags + M, kf.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
  k_fam_flip_compact(dim3(64, (unsigned)m), st, d_cols + M, d_flags + M, (long long)N, (long long)ld, c->d_Gp);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sync_stream(st));  // (d_cols / d_flags are freed on return)
  return RVT_OK;
}

// the key of a gene's counter-based shuffles: FNV-1a over the polymorphic column count and the per-column entry counts
static uint64_t burdenperm_key(int m, const std::vector<int>& cnt) {
  uint64_t key = 0xcbf29ce484222325ull;
  auto mix = [&](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) key = (key ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  };
  mix(&m, sizeof(m));
  mix(cnt.data(), sizeof(int) * cnt.size());
  return key;
}

constexpr int kBpChunk = 2048;  // shuffles per launch, both modes (exact_chunk() never exceeds it)

// Permutation's loop over counter-based shuffles, a chunk at a time.  launch(shuffle0, nb) leaves the chunk's statistics in
// c->d_bp_stat.  failed (optional): Madsen-Browning's rule for a statistic below zero, as in exact_permutations.
extern "C++" {
template <class Launch>
int counter_permutations(rvt_ctx* c, int nPerm, double alpha, double obs, Launch&& launch, int* actual_, int* numX_, int* numEq_,
                         int* failed_ = nullptr) {
  hipStream_t st = c->stream;
  // Permutation::init — `threshold` is an INT member of the reference's class (src/Permutation.h:153): the product is truncated
  const double threshold = (double)(int)(1.0 * nPerm * alpha * 2);
  int actual = 0, numX = 0, numEq = 0;
  unsigned drawn = 0;  // shuffle indices consumed (a failed statistic consumes one without being added)
  std::vector<double> Q(kBpChunk);
  bool more = true;
  while (more) {
    if (actual >= nPerm || numX + numEq >= threshold) break;  // Permutation::next() before every shuffle
    // the first chunk is short: a gene far from significance stops after ~2 threshold shuffles
    const int want = actual == 0 ? std::min<int>(kBpChunk, (int)std::max(64.0, 2.5 * threshold)) : kBpChunk;
    const int nb = std::min(want, nPerm - actual);
    launch(drawn, nb);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(Q.data(), c->d_bp_stat, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    for (int u = 0; u < nb; ++u) {
      if (actual >= nPerm || numX + numEq >= threshold) {
        more = false;
        break;
      }
      ++drawn;
      if (failed_ && Q[u] < 0) {
        if (*failed_ < 10) {
          ++*failed_;
          continue;
        }
        *failed_ = 11;
        more = false;
        break;
      }
      ++actual;  // Permutation::add
      if (Q[u] > obs) ++numX;
      if (Q[u] == obs) ++numEq;
    }
  }
  *actual_ = actual, *numX_ = numX, *numEq_ = numEq;
  return RVT_OK;
}
}  // extern "C++"

// RareCover (RareCoverTest::fit, src/Model.h:1427-1476) of one gene.  d_y: the 0 / 1 phenotype on the device, cases: its sum,
// valid: it is 0 / 1 with both classes present.
int rarecover_stage(rvt_ctx* c, const double* dG, int M, const double* d_y, double cases, bool valid, int nPerm, double alpha,
                    rvt_rarecover_result* r) {
  std::memset(r, 0, sizeof(*r));
  r->num_perm = nPerm;  // what Permutation holds after reset() (src/Permutation.h:99-105)
  r->perm_pvalue = 1.0;
  r->stat = -1.0;
  const int64_t N = c->nc.N, ld = c->nc.ld;
  hipStream_t st = c->stream;
  int m = 0;
  int rc = flipped_poly_block(c, dG, M, &m);
  if (rc) return rc;
  r->n_poly = m;
  if (m == 0 || !valid) return RVT_OK;  // genotype.cols == 0: fitOK = false before anything is drawn (src/Model.h:1448-1451)
  // ---- the carrier union and the bit matrix ----------------------------------------------------------------------------------
  const int nblk = (int)((N + 255) / 256);
  Layout L;
  const size_t o_cnt = L.take(sizeof(int) * (size_t)m), o_bcnt = L.take(sizeof(int) * (size_t)nblk),
               o_obs = L.take(sizeof(double) + sizeof(int));
  HIP_TRY(c, c->d_bp_ws.grow(L.total, L.total + L.total / 2, st, true));
  char* ws = c->d_bp_ws;
  int* d_cnt = (int*)(ws + o_cnt);
  int* d_bcnt = (int*)(ws + o_bcnt);
  double* d_obs = (double*)(ws + o_obs);
  hipLaunchKernelGGL((bp_count_kernel<kBpPositive>), dim3((unsigned)m), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, d_cnt);
  hipLaunchKernelGGL(bp_union_count_kernel, dim3((unsigned)nblk), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, m, d_bcnt);
  HIP_TRY(c, hipGetLastError());
  std::vector<int> cnt(m), boff(nblk);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(boff.data(), d_bcnt, sizeof(int) * nblk, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  long long K = 0;
  for (int b = 0; b < nblk; ++b) {
    const int n = boff[b];
    boff[b] = (int)K;
    K += n;
  }
  r->n_carrier = (int)K;
  const int W = (int)std::max<long long>(1, (K + 63) / 64);
  Layout E;
  const size_t o_samp = E.take(sizeof(uint32_t) * (size_t)std::max<long long>(K, 1)),
               o_bits = E.take(sizeof(unsigned long long) * (size_t)m * W);
  HIP_TRY(c, c->d_bp_ent.grow(E.total, E.total + E.total / 2, st, true));
  uint32_t* d_samp = (uint32_t*)(c->d_bp_ent.get() + o_samp);
  unsigned long long* d_bits = (unsigned long long*)(c->d_bp_ent.get() + o_bits);
  HIP_TRY(c, hipMemcpyAsync(d_bcnt, boff.data(), sizeof(int) * nblk, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d_bits, 0, sizeof(unsigned long long) * (size_t)m * W, st));
  hipLaunchKernelGGL(bp_union_pack_kernel, dim3((unsigned)nblk), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, m, d_bcnt,
                     (int)K, W, d_samp, d_bits);
  // c and Y of a shuffle: 16 W bytes of LDS when they fit the 64 KB a launch may ask for, else a slot of a global work space
  const size_t lds = sizeof(unsigned long long) * 2 * (size_t)W;
  const bool in_lds = lds <= 64 * 1024;
  unsigned long long* d_cy = nullptr;
  if (!in_lds) {
    const size_t need = lds * kBpChunk;
    HIP_TRY(c, c->d_bp_cy.grow(need, need, st, true));
    d_cy = c->d_bp_cy;
  }
  HIP_TRY(c, c->d_bp_stat.grow(sizeof(double) * kBpChunk, sizeof(double) * kBpChunk, st, true));
  const unsigned dyn = in_lds ? (unsigned)lds : 0u;
  // ---- observed statistic and NumIncludeMarker: the same kernel, no shuffle -----------------------------------------------------
  hipLaunchKernelGGL((rc_cover_kernel<kBpIdentity>), dim3(1), dim3(kRcThreads), dyn, st, d_bits, d_samp, (int)K, W, m, d_y,
                     (long long)N, cases, 0ull, 0ull, 0u, d_cy, d_obs, (int*)(d_obs + 1));
  HIP_TRY(c, hipGetLastError());
  struct {
    double s;
    int n;
  } ob;
  HIP_TRY(c, hipMemcpyAsync(&ob, d_obs, sizeof(double) + sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  const double obs = ob.s;
  r->stat = obs;
  r->n_selected = ob.n;
  int actual = 0, numX = 0, numEq = 0;
  if (!c->perm_exact) {
    const uint64_t key = burdenperm_key(m, cnt);
    rc = counter_permutations(
        c, nPerm, alpha, obs,
        [&](unsigned shuffle0, int nb) {
          hipLaunchKernelGGL((rc_cover_kernel<kBpCounter>), dim3((unsigned)nb), dim3(kRcThreads), dyn, st, d_bits, d_samp, (int)K, W, m,
                             d_y, (long long)N, cases, (unsigned long long)c->perm_seed, (unsigned long long)key, shuffle0, d_cy,
                             c->d_bp_stat.get(), (int*)nullptr);
        },
        &actual, &numX, &numEq);
  } else {
    // exact mode: the reference's rand() stream, N - 1 draws per shuffle, cumulative shuffles of the phenotype
    rc = exact_permutations(
        c, d_y, nPerm, alpha, obs, 0,
        [&](int nb, int, const double** d_out) -> int {
          hipLaunchKernelGGL((rc_cover_kernel<kBpMatrix>), dim3((unsigned)nb), dim3(kRcThreads), dyn, st, d_bits, d_samp, (int)K, W, m,
                             c->d_perm_R.get(), (long long)N, cases, 0ull, 0ull, 0u, d_cy, c->d_bp_stat.get(), (int*)nullptr);
          *d_out = c->d_bp_stat;
          return RVT_OK;
        },
        &actual, &numX, &numEq);
  }
  if (rc) return rc;
  r->fit_ok = 1;
  r->actual_perm = actual;
  r->num_greater = numX;
  r->num_equal = numEq;
  r->perm_pvalue = actual == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEq) / actual;
  return RVT_OK;
}

// Madsen-Browning (MadsonBrowningTest::fit, src/Model.h:1252-1305) of one gene; arguments as rarecover_stage.
int mb_stage(rvt_ctx* c, const double* dG, int M, const double* d_y, double cases, bool valid, int nPerm, double alpha,
             rvt_mb_result* r) {
  std::memset(r, 0, sizeof(*r));
  r->num_perm = nPerm;  // what Permutation holds after reset() (src/Permutation.h:99-105)
  r->perm_pvalue = 1.0;
  const int64_t N = c->nc.N, ld = c->nc.ld;
  hipStream_t st = c->stream;
  int m = 0;
  int rc = flipped_poly_block(c, dG, M, &m);
  if (rc) return rc;
  r->n_poly = m;
  if (m == 0 || !valid || !c->nc.binary) return RVT_OK;  // (a quantitative null model: the observed score test has no model)
  // ---- the entry list, column by column in sample order, cut into segments -------------------------------------------------------
  Layout L;
  const size_t o_cnt = L.take(sizeof(int) * (size_t)m), o_off = L.take(sizeof(long long) * (size_t)m),
               o_segoff = L.take(sizeof(int) * ((size_t)m + 1)), o_ac = L.take(sizeof(double) * (size_t)m),
               o_K = L.take(sizeof(double) * (size_t)m * m), o_col = L.take(sizeof(double) * (size_t)std::max(c->null_ld, ld));
  HIP_TRY(c, c->d_bp_ws.grow(L.total, L.total + L.total / 2, st, true));
  char* ws = c->d_bp_ws;
  int* d_cnt = (int*)(ws + o_cnt);
  long long* d_off = (long long*)(ws + o_off);
  int* d_segoff = (int*)(ws + o_segoff);
  double* d_AC = (double*)(ws + o_ac);
  double* d_K = (double*)(ws + o_K);
  double* d_col = (double*)(ws + o_col);
  hipLaunchKernelGGL((bp_count_kernel<kBpNonZero>), dim3((unsigned)m), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, d_cnt);
  HIP_TRY(c, hipGetLastError());
  std::vector<int> cnt(m);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  std::vector<long long> off(m);
  long long nnz = 0;
  for (int j = 0; j < m; ++j) {
    off[j] = nnz;
    nnz += cnt[j];
  }
  if (nnz > 0x7fffffffLL) return fail(c, RVT_E_INVALID, "Madsen-Browning test: %lld genotype entries", nnz);
  r->n_entries = nnz;
  const int seglen = (int)std::min<long long>(4096, std::max<long long>(64, (nnz / 512 + 63) / 64 * 64));  // (a function of the gene alone)
  std::vector<int2> segs;
  std::vector<int> segoff((size_t)m + 1, 0);
  for (int j = 0; j < m; ++j) {
    for (long long e = off[j]; e < off[j] + cnt[j]; e += seglen)
      segs.push_back(make_int2((int)e, (int)std::min<long long>(e + seglen, off[j] + cnt[j])));
    segoff[j + 1] = (int)segs.size();
  }
  const int nseg = (int)segs.size();
  Layout E;
  const size_t o_ent = E.take(sizeof(uint32_t) * (size_t)std::max<long long>(nnz, 1)),
               o_val = E.take(sizeof(double) * (size_t)std::max<long long>(nnz, 1)),
               o_segs = E.take(sizeof(int2) * (size_t)std::max(nseg, 1));
  HIP_TRY(c, c->d_bp_ent.grow(E.total, E.total + E.total / 2, st, true));
  uint32_t* d_ent = (uint32_t*)(c->d_bp_ent.get() + o_ent);
  double* d_val = (double*)(c->d_bp_ent.get() + o_val);
  int2* d_segs = (int2*)(c->d_bp_ent.get() + o_segs);
  HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), sizeof(long long) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_segs, segs.data(), sizeof(int2) * (size_t)nseg, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_segoff, segoff.data(), sizeof(int) * segoff.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL((bp_fill_kernel<kBpNonZero>), dim3((unsigned)m), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, d_off, d_cnt,
                     d_ent, d_val);
  hipLaunchKernelGGL(mb_colsum_kernel, dim3((unsigned)m), dim3(256), 0, st, d_val, d_off, d_cnt, d_AC);
  HIP_TRY(c, hipGetLastError());
  // K = G'G through the integer planes: exact for hard calls (the product the SKAT permutations use)
  rc = gemm_tn_planes(c, c->d_Gp, ld, m, c->d_Gp, ld, m, N, d_K, m, st);
  if (rc) return rc;
  {
    const size_t need = sizeof(double) * (size_t)std::max(nseg, m) * kBpChunk;
    HIP_TRY(c, c->d_bp_part.grow(need, need + need / 4, st, true));
    const size_t nw = sizeof(double) * (size_t)m * kBpChunk;
    HIP_TRY(c, c->d_bp_w.grow(nw, nw + nw / 4, st, true));
    HIP_TRY(c, c->d_bp_stat.grow(sizeof(double) * kBpChunk, sizeof(double) * kBpChunk, st, true));
  }
  const double n = (double)N;
  // ---- observed statistic: the binary score test of the fitted null model on the observed collapsed column ----------------------
  hipLaunchKernelGGL((mb_segsum_kernel<kBpIdentity>), dim3((unsigned)nseg, 1), dim3(64), 0, st, d_ent, d_val, d_segs, d_y, (long long)N,
                     0ull, 0ull, 0u, 1, c->d_bp_part.get());
  hipLaunchKernelGGL(mb_finish_kernel, dim3(1), dim3(64), 0, st, c->d_bp_part.get(), d_segoff, m, 1, d_AC, d_K, n, cases,
                     c->d_bp_w.get(), c->d_bp_stat.get(), 1);
  const long long ld_col = (long long)std::max(c->null_ld, ld);
  hipLaunchKernelGGL(mb_collapse_kernel, dim3((unsigned)((ld_col + 255) / 256)), dim3(256), 0, st, c->d_Gp, (long long)N, (long long)ld, m,
                     c->d_bp_w.get(), ld_col, d_col);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sync_stream(st));
  int ok = 0;
  double us = 0, vs = 0, eff = 0, se = 0, pv = 0;
  rc = rvt_score_block(c, d_col, 1, &ok, &us, &vs, &eff, &se, &pv);
  if (rc) return rc;
  if (!ok || !(vs > 0.0)) return RVT_OK;  // TestCovariate failed: fitOK = false before anything is drawn
  const double obs = us * us / vs;
  r->stat = obs;
  int actual = 0, numX = 0, numEq = 0, failed = 0;
  auto launch = [&](int srcKind, const double* src, unsigned shuffle0, int nb, uint64_t key) {
    const dim3 grid((unsigned)nseg, (unsigned)((nb + 63) / 64));
    if (srcKind == kBpCounter)
      hipLaunchKernelGGL((mb_segsum_kernel<kBpCounter>), grid, dim3(64), 0, st, d_ent, d_val, d_segs, src, (long long)N,
                         (unsigned long long)c->perm_seed, (unsigned long long)key, shuffle0, nb, c->d_bp_part.get());
    else
      hipLaunchKernelGGL((mb_segsum_kernel<kBpMatrix>), grid, dim3(64), 0, st, d_ent, d_val, d_segs, src, (long long)N, 0ull, 0ull, 0u, nb,
                         c->d_bp_part.get());
    hipLaunchKernelGGL(mb_finish_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, c->d_bp_part.get(), d_segoff, m, nb, d_AC,
                       d_K, n, cases, c->d_bp_w.get(), c->d_bp_stat.get(), 0);
  };
  if (!c->perm_exact) {
    const uint64_t key = burdenperm_key(m, cnt);
    rc = counter_permutations(
        c, nPerm, alpha, obs, [&](unsigned shuffle0, int nb) { launch(kBpCounter, d_y, shuffle0, nb, key); }, &actual, &numX, &numEq,
        &failed);
  } else {
    rc = exact_permutations(
        c, d_y, nPerm, alpha, obs, 0,
        [&](int nb, int, const double** d_out) -> int {
          launch(kBpMatrix, c->d_perm_R, 0u, nb, 0);
          *d_out = c->d_bp_stat;
          return RVT_OK;
        },
        &actual, &numX, &numEq, &failed);
  }
  if (rc) return rc;
  r->fit_ok = failed > 10 ? 0 : 1;  // the eleventh failed shuffle fails the gene; the counters stay as they stand
  r->actual_perm = actual;
  r->num_greater = numX;
  r->num_equal = numEq;
  r->perm_pvalue = actual == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEq) / actual;
  return RVT_OK;
}

}  // namespace

// ---- --vt price: Price's variable-threshold permutation test of device-resident blocks -------------------------------------
int rvt_vtprice_blocks(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* af, const double* y, int nperm,
                       double alpha, rvt_vtprice_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !M || !af || !y || !out)) || nperm < 0) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set (it defines the sample count)");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  const int64_t N = c->nc.N;
  // copyPhenotype + centerVector (src/LinearAlgebra.h:43-49): the mean as Vector::Average forms it, in sample order.  A 0 / 1
  // phenotype stays as it is: its sums over carriers are then exact integers and the mean enters once, in vtp_finish_kernel.
  bool binary = true;
  double sum = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    binary = binary && (y[i] == 0.0 || y[i] == 1.0);
    sum += y[i];
  }
  const double avg = sum / (double)N;
  std::vector<double> yv(y, y + N);
  if (!binary)
    for (int64_t i = 0; i < N; ++i) yv[i] -= avg;
  DevBuf<double> d_y;
  HIP_TRY(c, d_y.alloc(sizeof(double) * (size_t)N));
  HIP_TRY(c, hipMemcpyAsync(d_y, yv.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, sync_stream(c->stream));
  size_t afo = 0;
  for (int g = 0; g < n; ++g) {  // one gene at a time: the random stream is consumed in gene order
    if (M[g] < 1 || M[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M[g]);
    rc = vtprice_stage(c, dG[g], M[g], af + afo, d_y, binary ? avg : 0.0, nperm, alpha, out + g);
    if (rc) return rc;
    afo += (size_t)M[g];
  }
  return RVT_OK;
}

// ---- --burden rarecover / mb: the permutation burden tests of device-resident blocks -----------------------------------------------
namespace {
// the 0 / 1 phenotype on the device; *valid: every value is 0 or 1 and both classes are present
int binary_phenotype(rvt_ctx* c, const double* y, DevBuf<double>* d_y, double* cases, bool* valid) {
  const int64_t N = c->nc.N;
  bool binary = true;
  long long n1 = 0;
  for (int64_t i = 0; i < N; ++i) {
    binary = binary && (y[i] == 0.0 || y[i] == 1.0);
    n1 += y[i] == 1.0;
  }
  *valid = binary && n1 > 0 && n1 < N;
  *cases = (double)n1;
  HIP_TRY(c, d_y->alloc(sizeof(double) * (size_t)N));
  HIP_TRY(c, hipMemcpyAsync(d_y->get(), y, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, sync_stream(c->stream));
  return RVT_OK;
}
}  // namespace

int rvt_rarecover_blocks(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* y, int nperm, double alpha,
                         rvt_rarecover_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !M || !y || !out)) || nperm < 0) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set (it defines the sample count)");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  DevBuf<double> d_y;
  double cases = 0.0;
  bool valid = false;
  rc = binary_phenotype(c, y, &d_y, &cases, &valid);
  if (rc) return rc;
  for (int g = 0; g < n; ++g) {  // one gene at a time: the random stream is consumed in gene order
    if (M[g] < 1 || M[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M[g]);
    rc = rarecover_stage(c, dG[g], M[g], d_y, cases, valid, nperm, alpha, out + g);
    if (rc) return rc;
  }
  return RVT_OK;
}

int rvt_mb_blocks(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* y, int nperm, double alpha,
                  rvt_mb_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !M || !y || !out)) || nperm < 0) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set (it defines the sample count)");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  DevBuf<double> d_y;
  double cases = 0.0;
  bool valid = false;
  rc = binary_phenotype(c, y, &d_y, &cases, &valid);
  if (rc) return rc;
  for (int g = 0; g < n; ++g) {  // one gene at a time: the random stream is consumed in gene order
    if (M[g] < 1 || M[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M[g]);
    rc = mb_stage(c, dG[g], M[g], d_y, cases, valid, nperm, alpha, out + g);
    if (rc) return rc;
  }
  return RVT_OK;
}

// (kbac_stage for rvt_meta.hip's rvt_kbac_blocks)
int rvt_kbac_stage(rvt_ctx* c, const double* dG, int M, const double* af, const std::vector<unsigned char>& y, int nPerm,
                   double alpha, rvt_kbac_result* r) {
  return kbac_stage(c, dG, M, af, y, nPerm, alpha, r);
}

// analytic tests + permutation test, one gene at a time (the random stream is consumed in gene order)
int run_blocks_with_perm(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* af,
                         const int64_t* ids, uint32_t tests, const rvt_params* prm, rvt_gene_result* out) {
  size_t afo = 0;
  for (int g = 0; g < n; ++g) {
    DebugOut dbg;
    GeneDesc g0;
    dbg.desc0 = &g0;
    int64_t id = ids ? ids[g] : g;
    int rc = run_batch(c, 1, dG + g, M + g, af + afo, &id, tests, prm, out + g, &dbg);
    if (!rc) rc = rvt_sync(c);
    if (rc) return rc;
    afo += (size_t)M[g];
    if (out[g].skat_ok) {  // genotype.cols == 0 returns before the permutations (src/Model.h:2665-2668)
      rc = perm_stage(c, dG[g], M[g], g0, *prm, out + g);
      if (rc) return rc;
    }
  }
  return RVT_OK;
}

int rvt_rand_seed(rvt_ctx* c, unsigned seed) {
  if (!c) return RVT_E_INVALID;
  seed_rand_state(c->rand_state, seed);
  c->perm_seed = seed;
  return RVT_OK;
}

int rvt_set_perm_exact(rvt_ctx* c, int on) {
  if (!c) return RVT_E_INVALID;
  c->perm_exact = on != 0;
  return RVT_OK;
}

// Test hook: arm (stats == NULL: disarm) the trace of the next gene's SKAT permutation stage
int rvt_debug_perm_trace(rvt_ctx* c, double* stats, int cap, int* n_written) {
  if (!c) return RVT_E_INVALID;
  if (stats && (cap < 0 || !n_written)) return fail(c, RVT_E_INVALID, "bad arguments");
  c->perm_trace_stats = stats;
  c->perm_trace_cap = stats ? cap : 0;
  c->perm_trace_n = stats ? n_written : nullptr;
  if (stats) *n_written = 0;
  return RVT_OK;
}

}  // extern "C"
