// rvtests_amd — the tests that are not gene tests of the main pipeline: KBAC, MetaScore, MetaCov (bands and rectangles, the
// exact int8 band for hard calls) and the column operations of the adapters' device ring.  Part of librvtests_amd.so.
// this unit compiles (and ships) the META kernel family only: see "kernel families" in rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_META
#include "rvt_engine_int.h"
#include "gemm_f64.hip.h"
#include "band_rows.hip.h"
#include "bed_expand.hip.h"
#include "wald_logistic.hip.h"
#include "burdencol_kernels.hip.h"
#include "recode_kernels.hip.h"
#include "bed_band_kernels.hip.h"
#include <functional>

// row slices of MetaCov's column pass (cov_hc_prep_kernel): a function of N alone, so that a column's sums are the same numbers
// whether it is treated inside a block or alone behind its upload (rvt_block_upload_columns)
static constexpr int kCovSlices = 16;

// ---- column blocks: what the engine knows about a block of rvt_block_alloc (rvt_ctx::ColKind), every operation written once ----
using ColKind = rvt_ctx::ColKind;

static ColKind* find_block(rvt_ctx* c, const double* dG) {
  auto it = c->col_kind.find(dG);
  return it == c->col_kind.end() ? nullptr : &it->second;
}

// Columns [col0, col0 + ncols) lie inside the block — asked of every column operation before any device work.  Only a block
// the engine knows can be checked: a pointer it does not know (a caller's own allocation) is taken on trust.
static int check_columns(rvt_ctx* c, const double* dG, int col0, int ncols) {
  const ColKind* ck = find_block(c, dG);
  if (ck && (long long)col0 + ncols > ck->cols)
    return fail(c, RVT_E_INVALID, "columns [%d, %d) leave the block (%d columns)", col0, col0 + ncols, ck->cols);
  return RVT_OK;
}

// What was known about columns [col0, col0 + ncols) is void, they are being overwritten: their cache entries (a stale one
// would hand the OLD column to the integer product, which no longer tests what it reads once an entry is marked valid) and
// their content flags — unless a column pass behind the caller rewrites those (pass_follows: it does while hard calls are
// switched on).  Unknown = not hard calls.
static int invalidate_columns(rvt_ctx* c, ColKind* ck, int col0, int ncols, bool pass_follows) {
  if (!ck) return RVT_OK;
  if (!ck->valid.empty()) std::fill_n(ck->valid.begin() + col0, (size_t)ncols, (unsigned char)0);
  if (ck->d_flags && !(pass_follows && c->hc_enabled))
    HIP_TRY(c, hipMemsetAsync(ck->d_flags + col0, 0, sizeof(int) * (size_t)ncols, c->io_stream));
  return RVT_OK;
}

// (flags are allocated by the first column that arrives; the zeroed block of rvt_block_alloc holds hard calls only)
static int ensure_flags(rvt_ctx* c, ColKind& ck) {
  if (ck.d_flags) return RVT_OK;
  HIP_TRY(c, ck.d_flags.alloc(sizeof(int) * (size_t)ck.cols));
  HIP_TRY(c, hipMemsetAsync(ck.d_flags, 0x01, sizeof(int) * (size_t)ck.cols, c->io_stream));
  return RVT_OK;
}

static void free_col_cache(ColKind& ck) {
  ck.d_i8.reset();
  ck.d_i4.reset();
  ck.d_m4.reset();
  ck.d_mu.reset();
  ck.d_cs.reset();
  ck.d_poly.reset();
  ck.d_T.reset();
  std::fill(ck.valid.begin(), ck.valid.end(), 0);
}
static bool alloc_col_cache(ColKind& ck, int64_t ldk, int64_t ldk4, uint64_t gen, hipStream_t st) {
  const size_t cap = ((size_t)ck.cols + 255) / 256 * 256 + 256;  // (the products read whole tiles of columns)
  bool ok = ck.d_i8.alloc(cap * (size_t)ldk) == hipSuccess &&
            ck.d_i4.alloc(cap * (size_t)ldk4) == hipSuccess &&
            ck.d_m4.alloc(cap * (size_t)ldk4) == hipSuccess &&
            ck.d_mu.alloc(sizeof(double) * (size_t)ck.cols) == hipSuccess &&
            ck.d_cs.alloc(sizeof(double) * (size_t)ck.cols) == hipSuccess &&
            ck.d_poly.alloc(sizeof(int) * (size_t)ck.cols) == hipSuccess &&
            ck.d_T.alloc(sizeof(double) * (size_t)ck.cols * RVT_MAX_COV) == hipSuccess;
  ok = ok && hipMemsetAsync(ck.d_i8, 0, cap * (size_t)ldk, st) == hipSuccess &&
       hipMemsetAsync(ck.d_i4, 0, cap * (size_t)ldk4, st) == hipSuccess &&
       hipMemsetAsync(ck.d_m4, 0, cap * (size_t)ldk4, st) == hipSuccess &&
       hipMemsetAsync(ck.d_mu, 0, sizeof(double) * (size_t)ck.cols, st) == hipSuccess;
  ck.valid.assign((size_t)ck.cols, 0);
  if (!ok) {
    (void)hipGetLastError();
    free_col_cache(ck);
    return false;
  }
  ck.ldk = ldk;
  ck.ldk4 = ldk4;
  ck.gen = gen;
  return true;
}

// bytes between the int8 columns of a cache made for N samples (its E2M1 columns: two codes per byte)
static int64_t cache_ldk(int64_t N) { return (N + 127) / 128 * 128; }

// Make sure the block has a column cache of the INSTALLED model (unweighted null models only; one made under another model is
// freed, nothing of it is used; an allocation that failed once is not tried again) and say whether it has one.
static bool ensure_cache(rvt_ctx* c, ColKind& ck) {
  if (!c->have_null || c->nc.binary || getenv("RVT_METACOV_NO_CACHE")) return false;
  const int64_t ldk = cache_ldk(c->nc.N), ldk4 = cache_ldk((c->nc.N + 1) / 2);
  if (ck.d_i8 && (ck.ldk != ldk || ck.gen != c->null_gen || !ck.d_i4)) free_col_cache(ck);
  if (!ck.d_i8 && !ck.cache_failed && !alloc_col_cache(ck, ldk, ldk4, c->null_gen, c->io_stream)) ck.cache_failed = true;
  return ck.d_i8 != nullptr;
}

// The block's cache when a covariance call can start from it, else nullptr: made under the installed model, and every one of
// the W columns from col0 (of a ring of `ring` columns when ring > 0) has an entry.  State 1 (hard calls only) always counts;
// state 2 (hard calls plus one other value) where the caller can use the mask — it passes `masked` and multiplies E2M1 codes
// (fp4) — and *masked then says whether some column is in state 2.
static const ColKind* usable_cache(rvt_ctx* c, const double* dG, int ring, int col0, int W, bool fp4, bool* masked) {
  if (masked) *masked = false;
  const ColKind* ck = find_block(c, dG);
  if (!ck || !ck->d_i8 || ck->gen != c->null_gen || ck->ldk != cache_ldk(c->nc.N) || (fp4 && !ck->d_i4) ||
      (ring > 0 ? ring : col0 + W) > ck->cols || getenv("RVT_METACOV_NO_CACHE"))
    return nullptr;
  bool any2 = false;
  for (int j = 0; j < W; ++j) {
    int p = col0 + j;
    if (ring > 0 && p >= ring) p -= ring;
    const unsigned char v = ck->valid[(size_t)p];
    if (v == 0 || (v == 2 && !(masked && fp4 && ck->d_m4))) return nullptr;
    any2 = any2 || v == 2;
  }
  if (masked) *masked = any2;
  return ck;
}

// the cache entries of ncols columns from (block s, column sc) to (block t, column tc), both ranges inside their blocks; t == s
// allowed (a forward move: tc < sc); s == nullptr: nothing is known about the source.  Columns whose source has no valid entry
// become invalid in the target.
static int move_col_cache(rvt_ctx* c, ColKind* t, int tc, const ColKind* s, int sc, int ncols, hipStream_t st) {
  const bool usable = s && s->d_i8 && !(t->d_i8 && (t->ldk != s->ldk || t->gen != s->gen)) &&
                      (t->d_i8 || (s->d_i4 && alloc_col_cache(*t, s->ldk, s->ldk4, s->gen, st)));  // (no cache yet: one shaped as the source's)
  if (!usable) {
    if (!t->valid.empty()) std::fill_n(t->valid.begin() + tc, (size_t)ncols, (unsigned char)0);
    return RVT_OK;
  }
  // (forward, in pieces no longer than the shift: a piece never overwrites what it has not read)
  const int shift = (t == s) ? sc - tc : ncols;
  for (int k0 = 0; k0 < ncols; k0 += std::max(shift, 1)) {
    const int nk = std::min(std::max(shift, 1), ncols - k0);
    HIP_TRY(c, hipMemcpyAsync(t->d_i8 + (size_t)(tc + k0) * (size_t)s->ldk, s->d_i8 + (size_t)(sc + k0) * (size_t)s->ldk,
                              (size_t)nk * (size_t)s->ldk, hipMemcpyDeviceToDevice, st));
    if (t->d_i4 && s->d_i4)
      HIP_TRY(c, hipMemcpyAsync(t->d_i4 + (size_t)(tc + k0) * (size_t)s->ldk4, s->d_i4 + (size_t)(sc + k0) * (size_t)s->ldk4,
                                (size_t)nk * (size_t)s->ldk4, hipMemcpyDeviceToDevice, st));
    if (t->d_m4 && s->d_m4) {
      HIP_TRY(c, hipMemcpyAsync(t->d_m4 + (size_t)(tc + k0) * (size_t)s->ldk4, s->d_m4 + (size_t)(sc + k0) * (size_t)s->ldk4,
                                (size_t)nk * (size_t)s->ldk4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(t->d_mu + tc + k0, s->d_mu + sc + k0, sizeof(double) * (size_t)nk, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(c, hipMemcpyAsync(t->d_cs + tc + k0, s->d_cs + sc + k0, sizeof(double) * (size_t)nk, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(t->d_poly + tc + k0, s->d_poly + sc + k0, sizeof(int) * (size_t)nk, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(t->d_T + (size_t)(tc + k0) * RVT_MAX_COV, s->d_T + (size_t)(sc + k0) * RVT_MAX_COV,
                              sizeof(double) * (size_t)nk * RVT_MAX_COV, hipMemcpyDeviceToDevice, st));
  }
  std::copy_n(s->valid.begin() + sc, (size_t)ncols, t->valid.begin() + tc);  // (forward: tc < sc inside one block)
  return RVT_OK;
}

// rvt_block_alloc made dG (nothing of an earlier block at the same address, freed behind the engine's back, survives)
void block_register(rvt_ctx* c, const double* dG, int cols) {
  ColKind& ck = c->col_kind[dG];
  ck = ColKind();
  ck.cols = cols;
}
// rvt_block_free: queued columns of the block that goes away are dropped, another block's reach it first
int block_forget(rvt_ctx* c, const double* dG) {
  if (c->colq.dG == dG) c->colq.n = 0;
  else if (int rc = flush_col_queue(c)) return rc;
  (void)sync_stream(c->io_stream);
  c->col_kind.erase(dG);
  return RVT_OK;
}
// the block's whole content is replaced (rvt_block_upload): its flags and cache go, its width and whether its cache could be
// allocated stay
void block_replaced(rvt_ctx* c, const double* dG) {
  ColKind* ck = find_block(c, dG);
  if (!ck) return;
  ColKind fresh;
  fresh.cols = ck->cols;
  fresh.cache_failed = ck->cache_failed;
  *ck = std::move(fresh);
}

extern "C" {
// C (M x (Nb + Nb2), column-major, leading dimension ldc) = A' D [B | B2] in fp64 on the matrix cores (gemm_f64.hip.h).
// A: M columns (lda apart), B: Nb columns, B2: Nb2 further columns (the null-model columns), all N samples long and
// zero-padded to a multiple of 16; w: optional weights along the samples (D = diag(w)), else D = I.
// symmetric: A and B are the same columns, only the tiles that meet the upper triangle are computed (the rest of C is
// left unspecified).  K is split over the chip; the partial results are added in a fixed order.
// subtract: C -= A' D B instead (every entry is read and written by one thread); the product then runs as ONE K slice, the
// grid being the tile list — meant for short K (a rank-k update of a large C).
// halo >= 0 (symmetric only): a band — row m needs the columns m .. m + halo, only those tiles are computed.
// ring > 0: A = B = the base of a block used as a ring of `ring` columns, column m is physical column (col0 + m) mod ring.
int gemm_tn_f64(rvt_ctx* c, const double* A, int64_t lda, int M, const double* B, int64_t ldb, int Nb, const double* B2,
                int64_t ldb2, int Nb2, const double* w, int64_t N, double* C, int64_t ldc, bool symmetric, hipStream_t st,
                bool subtract, int halo, int ring, int col0) {
  const int Ntot = Nb + Nb2;
  if (M < 1 || Ntot < 1) return RVT_OK;
  if (!symmetric) halo = -1;
  int nct = 0;
  const int n_tiles = gemm_f64_tiles(M, Ntot, symmetric, &nct, halo);
  const int64_t chunks = (N + kGemmKC - 1) / kGemmKC;
  int64_t slices = gemm_f64_slices(n_tiles, chunks);
  if (const char* e = getenv("RVT_GEMM64_SLICES")) slices = std::max<int64_t>(1, atoll(e));
  if (subtract) slices = 1;
  const int64_t kslice = ((chunks + slices - 1) / slices) * kGemmKC;
  slices = (N + kslice - 1) / kslice;
  double* d_out = C;
  int64_t c_slice = 0;
  if (slices > 1) {
    c_slice = ldc * Ntot;
    const size_t need = sizeof(double) * (size_t)c_slice * (size_t)slices;
    HIP_TRY(c, c->d_rot_part.grow(need, need, st, true));
    d_out = c->d_rot_part;
  }
  const int64_t groups = (slices + 7) / 8;
  const dim3 grid(subtract ? (unsigned)n_tiles : (unsigned)(8 * (int64_t)n_tiles * groups));
  if (subtract)
    hipLaunchKernelGGL((gemm_tn_f64_kernel<3, true>), grid, dim3(kGemmThreads), 0, st, A, (long long)lda, M, B, (long long)ldb, Nb,
                       B2 ? B2 : B, (long long)(B2 ? ldb2 : ldb), Nb2, w, (long long)N, (long long)kslice, 1, d_out, (long long)ldc,
                       0LL, n_tiles, nct, symmetric ? 1 : 0, halo, ring, col0);
  else
    hipLaunchKernelGGL((gemm_tn_f64_kernel<3, false>), grid, dim3(kGemmThreads), 0, st, A, (long long)lda, M, B, (long long)ldb, Nb,
                       B2 ? B2 : B, (long long)(B2 ? ldb2 : ldb), Nb2, w, (long long)N, (long long)kslice, (int)slices, d_out,
                       (long long)ldc, (long long)c_slice, n_tiles, nct, symmetric ? 1 : 0, halo, ring, col0);
  if (slices > 1)
    k_rot_reduce_slices(st, d_out, (long long)ldc, (long long)M, (long long)Ntot, (long long)c_slice, (int)slices, C, 0);
  HIP_TRY(c, hipGetLastError());
  return RVT_OK;
}
}

extern "C" {

// What the engine wrote into the first V columns of a block it filled column by column (rvt_block_upload_columns records a
// flag per column behind the copy): 1 = hard calls only, 0 = something else, -1 = nothing known (a caller's own
// allocation, or a block filled another way).  A HINT for choosing the kernel to start on: the integer paths test every
// value they read and fall back.  colflag (optional) receives the per-column flags when they exist (empty otherwise).
static int block_hard_calls(rvt_ctx* c, const double* dG, int V, std::vector<int>* colflag, bool* any) {
  if (colflag) colflag->clear();
  if (any) *any = false;
  if (!c->hc_enabled) return 0;
  const ColKind* ck = find_block(c, dG);
  if (!ck || !ck->d_flags || V > ck->cols) {
    if (c->content_hint == 0) return 0;  // the caller said dosages (rvt_set_content_hint): do not try the integer path first
    if (any) *any = true;
    return -1;
  }
  std::vector<int> f((size_t)V);
  if (hipMemcpyAsync(f.data(), ck->d_flags, sizeof(int) * (size_t)V, hipMemcpyDeviceToHost, c->io_stream) != hipSuccess ||
      sync_stream(c->io_stream) != hipSuccess)
    return 0;
  bool all = true, some = false;
  for (int j = 0; j < V; ++j) {
    all = all && f[j] != 0;
    some = some || f[j] != 0;
  }
  if (any) *any = some;
  if (colflag) *colflag = std::move(f);
  return all ? 1 : 0;
}

// ---- KBAC (--kernel kbac): genotype-pattern permutation test, binary traits without covariates ---------------------------------
int rvt_kbac_blocks(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* af, const double* y,
                    int nperm, double alpha, rvt_kbac_result* out) {
  if (!c || n < 0 || (n > 0 && (!dG || !M || !af || !y || !out)) || nperm < 0) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set (it defines the sample count)");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  const int64_t N = c->nc.N;
  std::vector<unsigned char> yb((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    if (y[i] != 0.0 && y[i] != 1.0) return fail(c, RVT_E_INVALID, "KBAC needs a 0 / 1 phenotype");
    yb[i] = y[i] == 1.0;
  }
  size_t afo = 0;
  for (int g = 0; g < n; ++g) {  // one gene at a time: the random stream is consumed in gene order
    if (M[g] < 1 || M[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M[g]);
    rc = rvt_kbac_stage(c, dG[g], M[g], af + afo, yb, nperm, alpha, out + g);
    if (rc) return rc;
    afo += (size_t)M[g];
  }
  return RVT_OK;
}

// ---- MetaScore: single-variant score statistics of a block of variants (unrelated samples) -----------------
// The block as slices through run_batch and the score finisher; with proto.wald the linear Wald finisher instead (outputs
// d per column).  proto holds the host destinations of column 0.
static int score_slices(rvt_ctx* c, const double* dG, int V, const CovOut& proto) {
  int rc = rvt_sync(c);  // processed synchronously
  if (rc) return rc;
  // Which slices START on the hard-call kernel: all of them unless the per-column flags of rvt_block_upload_columns say a
  // slice holds something else.  The kernel tests what it reads; a slice it hands back is computed by the fp64 kernel in
  // the same batch (run_batch).
  std::vector<int> colflag;
  bool any_hc = false;
  bool all_hc = block_hard_calls(c, dG, V, &colflag, &any_hc) != 0;
  if (!c->hc_enabled) all_hc = any_hc = false;
  if (c->nc.binary && !(c->d_nulltile_w && c->d_vq)) all_hc = any_hc = false;  // (no digit planes: fp64 kernel)
  if (!all_hc && colflag.empty()) any_hc = false;
  // columns per slice.  General kernel: with M = 32 - (d + 1) the slice and its [X | rr] columns fill exactly two column
  // tiles, tile class (2,2).  Hard-call kernel: the null-model columns have a tile of their own, so a slice is two
  // full genotype tiles (32 columns, class MT = 2) when the whole block qualifies.
  int kSlice = all_hc ? 32 : 32 - (c->nc.d + 1);
  if (const char* e = getenv("RVT_SCORE_SLICE")) kSlice = std::max(1, std::min(64, atoi(e)));
  constexpr int kChunk = 256;  // slices per launch
  const int64_t ld = c->null_ld;
  const size_t d = (size_t)c->nc.d;
  std::vector<double> af((size_t)kSlice * kChunk, 0.01);
  std::vector<rvt_gene_result> rs(kChunk);
  std::vector<unsigned char> shc(kChunk);
  for (int c0 = 0; c0 < V; c0 += kSlice * kChunk) {
    const int cols = std::min(V - c0, kSlice * kChunk), n = (cols + kSlice - 1) / kSlice;
    std::vector<const double*> ptr(n);
    std::vector<int> Ms(n);
    std::vector<int64_t> ids(n);
    for (int g = 0; g < n; ++g) {
      ptr[g] = dG + (size_t)(c0 + g * kSlice) * ld;
      Ms[g] = std::min(kSlice, cols - g * kSlice);
      ids[g] = (int64_t)g * kSlice;
      bool hc = all_hc;
      if (!all_hc && any_hc) {
        hc = true;
        for (int j = 0; j < Ms[g]; ++j) hc = hc && colflag[(size_t)c0 + (size_t)g * kSlice + j] != 0;
      }
      shc[g] = hc ? 1 : 0;
    }
    CovOut co = proto;
    co.score = true;
    co.slice_hc = any_hc ? shc.data() : nullptr;
    co.ok = proto.ok + c0;
    if (proto.wald) {
      co.wbeta = proto.wbeta + (size_t)c0 * d;
      co.wse = proto.wse + (size_t)c0 * d;
      co.wpval = proto.wpval + (size_t)c0 * d;
    } else {
      co.ustat = proto.ustat + c0;
      co.vstat = proto.vstat + c0;
      co.effect = proto.effect + c0;
      co.se = proto.se + c0;
      co.pval = proto.pval + c0;
    }
    rc = run_batch(c, n, ptr.data(), Ms.data(), af.data(), ids.data(), 0u, nullptr, rs.data(), nullptr, &co);
    if (rc) return rc;
  }
  return RVT_OK;
}

// rvt_score_block behind its argument checks (rvt_burden_blocks runs the Fp columns through it)
static int score_block_impl(rvt_ctx* c, const double* dG, int V, int* ok, double* ustat, double* vstat, double* effect,
                            double* effect_se, double* pvalue) {
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  CovOut co;
  co.ok = ok;
  co.ustat = ustat;
  co.vstat = vstat;
  co.effect = effect;
  co.se = effect_se;
  co.pval = pvalue;
  return score_slices(c, dG, V, co);
}

int rvt_score_block(rvt_ctx* c, const double* dG, int V, int* ok, double* ustat, double* vstat, double* effect,
                    double* effect_se, double* pvalue) {
  if (!c || !dG || V < 1 || !ok || !ustat || !vstat || !effect || !effect_se || !pvalue)
    return fail(c, RVT_E_INVALID, "bad arguments");
  return score_block_impl(c, dG, V, ok, ustat, vstat, effect, effect_se, pvalue);
}

// ---- SingleVariantWaldTest: the full regression of every column of a block on [1, g, cov] ----------------------------
// (behind its argument checks: rvt_burden_blocks runs the collapsed columns through wald_block_impl)
static int wald_block_impl(rvt_ctx* c, const double* dG, int V, int* ok, double* beta, double* se, double* pvalue, int* rounds);
int rvt_wald_block(rvt_ctx* c, const double* dG, int V, int* ok, double* beta, double* se, double* pvalue, int* rounds) {
  if (!c || !dG || V < 1 || !ok || !beta || !se || !pvalue) return fail(c, RVT_E_INVALID, "bad arguments");
  return wald_block_impl(c, dG, V, ok, beta, se, pvalue, rounds);
}
static int wald_block_impl(rvt_ctx* c, const double* dG, int V, int* ok, double* beta, double* se, double* pvalue, int* rounds) {
  using namespace rvt_wald;
  if (!c->have_null || !c->have_null_beta) return fail(c, RVT_E_STATE, "no null model fitted by rvt_fit_null");
  const NullConsts& nc = c->nc;
  const int d = nc.d;
  if (!nc.binary) {  // closed form of the score partials (wald_linear_finish_kernel)
    CovOut co;
    co.wald = true;
    for (int k = 0; k < d; ++k) co.wald_beta0[k] = c->null_beta[k];
    co.ok = ok;
    co.wbeta = beta;
    co.wse = se;
    co.wpval = pvalue;
    int rc = score_slices(c, dG, V, co);
    if (rc == RVT_OK && rounds) std::fill(rounds, rounds + V, 0);
    return rc;
  }
  if (!c->d_null_y) return fail(c, RVT_E_STATE, "no binary null model fitted by rvt_fit_null");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = nc.N, ld = c->null_ld;
  const int P = d + 1, E = wald_entries(P);
  const int n_chunks = (int)((N + kWaldChunk - 1) / kWaldChunk);
  constexpr int kBatch = 4096;  // variants per launch chunk
  const int Vb = std::min(V, kBatch);
  // work space: beta | last deviance | beta, se, p out | chunk partials | iteration | two lists | ok | rounds | two counters
  Layout L;
  const size_t o_beta = L.take(sizeof(double) * (size_t)Vb * kWaldMaxP), o_last = L.take(sizeof(double) * (size_t)Vb);
  const size_t o_ob = L.take(sizeof(double) * (size_t)Vb * d), o_os = L.take(sizeof(double) * (size_t)Vb * d),
               o_op = L.take(sizeof(double) * (size_t)Vb * d);
  const size_t o_part = L.take(sizeof(double) * (size_t)Vb * n_chunks * E);
  const size_t o_iter = L.take(sizeof(int) * (size_t)Vb), o_l0 = L.take(sizeof(int) * (size_t)Vb),
               o_l1 = L.take(sizeof(int) * (size_t)Vb), o_ok = L.take(sizeof(int) * (size_t)Vb),
               o_rounds = L.take(sizeof(int) * (size_t)Vb), o_cnt = L.take(sizeof(int) * 2);
  HIP_TRY(c, c->d_wald_ws.grow(L.total, L.total, st, true));
  char* ws = c->d_wald_ws;
  double* d_beta = reinterpret_cast<double*>(ws + o_beta);
  double* d_last = reinterpret_cast<double*>(ws + o_last);
  double* d_ob = reinterpret_cast<double*>(ws + o_ob);
  double* d_os = reinterpret_cast<double*>(ws + o_os);
  double* d_op = reinterpret_cast<double*>(ws + o_op);
  double* d_part = reinterpret_cast<double*>(ws + o_part);
  int* d_iter = reinterpret_cast<int*>(ws + o_iter);
  int* d_list[2] = {reinterpret_cast<int*>(ws + o_l0), reinterpret_cast<int*>(ws + o_l1)};
  int* d_ok = reinterpret_cast<int*>(ws + o_ok);
  int* d_rounds = reinterpret_cast<int*>(ws + o_rounds);
  int* d_cnt = reinterpret_cast<int*>(ws + o_cnt);
  for (int c0 = 0; c0 < V; c0 += kBatch) {
    const int nb = std::min(kBatch, V - c0);
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * 2, st));
    hipLaunchKernelGGL(wald_logistic_init_kernel, dim3((unsigned)nb), dim3(256), 0, st, dG, (long long)ld, c0, (long long)N, d,
                       d_beta, d_last, d_iter, d_list[0], d_cnt, d_ok, d_rounds, d_ob, d_os, d_op);
    HIP_TRY(c, hipGetLastError());
    int n_active = 0, cur = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_active, d_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    for (int round = 0; n_active > 0 && round < kWaldRounds; ++round) {
      const int nxt = 1 - cur;
      hipLaunchKernelGGL(wald_logistic_round_kernel, dim3((unsigned)((n_active + kWaldSlice - 1) / kWaldSlice), (unsigned)n_chunks),
                         dim3(256), wald_round_lds_bytes(d), st, dG, (long long)ld, c0, c->d_X, c->d_null_y, (long long)N, d, d_list[cur], n_active,
                         d_beta, n_chunks, d_part);
      HIP_TRY(c, hipMemsetAsync(d_cnt + nxt, 0, sizeof(int), st));
      hipLaunchKernelGGL(wald_logistic_step_kernel, dim3((unsigned)((n_active + 63) / 64)), dim3(64), 0, st, d_list[cur], n_active, d,
                         n_chunks, d_part, d_beta, d_last, d_iter, d_list[nxt], d_cnt + nxt, d_ok, d_rounds, d_ob, d_os, d_op);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(&n_active, d_cnt + nxt, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, sync_stream(st));
      cur = nxt;
    }
    if (n_active > 0) return fail(c, RVT_E_HIP, "logistic Wald fits did not end in %d rounds", kWaldRounds);
    const size_t vd = sizeof(double) * (size_t)nb * d;
    HIP_TRY(c, hipMemcpyAsync(ok + c0, d_ok, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, st));
    if (rounds) HIP_TRY(c, hipMemcpyAsync(rounds + c0, d_rounds, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(beta + (size_t)c0 * d, d_ob, vd, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(se + (size_t)c0 * d, d_os, vd, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(pvalue + (size_t)c0 * d, d_op, vd, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
  }
  return RVT_OK;
}

// ---- --burden cmcWald / zegginiWald / fp / exactCMC: the analytic burden tests of a batch of device-resident genes ---------------
// (CMCWaldTest, ZegginiWaldTest, CMCFisherExactTest src/Model.h:909-1168, FpTest :1344-1417)
// The flip / keep decisions of every column of the batch come from fam_colstat_kernel (what flipped_poly_block uses); the host
// turns them into the kept-column lists and the Fp weights (af indexed by the FILTERED column, quirk #3); burden_columns_kernel
// then streams every gene once and writes its collapsed columns; the fits run once per chunk of genes on the N x n blocks.
// genes per chunk: three blocks of at most 256 MB each, at least 16 and at most 1024 genes (67 at N = 500 000).  RVT_BURDEN_CHUNK
// sets it (read per call: the tests run a batch in several chunks with it).
static int burden_chunk_genes(int64_t ld) {
  if (const char* e = getenv("RVT_BURDEN_CHUNK")) return std::max(1, std::min(1024, atoi(e)));
  return (int)std::max<int64_t>(16, std::min<int64_t>(1024, ((int64_t)256 << 20) / (int64_t)(sizeof(double) * ld)));
}

int rvt_burden_blocks(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* af, const double* y, uint32_t which,
                      rvt_burden_more_result* out) {
  constexpr uint32_t kAll = RVT_BURDEN_CMCWALD | RVT_BURDEN_ZEGGINIWALD | RVT_BURDEN_FP | RVT_BURDEN_EXACTCMC;
  if (!c || n < 0 || (n > 0 && (!dG || !M || !af || !out)) || which == 0 || (which & ~kAll) || ((which & RVT_BURDEN_EXACTCMC) && !y))
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  const bool want_cmc = which & RVT_BURDEN_CMCWALD, want_zeg = which & RVT_BURDEN_ZEGGINIWALD, want_fp = which & RVT_BURDEN_FP,
             want_exact = which & RVT_BURDEN_EXACTCMC;
  if ((want_cmc || want_zeg) && (!c->have_null_beta || (c->nc.binary && !c->d_null_y)))
    return fail(c, RVT_E_STATE, "no null model fitted by rvt_fit_null");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  c->burden_cols_n = 0;
  if (n == 0) return RVT_OK;
  hipStream_t st = c->stream;
  const int64_t N = c->nc.N, ld = c->null_ld;
  const int d = c->nc.d;
  size_t T = 0;
  for (int g = 0; g < n; ++g) {
    if (M[g] < 1 || M[g] > RVT_MAX_VARIANTS) return fail(c, RVT_E_INVALID, "gene %d has M=%d", g, M[g]);
    if (!dG[g]) return fail(c, RVT_E_INVALID, "gene %d has no block", g);
    T += (size_t)M[g];
  }
  // exactCMC: a 0 / 1 phenotype, a binary null model without covariates (src/Model.h:1099-1116)
  bool exact_valid = want_exact && c->nc.binary && d == 1;
  if (exact_valid)
    for (int64_t i = 0; i < N && exact_valid; ++i) exact_valid = y[i] == 0.0 || y[i] == 1.0;
  std::memset(out, 0, sizeof(*out) * (size_t)n);
  for (int g = 0; g < n; ++g) {
    out[g].fp_pvalue = out[g].exact_p_two = out[g].exact_p_less = out[g].exact_p_greater = 1.0;
    for (int k = 0; k < RVT_MAX_COV; ++k) out[g].cmc_wald.pvalue[k] = out[g].zeggini_wald.pvalue[k] = 1.0;
  }
  // ---- flip / keep flags of all T columns --------------------------------------------------------------------------------------
  std::vector<const double*> cols(T);
  {
    size_t t = 0;
    for (int g = 0; g < n; ++g)
      for (int j = 0; j < M[g]; ++j) cols[t++] = dG[g] + (size_t)j * ld;
  }
  const int nchunk = std::min(n, burden_chunk_genes(ld));
  Layout L;
  const size_t o_cols = L.take(sizeof(double*) * T), o_flags = L.take(sizeof(int) * T), o_kc = L.take(sizeof(int) * T),
               o_kw = L.take(sizeof(double) * T), o_genes = L.take(sizeof(BurdenColGene) * (size_t)n),
               o_cnt = L.take(sizeof(int) * (size_t)n * kBurdenColCounters), o_pv = L.take(sizeof(double) * (size_t)n * 3),
               o_y = L.take(sizeof(double) * (size_t)N);
  HIP_TRY(c, c->d_burden_ws.grow(L.total, L.total + L.total / 4, st, true));
  char* ws = c->d_burden_ws;
  const double** d_cols = reinterpret_cast<const double**>(ws + o_cols);
  int* d_flags = reinterpret_cast<int*>(ws + o_flags);
  int* d_kc = reinterpret_cast<int*>(ws + o_kc);
  double* d_kw = reinterpret_cast<double*>(ws + o_kw);
  BurdenColGene* d_genes = reinterpret_cast<BurdenColGene*>(ws + o_genes);
  int* d_cnt = reinterpret_cast<int*>(ws + o_cnt);
  double* d_pv = reinterpret_cast<double*>(ws + o_pv);
  double* d_y = reinterpret_cast<double*>(ws + o_y);
  std::vector<int> flags(T);
  HIP_TRY(c, hipMemcpyAsync(d_cols, cols.data(), sizeof(double*) * T, hipMemcpyHostToDevice, st));
  for (size_t t0 = 0; t0 < T; t0 += 65535) {
    const size_t nt = std::min<size_t>(65535, T - t0);
    k_fam_colstat(dim3((unsigned)nt), st, d_cols + t0, (long long)N, d_flags + t0);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * T, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  // ---- the kept columns of every gene and their Fp weights -------------------------------------------------------------------------
  std::vector<int> kc;
  std::vector<double> kw;
  std::vector<BurdenColGene> genes((size_t)n);
  kc.reserve(T), kw.reserve(T);
  {
    size_t t = 0;
    for (int g = 0; g < n; ++g) {
      genes[g].G = dG[g];
      genes[g].kept0 = (int)kc.size();
      int m = 0;
      for (int j = 0; j < M[g]; ++j) {
        const int f = flags[t + j];
        if (!(f & 2)) continue;
        const double freq = af[t + m];  // dc->getMarkerFrequency(m) of the filtered column m (fpCollapse, src/Model.cpp:188)
        kc.push_back(j | ((f & 1) ? 0x40000000 : 0));
        kw.push_back((freq <= 0.0 || freq >= 1.0) ? 0.0 : 1.0 / sqrt(freq * (1.0 - freq)));
        ++m;
      }
      genes[g].m = m;
      out[g].n_poly = m;
      t += (size_t)M[g];
    }
  }
  if (!kc.empty()) {
    HIP_TRY(c, hipMemcpyAsync(d_kc, kc.data(), sizeof(int) * kc.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_kw, kw.data(), sizeof(double) * kw.size(), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemcpyAsync(d_genes, genes.data(), sizeof(BurdenColGene) * (size_t)n, hipMemcpyHostToDevice, st));
  if (exact_valid) HIP_TRY(c, hipMemcpyAsync(d_y, y, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)n * kBurdenColCounters, st));
  // ---- the collapsed blocks of a chunk of genes, then the fits on them ---------------------------------------------------------------
  const int n_blocks = (want_cmc ? 1 : 0) + (want_zeg ? 1 : 0) + (want_fp ? 1 : 0);
  const size_t blk = (size_t)ld * (size_t)nchunk;
  if (n_blocks) HIP_TRY(c, c->d_burden_cols.grow(sizeof(double) * blk * n_blocks, sizeof(double) * blk * n_blocks, st, true));
  double *d_cmc = nullptr, *d_zeg = nullptr, *d_fp = nullptr;
  {
    double* q = c->d_burden_cols;
    if (want_cmc) d_cmc = q, q += blk;
    if (want_zeg) d_zeg = q, q += blk;
    if (want_fp) d_fp = q, q += blk;
  }
  std::vector<int> ok((size_t)nchunk), rounds((size_t)nchunk), cnt((size_t)nchunk * kBurdenColCounters);
  std::vector<double> b((size_t)nchunk * d), s((size_t)nchunk * d), p((size_t)nchunk * d), pv((size_t)nchunk * 3);
  std::vector<double> us((size_t)nchunk), vs((size_t)nchunk), ef((size_t)nchunk), es((size_t)nchunk), ps((size_t)nchunk);
  const unsigned parts = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (ld / 2 + 255) / 256));
  for (int g0 = 0; g0 < n; g0 += nchunk) {
    const int ng = std::min(nchunk, n - g0);
    hipLaunchKernelGGL(burden_columns_kernel, dim3(parts, (unsigned)ng), dim3(256), 0, st, d_genes + g0, d_kc, d_kw, (long long)N,
                       (long long)ld, exact_valid ? d_y : (const double*)nullptr, d_cmc, d_zeg, d_fp,
                       d_cnt + (size_t)g0 * kBurdenColCounters);
    if (exact_valid)
      hipLaunchKernelGGL(fisher_2x2_kernel, dim3((unsigned)ng), dim3(256), 0, st, d_cnt + (size_t)g0 * kBurdenColCounters, ng, d_pv);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt + (size_t)g0 * kBurdenColCounters, sizeof(int) * (size_t)ng * kBurdenColCounters,
                              hipMemcpyDeviceToHost, st));
    if (exact_valid) HIP_TRY(c, hipMemcpyAsync(pv.data(), d_pv, sizeof(double) * (size_t)ng * 3, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    c->burden_cols_n = ng, c->burden_cols_which = which, c->burden_cols_chunk = nchunk, c->burden_cols_gen = c->null_gen;
    for (int g = 0; g < ng; ++g) {
      rvt_burden_more_result& r = out[g0 + g];
      const int* q = cnt.data() + (size_t)g * kBurdenColCounters;
      r.nonref_site = q[0];
      if (exact_valid && r.n_poly > 0) {
        r.exact_ok = 1;
        r.n00 = q[1], r.n01 = q[2], r.n10 = q[3], r.n11 = q[4];
        r.exact_p_two = pv[(size_t)g * 3], r.exact_p_less = pv[(size_t)g * 3 + 1], r.exact_p_greater = pv[(size_t)g * 3 + 2];
      }
    }
    for (int w = 0; w < 2; ++w) {
      const double* blkp = w == 0 ? d_cmc : d_zeg;
      if (!blkp) continue;
      rc = wald_block_impl(c, blkp, ng, ok.data(), b.data(), s.data(), p.data(), rounds.data());
      if (rc) return rc;
      for (int g = 0; g < ng; ++g) {
        rvt_burden_more_result& r = out[g0 + g];
        rvt_burden_wald_fit& f = w == 0 ? r.cmc_wald : r.zeggini_wald;
        if (r.n_poly == 0) continue;  // genotype.cols == 0: nothing is fitted
        f.rounds = rounds[g];
        if (ok[g] != 1) continue;     // a constant collapsed column or a failed fit
        f.ok = 1;
        for (int k = 0; k < d; ++k) f.beta[k] = b[(size_t)g * d + k], f.se[k] = s[(size_t)g * d + k], f.pvalue[k] = p[(size_t)g * d + k];
      }
    }
    if (d_fp) {
      rc = score_block_impl(c, d_fp, ng, ok.data(), us.data(), vs.data(), ef.data(), es.data(), ps.data());
      if (rc) return rc;
      for (int g = 0; g < ng; ++g) {
        rvt_burden_more_result& r = out[g0 + g];
        if (r.n_poly == 0 || !ok[g]) continue;
        r.fp_ok = 1;
        r.fp_u = us[g], r.fp_v = vs[g], r.fp_pvalue = ps[g];
      }
    }
  }
  return RVT_OK;
}

// Tests: column-major N x n copy of one collapsed block the last rvt_burden_blocks call of this context left on the device
// (test = RVT_BURDEN_CMCWALD, _ZEGGINIWALD or _FP; n = the genes of the call's LAST chunk: all of them for a call of at most 16
// genes, and whenever the call fits one chunk of burden_chunk_genes — 256 MB per block, 1024 genes at the most)
int rvt_burden_last_columns(rvt_ctx* c, uint32_t test, int n, double* cols) {
  if (!c || !cols || n < 1) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null || c->burden_cols_gen != c->null_gen || n != c->burden_cols_n || !(c->burden_cols_which & test) ||
      (test != RVT_BURDEN_CMCWALD && test != RVT_BURDEN_ZEGGINIWALD && test != RVT_BURDEN_FP))
    return fail(c, RVT_E_STATE, "no such block from the last rvt_burden_blocks call");
  const int64_t N = c->nc.N, ld = c->null_ld;
  const uint32_t w = c->burden_cols_which;
  int idx = 0;  // blocks lie in the order cmc, zeggini, fp, those asked for only
  if (test != RVT_BURDEN_CMCWALD && (w & RVT_BURDEN_CMCWALD)) ++idx;
  if (test == RVT_BURDEN_FP && (w & RVT_BURDEN_ZEGGINIWALD)) ++idx;
  const int nchunk = c->burden_cols_chunk;
  const double* src = c->d_burden_cols.get() + (size_t)idx * (size_t)ld * nchunk;
  HIP_TRY(c, hipMemcpy2D(cols, sizeof(double) * (size_t)N, src, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)N, (size_t)n,
                         hipMemcpyDeviceToHost));
  return RVT_OK;
}

int rvt_null_dims(rvt_ctx* c, int64_t* N, int* d) {
  if (!c) return RVT_E_INVALID;
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  if (N) *N = c->nc.N;
  if (d) *d = c->nc.d;
  return RVT_OK;
}

int rvt_null_summary(rvt_ctx* c, double* beta, double* covb_diag, double* sigma2) {
  if (!c || !covb_diag) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  const NullConsts& nc = c->nc;
  if (beta)
    for (int k = 0; k < nc.d; ++k) beta[k] = c->have_null_beta ? c->null_beta[k] : NAN;
  for (int k = 0; k < nc.d; ++k) covb_diag[k] = nc.Cinv[k * nc.d + k] * (nc.binary ? 1.0 : nc.sigma2);
  if (sigma2) *sigma2 = nc.sigma2;
  return RVT_OK;
}

// ---- MetaCov: covariance band of one block of consecutive variants ---------------------------------------
static int cov_rect_impl(rvt_ctx* c, const double* dG, int col0, int H, int W, double* cov, double* xz, double* zz,
                         int* polymorphic, bool allow_fast);
int rvt_cov_block(rvt_ctx* c, const double* dG, int V, double* cov, double* xz, double* zz, int* polymorphic) {
  if (!c || !dG || V < 1 || !cov || !xz || !polymorphic) return fail(c, RVT_E_INVALID, "bad arguments");
  if (V > RVT_MAX_VARIANTS) return fail(c, RVT_E_TOO_LARGE, "block of %d variants exceeds RVT_MAX_VARIANTS", V);
  int rc = rvt_sync(c);  // the block is processed alone and synchronously
  if (rc) return rc;
  // Hard calls and an unweighted model: G'G is an integer matrix — the band comes from the exact int8 product
  // (rvt_cov_rect with heads = window) instead of the fp64 matrix cores, ~6x faster at V = 1024.
  if (c->have_null && !c->nc.binary && V >= 64 && !getenv("RVT_METACOV_FP64") && block_hard_calls(c, dG, V, nullptr, nullptr))
    return rvt_cov_rect(c, dG, 0, V, V, cov, xz, zz, polymorphic);  // (tests what it reads; falls back by itself)
  // Anything else — dosages, or a binary trait's weights: the LDS-tiled fp64 product (gemm_f64.hip.h) from V = 64 on;
  // RVT_METACOV_PANEL=1 keeps round 4's path through the one-wave sufficient-statistics kernel (22 TFLOP/s at V = 1024)
  if (c->have_null && V >= 64 && !getenv("RVT_METACOV_PANEL")) return cov_rect_impl(c, dG, 0, V, V, cov, xz, zz, polymorphic, false);
  std::vector<double> af(V, 0.01);
  rvt_gene_result r;
  CovOut co;
  co.cov = cov;
  co.xz = xz;
  co.zz = zz;
  co.poly = polymorphic;
  const double* p = dG;
  rc = run_batch(c, 1, &p, &V, af.data(), nullptr, 0u, nullptr, &r, nullptr, &co);
  if (rc) return rc;
  // run_batch marked the slot busy without enqueuing a record copy: clear it
  for (auto& sl : c->slots) {
    if (sl.pending_out == &r) {
      sl.pending_out = nullptr;
      sl.pending_n = 0;
    }
  }
  return RVT_OK;
}

static int cov_rect_impl(rvt_ctx* c, const double* dG, int col0, int H, int W, double* cov, double* xz, double* zz,
                         int* polymorphic, bool allow_fast);
int rvt_cov_rect(rvt_ctx* c, const double* dG, int col0, int H, int W, double* cov, double* xz, double* zz,
                 int* polymorphic) {
  return cov_rect_impl(c, dG, col0, H, W, cov, xz, zz, polymorphic, true);
}
static int cov_rect_impl(rvt_ctx* c, const double* dG, int col0, int H, int W, double* cov, double* xz, double* zz,
                         int* polymorphic, bool allow_fast) {
  if (!c || !dG || col0 < 0 || H < 1 || W < H || !cov || !xz || !polymorphic)
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const NullConsts& nc = c->nc;
  const int64_t N = nc.N, ld = nc.ld;
  const int d = nc.d;
  CovConsts cc;
  std::vector<double> zzv;
  rc = cov_constants(c, false, &cc, &zzv);
  if (rc) return rc;
  const double* GW = dG + (size_t)col0 * ld;
  // work space: one grow-only allocation of the context (a window walk calls this per eviction: six hipMalloc / hipFree
  // pairs per call cost more than the kernels of a small window)
  double *d_S = nullptr, *d_T = nullptr, *d_cs = nullptr, *d_xz = nullptr, *d_cov = nullptr, *d_tmp = nullptr;
  int* d_poly = nullptr;
  {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t bS = up(sizeof(double) * (size_t)H * (W + d)), bC = up(sizeof(double) * (size_t)H * W),
                 bT = up(sizeof(double) * (size_t)W * d), bV = up(sizeof(double) * (size_t)W), bP = up(sizeof(int) * (size_t)W);
    const size_t bM = up(sizeof(double) * (size_t)64 * W * (RVT_MAX_COV + 3));   // slice partials of the column pass (<= 64 slices)
    const size_t need = bS + bC + 2 * bT + bV + bP + bM;
    HIP_TRY(c, c->d_cov_work.grow(need, need + need / 4, st, true));
    char* q = c->d_cov_work;
    d_S = reinterpret_cast<double*>(q);      // H x (W + d): T sits behind S when heads = window
    q += bS;
    d_cov = reinterpret_cast<double*>(q);
    q += bC;
    d_T = reinterpret_cast<double*>(q);
    q += bT;
    d_xz = reinterpret_cast<double*>(q);
    q += bT;
    d_cs = reinterpret_cast<double*>(q);
    q += bV;
    d_poly = reinterpret_cast<int*>(q);
    q += bP;
    d_tmp = reinterpret_cast<double*>(q);
  }
  const double* T_used = d_T;
  // T = G_W' D X (W x d) and S = G_H' D G_W (H x W): for a hard-call block under an unweighted model the exact integer
  // product of rot_gemm.hip.h, else the fp64 matrix cores (round 4 quantised such operands to six digit planes, 36
  // int8 products, ~2^-40 relative)
  // (hard calls are a prediction — the engine's own per-column flags when it filled the block, optimism otherwise —
  // that cov_hc_prep_kernel verifies on every value it converts; a block that fails is computed again the general way)
  // (round 5: rectangles too — heads against a wider window, as the adapter's ring hands them over from 1 025 columns on)
  const bool fast = allow_fast && !nc.binary && W >= 64 && block_hard_calls(c, dG, col0 + W, nullptr, nullptr) != 0;
  int* d_bad = nullptr;
  int h_bad = 0;
  // one pass over the window's columns for the column statistics and T = G_W' D X (and, on the hard-call path, the int8
  // copy): rows sliced across workgroups, partial results added in a fixed order
  const int dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
  const int wgs = (W + kCovHcCols - 1) / kCovHcCols;
  // (the slice count depends on N alone: a column's sums then come out the same whether the column is treated with 1 023
  //  others here or alone behind its upload, rvt_block_upload_columns)
  const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(kCovSlices, N / 4096 + 1));
  if (!fast) {
    const dim3 grid((unsigned)wgs, (unsigned)slices);
    const double* wts = nc.binary ? c->d_v : nullptr;
    if (dmax == 4)
      hipLaunchKernelGGL((cov_hc_prep_kernel<4, false>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W, c->d_X,
                         (long long)ld, d, (signed char*)nullptr, 0LL, d_tmp, (int*)nullptr, wts);
    else if (dmax == 8)
      hipLaunchKernelGGL((cov_hc_prep_kernel<8, false>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W, c->d_X,
                         (long long)ld, d, (signed char*)nullptr, 0LL, d_tmp, (int*)nullptr, wts);
    else
      hipLaunchKernelGGL((cov_hc_prep_kernel<RVT_MAX_COV, false>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W,
                         c->d_X, (long long)ld, d, (signed char*)nullptr, 0LL, d_tmp, (int*)nullptr, wts);
    hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((W * (dmax + 3) + 255) / 256)), dim3(256), 0, st, d_tmp, slices,
                       W, d, dmax, d_cs, d_poly, d_T);
  }
  // the block's own column cache (rvt_block_upload_columns made it behind the PCIe copies): every column of the window has its
  // int8 copy, sum, flag and row of T under THIS null model -> the call starts at the integer product
  // (state 1 only; 2 = hard calls + an other value: MXFP4 band only)
  const ColKind* ckc = fast ? usable_cache(c, dG, 0, col0, W, false, nullptr) : nullptr;
  if (fast && ckc) {
    const int64_t ldk = ckc->ldk;
    hipLaunchKernelGGL(cov_cache_gather_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, ckc->d_cs + col0,
                       ckc->d_poly + col0, ckc->d_T + (size_t)col0 * RVT_MAX_COV, W, d, RVT_MAX_COV, d_cs, d_poly, d_T);
    const signed char* A8 = ckc->d_i8 + (size_t)col0 * (size_t)ldk;
    std::vector<int> zero_exp((size_t)W, 0);
    rc = rvt_planes_gemm(c, A8, 0, 1, H, zero_exp.data(), 0, A8, 0, 1, W, zero_exp.data(), N, ldk, d_S, H, st);
    if (rc) return rc;
  } else if (fast) {
    // a hard-call block (rvt_cov_block's fast path; heads = the first H of the W columns): ONE pass over G gives the column
    // statistics, T = G'X and the int8 copy (cov_hc_prep_kernel); S = G'G is then one exact integer product
    const int64_t ldk = (N + 127) / 128 * 128;
    const int64_t cols_pad = ((int64_t)W + kRotBM - 1) / kRotBM * kRotBM;
    const size_t need = (size_t)cols_pad * (size_t)ldk;
    HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
    // the product reads cols_pad columns of ldk bytes: the column pass writes the W columns' rows up to N rounded to 4 — only
    // the pad rows behind them and the pad columns have to be zeroed (the whole 0.5 GB copy cost 0.1 ms of a 2.3 ms block)
    {
      const int64_t n4 = (N + 3) / 4 * 4;
      if (ldk > n4)
        HIP_TRY(c, hipMemset2DAsync(c->d_rotB + n4, (size_t)ldk, 0, (size_t)(ldk - n4), (size_t)W, st));
      if (cols_pad > W) HIP_TRY(c, hipMemsetAsync(c->d_rotB + (size_t)W * ldk, 0, (size_t)(cols_pad - W) * (size_t)ldk, st));
    }
    HIP_TRY(c, c->d_kind.grow(sizeof(int), sizeof(int), st, true));
    d_bad = c->d_kind;
    HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(int), st));
    {
      const dim3 grid((unsigned)wgs, (unsigned)slices);
      if (dmax == 4)
        hipLaunchKernelGGL((cov_hc_prep_kernel<4>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W, c->d_X,
                           (long long)ld, d, c->d_rotB, (long long)ldk, d_tmp, d_bad);
      else if (dmax == 8)
        hipLaunchKernelGGL((cov_hc_prep_kernel<8>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W, c->d_X,
                           (long long)ld, d, c->d_rotB, (long long)ldk, d_tmp, d_bad);
      else
        hipLaunchKernelGGL((cov_hc_prep_kernel<RVT_MAX_COV>), grid, dim3(256), 0, st, GW, (long long)N, (long long)ld, W,
                           c->d_X, (long long)ld, d, c->d_rotB, (long long)ldk, d_tmp, d_bad);
      hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((W * (dmax + 3) + 255) / 256)), dim3(256), 0, st, d_tmp, slices,
                         W, d, dmax, d_cs, d_poly, d_T);
    }
    std::vector<int> zero_exp((size_t)W, 0);
    rc = rvt_planes_gemm(c, c->d_rotB, need, 1, H, zero_exp.data(), 0, c->d_rotB, need, 1, W, zero_exp.data(), N, ldk, d_S, H, st);
    if (rc) return rc;
  } else {
    // anything else — dosages, a binary trait's weights — on the fp64 matrix cores (gemm_f64.hip.h): the upper triangle of
    // S = G_H' D G_W
    // (T came out of the pass above: a 128-column tile for d columns of X would cost as much as a whole tile of S)
    const double* wts = nc.binary ? c->d_v : nullptr;
    rc = gemm_tn_f64(c, GW, ld, H, GW, ld, W, nullptr, 0, 0, wts, N, d_S, H, true, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(cov_rect_xz_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, cc, T_used, d_cs, W, d_xz);
  // (the rows kernel writes cov[h, j] for j >= h only, and the whole rectangle goes to the caller: zeros below the diagonal,
  //  not what an earlier call left in the work space)
  HIP_TRY(c, hipMemsetAsync(d_cov, 0, sizeof(double) * (size_t)H * W, st));
  hipLaunchKernelGGL(cov_rect_rows_kernel, dim3((unsigned)H), dim3(256), 0, st, cc, d_S, d_cs, d_xz, H, W, d_cov);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)H * W, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(xz, d_xz, sizeof(double) * (size_t)W * d, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(polymorphic, d_poly, sizeof(int) * (size_t)W, hipMemcpyDeviceToHost, st));
  if (d_bad) HIP_TRY(c, hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  if (h_bad) return cov_rect_impl(c, dG, col0, H, W, cov, xz, zz, polymorphic, false);  // not hard calls after all
  if (zz) std::memcpy(zz, zzv.data(), sizeof(double) * (size_t)d * d);
  return RVT_OK;
}



// one launch of MetaCov's column pass (cov_hc_prep_kernel) for d covariates; pack: the hard-call variant (value test, int8 / E2M1
// copies), else the general one (optional weights)
static void launch_cov_prep(hipStream_t st, int d, bool pack, dim3 grid, const double* G, int64_t N, int64_t ld, int W, const double* X,
                            signed char* out8, int64_t ldk, double* part, int* bad, const double* wts, int* hard_flag, int ring,
                            int col0, unsigned char* out4, int64_t ldk4, const double* mu_known = nullptr,
                            unsigned char* out4m = nullptr) {
  const int dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
#define RVT_PREP(DM, PK)                                                                                                          \
  hipLaunchKernelGGL((cov_hc_prep_kernel<DM, PK>), grid, dim3(256), 0, st, G, (long long)N, (long long)ld, W, X, (long long)ld, d, \
                     out8, (long long)ldk, part, bad, wts, hard_flag, ring, col0, out4, (long long)ldk4, mu_known, out4m)
  if (pack) {
    if (dmax == 4) RVT_PREP(4, true);
    else if (dmax == 8) RVT_PREP(8, true);
    else RVT_PREP(RVT_MAX_COV, true);
  } else {
    if (dmax == 4) RVT_PREP(4, false);
    else if (dmax == 8) RVT_PREP(8, false);
    else RVT_PREP(RVT_MAX_COV, false);
  }
#undef RVT_PREP
}

// ---- MetaCov on a circular ring: the band of a sliding window ----------------------------------------------------------------
// flags of the W logical columns of a ring (physical (col0 + j) mod ring): 1 = every column holds hard calls only, 0 = some
// column holds something else, -1 = nothing known about the block
// (masked_ok: the block's per-column cache states — a column in state 2, hard calls plus ONE other value known from its packed
//  upload, counts as usable although its content flag says "not hard calls only")
static int ring_hard_calls(rvt_ctx* c, const double* dG, int ring, int col0, int W, const unsigned char* masked_ok = nullptr) {
  if (!c->hc_enabled) return 0;
  const ColKind* ck = find_block(c, dG);
  const int span = ring > 0 ? ring : col0 + W;
  if (!ck || !ck->d_flags || span > ck->cols) return c->content_hint == 0 ? 0 : -1;
  std::vector<int> f((size_t)span);
  if (hipMemcpyAsync(f.data(), ck->d_flags, sizeof(int) * (size_t)span, hipMemcpyDeviceToHost, c->io_stream) != hipSuccess ||
      sync_stream(c->io_stream) != hipSuccess)
    return 0;
  for (int j = 0; j < W; ++j) {
    int p = col0 + j;
    if (ring > 0 && p >= ring) p -= ring;
    if (!f[(size_t)p] && !(masked_ok && masked_ok[(size_t)p] == 2)) return 0;
  }
  return 1;
}

// The work space of a band call (c->d_cov_work), shared by rvt_cov_band and rvt_cov_band_bed_dev: T and covXZ of the W markers,
// their sums, imputation values and flags, the column pass's partial results, two band buffers of Hp heads and — for the fp64
// product — the rectangle of one pass; `extra` bytes behind them for the caller's own use.
struct BandWork {
  double *d_T = nullptr, *d_xz = nullptr, *d_cs = nullptr, *d_mu_l = nullptr, *d_tmp = nullptr, *d_S = nullptr;
  float* d_band = nullptr;
  int* d_poly = nullptr;
  char* extra = nullptr;
};
static int band_work(rvt_ctx* c, hipStream_t st, int W, int d, int Hp, int Wp, int halo, bool fast, size_t extra, BandWork* w) {
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t bT = up(sizeof(double) * (size_t)W * d), bV = up(sizeof(double) * (size_t)W), bP = up(sizeof(int) * (size_t)W);
  const size_t bM = up(sizeof(double) * (size_t)kCovSlices * W * (RVT_MAX_COV + 3));
  const size_t bB = 2 * up(sizeof(float) * (size_t)Hp * ((size_t)halo + 1));
  const size_t bS = fast ? 0 : up(sizeof(double) * (size_t)Hp * Wp);
  const size_t need = 2 * bT + 2 * bV + bP + bM + bB + bS + extra;
  HIP_TRY(c, c->d_cov_work.grow(need, need + need / 4, st, true));
  char* q = c->d_cov_work;
  w->d_T = reinterpret_cast<double*>(q);
  q += bT;
  w->d_xz = reinterpret_cast<double*>(q);
  q += bT;
  w->d_cs = reinterpret_cast<double*>(q);
  q += bV;
  w->d_mu_l = reinterpret_cast<double*>(q);
  q += bV;
  w->d_poly = reinterpret_cast<int*>(q);
  q += bP;
  w->d_tmp = reinterpret_cast<double*>(q);
  q += bM;
  w->d_band = reinterpret_cast<float*>(q);
  q += bB;
  w->d_S = reinterpret_cast<double*>(q);
  q += bS;
  w->extra = q;
  return RVT_OK;
}

// What the passes of a band call multiply, behind the column statistics: the nibble / int8 stores of the exact products (fast)
// or the fp64 columns.
struct BandRun {
  int H = 0, W = 0, halo = 0;
  float scale = 1.0f;
  int Hc = 1024, Hp = 0;  // heads per pass, heads of the largest pass
  bool fast = false, masked = false, fp4 = true;
  const int8_t* R8 = nullptr;                     // the store of the one product (not masked)
  const int8_t *Hs = nullptr, *Ms = nullptr;      // masked: the stores of h and m of the four products
  int r8_ring = 0, r8_col0 = 0;                   // the stores' ring and first column
  int64_t ldk = 0;
  const double* dG = nullptr;                     // not fast: the block of the fp64 columns, its ring and first column
  int ring = 0, col0 = 0;
  // not fast, optional: called at the head of a pass (heads [h0, h0 + nh), markers [h0, h0 + wsub)) to MAKE that pass's
  // columns and their statistics; *base then is their first column (a linear range)
  std::function<int(int h0, int nh, int wsub, const double** base)> stage;
};

// The heads in passes of up to Hc: pass (h0, nh) covers the logical columns [h0, h0 + wsub); its rows are copied to `band` on
// copy_stream while the next pass multiplies (two band buffers).  The last pass's event is recorded; the caller synchronises.
static int band_passes(rvt_ctx* c, hipStream_t st, const CovConsts& cc, const BandRun& r, const BandWork& w, float* band) {
  const NullConsts& nc = c->nc;
  const int64_t N = nc.N, ld = nc.ld;
  const int d = nc.d, H = r.H, W = r.W, halo = r.halo, Hc = r.Hc;
  for (int i = 0; i < 2; ++i) {
    if (!c->ev_band_fin[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_band_fin[i], hipEventDisableTiming));
    if (!c->ev_band_copied[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_band_copied[i], hipEventDisableTiming));
  }
  float* const d_band2[2] = {w.d_band, w.d_band + (size_t)r.Hp * ((size_t)halo + 1)};
  int pass = 0;
  for (int h0 = 0; h0 < H; h0 += Hc, ++pass) {
    float* const d_band = d_band2[pass & 1];
    if (pass >= 2) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_band_copied[pass & 1], 0));  // (the buffer's previous rows have left)
    const int nh = std::min(Hc, H - h0);
    const int wsub = (int)std::min<long long>((long long)W - h0, (long long)nh + halo);
    if (r.fast) {
      const int n_tiles = band_tiles(nh, wsub, halo);
      const int64_t kbytes = r.ldk, chunks = kbytes / kRotKC;
      const int n_sets = r.masked ? 4 : 1;  // (mean-imputed columns: h'h, h'm, m'h, m'm)
      int64_t nsl = band_slices(n_tiles, chunks, ((size_t)3 << 30) / (size_t)n_sets);
      if (const char* e = getenv("RVT_BAND_SLICES"))
        if (atoll(e) > 0) nsl = atoll(e);
      int64_t kslice = ((chunks + nsl - 1) / nsl) * kRotKC;
      // a slice's sums are exact in the accumulator: int32 holds 4 N for any N the engine takes; fp32 holds integers below 2^24,
      // i.e. at most 2^22 samples = 2^21 bytes of E2M1 codes per slice
      if (r.fp4) kslice = std::min<int64_t>(kslice, (int64_t)1 << 21);
      nsl = (kbytes + kslice - 1) / kslice;
      const long long set_stride = (long long)n_tiles * (long long)nsl * kBandBT * kBandBT;
      const size_t need = sizeof(int) * (size_t)set_stride * (size_t)n_sets;
      HIP_TRY(c, c->d_rot_part.grow(need, need, st, true));
      int* d_part = reinterpret_cast<int*>(c->d_rot_part.get());
      int pc = r.r8_col0 + h0;
      if (r.r8_ring > 0 && pc >= r.r8_ring) pc -= r.r8_ring;
      const int pr = (r.r8_ring > 0 && pc + wsub > r.r8_ring) ? r.r8_ring : 0;
      const unsigned grid = (unsigned)(8 * (int64_t)n_tiles * ((nsl + 7) / 8));
      if (r.masked) {
        const int8_t* sideA[4] = {r.Hs, r.Hs, r.Ms, r.Ms};
        const int8_t* sideB[4] = {r.Hs, r.Ms, r.Hs, r.Ms};
        for (int k = 0; k < 4; ++k)
          hipLaunchKernelGGL(band_gemm_fp4, dim3(grid), dim3(kBandThreads), 0, st, sideA[k], sideB[k], (long long)r.ldk, pr, pc, nh, wsub,
                             halo, (long long)kbytes, (long long)kslice, (int)nsl, n_tiles, d_part + (size_t)k * (size_t)set_stride);
      } else if (r.fp4) {
        hipLaunchKernelGGL(band_gemm_fp4, dim3(grid), dim3(kBandThreads), 0, st, r.R8, r.R8, (long long)r.ldk, pr, pc, nh, wsub, halo,
                           (long long)kbytes, (long long)kslice, (int)nsl, n_tiles, d_part);
      } else {
        hipLaunchKernelGGL(band_gemm_i8, dim3(grid), dim3(kBandThreads), 0, st, r.R8, r.R8, (long long)r.ldk, pr, pc, nh, wsub, halo,
                           (long long)kbytes, (long long)kslice, (int)nsl, n_tiles, d_part);
      }
      hipLaunchKernelGGL(band_finish_i32_kernel, dim3((unsigned)nh), dim3(256), 0, st, cc, d_part, (int)nsl, n_tiles, w.d_cs + h0,
                         w.d_xz + (size_t)h0 * d, nh, wsub, halo, r.scale, d_band, (double*)nullptr,
                         r.masked ? w.d_mu_l + h0 : (const double*)nullptr, set_stride);
    } else {
      // dosages, a binary trait's weights: the band tiles of S = G_H' D G_W on the fp64 matrix cores (gemm_f64.hip.h)
      const double* wts = nc.binary ? c->d_v : nullptr;
      int pc = r.col0 + h0;
      if (r.ring > 0 && pc >= r.ring) pc -= r.ring;
      int pr = (r.ring > 0 && pc + wsub > r.ring) ? r.ring : 0;
      const double* base = pr ? r.dG : r.dG + (size_t)pc * ld;
      if (r.stage) {
        pr = 0;
        if (int rc = r.stage(h0, nh, wsub, &base)) return rc;
      }
      int rc = gemm_tn_f64(c, base, ld, nh, base, ld, wsub, nullptr, 0, 0, wts, N, w.d_S, nh, true, st, false, halo, pr, pr ? pc : 0);
      if (rc) return rc;
      hipLaunchKernelGGL(band_rows_f64_kernel, dim3((unsigned)nh), dim3(256), 0, st, cc, w.d_S, (long long)nh, w.d_cs + h0,
                         w.d_xz + (size_t)h0 * d, (const double*)nullptr, nh, wsub, halo, 1.0, r.scale, d_band, (double*)nullptr);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_band_fin[pass & 1], st));
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_band_fin[pass & 1], 0));
    HIP_TRY(c, hipMemcpyAsync(band + (size_t)h0 * ((size_t)halo + 1), d_band, sizeof(float) * (size_t)nh * ((size_t)halo + 1),
                              hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(c, hipEventRecord(c->ev_band_copied[pass & 1], c->copy_stream));
  }
  return RVT_OK;
}

static int cov_band_impl(rvt_ctx* c, const double* dG, int ring, int col0, int H, int W, int halo, float scale, float* band,
                         double* xz, double* zz, int* polymorphic, bool allow_fast) {
  if (!c || !dG || ring < 0 || col0 < 0 || H < 1 || W < H || halo < 0 || !band || !xz || !polymorphic)
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  if (ring > 0 && (col0 >= ring || W > ring)) return fail(c, RVT_E_INVALID, "window of %d columns from %d in a ring of %d", W, col0, ring);
  if ((long long)W > (long long)H + halo) W = H + halo;  // (markers behind the last head's window are never read)
  if (const ColKind* ck = find_block(c, dG))
    if ((ring > 0 ? ring : col0 + W) > ck->cols) return fail(c, RVT_E_INVALID, "the window leaves the block (%d columns)", ck->cols);
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const NullConsts& nc = c->nc;
  const int64_t N = nc.N, ld = nc.ld;
  const int d = nc.d;
  CovConsts cc;
  std::vector<double> zzv;
  rc = cov_constants(c, false, &cc, &zzv);
  if (rc) return rc;
  const int ringk = (ring > 0 && col0 + W > ring) ? ring : 0;   // (a window that does not wrap is a linear range)
  // what the product reads: the columns' hard calls as E2M1 codes, two per byte, on the MXFP4 matrix instruction (exact, see
  // band_gemm.hip.h; RVT_BAND_INT8=1: one byte per genotype on the int8 one)
  const bool fp4 = !getenv("RVT_BAND_INT8");
  // the ring's own column cache (rvt_block_upload_columns made it behind the uploads): usable when every column of the window
  // has an entry made under THIS null model — state 1 hard calls only, state 2 hard calls plus one other value (MXFP4 only)
  bool masked = false;
  const ColKind* ckc = usable_cache(c, dG, ring, col0, W, fp4, &masked);
  const bool fast = allow_fast && !nc.binary && !getenv("RVT_METACOV_FP64") &&
                    ring_hard_calls(c, dG, ring, col0, W, (ckc && masked) ? ckc->valid.data() : nullptr) != 0;
  if (!fast) {
    ckc = nullptr;
    masked = false;
  }
  c->band_last_path = !fast ? 0 : (masked ? 4 : (ckc ? (fp4 ? 1 : 11) : (fp4 ? 2 : 12)));
  // heads per pass: the rectangle of doubles (fp64) of a pass stays within a few hundred MB; the integer band in passes of 1 024
  // so that the rows of one pass cross PCIe while the next pass multiplies (two band buffers, the copies on copy_stream)
  int Hc = 1024;
  if (const char* e = getenv("RVT_BAND_PASS")) Hc = std::max(256, atoi(e) / 256 * 256);
  const int Hp = std::min(H, Hc), Wp = (int)std::min<long long>(W, (long long)Hp + halo);
  BandWork bw;
  rc = band_work(c, st, W, d, Hp, Wp, halo, fast, 0, &bw);
  if (rc) return rc;
  double *const d_T = bw.d_T, *const d_cs = bw.d_cs, *const d_xz = bw.d_xz, *const d_tmp = bw.d_tmp, *const d_mu_l = bw.d_mu_l;
  int* const d_poly = bw.d_poly;
  const int dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
  const int wgs = (W + kCovHcCols - 1) / kCovHcCols;
  const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(kCovSlices, N / 4096 + 1));
  const double* Gbase = ringk ? dG : dG + (size_t)col0 * ld;   // what the column pass indexes from
  const int pcol0 = ringk ? col0 : 0;
  int* d_bad = nullptr;
  int h_bad = 0;
  // (the store the product reads, its ring and first column)
  const int8_t* R8 = nullptr;
  int r8_ring = 0, r8_col0 = 0;
  const int64_t ldk8 = (N + 127) / 128 * 128, ldk4 = ((N + 1) / 2 + 127) / 128 * 128;
  int64_t ldk = fp4 ? ldk4 : ldk8;
  if (fast && ckc) {
    hipLaunchKernelGGL(band_cache_gather_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, ckc->d_cs, ckc->d_poly,
                       ckc->d_T, ringk, col0, W, d, RVT_MAX_COV, d_cs, d_poly, d_T, masked ? ckc->d_mu : (const double*)nullptr,
                       masked ? d_mu_l : (double*)nullptr);
    R8 = fp4 ? reinterpret_cast<const int8_t*>(ckc->d_i4.get()) : reinterpret_cast<const int8_t*>(ckc->d_i8.get());
    r8_ring = ringk;
    r8_col0 = col0;
  } else if (fast) {
    // no cache: ONE pass over the window's columns gives the statistics, T = G'X and a linear copy of the window's hard calls
    const size_t need = ((size_t)W + kBandBT) * (size_t)ldk;
    HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
    const int64_t n4 = (N + 3) / 4 * 4, nw = fp4 ? n4 / 2 : n4;   // bytes of a column the pass writes; the pad behind them: zero
    if (ldk > nw) HIP_TRY(c, hipMemset2DAsync(c->d_rotB + nw, (size_t)ldk, 0, (size_t)(ldk - nw), (size_t)W, st));
    HIP_TRY(c, c->d_kind.grow(sizeof(int), sizeof(int), st, true));
    d_bad = c->d_kind;
    HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(int), st));
    launch_cov_prep(st, d, true, dim3((unsigned)wgs, (unsigned)slices), Gbase, N, ld, W, c->d_X, fp4 ? nullptr : c->d_rotB, ldk8, d_tmp,
                    d_bad, nullptr, nullptr, ringk, pcol0, fp4 ? reinterpret_cast<unsigned char*>(c->d_rotB.get()) : nullptr, ldk4);
    hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((W * (dmax + 3) + 255) / 256)), dim3(256), 0, st, d_tmp, slices,
                       W, d, dmax, d_cs, d_poly, d_T);
    R8 = reinterpret_cast<const int8_t*>(c->d_rotB.get());
  } else {
    launch_cov_prep(st, d, false, dim3((unsigned)wgs, (unsigned)slices), Gbase, N, ld, W, c->d_X, nullptr, 0, d_tmp, nullptr,
                    nc.binary ? c->d_v : nullptr, nullptr, ringk, pcol0, nullptr, 0);
    hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((W * (dmax + 3) + 255) / 256)), dim3(256), 0, st, d_tmp, slices,
                       W, d, dmax, d_cs, d_poly, d_T);
  }
  hipLaunchKernelGGL(cov_rect_xz_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, cc, d_T, d_cs, W, d_xz);
  HIP_TRY(c, hipGetLastError());
  // the heads in passes of up to Hc (band_passes)
  BandRun br;
  br.H = H, br.W = W, br.halo = halo, br.scale = scale, br.Hc = Hc, br.Hp = Hp;
  br.fast = fast, br.masked = masked, br.fp4 = fp4;
  br.R8 = R8, br.r8_ring = r8_ring, br.r8_col0 = r8_col0, br.ldk = ldk;
  if (masked) {
    br.Hs = reinterpret_cast<const int8_t*>(ckc->d_i4.get());
    br.Ms = reinterpret_cast<const int8_t*>(ckc->d_m4.get());
  }
  br.dG = dG, br.ring = ring, br.col0 = col0;
  rc = band_passes(c, st, cc, br, bw, band);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(xz, d_xz, sizeof(double) * (size_t)W * d, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(polymorphic, d_poly, sizeof(int) * (size_t)W, hipMemcpyDeviceToHost, st));
  if (d_bad) HIP_TRY(c, hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  HIP_TRY(c, sync_stream(c->copy_stream));
  if (h_bad) return cov_band_impl(c, dG, ring, col0, H, W, halo, scale, band, xz, zz, polymorphic, false);  // not hard calls after all
  if (zz) std::memcpy(zz, zzv.data(), sizeof(double) * (size_t)d * d);
  return RVT_OK;
}
int rvt_cov_band_last_path(rvt_ctx* c) { return c ? c->band_last_path : -1; }
int rvt_cov_band(rvt_ctx* c, const double* dG, int ring_cols, int col0, int H, int W, int halo, float scale, float* band,
                 double* xz, double* zz, int* polymorphic) {
  return cov_band_impl(c, dG, ring_cols, col0, H, W, halo, scale, band, xz, zz, polymorphic, true);
}

// ---- MetaCov's band from rows of a resident .bed matrix (bed_band_kernels.hip.h) -------------------------------------------------
// measurement (rvt_set_profiling): HIP events at the call's start (0), behind the front stage (1), directly in front of and
// behind the passes (2, 3) and at the end (4)
static int band_bed_mark(rvt_ctx* c, int k, hipStream_t st) {
  if (!c->profiling) return RVT_OK;
  if (!c->ev_band_bed[k]) HIP_TRY(c, hipEventCreate(&c->ev_band_bed[k]));
  HIP_TRY(c, hipEventRecord(c->ev_band_bed[k], st));
  return RVT_OK;
}
static int band_bed_times(rvt_ctx* c) {  // (behind the call's last synchronisation)
  if (!c->profiling) return RVT_OK;
  float a = 0.0f, b = 0.0f, t = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&a, c->ev_band_bed[0], c->ev_band_bed[1]));
  HIP_TRY(c, hipEventElapsedTime(&b, c->ev_band_bed[2], c->ev_band_bed[3]));
  HIP_TRY(c, hipEventElapsedTime(&t, c->ev_band_bed[0], c->ev_band_bed[4]));
  c->band_bed_ms[0] = a, c->band_bed_ms[1] = b, c->band_bed_ms[2] = t;
  return RVT_OK;
}
int rvt_cov_band_bed_last_timing(rvt_ctx* c, double* ms3) {
  if (!c || !ms3) return RVT_E_INVALID;
  for (int k = 0; k < 3; ++k) ms3[k] = c->band_bed_ms[k];
  return RVT_OK;
}

// Heads = rows [0, H), markers = rows [0, W) of the W consecutive rows at d_rows; the columns are the rows with missing calls
// imputed to the row's mean, g = h + mu m.  Quantitative model: the front stage writes the nibble rows of h (d_rotA) and m
// (d_rotB) and the rows' statistics; a read-back of one flag chooses one product (no missing call in the window, path 21) or
// four (path 24).  Binary model or RVT_METACOV_FP64=1 (path 20): counts -> mu, then every pass expands its rows into an fp64
// block of at most 1 024 + halo columns (d_rotA), takes their statistics from it and multiplies on the fp64 matrix cores.
int rvt_cov_band_bed_dev(rvt_ctx* c, const unsigned char* d_rows, int H, int W, int halo, float scale, float* band, double* xz,
                         double* zz, int* polymorphic, long long* counts) {
  if (!c || !d_rows || H < 1 || W < H || halo < 0 || !band || !xz || !polymorphic) return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  // (as rvt_score_bed_dev: the resident-row calls are one family behind the same two switches)
  if (getenv("RVT_PACKED") && atoi(getenv("RVT_PACKED")) == 0)
    return fail(c, RVT_E_STATE, "rvt_cov_band_bed_dev: the packed-row kernels are switched off (RVT_PACKED=0)");
  if (!c->hc_enabled)
    return fail(c, RVT_E_STATE, "rvt_cov_band_bed_dev: the packed rows need the hard-call kernels, which are switched off (RVT_HARDCALL=0)");
  if ((long long)W > (long long)H + halo) W = H + halo;  // (markers behind the last head's window are never read)
  int64_t cb = 0;
  int rc = bed_rows_span(c, "rvt_cov_band_bed_dev", d_rows, W, BedModel::kNull, &cb);
  if (rc) return rc;
  hipSetDevice(c->device);
  rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const NullConsts& nc = c->nc;
  const int64_t N = nc.N, ld = nc.ld;
  const int d = nc.d;
  CovConsts cc;
  std::vector<double> zzv;
  rc = cov_constants(c, false, &cc, &zzv);
  if (rc) return rc;
  const bool fast = !nc.binary && !getenv("RVT_METACOV_FP64");
  int Hc = 1024;
  if (const char* e = getenv("RVT_BAND_PASS")) Hc = std::max(256, atoi(e) / 256 * 256);
  const int Hp = std::min(H, Hc), Wp = (int)std::min<long long>(W, (long long)Hp + halo);
  const int dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
  const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(kCovSlices, N / 4096 + 1));
  Layout X;  // (behind the shared work space: the front stage's partial results, the counts, the flag)
  const size_t o_pt = X.take(fast ? sizeof(double) * (size_t)slices * W * 2 * dmax : 0);
  const size_t o_pc = X.take(fast ? sizeof(int) * (size_t)slices * W * 4 : 0);
  const size_t o_cnt = X.take(sizeof(long long) * 4 * (size_t)W);
  const size_t o_flag = X.take(sizeof(int));
  BandWork bw;
  rc = band_work(c, st, W, d, Hp, Wp, halo, fast, X.total, &bw);
  if (rc) return rc;
  if ((rc = band_bed_mark(c, 0, st))) return rc;
  long long* d_cnt = reinterpret_cast<long long*>(bw.extra + o_cnt);
  std::vector<long long> cnt(4 * (size_t)W);
  BandRun br;
  br.H = H, br.W = W, br.halo = halo, br.scale = scale, br.Hc = Hc, br.Hp = Hp, br.fast = fast;
  if (fast) {
    const int64_t ldk4 = ((N + 1) / 2 + 127) / 128 * 128;
    const size_t need = ((size_t)W + kBandBT) * (size_t)ldk4;
    HIP_TRY(c, c->d_rotA.grow(need, need + need / 4, st, true));
    HIP_TRY(c, c->d_rotB.grow(need, need + need / 4, st, true));
    unsigned char* outH = reinterpret_cast<unsigned char*>(c->d_rotA.get());
    unsigned char* outM = reinterpret_cast<unsigned char*>(c->d_rotB.get());
    const int64_t nw = (N + 15) / 16 * 8;  // bytes of a nibble row the front stage writes; the pad behind them: zero
    if (ldk4 > nw) {
      HIP_TRY(c, hipMemset2DAsync(outH + nw, (size_t)ldk4, 0, (size_t)(ldk4 - nw), (size_t)W, st));
      HIP_TRY(c, hipMemset2DAsync(outM + nw, (size_t)ldk4, 0, (size_t)(ldk4 - nw), (size_t)W, st));
    }
    double* d_pt = reinterpret_cast<double*>(bw.extra + o_pt);
    int* d_pc = reinterpret_cast<int*>(bw.extra + o_pc);
    int* d_flag = reinterpret_cast<int*>(bw.extra + o_flag);
    HIP_TRY(c, hipMemsetAsync(d_flag, 0, sizeof(int), st));
#define RVT_BED_PREP(DM)                                                                                                      \
  hipLaunchKernelGGL((bed_band_prep_kernel<DM>), dim3((unsigned)((W + BedBandRows<DM>::value - 1) / BedBandRows<DM>::value),  \
                                                      (unsigned)slices),                                                     \
                     dim3(256), 0, st, d_rows, (long long)cb, (long long)N, W, c->d_X, (long long)ld, d, outH, outM,          \
                     (long long)ldk4, d_pt, d_pc)
    if (dmax == 4) RVT_BED_PREP(4);
    else if (dmax == 8) RVT_BED_PREP(8);
    else RVT_BED_PREP(RVT_MAX_COV);
#undef RVT_BED_PREP
    hipLaunchKernelGGL(bed_band_finish_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, d_pt, d_pc, slices, W, d, dmax,
                       bw.d_cs, bw.d_poly, bw.d_T, bw.d_mu_l, d_cnt, d_flag);
    HIP_TRY(c, hipGetLastError());
    if ((rc = band_bed_mark(c, 1, st))) return rc;
    hipLaunchKernelGGL(cov_rect_xz_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, cc, bw.d_T, bw.d_cs, W, bw.d_xz);
    HIP_TRY(c, hipGetLastError());
    int h_any = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_any, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(long long) * cnt.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, sync_stream(st));
    br.masked = h_any != 0;  // (no missing call in the window: m = 0, the one product h'h is the whole of S)
    br.fp4 = true;
    br.R8 = br.Hs = reinterpret_cast<const int8_t*>(outH);
    br.Ms = reinterpret_cast<const int8_t*>(outM);
    br.ldk = ldk4;
    c->band_last_path = br.masked ? 24 : 21;
  } else {
    rc = bed_piece_counts(c, st, d_rows, cb, N, W, reinterpret_cast<unsigned long long*>(d_cnt), nullptr, cnt.data());
    if (rc) return rc;
    constexpr int kRows = 32768;  // rows per launch (gridDim.y)
    std::vector<double> mu((size_t)W);
    for (int j = 0; j < W; ++j) {  // (a row without a missing call is its calls: mu = 0)
      const long long* q = &cnt[4 * (size_t)j];
      mu[(size_t)j] = q[3] > 0 ? bed_site(q[0], q[1], q[2], q[3]).mean : 0.0;
    }
    HIP_TRY(c, hipMemcpyAsync(bw.d_mu_l, mu.data(), sizeof(double) * (size_t)W, hipMemcpyHostToDevice, st));
    HIP_TRY(c, sync_stream(st));  // (mu goes out of use on the host)
    if ((rc = band_bed_mark(c, 1, st))) return rc;
    const size_t need = sizeof(double) * (size_t)Wp * (size_t)ld;
    HIP_TRY(c, c->d_rotA.grow(need, need, st, true));
    double* E = reinterpret_cast<double*>(c->d_rotA.get());
    if (ld > N)  // (the expansion writes rows [0, N) of a column; the pad rows behind them: zero)
      HIP_TRY(c, hipMemset2DAsync(E + N, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)(ld - N), (size_t)Wp, st));
    const double* wts = nc.binary ? c->d_v : nullptr;
    br.stage = [=](int h0, int nh, int wsub, const double** base) -> int {
      (void)nh;
      for (int k0 = 0; k0 < wsub; k0 += kRows)
        bed_rows_expand(st, d_rows + (size_t)(h0 + k0) * (size_t)cb, cb, bw.d_mu_l + h0 + k0, N, ld, std::min(kRows, wsub - k0),
                        E + (size_t)k0 * (size_t)ld);
      launch_cov_prep(st, d, false, dim3((unsigned)((wsub + kCovHcCols - 1) / kCovHcCols), (unsigned)slices), E, N, ld, wsub, c->d_X,
                      nullptr, 0, bw.d_tmp, nullptr, wts, nullptr, 0, 0, nullptr, 0);
      hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((wsub * (dmax + 3) + 255) / 256)), dim3(256), 0, st, bw.d_tmp, slices,
                         wsub, d, dmax, bw.d_cs + h0, bw.d_poly + h0, bw.d_T);
      hipLaunchKernelGGL(cov_rect_xz_kernel, dim3((unsigned)((wsub + 255) / 256)), dim3(256), 0, st, cc, bw.d_T, bw.d_cs + h0, wsub,
                         bw.d_xz + (size_t)h0 * d);
      HIP_TRY(c, hipGetLastError());
      *base = E;
      return RVT_OK;
    };
    c->band_last_path = 20;
  }
  if ((rc = band_bed_mark(c, 2, st))) return rc;
  rc = band_passes(c, st, cc, br, bw, band);
  if (rc) return rc;
  if ((rc = band_bed_mark(c, 3, st))) return rc;
  HIP_TRY(c, hipMemcpyAsync(xz, bw.d_xz, sizeof(double) * (size_t)W * d, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(polymorphic, bw.d_poly, sizeof(int) * (size_t)W, hipMemcpyDeviceToHost, st));
  if (c->profiling) {  // (the whole call ends when the last pass's rows have left)
    const int last = ((H + Hc - 1) / Hc - 1) & 1;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_band_copied[last], 0));
    if ((rc = band_bed_mark(c, 4, st))) return rc;
  }
  HIP_TRY(c, sync_stream(st));
  HIP_TRY(c, sync_stream(c->copy_stream));
  if (zz) std::memcpy(zz, zzv.data(), sizeof(double) * (size_t)d * d);
  if (counts) std::memcpy(counts, cnt.data(), sizeof(long long) * cnt.size());
  return band_bed_times(c);
}

// MetaCov with kinship for windows wider than one block (MetaCovFamQtl / MetaCovFamBinary, src/Model.cpp:437-504,595-692):
// heads [col0, col0 + H) against markers [col0, col0 + W) of the RAW block dG.  The W columns are rotated by U'
// (integer planes), then S = (D G~_H)' G~_W and T = G~_W' D [U'X | u1] are two more integer-plane products and the
// centring algebra of the block kernel finishes the rows.  Same outputs as rvt_cov_rect.
// (ring > 0: dG is a block used as a ring of `ring` columns, logical column j = physical (col0 + j) mod ring.
//  halo < 0: the rectangle cov[h + j H]; halo >= 0: the band, band[h (halo + 1) + t] = (float)value(h, h + t) * scale.)
static int cov_rect_fam_impl(rvt_ctx* c, const double* dG, int ring, int col0, int H, int W, int halo, float scale, double* cov,
                             float* band, double* xz, double* zz, int* polymorphic) {
  if (!c || !dG || col0 < 0 || H < 1 || W < H || (!cov && !band) || !xz || !polymorphic)
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  if (ring > 0 && (col0 >= ring || W > ring)) return fail(c, RVT_E_INVALID, "window of %d columns from %d in a ring of %d", W, col0, ring);
  hipSetDevice(c->device);
  int rc = rvt_sync(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t N = c->fam_nc.N, ld = c->fam_nc.ld;
  const int du = c->famcov_nc.d - 2;  // columns of U'X
  CovConsts cc;
  std::vector<double> zzv;
  {
    const NullConsts keep = c->nc;
    c->nc = c->famcov_nc;
    rc = cov_constants(c, true, &cc, &zzv);
    c->nc = keep;
    if (rc) return rc;
  }
  rc = ensure_fam_cols(c, (size_t)W, ld);
  if (rc) return rc;
  // the window's columns as at most two contiguous runs of the ring
  struct Seg {
    int phys, n, at;
  };
  Seg segs[2];
  int nseg = 1;
  segs[0] = Seg{col0, W, 0};
  if (ring > 0 && col0 + W > ring) {
    segs[0].n = ring - col0;
    segs[1] = Seg{0, W - segs[0].n, segs[0].n};
    nseg = 2;
  }
  DevBuf<double> d_S, d_T, d_cs, d_xz, d_cov, d_w, d_t1;
  DevBuf<float> d_band;
  DevBuf<int> d_poly;
  HIP_TRY(c, d_S.alloc(sizeof(double) * (size_t)H * W));
  if (halo < 0) HIP_TRY(c, d_cov.alloc(sizeof(double) * (size_t)H * W));
  else HIP_TRY(c, d_band.alloc(sizeof(float) * (size_t)H * ((size_t)halo + 1)));
  HIP_TRY(c, d_T.alloc(sizeof(double) * (size_t)W * (du + 1)));
  HIP_TRY(c, d_xz.alloc(sizeof(double) * (size_t)W * du));
  HIP_TRY(c, d_t1.alloc(sizeof(double) * (size_t)W));
  HIP_TRY(c, d_cs.alloc(sizeof(double) * (size_t)W));
  HIP_TRY(c, d_poly.alloc(sizeof(int) * (size_t)W));
  HIP_TRY(c, d_w.alloc(sizeof(double) * (size_t)ld * (size_t)(du + 1 + H)));
  HIP_TRY(c, hipMemsetAsync(c->d_Gt, 0, sizeof(double) * (size_t)ld * W, st));
  for (int k = 0; k < nseg; ++k) {
    const double* GW = dG + (size_t)segs[k].phys * ld;
    k_raw_colstat(dim3((unsigned)segs[k].n), st, GW, (long long)N, (long long)ld, d_cs + segs[k].at, d_poly + segs[k].at);
    rc = rotate_columns(c, GW, ld, segs[k].n, c->d_Gt + (size_t)segs[k].at * ld, ld, st);
    if (rc) return rc;
  }
  // the weights D = 1 / ((|lambda| + delta) sigma2) ride on the small operands: D [U'X | u1] and D G~_H
  HIP_TRY(c, hipMemsetAsync(d_w, 0, sizeof(double) * (size_t)ld * (size_t)(du + 1 + H), st));
  hipLaunchKernelGGL(scale_rows_kernel, dim3(64, (unsigned)(du + 1)), dim3(256), 0, st, c->d_cX, c->d_cv, (long long)N,
                     (long long)ld, d_w);
  hipLaunchKernelGGL(scale_rows_kernel, dim3(64, (unsigned)H), dim3(256), 0, st, c->d_Gt, c->d_cv, (long long)N,
                     (long long)ld, d_w + (size_t)ld * (du + 1));
  rc = gemm_tn_planes(c, c->d_Gt, ld, W, d_w, ld, du + 1, N, d_T, W, st);
  if (rc) return rc;
  rc = gemm_tn_planes(c, d_w + (size_t)ld * (du + 1), ld, H, c->d_Gt, ld, W, N, d_S, H, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cov_rect_fam_xz_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, cc, d_T, d_cs, W, d_xz,
                     d_t1);
  const double b2 = c->famcov_b2;  // MetaCovFamBinary: covXX, covXZ, covZZ each carry b^2 (Model.cpp:651-668)
  if (halo < 0) {
    HIP_TRY(c, hipMemsetAsync(d_cov, 0, sizeof(double) * (size_t)H * W, st));  // (zeros below the diagonal, as cov_rect_impl)
    hipLaunchKernelGGL(cov_rect_fam_rows_kernel, dim3((unsigned)H), dim3(256), 0, st, cc, d_S, d_cs, d_xz, d_t1, H, W,
                       d_cov);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)H * W, hipMemcpyDeviceToHost, st));
  } else {
    hipLaunchKernelGGL(band_rows_f64_kernel, dim3((unsigned)H), dim3(256), 0, st, cc, d_S, (long long)H, d_cs, d_xz,
                       (const double*)d_t1, H, W, halo, b2, scale, d_band, (double*)nullptr);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(band, d_band, sizeof(float) * (size_t)H * ((size_t)halo + 1), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipMemcpyAsync(xz, d_xz, sizeof(double) * (size_t)W * du, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(polymorphic, d_poly, sizeof(int) * (size_t)W, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  if (zz) std::memcpy(zz, zzv.data(), sizeof(double) * (size_t)du * du);
  if (b2 != 1.0) {
    if (halo < 0)
      for (int h = 0; h < H; ++h)
        for (int j = h; j < W; ++j) cov[(size_t)h + (size_t)j * H] *= b2;
    for (size_t i = 0; i < (size_t)W * du; ++i) xz[i] *= b2;
    if (zz)
      for (int i = 0; i < du * du; ++i) zz[i] *= b2;
  }
  return RVT_OK;
}
int rvt_cov_rect_fam(rvt_ctx* c, const double* dG, int col0, int H, int W, double* cov, double* xz, double* zz,
                     int* polymorphic) {
  if (!cov) return fail(c, RVT_E_INVALID, "bad arguments");
  return cov_rect_fam_impl(c, dG, 0, col0, H, W, -1, 1.0f, cov, nullptr, xz, zz, polymorphic);
}
// The family counterpart of rvt_cov_band: the heads in passes of up to 1 024 (every pass rotates the columns of its heads and
// of the window behind them).  xz / polymorphic: the W logical columns.
int rvt_cov_band_fam(rvt_ctx* c, const double* dG, int ring_cols, int col0, int H, int W, int halo, float scale, float* band,
                     double* xz, double* zz, int* polymorphic) {
  if (!c || !dG || ring_cols < 0 || col0 < 0 || H < 1 || W < H || halo < 0 || !band || !xz || !polymorphic)
    return fail(c, RVT_E_INVALID, "bad arguments");
  if (!c->have_fam) return fail(c, RVT_E_STATE, "rvt_set_kinship + rvt_fit_fam_null first");
  if ((long long)W > (long long)H + halo) W = H + halo;
  const int du = c->famcov_nc.d - 2, Hc = 1024;
  std::vector<double> xzp;
  std::vector<int> pp;
  for (int h0 = 0; h0 < H; h0 += Hc) {
    const int nh = std::min(Hc, H - h0);
    const int wsub = (int)std::min<long long>((long long)W - h0, (long long)nh + halo);
    int pc = col0 + h0;
    if (ring_cols > 0 && pc >= ring_cols) pc -= ring_cols;
    xzp.assign((size_t)wsub * du, 0.0);
    pp.assign((size_t)wsub, 0);
    int rc = cov_rect_fam_impl(c, dG, ring_cols, pc, nh, wsub, halo, scale, nullptr, band + (size_t)h0 * ((size_t)halo + 1),
                               xzp.data(), zz, pp.data());
    if (rc) return rc;
    std::memcpy(xz + (size_t)h0 * du, xzp.data(), sizeof(double) * xzp.size());
    std::memcpy(polymorphic + h0, pp.data(), sizeof(int) * pp.size());
  }
  return RVT_OK;
}

// ---- the column operations of the adapters' device ring ---------------------------------------------------------------------
int rvt_block_copy_columns(rvt_ctx* c, double* dst, int dst_col, const double* src, int src_col, int ncols) {
  if (!c || !dst || !src || dst_col < 0 || src_col < 0 || ncols < 0) return fail(c, RVT_E_INVALID, "bad copy");
  if (int rc = check_columns(c, dst, dst_col, ncols)) return rc;
  if (int rc = check_columns(c, src, src_col, ncols)) return rc;
  if (ncols == 0) return RVT_OK;
  hipSetDevice(c->device);
  if (int rc = flush_col_queue(c)) return rc;
  HIP_TRY(c, sync_stream(c->io_stream));  // (queued uploads and the passes behind them write what is copied here)
  const size_t ld = (size_t)block_dims(c).ld;
  HIP_TRY(c, hipMemcpy(dst + (size_t)dst_col * ld, src + (size_t)src_col * ld, sizeof(double) * ld * ncols,
                       hipMemcpyDeviceToDevice));
  // what the engine knows about the columns travels with them: content flags and the column cache
  ColKind* t = find_block(c, dst);
  if (!t) return RVT_OK;
  const ColKind* s = find_block(c, src);
  if (s && s->d_flags && dst != src) {
    if (int rc = ensure_flags(c, *t)) return rc;
    HIP_TRY(c, hipMemcpyAsync(t->d_flags + dst_col, s->d_flags + src_col, sizeof(int) * (size_t)ncols, hipMemcpyDeviceToDevice,
                              c->io_stream));
  } else {
    // nothing known about the source — or a copy inside one block (not the forward move of rvt_block_move_columns), where the
    // target's flags and cache entries describe what was there before
    if (int rc = invalidate_columns(c, t, dst_col, ncols, false)) return rc;
  }
  if (dst != src)
    if (int rc = move_col_cache(c, t, dst_col, s, src_col, ncols, c->io_stream)) return rc;
  HIP_TRY(c, sync_stream(c->io_stream));
  return RVT_OK;
}

// What the engine keeps per column of a block, for n <= kColQueue columns whose content is KNOWN (they crossed PCIe packed, or
// were recoded: hard[k] = hard calls only, otherwise hard calls plus the one other value mu[k]) and which have been written
// into dG on io_stream: the content flags, and under an unweighted null model the column pass of MetaCov's band on these
// columns (int8 copy, E2M1 codes of the hard calls and of the other value's mask, sum, flag, row of T) — cache state 1 / 2.
static int packed_columns_pass(rvt_ctx* c, double* dG, int col0, int n, const double* mu, const int* hard) {
  ColKind* ck = find_block(c, dG);
  if (!ck || !c->hc_enabled) return RVT_OK;
  hipStream_t st = c->io_stream;
  const size_t N = (size_t)block_dims(c).N, ld = (size_t)block_dims(c).ld;
  int rc = ensure_flags(c, *ck);
  if (!rc) rc = small_h2d(c, ck->d_flags + col0, hard, sizeof(int) * (size_t)n);
  if (rc || !ensure_cache(c, *ck)) return rc;
  const int d = c->nc.d, dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
  const int64_t ldk = ck->ldk, ldk4 = ck->ldk4;
  const size_t part_doubles = (size_t)kCovSlices * rvt_ctx::kColQueue * (RVT_MAX_COV + 3);
  HIP_TRY(c, c->d_cc_part.grow(sizeof(double) * part_doubles, sizeof(double) * part_doubles, st, true, 0, "d_cc_part"));
  const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(kCovSlices, (int64_t)N / 4096 + 1));
  // (the columns' other values, NaN where a column has none: the pass splits g = h + mu m by them)
  double mu_nan[rvt_ctx::kColQueue];
  for (int k = 0; k < n; ++k) mu_nan[k] = hard[k] ? (double)NAN : mu[k];
  HIP_TRY(c, c->d_mu_nan.grow(sizeof(double) * (size_t)rvt_ctx::kColQueue, sizeof(double) * (size_t)rvt_ctx::kColQueue, st, true));
  double* d_mu_nan = c->d_mu_nan;
  rc = small_h2d(c, d_mu_nan, mu_nan, sizeof(double) * (size_t)n);
  if (!rc) rc = small_h2d(c, ck->d_mu + col0, mu, sizeof(double) * (size_t)n);
  if (rc) return rc;
  launch_cov_prep(st, d, true, dim3((unsigned)((n + kCovHcCols - 1) / kCovHcCols), (unsigned)slices), dG + (size_t)col0 * ld,
                  (int64_t)N, (int64_t)ld, n, c->d_X, ck->d_i8 + (size_t)col0 * (size_t)ldk, ldk, c->d_cc_part, nullptr, nullptr,
                  nullptr, 0, 0, ck->d_i4 + (size_t)col0 * (size_t)ldk4, ldk4, d_mu_nan, ck->d_m4 + (size_t)col0 * (size_t)ldk4);
  hipLaunchKernelGGL(cov_hc_finish_kernel, dim3((unsigned)((n * (dmax + 3) + 255) / 256)), dim3(256), 0, st, c->d_cc_part, slices,
                     n, d, dmax, ck->d_cs + col0, ck->d_poly + col0, ck->d_T + (size_t)col0 * RVT_MAX_COV, RVT_MAX_COV);
  HIP_TRY(c, hipGetLastError());
  for (int k = 0; k < n; ++k) ck->valid[(size_t)(col0 + k)] = (unsigned char)(hard[k] ? 1 : 2);
  return RVT_OK;
}
// ... of any number of such columns, kColQueue at a time
static int packed_columns_passes(rvt_ctx* c, double* dG, int col0, int ncols, const double* mu, const int* hard) {
  for (int k0 = 0; k0 < ncols; k0 += rvt_ctx::kColQueue) {
    int rc = packed_columns_pass(c, dG, col0 + k0, std::min(rvt_ctx::kColQueue, ncols - k0), mu + k0, hard + k0);
    if (rc) return rc;
  }
  return RVT_OK;
}

// n columns that lie in d_colpack as 2-bit rows, `pitch` bytes apart, become the doubles of columns [col0, col0 + n) of dG on
// io_stream; their other values mu (0 for a column without one) go behind `rows_cap` rows of the same buffer first
static int expand_packed_rows(rvt_ctx* c, size_t pitch, size_t rows_cap, const double* mu, int n, double* dG, int col0) {
  const size_t N = (size_t)block_dims(c).N, ld = (size_t)block_dims(c).ld;
  double* d_mu = reinterpret_cast<double*>(c->d_colpack + pitch * rows_cap);
  int rc = small_h2d(c, d_mu, mu, sizeof(double) * (size_t)n);
  if (rc) return rc;
  hipLaunchKernelGGL(bed_expand_columns_kernel<BedRowsAt>, dim3((unsigned)((N + 1023) / 1024), (unsigned)n), dim3(256), 0,
                     c->io_stream, BedRowsAt{reinterpret_cast<const unsigned char*>(c->d_colpack.get()), (long long)pitch}, d_mu,
                     (long long)N, (long long)ld, dG + (size_t)col0 * ld);
  HIP_TRY(c, hipGetLastError());
  return RVT_OK;
}

// What rvt_block_upload_columns queued (rvt_ctx::ColQueue: up to 32 consecutive columns of one block, packed to 2-bit rows in
// pinned memory, their other values and hard-call flags known on the host) goes to the device: ONE DMA of the rows, the other
// values, the flags; the expansion to doubles; and — when the block keeps a column cache — the column pass over all of them.
// Nothing queued: nothing happens.
int flush_col_queue(rvt_ctx* c) {
  rvt_ctx::ColQueue& q = c->colq;
  const int n = q.n;
  if (n == 0) return RVT_OK;
  q.n = 0;
  hipSetDevice(c->device);
  const size_t need = q.pitch * (size_t)rvt_ctx::kColQueue + 2 * sizeof(double) * (size_t)rvt_ctx::kColQueue;
  HIP_TRY(c, c->d_colpack.grow(need, need + need / 2, c->io_stream, true, 0, "d_colpack"));
  HIP_TRY(c, hipMemcpyAsync(c->d_colpack, q.h[q.cur], q.pitch * (size_t)n, hipMemcpyHostToDevice, c->io_stream));
  if (!q.ev[q.cur]) HIP_TRY(c, hipEventCreateWithFlags(&q.ev[q.cur], hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(q.ev[q.cur], c->io_stream));
  q.used[q.cur] = true;
  q.cur ^= 1;
  int rc = expand_packed_rows(c, q.pitch, rvt_ctx::kColQueue, q.mu, n, q.dG, q.col0);
  return rc ? rc : packed_columns_pass(c, q.dG, q.col0, n, q.mu, q.hard);
}
// ... and wait until what was flushed is in its block (earlier_flushes_too: also what earlier calls flushed — rvt_sync)
int flush_col_queue_wait(rvt_ctx* c, bool earlier_flushes_too) {
  const bool queued = c->colq.n > 0;
  if (int rc = flush_col_queue(c)) return rc;
  if (queued || (earlier_flushes_too && (c->colq.used[0] || c->colq.used[1]))) HIP_TRY(c, sync_stream(c->io_stream));
  return RVT_OK;
}

// rvt_block_upload_columns, ONE column (a site of MetaCovTest / MetaScoreTest::fit): packed by the staging threads into pinned
// memory and queued; the device work runs once per 32 consecutive columns (flush_col_queue).  *queued = false: the column is
// not representable (a dosage) and has to cross as doubles.
static int queue_column(rvt_ctx* c, double* dG, int col0, const double* G, bool* queued) {
  *queued = false;
  rvt_ctx::ColQueue& q = c->colq;
  const size_t N = (size_t)block_dims(c).N, pitch = hcp_row_pitch(N);
  if (q.n > 0 && (q.dG != dG || col0 != q.col0 + q.n || q.n == rvt_ctx::kColQueue || q.pitch != pitch)) {
    int rc = flush_col_queue(c);
    if (rc) return rc;
  }
  if (q.pitch != pitch) {  // (another N: new pinned rows)
    HIP_TRY(c, sync_stream(c->io_stream));
    for (int i = 0; i < 2; ++i) {
      q.h[i].reset();
      q.used[i] = false;
    }
    q.pitch = pitch;
  }
  for (int i = 0; i < 2; ++i)
    HIP_TRY(c, q.h[i].grow(pitch * (size_t)rvt_ctx::kColQueue, pitch * (size_t)rvt_ctx::kColQueue));
  if (q.n == 0) {
    if (q.used[q.cur]) {  // the DMA that last read these rows has finished?
      while (hipEventQuery(q.ev[q.cur]) == hipErrorNotReady) {
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
      }
      (void)hipGetLastError();
    }
    q.dG = dG;
    q.col0 = col0;
  }
  PackedColumn pc;
  if (!StageRing::pack_columns_to(reinterpret_cast<char*>(q.h[q.cur].get()) + pitch * (size_t)q.n, pitch, G, N, N, 1,
                                  CopyPool::column_instance(), &pc, /*negative_mu=*/true))
    return RVT_OK;
  q.mu[q.n] = pc.has_mu ? pc.mu : 0.0;
  q.hard[q.n] = pc.has_mu ? 0 : 1;
  ++q.n;
  *queued = true;
  return invalidate_columns(c, find_block(c, dG), col0, 1, true);
}

// rvt_block_upload_columns, columns that are what consolidate() almost always leaves — hard calls plus at most one other value
// per column (the imputed mean): they cross PCIe as 2-bit codes.  The staging threads pack them (host_stage.h pack_column_f64,
// as for the genes of rvt_submit_gene), 1/32 of the bytes go over the link, a small kernel writes the doubles of the block
// back; their content is known from the packing, so the same column pass follows as behind the queued single columns.
// *packed = false: some column holds more (dosages) — nothing has been written.
static int upload_packed_columns(rvt_ctx* c, double* dG, int col0, int ncols, const double* G, bool* packed) {
  *packed = false;
  int rc = stage_ready(c);
  if (rc) return rc;
  const size_t N = (size_t)block_dims(c).N, pitch = hcp_row_pitch(N);
  const size_t need = pitch * (size_t)ncols + sizeof(double) * (size_t)ncols;
  // (io_stream: the stream of the expansion that last read the rows, and — outside a gene submission — of the staged DMA)
  HIP_TRY(c, c->d_colpack.grow(need, need + need / 2, c->io_stream, true, 0, "d_colpack"));
  if (pitch > c->stage.chunk_bytes) return RVT_OK;
  std::vector<PackedColumn> pc((size_t)ncols);
  const int prc = c->stage.pack_f64(c->d_colpack, pitch, G, N, N, (size_t)ncols, CopyPool::pack_instance(), pc.data());
  if (prc == 1) return fail(c, RVT_E_HIP, "packing the uploaded columns failed");
  if (prc != 0) return RVT_OK;
  std::vector<double> mu((size_t)ncols);
  std::vector<int> hard((size_t)ncols);
  for (int j = 0; j < ncols; ++j) {
    mu[(size_t)j] = pc[(size_t)j].has_mu ? pc[(size_t)j].mu : 0.0;
    hard[(size_t)j] = pc[(size_t)j].has_mu ? 0 : 1;
  }
  *packed = true;
  rc = expand_packed_rows(c, pitch, (size_t)ncols, mu.data(), ncols, dG, col0);
  if (!rc) rc = invalidate_columns(c, find_block(c, dG), col0, ncols, true);
  return rc ? rc : packed_columns_passes(c, dG, col0, ncols, mu.data(), hard.data());
}

// rvt_block_upload_columns, anything else (dosages; hard calls switched off; N below 4096): the columns cross as doubles, and
// their content (hard calls or not) is found by one read of data that has just crossed PCIe at a hundredth of the rate —
// rvt_score_block picks its kernel by it.  Under an unweighted null model that read is the column pass of MetaCov's hard-call
// band itself (cov_hc_prep_kernel on the one column): int8 copy, sum and the row of T = G'X stay with the block, the flag
// falls out of its value test.
static int upload_fp64_columns(rvt_ctx* c, double* dG, int col0, int ncols, const double* G) {
  const size_t N = (size_t)block_dims(c).N, ld = (size_t)block_dims(c).ld;
  HIP_TRY(c, hipMemcpy2D(dG + (size_t)col0 * ld, sizeof(double) * ld, G, sizeof(double) * N, sizeof(double) * N, ncols,
                         hipMemcpyHostToDevice));
  ColKind* ck = find_block(c, dG);
  int rc = invalidate_columns(c, ck, col0, ncols, true);
  if (rc || !ck || !c->hc_enabled) return rc;
  if ((rc = ensure_flags(c, *ck))) return rc;
  const bool cache = ensure_cache(c, *ck);
  const int d = c->nc.d, dmax = d <= 4 ? 4 : (d <= 8 ? 8 : RVT_MAX_COV);
  const int64_t ldk = ck->ldk, ldk4 = ck->ldk4;
  const size_t part_bytes = sizeof(double) * (size_t)kCovSlices * rvt_ctx::kColQueue * (RVT_MAX_COV + 3);
  if (cache) HIP_TRY(c, c->d_cc_part.grow(part_bytes, part_bytes, c->io_stream, true));
  for (int col = col0; col < col0 + ncols; ++col) {
    if (!cache) {
      rc = enqueue_classify(c, dG + (size_t)col * ld, 1, (int64_t)N, (int64_t)ld, c->io_stream, ck->d_flags + col);
      if (rc) return rc;
      continue;
    }
    static const int one = 1;
    HIP_TRY(c, hipMemcpyAsync(ck->d_flags + col, &one, sizeof(int), hipMemcpyHostToDevice, c->io_stream));
    // (this pass knows no other value: the slot's mask of an earlier occupant must not survive it — a window that mixes
    //  this column with mean-imputed ones reads the masks of all its columns)
    if (ck->d_m4) HIP_TRY(c, hipMemsetAsync(ck->d_m4 + (size_t)col * (size_t)ldk4, 0, (size_t)ldk4, c->io_stream));
    const int slices = (int)std::max<int64_t>(1, std::min<int64_t>(kCovSlices, (int64_t)N / 4096 + 1));
    launch_cov_prep(c->io_stream, d, true, dim3(1, (unsigned)slices), dG + (size_t)col * ld, (int64_t)N, (int64_t)ld, 1, c->d_X,
                    ck->d_i8 + (size_t)col * (size_t)ldk, ldk, c->d_cc_part, nullptr, nullptr, ck->d_flags + col, 0, 0,
                    ck->d_i4 + (size_t)col * (size_t)ldk4, ldk4);
    hipLaunchKernelGGL(cov_hc_finish_kernel, dim3(1), dim3(256), 0, c->io_stream, c->d_cc_part, slices, 1, d, dmax,
                       ck->d_cs + col, ck->d_poly + col, ck->d_T + (size_t)col * RVT_MAX_COV);
    HIP_TRY(c, hipGetLastError());
    ck->valid[(size_t)col] = 1;
  }
  return RVT_OK;
}

int rvt_block_upload_columns(rvt_ctx* c, double* dG, int col0, int ncols, const double* G) {
  if (!c || !dG || !G || col0 < 0 || ncols < 1) return fail(c, RVT_E_INVALID, "bad upload");
  if (!c->have_null && !c->have_fam) return fail(c, RVT_E_STATE, "set the null model first");
  if (int rc = check_columns(c, dG, col0, ncols)) return rc;
  hipSetDevice(c->device);
  const bool pack = c->hc_enabled && !getenv("RVT_UPLOAD_FP64") && block_dims(c).N >= 4096;
  if (pack && ncols == 1 && !getenv("RVT_UPLOAD_NO_QUEUE")) {
    bool queued = false;
    int rc = queue_column(c, dG, col0, G, &queued);
    if (rc || queued) return rc;
  }
  // (a column that cannot be packed goes behind whatever was queued before it)
  if (int rc = flush_col_queue(c)) return rc;
  if (pack) {
    bool packed = false;
    int rc = upload_packed_columns(c, dG, col0, ncols, G, &packed);
    if (rc || packed) return rc;
  }
  return upload_fp64_columns(c, dG, col0, ncols, G);
}

// ---- dominant / recessive recoding on the device (recode_kernels.hip.h) ---------------------------------------------------------
// measurement (rvt_set_profiling): HIP events directly in front of and behind the count pass (0, 1) and the write pass (2, 3)
static int recode_mark(rvt_ctx* c, int k, hipStream_t st) {
  if (!c->profiling) return RVT_OK;
  if (!c->ev_recode[k]) HIP_TRY(c, hipEventCreate(&c->ev_recode[k]));
  HIP_TRY(c, hipEventRecord(c->ev_recode[k], st));
  return RVT_OK;
}
static int recode_times(rvt_ctx* c) {  // (behind the call's last synchronisation)
  if (!c->profiling) return RVT_OK;
  float a = 0.0f, b = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&a, c->ev_recode[0], c->ev_recode[1]));
  HIP_TRY(c, hipEventElapsedTime(&b, c->ev_recode[2], c->ev_recode[3]));
  c->recode_ms[0] = a, c->recode_ms[1] = b;
  return RVT_OK;
}
int rvt_recode_last_timing(rvt_ctx* c, double* ms2) {
  if (!c || !ms2) return RVT_E_INVALID;
  ms2[0] = c->recode_ms[0], ms2[1] = c->recode_ms[1];
  return RVT_OK;
}

// The skeleton of both recodings of ncols columns into [dst_col, dst_col + ncols) of dst, the arguments checked by the caller:
// a count pass over the source (`per` integer counts per column; count(k0, nk, d_cnt) launches it for columns [k0, k0 + nk)),
// the counts to the host (and to `counts`), tally(q, &nonmissing, &carriers) on a column's counts, avg = carriers / nonmissing
// (0 when nothing is called): the one division of the reference's s / numGeno, on exact integers; then the write pass
// (write(k0, nk, d_avg)) and the columns' bookkeeping.  The recoded column holds 0 / 1 and, where a call was missing, avg —
// "hard calls plus one other value" unless avg is 0 or 1: what a packed upload of the same columns leaves.  Synchronous, as
// rvt_block_copy_columns: the device calls run on other streams.
}  // extern "C"
template <class Count, class Tally, class Write>
static int recode_columns(rvt_ctx* c, double* dst, int dst_col, int ncols, int per, long long* counts, Count count, Tally tally,
                          Write write) {
  if (ncols == 0) return RVT_OK;
  hipSetDevice(c->device);
  if (int rc = flush_col_queue(c)) return rc;  // (source columns may still be queued; the target's land first and are overwritten)
  hipStream_t st = c->io_stream;               // behind the uploads and the passes that follow them
  Layout L;
  const size_t n_cnt = (size_t)per * (size_t)ncols;
  const size_t o_cnt = L.take(sizeof(unsigned long long) * n_cnt), o_avg = L.take(sizeof(double) * (size_t)ncols);
  // (the poison fill runs on `st`, in front of the clearing of the counts)
  HIP_TRY(c, c->d_recode_ws.grow(L.total, L.total + L.total / 2, st, true));
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(c->d_recode_ws + o_cnt);
  double* d_avg = reinterpret_cast<double*>(c->d_recode_ws + o_avg);
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * n_cnt, st));
  if (int rc = recode_mark(c, 0, st)) return rc;
  constexpr int kCols = 32768;  // columns per launch (gridDim.y)
  for (int k0 = 0; k0 < ncols; k0 += kCols) count(k0, std::min(kCols, ncols - k0), d_cnt + (size_t)per * (size_t)k0, st);
  HIP_TRY(c, hipGetLastError());
  if (int rc = recode_mark(c, 1, st)) return rc;
  std::vector<unsigned long long> cnt(n_cnt);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(unsigned long long) * n_cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  const long long N = c->nc.N;
  std::vector<double> avg((size_t)ncols), mu((size_t)ncols);
  std::vector<int> hard((size_t)ncols);
  for (int k = 0; k < ncols; ++k) {
    long long nonmissing = 0, carriers = 0;
    tally(cnt.data() + (size_t)per * (size_t)k, &nonmissing, &carriers);
    avg[(size_t)k] = nonmissing > 0 ? (double)carriers / (double)nonmissing : 0.0;
    hard[(size_t)k] = (nonmissing == N || avg[(size_t)k] == 0.0 || avg[(size_t)k] == 1.0) ? 1 : 0;
    mu[(size_t)k] = hard[(size_t)k] ? 0.0 : avg[(size_t)k];
  }
  if (counts)
    for (size_t i = 0; i < n_cnt; ++i) counts[i] = (long long)cnt[i];
  int rc = small_h2d(c, d_avg, avg.data(), sizeof(double) * (size_t)ncols);
  if (!rc) rc = invalidate_columns(c, find_block(c, dst), dst_col, ncols, true);
  if (!rc) rc = recode_mark(c, 2, st);
  if (rc) return rc;
  for (int k0 = 0; k0 < ncols; k0 += kCols) write(k0, std::min(kCols, ncols - k0), d_avg + k0, st);
  HIP_TRY(c, hipGetLastError());
  if ((rc = recode_mark(c, 3, st))) return rc;
  if ((rc = packed_columns_passes(c, dst, dst_col, ncols, mu.data(), hard.data()))) return rc;
  HIP_TRY(c, sync_stream(st));
  return recode_times(c);
}
extern "C" {

int rvt_block_recode(rvt_ctx* c, double* dst, int dst_col, const double* src, int src_col, int ncols, int coding, long long* counts) {
  if (!c || !dst || !src || dst_col < 0 || src_col < 0 || ncols < 0) return fail(c, RVT_E_INVALID, "bad recode");
  if (coding != RVT_CODING_DOMINANT && coding != RVT_CODING_RECESSIVE)
    return fail(c, RVT_E_INVALID, "coding %d: 1 = dominant, 2 = recessive", coding);
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  if (int rc = check_columns(c, src, src_col, ncols)) return rc;
  if (int rc = check_columns(c, dst, dst_col, ncols)) return rc;
  // one block, two ranges that overlap without being the same: a workgroup would read columns another one is writing
  if (dst == src && dst_col != src_col && std::abs(dst_col - src_col) < ncols)
    return fail(c, RVT_E_INVALID, "source and target columns overlap without being the same");
  const long long N = c->nc.N, ld = c->null_ld;
  const double threshold = coding == RVT_CODING_DOMINANT ? 0.5 : 1.5;
  return recode_columns(
      c, dst, dst_col, ncols, 2, counts,
      [&](int k0, int nk, unsigned long long* d_cnt, hipStream_t st) {
        hipLaunchKernelGGL(recode_count_kernel, dim3(recode_slices(N / 2, nk), (unsigned)nk), dim3(kRecodeThreads), 0, st,
                           src + (size_t)(src_col + k0) * (size_t)ld, N, ld, threshold, d_cnt);
      },
      [](const unsigned long long* q, long long* nonmissing, long long* carriers) {
        *nonmissing = (long long)q[0], *carriers = (long long)q[1];
      },
      [&](int k0, int nk, const double* d_avg, hipStream_t st) {
        hipLaunchKernelGGL(recode_write_kernel, dim3(recode_slices(N / 2, nk), (unsigned)nk), dim3(kRecodeThreads), 0, st,
                           src + (size_t)(src_col + k0) * (size_t)ld, dst + (size_t)(dst_col + k0) * (size_t)ld, N, ld, threshold,
                           d_avg);
      });
}

// counts[4 r + (0 .. 3)] += the calls of 0 / 1 / 2 / missing of row r of n_rows (at most 65 535) consecutive .bed rows; the
// counts must be zero before.  rvt_kinship.hip's site pass counts with the same kernel through this launcher.
void bed_row_counts(hipStream_t st, const unsigned char* d_rows, long long cb, long long N, int n_rows, unsigned long long* d_cnt) {
  hipLaunchKernelGGL(recode_bed_count_kernel, dim3(recode_slices((cb + 3) / 4, n_rows), (unsigned)n_rows), dim3(kRecodeThreads), 0, st,
                     d_rows, cb, N, d_cnt);
}

// n_rows (at most 65 535) consecutive .bed rows as fp64 columns of leading dimension ld, missing calls -> d_mu[row]
// (bed_expand_columns_kernel).  rvt_fam.hip's front stage over resident rows expands with it when U is column-compressed.
void bed_rows_expand(hipStream_t st, const unsigned char* d_rows, long long cb, const double* d_mu, long long N, long long ld,
                     int n_rows, double* G) {
  hipLaunchKernelGGL(bed_expand_columns_kernel<BedRowsAt>, dim3((unsigned)((N + 1023) / 1024), (unsigned)n_rows), dim3(256), 0, st,
                     BedRowsAt{d_rows, cb}, d_mu, N, ld, G);
}

// The site pass's counts of n_rows consecutive rows (n0 n1 n2 missing per row) into d_cnt, which is zeroed here, in launches of
// at most kBedCountRows rows (gridDim.y); with host or counts, bed_counts_host behind it.
int bed_piece_counts(rvt_ctx* c, hipStream_t st, const unsigned char* d_rows, long long cb, long long N, long long n_rows,
                     unsigned long long* d_cnt, std::vector<unsigned long long>* host, long long* counts) {
  constexpr long long kBedCountRows = 32768;
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 4 * (size_t)n_rows, st));
  for (long long k0 = 0; k0 < n_rows; k0 += kBedCountRows)
    bed_row_counts(st, d_rows + (size_t)k0 * (size_t)cb, cb, N, (int)std::min(kBedCountRows, n_rows - k0), d_cnt + 4 * (size_t)k0);
  HIP_TRY(c, hipGetLastError());
  return host || counts ? bed_counts_host(c, st, d_cnt, n_rows, host, counts) : RVT_OK;
}

// The counts of n_rows rows copied to the host, st waited for: into host (optional) and, as long long, into the caller's counts
// (optional).  On its own where a caller queues its site kernel between the count and the copy.
int bed_counts_host(rvt_ctx* c, hipStream_t st, const unsigned long long* d_cnt, long long n_rows,
                    std::vector<unsigned long long>* host, long long* counts) {
  std::vector<unsigned long long> own;
  if (!host) host = &own;
  host->resize(4 * (size_t)n_rows);
  HIP_TRY(c, hipMemcpyAsync(host->data(), d_cnt, sizeof(unsigned long long) * host->size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, sync_stream(st));
  if (counts)
    for (size_t i = 0; i < host->size(); ++i) counts[i] = (long long)(*host)[i];
  return RVT_OK;
}

// (rvt_engine_int.h has the contract.)  First the refusals by the models present, which hold for rows the engine does not know
// as well: rvt_bed_alloc sizes a matrix for the ordinary null model's N when one is set, so an ordinary null model of another N
// beside the consuming one means rows of another pitch; and the multiple-trait call refuses a family null model of another N in
// a context without an ordinary one.  Then the record of the matrix the rows lie in.
int bed_rows_span(rvt_ctx* c, const char* who, const unsigned char* d_rows, int64_t V, BedModel model, int64_t* pitch) {
  static const char* const kName[] = {"ordinary", "family", "multiple-trait", "GrammarGamma"};
  const char* name = kName[(int)model];
  const long long N = model == BedModel::kNull ? c->nc.N : model == BedModel::kFam ? c->fam_nc.N : model == BedModel::kMt ? c->mt_N : c->gg_N;
  if (c->have_null && c->nc.N != N)
    return fail(c, RVT_E_STATE, "%s: the null model has N = %lld, the %s null model N = %lld (the resident rows have the former's pitch)",
                who, (long long)c->nc.N, name, N);
  if (model == BedModel::kMt && !c->have_null && c->have_fam && c->fam_nc.N != N)
    return fail(c, RVT_E_STATE, "%s: the multiple-trait null and the context's null model differ in N", who);
  *pitch = bed_pitch(N);
  auto it = c->bed_mats.upper_bound(d_rows);  // the matrix with the last base at or below d_rows, if the rows lie inside it
  if (it == c->bed_mats.begin()) return RVT_OK;
  const rvt_ctx::BedMatrix& m = (--it)->second;
  const long long first = bed_span((uint64_t)(uintptr_t)it->first, m.n_variants, m.pitch, (uint64_t)(uintptr_t)d_rows, V);
  if (first == kBedSpanOutside) return RVT_OK;
  if (m.N != N)
    return fail(c, RVT_E_STATE, "%s: the resident matrix was sized for N = %lld, the %s null model has N = %lld", who, (long long)m.N,
                name, N);
  if (first == kBedSpanOffRow)
    return fail(c, RVT_E_INVALID, "%s: the address is not on a row boundary of its resident matrix (rows of %lld bytes)", who,
                (long long)m.pitch);
  if (first == kBedSpanLeaves)
    return fail(c, RVT_E_INVALID, "%s: %lld rows leave the resident matrix (%lld rows)", who, (long long)V, (long long)m.n_variants);
  *pitch = m.pitch;
  return RVT_OK;
}

int rvt_bed_recode_block(rvt_ctx* c, const unsigned char* d_rows, int V, int coding, double* dG, int col0, long long* counts) {
  if (!c || !d_rows || !dG || V < 0 || col0 < 0) return fail(c, RVT_E_INVALID, "bad recode");
  if (coding != RVT_CODING_DOMINANT && coding != RVT_CODING_RECESSIVE)
    return fail(c, RVT_E_INVALID, "coding %d: 1 = dominant, 2 = recessive", coding);
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  if (int rc = check_columns(c, dG, col0, V)) return rc;
  int64_t cb = 0;
  if (int rc = bed_rows_span(c, "rvt_bed_recode_block", d_rows, V, BedModel::kNull, &cb)) return rc;
  const long long N = c->nc.N, ld = c->null_ld;
  return recode_columns(
      c, dG, col0, V, 4, counts,
      [&](int k0, int nk, unsigned long long* d_cnt, hipStream_t st) {
        bed_row_counts(st, d_rows + (size_t)k0 * (size_t)cb, cb, N, nk, d_cnt);
      },
      [&](const unsigned long long* q, long long* nonmissing, long long* carriers) {
        *nonmissing = (long long)(q[0] + q[1] + q[2]);
        *carriers = (long long)(coding == RVT_CODING_DOMINANT ? q[1] + q[2] : q[2]);
      },
      [&](int k0, int nk, const double* d_avg, hipStream_t st) {
        hipLaunchKernelGGL(recode_bed_expand_kernel, dim3(recode_slices(cb, nk), (unsigned)nk), dim3(kRecodeThreads), 0, st,
                           d_rows + (size_t)k0 * (size_t)cb, cb, N, ld, coding == RVT_CODING_RECESSIVE ? 1 : 0, d_avg,
                           dG + (size_t)(col0 + k0) * (size_t)ld);
      });
}

int rvt_block_download_columns(rvt_ctx* c, const double* dG, int col0, int ncols, double* G_host) {
  if (!c || !dG || !G_host || col0 < 0 || ncols < 0) return fail(c, RVT_E_INVALID, "bad download");
  if (!c->have_null && !c->have_fam) return fail(c, RVT_E_STATE, "set the null model first");
  if (int rc = check_columns(c, dG, col0, ncols)) return rc;
  if (ncols == 0) return RVT_OK;
  hipSetDevice(c->device);
  if (int rc = flush_col_queue(c)) return rc;
  HIP_TRY(c, sync_stream(c->io_stream));  // (queued uploads, expansions and recodings write what is copied here)
  const size_t N = (size_t)block_dims(c).N, ld = (size_t)block_dims(c).ld;
  HIP_TRY(c, hipMemcpy2D(G_host, sizeof(double) * N, dG + (size_t)col0 * ld, sizeof(double) * ld, sizeof(double) * N, (size_t)ncols,
                         hipMemcpyDeviceToHost));
  return RVT_OK;
}

int rvt_block_move_columns(rvt_ctx* c, double* dG, int dst_col, int src_col, int ncols) {
  if (!c || !dG || dst_col < 0 || src_col < dst_col || ncols < 0) return fail(c, RVT_E_INVALID, "bad move");
  if (int rc = check_columns(c, dG, src_col, ncols)) return rc;  // (dst_col <= src_col: the target lies inside then)
  if (ncols == 0 || dst_col == src_col) return RVT_OK;
  hipSetDevice(c->device);
  if (int rc = flush_col_queue(c)) return rc;
  const size_t ld = (size_t)block_dims(c).ld;
  HIP_TRY(c, sync_stream(c->io_stream));  // (the passes behind the last uploads write the cache this call moves)
  // forward move of a possibly overlapping range: in pieces no longer than the shift, in increasing order — a piece never
  // overwrites data that has not been read (a ring that drops more than it keeps moves in ONE copy)
  const int shift = src_col - dst_col;
  for (int k0 = 0; k0 < ncols; k0 += shift) {
    const int nk = std::min(shift, ncols - k0);
    HIP_TRY(c, hipMemcpyAsync(dG + (size_t)(dst_col + k0) * ld, dG + (size_t)(src_col + k0) * ld, sizeof(double) * ld * (size_t)nk,
                              hipMemcpyDeviceToDevice, c->stream));
  }
  ColKind* ck = find_block(c, dG);
  if (ck)
    if (int rc = move_col_cache(c, ck, dst_col, ck, src_col, ncols, c->stream)) return rc;
  HIP_TRY(c, sync_stream(c->stream));
  if (ck && ck->d_flags) {
    std::vector<int> f((size_t)ck->cols);
    HIP_TRY(c, hipMemcpyAsync(f.data(), ck->d_flags, sizeof(int) * f.size(), hipMemcpyDeviceToHost, c->io_stream));
    HIP_TRY(c, sync_stream(c->io_stream));
    std::memmove(f.data() + dst_col, f.data() + src_col, sizeof(int) * (size_t)ncols);
    HIP_TRY(c, hipMemcpyAsync(ck->d_flags, f.data(), sizeof(int) * f.size(), hipMemcpyHostToDevice, c->io_stream));
    HIP_TRY(c, sync_stream(c->io_stream));
  }
  return RVT_OK;
}

}  // extern "C"
