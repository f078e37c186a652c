// rvtests_amd — what the engine's translation units share: the context, its pools and streams, the small host helpers
// (error reporting, stream waits, arenas, launch timing, the split of the sample axis) and the kernel headers.  Everything here
// has internal linkage or is a type: each translation unit (rvt_engine.hip, rvt_stream.hip) gets its own copy of the helpers;
// what one unit calls in another is declared at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <map>
#include <string>
#include <unordered_map>
#include <thread>
#include <vector>
#include <cmath>
#include <functional>
#include "kernels.hip.h"
#include "suffstat_lat.hip.h"
#include "suffstat_hcp.hip.h"
#include "suffstat_hcx.hip.h"
#include "suffstat_fdx.hip.h"
#include "host_stage.h"
#include "block_pool.h"

namespace rvt {  // defined in k2_unweighted.hip / k2_weighted.hip
void k2_launch_group_w0(int group, dim3 grid, hipStream_t st, const GeneDesc* d_desc, const int* list, int n_wparts,
                        NullDev nd, long long N, long long ld, int d);
void k2_launch_group_w1(int group, dim3 grid, hipStream_t st, const GeneDesc* d_desc, const int* list, int n_wparts,
                        NullDev nd, long long N, long long ld, int d);
void k2_launch_panel_w0(dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullDev nd, long long N, long long ld,
                        int d);
void k2_launch_panel_w1(dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullDev nd, long long N, long long ld,
                        int d);
// (false: no kernel of that launch shape is compiled in)
bool k2_launch_hc(int MT, int depth, int waves, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, long long N,
                  long long ld, int d);
bool k2_hc_has_shape(int MT, int depth, int waves);
int k2_hc_any_depth(int MT);
void k2_launch_hc_any(unsigned classes, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, long long N,
                      long long ld, int d);
void k2_launch_hcw(int MT, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTileW nt, long long N, long long ld,
                   int d);
void k2_launch_hcx(int MT, dim3 grid, hipStream_t st, const GeneDesc* d_desc, const NullTileX& nt, long long N, long long ld,
                   int d);
void k2_launch_fdx(int MT, dim3 grid, hipStream_t st, const GeneDesc* d_desc, const NullTileF& nt, long long N, long long ld,
                   int d);
void k2_launch_lat(int MT, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, double den, long long N,
                   long long ld, int d);
void k2_launch_hcp(int MT, dim3 grid, hipStream_t st, const GeneDesc* d_desc, NullTile nt, long long N, long long ld,
                   int d, const HcpPlanes* planes = nullptr, bool score_only = false);
void k2_launch_hcp_binary_score(dim3 grid, hipStream_t st, const GeneDesc* d_desc, const HcpPlanes& pl, long long N, long long ld);
void k2_launch_classify(dim3 grid, hipStream_t st, const double* G, long long N, long long ld, int M, int* flag);
}  // namespace rvt
#include "fam_kernels.hip.h"
#include "rot_gemm.hip.h"
#include "perm_kernels.hip.h"
#include "vtprice_kernels.hip.h"
#include "burdenperm_kernels.hip.h"
#include "vcf_kernels.hip.h"
#include "bgen_kernels.hip.h"
#include "jacobi_tile.h"
#include "rvt_hyper.h"

using namespace rvt;

namespace {

constexpr int kMaxMT = 6;  // widest single-pass tile configuration instantiated below

// Wait for a stream by polling.  A blocking hipStreamSynchronize() relies on a completion interrupt; on a fresh box
// one such wake-up was seen to go missing (the kernels had long finished while the host slept for seconds), so the
// engine never blocks in the runtime: it spins briefly, then sleeps in 20 us slices between hipStreamQuery calls.
hipError_t sync_stream(hipStream_t st) {
  hipError_t e;
  int spins = 0;
  while ((e = hipStreamQuery(st)) == hipErrorNotReady) {
    if (++spins > 64) {
      struct timespec ts = {0, 20000};
      nanosleep(&ts, nullptr);
    }
  }
  return e;
}

// Owner of one device allocation (Pinned: one pinned host allocation) of T; `cap` is its size in BYTES.  Freed by reset()
// and by the destructor, so the context's members and per-call temporaries need no teardown of their own.  It converts to
// T* where a raw pointer is expected (kernel arguments, copies, pointer arithmetic).
template <class T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p), std::swap(cap, o.cap); return *this; }
  ~DevBuf() { reset(); }
  T* get() const { return p; }
  operator T*() const { return p; }
  hipError_t reset() {
    const hipError_t e = !p ? hipSuccess : Pinned ? hipHostFree((void*)p) : hipFree((void*)p);
    p = nullptr, cap = 0;
    return e;
  }
  // Grow-only: when fewer than `need` bytes are held, the old block is freed (after `sync` has drained, when given: its last
  // reader may still be queued there) and `want` bytes are allocated — uninitialised, or filled with the RVT_POISON byte
  // when `poison` is set (tests: no result may depend on what a fresh allocation happens to hold).
  // A block that is already large enough is handed over as the last call left it — unless RVT_SCRIBBLE=<byte> is set (tests:
  // no result may depend on what an earlier call left in a work space): a `poison` request then refills it (scribble).
  // `what` names the buffer in the trace of the refills.
  hipError_t grow(size_t need, size_t want, hipStream_t sync = nullptr, bool poison = false, unsigned flags = 0,
                  const char* what = nullptr) {
    if (cap >= need) return poison ? scribble(sync, what) : hipSuccess;
    hipError_t e = (p && sync) ? sync_stream(sync) : hipSuccess;
    if (e == hipSuccess) e = reset();
    if (e != hipSuccess) return e;
    void* q = nullptr;
    e = Pinned ? hipHostMalloc(&q, want, flags) : hipMalloc(&q, want);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q), cap = want;
    // With a stream given the fill is queued there — the stream the block's users run on, so they see it done.  On the null
    // stream it may still be pending when hipMemset returns, and a non-blocking stream does not wait for it: a late fill
    // overwrote the first results written into the block.  Without a stream the blocking fill stays as it was.
    if (const char* v = poison ? getenv("RVT_POISON") : nullptr)
      e = sync ? hipMemsetAsync(q, atoi(v) & 0xff, want, sync) : hipMemset(q, atoi(v) & 0xff, want);
    return e;
  }
  // RVT_SCRIBBLE=<byte> (tests; a no-op otherwise): fill the WHOLE held block with the byte, on `st` — the stream the block's
  // users run on: behind the last reader of the previous call, in front of the first kernel of this one —, or, without a
  // stream, blocking between two drains of the device.  RVT_SCRIBBLE_TRACE=1 prints one line per refill to stderr.
  hipError_t scribble(hipStream_t st, const char* what = nullptr) {
    const char* v = p ? getenv("RVT_SCRIBBLE") : nullptr;
    if (!v) return hipSuccess;
    hipError_t e;
    if (st) {
      e = hipMemsetAsync((void*)p, atoi(v) & 0xff, cap, st);
    } else {
      e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipMemset((void*)p, atoi(v) & 0xff, cap);
      if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (getenv("RVT_SCRIBBLE_TRACE")) fprintf(stderr, "rvt: scribble %s %zu bytes\n", what ? what : "-", cap);
    return e;
  }
  hipError_t alloc(size_t bytes, unsigned flags = 0) {  // a fresh block of `bytes`
    reset();
    return grow(bytes, bytes, nullptr, false, flags);
  }
};
template <class T>
using PinBuf = DevBuf<T, true>;

// 256-byte-aligned offsets of the sub-buffers of one work-space allocation, in one pass: `total` is the bytes to allocate
struct Layout {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t o = total;
    total += (bytes + 255) / 256 * 256;
    return o;
  }
};

struct ProfEvent {
  int family;  // 0 suffstat (general fp64 kernel), 1 burden, 2 stats, 3 pvalue, 4 suffstat (hard-call kernel)
  hipEvent_t a, b;
};

}  // namespace

// One in-flight batch: its stream, workspace, pinned staging and where the results go.  Several slots let the
// latency-bound tail of batch i (eigen / p-value kernels, few waves) overlap the bandwidth-bound head of
// batch i+1 (sufficient statistics) on a second HIP stream.
struct Slot {
  hipStream_t stream = nullptr;
  DevBuf<char> arena;   // the batch's work space (grow-only)
  PinBuf<char> h_stage;
  rvt_gene_result* pending_out = nullptr;
  bool* pending_done = nullptr;  // set when the batch's records have been handed over (streaming interface)
  rvt_gene_result* h_results = nullptr;
  int pending_n = 0;
  unsigned long long seq = 0;  // launch order
};
constexpr int kSlots = RVT_MAX_INFLIGHT;

// What the engine's own decoder wrote into a gene's block: Pending::kind, and — as one byte per gene — run_batch's `kind`.
enum BlockKind : int {
  kKindUnknown = -1,  // fp64 from the caller: the content hint decides (rvt_set_content_hint)
  kKindDosage = 0,    // dosages (BGEN)
  kKindHardCall = 1,  // hard calls (+ imputed means)
  kKindDecimal = 2,   // decimal dosages (VCF text)
  kKindPacked = 3,    // the block holds PLINK 2-bit rows, not doubles
};
constexpr int kKindPlanesFlag = 0x10;  // beside kKindPacked: T = G'[X | rr] from the null tile's digit planes (resident .bed genes)
struct KindBits {
  int kind;     // a BlockKind
  bool planes;
};
inline signed char encode_kind(int kind, bool planes) {
  return (signed char)(kind == kKindPacked && planes ? (kind | kKindPlanesFlag) : kind);
}
inline KindBits decode_kind(const signed char* kind, int g) {
  if (!kind || kind[g] < 0) return {kKindUnknown, false};
  return {kind[g] & 0xf, (kind[g] & kKindPlanesFlag) != 0};
}

// What a streaming entry point is handed (submit_common's `in`).  The values of kRaw, kI8, kBed and kBedDev are public: they are
// the `kind` of rvt_submit_genes.
enum class GeneInput : int {
  kF64 = 0,        // imputed doubles and the caller's allele frequencies (rvt_submit_gene)
  kRaw = 1,        // doubles with missing codes, consolidated on the device
  kI8 = 2,         // one byte per hard call
  kBed = 3,        // PLINK 2-bit rows in host memory
  kVcfGt = 4,      // VCF record text, genotypes
  kVcfDosage = 5,  // VCF record text, a dosage tag
  kBgen = 6,       // BGEN probability blocks
  kBedDev = 7,     // PLINK 2-bit rows of a matrix resident on the device
};
struct GeneInputTraits {
  BlockKind expanded;  // what the gene's fp64 block holds when the input is expanded
  int decoded;         // Pending::decoded: 1 VCF text, 2 BGEN blocks (the submission has an input-error word), else 0
  bool packs;          // may stay a block of 2-bit rows when the gene's tests allow it (packed_eligible)
};
inline GeneInputTraits gene_input_traits(GeneInput in) {
  switch (in) {
    case GeneInput::kF64: return {kKindUnknown, 0, true};
    case GeneInput::kRaw: return {kKindUnknown, 0, false};
    case GeneInput::kI8: return {kKindHardCall, 0, true};
    case GeneInput::kBed: return {kKindHardCall, 0, true};
    case GeneInput::kVcfGt: return {kKindHardCall, 1, false};
    case GeneInput::kVcfDosage: return {kKindDecimal, 1, false};
    case GeneInput::kBgen: return {kKindDosage, 2, false};
    case GeneInput::kBedDev: return {kKindHardCall, 0, true};
  }
  return {kKindUnknown, 0, false};
}
constexpr rvt_params kDefaultParams{1.0, 25.0, 1.0, 25.0, 0, 0.05};

struct rvt_ctx {
  int device = 0;
  Slot slots[kSlots];
  unsigned long long launch_seq = 0;
  hipStream_t stream = nullptr;  // == slots[0].stream (set-up work, rvt_stream())
  hipStream_t io_stream = nullptr;  // host copies + consolidation of the streaming interface: never behind a batch
  hipStream_t k2_stream = nullptr;  // the sufficient-statistics launches of all slots serialise here
  hipStream_t k2b_stream = nullptr; // ... except the general-path launches of a batch that also has hard-call genes: a
                                    // handful of genes per launch cannot fill the chip, so they run beside the others
  bool cu_partitioned = false;
  // ---- related samples (FastLMM null + FamSKAT) ----
  bool have_kin = false, have_fam = false;
  int64_t kin_N = 0;
  // eigenvectors of the kinship as kRotPlanesU signed base-128 digit planes (rot_gemm.hip.h): plane p at
  // d_Uq + p * uq_plane, row k (= column k of U) at k * uq_ldk; scaled by 2^uq_sexp
  DevBuf<signed char> d_Uq;
  // sparse form of U (<= 64 non-zeros per eigenvector on average: families in any sample order), column-compressed;
  // used by the rotation when the K-chunk ranges (d_uq_range) do not apply; null otherwise
  DevBuf<long long> d_csc_ptr;
  // row-compressed copy of the same sparse U (U v for rvt_fit_grammar_null), made from d_csc_* on first use
  DevBuf<long long> d_csr_ptr;
  DevBuf<int> d_csr_cols;
  DevBuf<double> d_csr_vals;
  DevBuf<int> d_csc_rows;
  DevBuf<double> d_csc_vals;
  // family form (rvt_set_kinship_families): d_csc_* then hold every entry of every family's block (eigenpair fam_ptr[f] + j =
  // column j of block f, rows = the family's members in ascending sample order), d_Uq / d_uq_range stay null, and the rotation
  // takes rot_fam_kernel over the descriptors below; all null after a dense installation
  DevBuf<long long> d_fam_ptr;  // n_fam + 1
  DevBuf<int> d_fam_members;    // N: the permutation `members`, ascending inside every family
  DevBuf<int> d_fam_of;         // N: family of every eigenpair
  DevBuf<int> d_fam_run;        // fam_runs + 1: first eigenpair of every run of whole families (<= kRotFamRows eigenpairs)
  int64_t fam_count = 0;
  int fam_runs = 0;
  DevBuf<int2> d_uq_range;  // per 256-row panel of the planes: K chunks [x, y) that hold its non-zeros; null = dense U
  double uq_visit = 1.0;       // fraction of the K chunks the rotation visits (1 = dense)
  size_t uq_plane = 0;
  int64_t uq_ldk = 0, uq_rows_pad = 0;
  int uq_sexp = 0;
  DevBuf<signed char> d_rotB;  // digit planes of the columns being rotated (B side of an integer-plane product)
  DevBuf<signed char> d_rotA;  // A side of gemm_tn_planes
  DevBuf<double> d_rot_scale;  // per-column scale (RVT_ROT_MAXCOLS doubles) | column maxima
  DevBuf<int> d_rot_sexp;
  DevBuf<double> d_S;   // N raw eigenvalues
  DevBuf<double> d_u1;  // U'1
  std::vector<double> h_S, h_u1;
  DevBuf<double> d_uxy;  // N x (d+1): U'X | U'y
  DevBuf<double> d_lmm_part;
  NullConsts fam_nc;
  DevBuf<NullConsts> d_fam_nc;
  DevBuf<double> d_fX, d_frr, d_fv, d_fzeros, d_fbeta;
  // family MetaCov null set + constants
  NullConsts famcov_nc;
  DevBuf<NullConsts> d_famcov_nc;
  DevBuf<double> d_cX, d_cv;
  double fam_delta = 0.0;   // delta of the fitted FastLMM null (rvt_fam_null_summary)
  double famcov_b2 = 1.0;  // MetaCovFamBinary: b^2
  double famcov_k1r = 0.0; // u1' D uResid
  DevBuf<double> d_cr;  // uResid (the rr column of the family-covariance null set)
  double famcov_c11 = 0.0, famcov_c1x[RVT_MAX_COV], famcov_zz[RVT_MAX_COV * RVT_MAX_COV],
         famcov_zzinv[RVT_MAX_COV * RVT_MAX_COV];
  DevBuf<double> d_Gp;  // flipped / filtered genotypes of a FamSKAT batch (ld x T)
  DevBuf<double> d_Gt;  // ... rotated by U'
  DevBuf<char> d_bedbatch;   // rvt_submit_genes kind 7: row / gene references and partial counts of one call
  // gene_tnull_hcp: eight digit planes of [X | rr] in operand order + the columns' scales (quantitative null models); under a
  // binary null model those of [v X | res | v] (rvt_score_bed_dev) — a context holds one null model at a time
  DevBuf<unsigned char> d_hcp_xq;
  DevBuf<double> d_hcp_scale;
  DevBuf<char> d_score_bed_w;   // rvt_score_bed_dev, binary trait: descriptors, wave-part records, statistics and results of a chunk
  int hcp_planes_state = 0;     // 0 not built for this null model, 1 ready, -1 the model's columns cannot be carried
  int submit_group = 32;   // genes per asynchronous sub-batch of the streaming interface (RVT_SUBMIT_GROUP, rvt_set_submit_group)
  int64_t fam_cols_ld = 0;  // (the leading dimension d_Gp / d_Gt were sized for)
  // raw / packed genotype submission
  DevBuf<double> d_consol_af;  // af (RVT_MAX_VARIANTS) | fill values (RVT_MAX_VARIANTS)
  DevBuf<ConsolPart> d_consol_parts;
  // allele frequencies of raw / packed submissions whose caller did not ask for them: written into a ring slot and
  // copied back asynchronously; resolved (one stream wait) when the gene's group is launched
  static constexpr int kAfSlots = 128;
  PinBuf<double> h_af_ring;  // kAfSlots x RVT_MAX_VARIANTS, pinned and device-mapped: the kernels write it directly
  unsigned long long af_seq = 0;
  int af_unresolved = 0;
  DevBuf<void> d_consol_i8;
  // packed hand-offs from the host (int8 / 2-bit): a ring of landing buffers and a copy stream of their own, so that the DMA of
  // gene g + 1 runs while the consolidation kernels of gene g read another buffer (one stream serialised them: 3.3 k
  // 2-bit genes/s where the link carries 8 k)
  static constexpr int kPack = 16;  // landing buffers: a consolidation delayed by a batch launch does not stop the copies
  DevBuf<void> d_pack[kPack];
  hipEvent_t ev_pack_copied[kPack] = {}, ev_pack_free[kPack] = {};
  int pack_next = 0;
  hipStream_t copy_stream = nullptr;
  hipStream_t h2d_stream = nullptr;  // where staged_h2d enqueues: io_stream, or copy_stream for the packed hand-offs
  DevBuf<double> d_rot_part;  // split-K partial results of the integer GEMM
  int band_last_path = -1;       // which product the last rvt_cov_band took (rvt_cov_band_last_path)
  DevBuf<double> d_mu_nan;    // packed_columns_pass: the other values of up to kColQueue columns (NaN = none)
  DevBuf<char> d_colpack;     // rvt_block_upload_columns: the columns as 2-bit rows + their other values, before they are expanded
  DevBuf<char> d_recode_ws;   // rvt_block_recode / rvt_bed_recode_block: the columns' integer counts and their avg (grow-only)
  hipEvent_t ev_recode[4] = {};  // with profiling on: around the count pass (0, 1) and the write pass (2, 3) of the last recoding
  double recode_ms[2] = {0.0, 0.0};
  // rvt_cov_band_bed_dev with profiling on: the call's start (0), behind the front stage (1), around the passes (2, 3), the end (4)
  hipEvent_t ev_band_bed[5] = {};
  double band_bed_ms[3] = {0.0, 0.0, 0.0};  // front stage, products + band finish, whole call (rvt_cov_band_bed_last_timing)
  // single columns uploaded one call at a time (MetaCovTest / MetaScoreTest: one site per fit()) are packed into pinned memory
  // and QUEUED: the DMA, the expansion and the column pass run once per kColQueue consecutive columns (flush_col_queue) — the
  // per-call device work (eight HIP calls, ~70 us) was what held the adapter at 9 k sites/s.  ONE RULE: whatever reads a block,
  // or replaces the model the queue was packed for, flushes first (flush_col_queue returns at once on an empty queue).
  static constexpr int kColQueue = 32;
  struct ColQueue {
    PinBuf<unsigned char> h[2];  // kColQueue rows of `pitch` bytes each
    hipEvent_t ev[2] = {nullptr, nullptr};     // recorded behind the DMA that read h[k]
    bool used[2] = {false, false};
    size_t pitch = 0;
    int cur = 0, n = 0, col0 = 0;
    double* dG = nullptr;
    double mu[kColQueue];
    int hard[kColQueue];
    ~ColQueue() {
      for (hipEvent_t e : ev)
        if (e) hipEventDestroy(e);
    }
  } colq;
  DevBuf<char> d_cov_work;    // work space of the MetaCov rectangles (S, T, the band, column statistics): grow-only
  hipEvent_t ev_band_fin[2] = {}, ev_band_copied[2] = {};  // rvt_cov_band: a pass's rows are copied out while the next pass multiplies
  // What the engine knows about a block of rvt_block_alloc, and the one owner of it (the operations are in rvt_meta.hip, "column
  // blocks"): its width; per-column content flags (nonzero = hard calls only; allocated by the first column upload); and, for a
  // ring that MetaCov will read (unweighted model), what the column pass of the hard-call band would compute for a column
  // anyway — int8 copy, E2M1 codes, the mask of the ONE other value, sum, polymorphic flag, row of T = G'X — made behind the
  // column's upload and moved and copied with it, so that a covariance call starts at the integer product.  The cache is an
  // optimisation: a failed allocation leaves the block without one, it does not fail a call.
  struct ColKind {
    int cols = 0;
    DevBuf<int> d_flags;
    DevBuf<signed char> d_i8;    // [cols rounded up + a tile of slack][ldk]
    DevBuf<unsigned char> d_i4;  // [cols][ldk4]: the same hard calls as E2M1 codes, two per byte (band_gemm.hip.h, FP4)
    DevBuf<unsigned char> d_m4;  // [cols][ldk4]: the mask of a column's ONE other value (the imputed mean), same codes
    DevBuf<double> d_mu;         // [cols]: that other value (0 for a column without one)
    DevBuf<double> d_cs;         // [cols] column sums
    DevBuf<int> d_poly;          // [cols]
    DevBuf<double> d_T;          // [cols][RVT_MAX_COV]
    int64_t ldk = 0, ldk4 = 0;
    uint64_t gen = 0;            // the cache was made under null model number `gen`
    bool cache_failed = false;   // the cache could not be allocated once: not retried for this block
    std::vector<unsigned char> valid;  // per column: 0 nothing known / not usable, 1 hard calls only, 2 hard calls + one other value
  };
  int handed_back_recently = 0;   // > 0: a hard-call gene was handed back within the last 16 batches (launch_suffstat's list grid)
  uint64_t null_gen = 0;          // counts rvt_set_null / rvt_fit_null: a column cache made under another model is not used
  DevBuf<double> d_cc_part;    // slice partials of the one-column pass (64 slices x (RVT_MAX_COV + 3))
  std::unordered_map<const double*, ColKind> col_kind;
  // What the engine knows about a resident .bed matrix of rvt_bed_alloc, by base address (ordered: the rows of a call lie
  // anywhere inside a matrix, bed_rows_span looks up by containment).  rvt_bed_free drops the record; rvt_destroy frees no matrix.
  struct BedMatrix {
    int64_t n_variants, N, pitch;  // rows; the N they were sized for; bed_pitch(N)
  };
  std::map<const unsigned char*, BedMatrix> bed_mats;
  // VCF text front end (vcf_kernels.hip.h)
  char* d_vcf_text = nullptr;   // the text / block buffer of the gene being submitted: aliases text_buf[text_cur]
  static constexpr int kTextBufs = 3;  // ring: the copies of gene g + 1 run while the decode kernels of gene g read theirs
  DevBuf<char> text_buf[kTextBufs];
  hipEvent_t ev_text_copied[kTextBufs] = {}, ev_text_free[kTextBufs] = {};
  int text_next = 0, text_cur = 0;
  DevBuf<VcfRecord> d_vcf_rec;
  DevBuf<int> d_vcf_seg;
  DevBuf<int> d_vcf_rows;   // output row of every sample column of the file (-1: not analysed)
  int vcf_n_file = 0;
  int64_t vcf_n_rows = 0;      // rows the map addresses (must equal the null model's N)
  VcfFilters vcf_flt{0, 0, 0, 0};
  std::vector<int> vcf_alt;    // rvt_vcf_set_alt_alleles: alternative-allele index per record of the NEXT VCF call
  bool vcf_dosage = false;     // rvt_vcf_set_dosage: the index handed over is a dosage tag's, values through atof
  // BGEN probability blocks (bgen_kernels.hip.h); the blocks are staged in d_vcf_text
  DevBuf<char> d_fam_list;  // rvt_run_fam_tests: column pointers + flags of a batch (grow-only)
  DevBuf<signed char> d_vcf_sex;  // PLINK sex code per file sample (rvt_vcf_set_sex); hemizygous records only
  std::vector<int> vcf_hemi;         // per record of the NEXT decode call (rvt_vcf_set_hemi)
  DevBuf<BgenRecord> d_bgen_rec;
  DevBuf<long long> d_bgen_seg;
  // pinned, device-visible input-error words of the VCF / BGEN decoders: record index + 1 of a record with a wrong column
  // count (negative: a dosage the device cannot round exactly) resp. variant index + 1 of a block shorter than its ploidy
  // bytes demand.  One word per allele-frequency ring slot (the streaming submissions: read when the gene's frequencies
  // are resolved, so the error lands on the gene that caused it) + word kAfSlots for the synchronous calls.
  PinBuf<int> h_io_err;
  // ---- SKAT permutations: the emulated glibc rand() stream (TYPE_3), oldest word first ----
  // Permutation mode: exact (the DEFAULT of a single context: `--kernel skat[nPerm=..]` reproduces the reference's
  // ActualPerm / NumGreater / NumEqual / PermPvalue) = the reference's own rand() stream replayed (one sequential stream in
  // gene order: bit-identical counters, ~3 k shuffles/s at N = 500 000); counter-based = permutations keyed by (seed, gene
  // id, shuffle) (perm_counter.h: statistical parity — SURVEY 8e grants it to SHARDED runs only —, any context / device /
  // gene order, ~10^5 shuffles/s): selected by rvt_set_perm_exact(ctx, 0) / RVT_PERM_EXACT=0, and by a device group that
  // deals genes over more than one member (rvt_group_init).
  bool perm_exact = true;
  uint64_t perm_seed = 1;
  DevBuf<double> d_pc_part;  // counter mode: partial products [slice][shuffle][variant]
  DevBuf<double> d_pc_Q;
  // Price's variable-threshold test (vtprice_kernels.hip.h; grow-only): the gene's carrier list and tables, the partial sums
  // [segment][shuffle] of a chunk, the chunk's zmax
  DevBuf<char> d_vtp_ws, d_vtp_ent;
  DevBuf<double> d_vtp_part, d_vtp_z;
  // RareCover and Madsen-Browning (burdenperm_kernels.hip.h; grow-only, sized per gene from N, K and the entry count): the gene's
  // tables | its carrier numbering and bit matrix, or its entry list | c and Y of a chunk's shuffles when they do not fit the LDS |
  // the partial sums [segment][shuffle] | the weights [column][shuffle] | the chunk's statistics
  DevBuf<char> d_bp_ws, d_bp_ent;
  DevBuf<unsigned long long> d_bp_cy;
  DevBuf<double> d_bp_part, d_bp_w, d_bp_stat;
  // rvt_burden_blocks (burdencol_kernels.hip.h; grow-only): column pointers, flags, kept-column lists, gene table, counters, Fisher
  // p-values and y | the collapsed N x n blocks of a chunk of genes (cmc, zeggini, fp: those asked for).  burden_cols_*: what the
  // last call left there (rvt_burden_last_columns)
  DevBuf<char> d_burden_ws;
  DevBuf<double> d_burden_cols;
  int burden_cols_n = 0, burden_cols_chunk = 0;
  uint32_t burden_cols_which = 0;
  unsigned long long burden_cols_gen = 0;
  uint32_t rand_state[31];
  int64_t jump_N = -1;                 // J = A^(jump_N - 1) is cached for this sample count
  std::vector<uint32_t> jump;          // 31 x 31, row-major
  DevBuf<uint32_t> d_perm_idx;      // N x B
  DevBuf<uint32_t> d_perm_states;   // B x 31
  DevBuf<double> d_perm_R, d_perm_C, d_perm_Q, d_perm_cur;
  int perm_cap_B = 0;
  // rvt_debug_perm_trace (test-only): where the next SKAT permutation stage writes the statistics it hands to the stop rule
  // (caller-owned host memory; perm_stage takes the three over and clears them)
  double* perm_trace_stats = nullptr;
  int perm_trace_cap = 0;
  int* perm_trace_n = nullptr;
  hipEvent_t ev_in[kSlots] = {}, ev_k2[kSlots] = {}, ev_k2b[kSlots] = {};
  // The p-value kernel on CUs of its own (RVT_PV_CUS, see rvt_init): two streams restricted to the first pv_cus mask bits,
  // used by alternate batches; the batch's stream hands over by event and takes the records back by event.
  hipStream_t pv_stream[2] = {nullptr, nullptr};
  hipEvent_t ev_pv_in[kSlots] = {}, ev_pv_out[kSlots] = {};
  int pv_cus = 0;
  unsigned pv_turn = 0;
  std::vector<int> pv_order;  // scratch of run_batch: the batch's genes by falling M (GeneDesc::pv_gene)
  // host -> device copies of the streaming interface: pinned staging ring filled by the process-wide copy threads
  // (host_stage.h), drained by DMA on io_stream.  RVT_STAGE=0 restores the runtime's own pageable copies.
  static constexpr int kStageChunks = 4;
  static constexpr size_t kStageBytes = (size_t)32 << 20;
  StageRing stage;
  PinBuf<char> stage_buf[kStageChunks];  // the memory of stage.chunk
  hipEvent_t stage_ev[kStageChunks] = {};
  bool stage_on = true;
  static constexpr int kSmallSlots = 8;
  static constexpr size_t kSmallBytes = (size_t)128 << 10;
  PinBuf<char> h_small;      // kSmallSlots x kSmallBytes (record tables of the VCF / BGEN decoders)
  hipEvent_t small_ev[kSmallSlots] = {};
  int small_next = 0;
  // RVT_TRACE_SUBMIT=1: host seconds spent in the phases of the streaming submissions, printed by rvt_destroy
  bool trace_submit = false;
  double tr_block = 0, tr_copy = 0, tr_consol = 0, tr_af = 0, tr_launch = 0, tr_collect = 0;
  long long tr_genes = 0;
  hipEvent_t ev_io = nullptr;   // recorded on io_stream when a group of submitted genes is launched
  bool io_wait_pending = false;  // the next batch waits for ev_io (its blocks may still be crossing the link)
  std::string err;
  // null model
  bool have_null = false;
  NullConsts nc;
  // the null set the kernels read: raw pointers into the buffers below, which the family paths point at a family set for
  // the length of a call (famcov_run, Swap)
  NullConsts* d_nc = nullptr;
  double *d_X = nullptr, *d_res = nullptr, *d_rr = nullptr, *d_v = nullptr, *d_zeros = nullptr;
  DevBuf<NullConsts> nc_buf;
  DevBuf<double> d_nulltile;  // ONE allocation [X_0 .. X_{d-1} | rr | zeros]: d_X, d_rr and d_zeros point into it
  DevBuf<double> res_buf, v_buf;
  // binary trait: the weighted hard-call kernel's tile [vX_0 .. vX_{d-1} | res | v | zeros] and the digit planes of v
  DevBuf<double> d_nulltile_w;
  DevBuf<unsigned char> d_vq;
  // ... and the integer operands of the workgroup-cooperative kernel (suffstat_hcx.hip.h): the digits of v and of the null
  // tile in operand order, the power-of-two scale of every null column (host copy in hcx_tile, device copy for gene_assemble)
  DevBuf<unsigned char> d_dq, d_xq;
  DevBuf<double> d_xscale;
  NullTileX hcx_tile;
  bool hcx_ok = false;
  // ... and of the float-digit dosage kernel (suffstat_fdx.hip.h; quantitative trait): five base-256 digit planes of [X | res | 1]
  bool reg_defer = false;  // inside rvt_submit_genes: the wait for the DMAs out of registered caller memory comes once, at the end
  DevBuf<unsigned char> d_fxq;
  NullTileF fdx_tile;
  bool fdx_ok = false;
  bool dosage_float = false;  // rvt_set_dosage_float: blocks of unknown content hold float-precision dosages
  int as_threads = 256;   // workgroup size of gene_assemble_kernel (RVT_AS_THREADS).  Round 5: 256 instead of 1024 — many of its phases
                          // keep M threads busy while the rest wait at the barriers, and with the eigenvalue stage cut down its
                          // resident waves were 56 % of the per-gene tail (configs[1]: 347 k -> 369 k; the other shapes unchanged)
  bool hcx_fused = true;  // one launch for every tile class of a batch (gene_suffstat_hcx_any); RVT_HCX_FUSED=0: one per class
  // launch shape of gene_suffstat_hc per tile class (k2_hardcall.hip has the rule; RVT_HC_CFG = "3:3x1,4:2x2,.." overrides
  // classes; a shape that is not compiled in fails rvt_init), and whether the classes whose shape is the one-wave shape of gene_suffstat_hc_any share that one launch
  // (RVT_HC_FUSE=0: one launch per class).  Read when the context is created.
  struct HcShape {
    int depth, waves;
  };
  HcShape hc_shape[kHcMaxMT + 1] = {{0, 0}, {2, 4}, {4, 1}, {3, 1}, {2, 2}, {1, 1}, {1, 1}};
  bool hc_fuse = true;
  int64_t null_ld = 0;
  // Which sufficient-statistics kernel a gene STARTS on is a prediction, never a trust: the hard-call kernel tests every
  // double it loads and hands back genes that hold anything but hard calls and one imputed value per column
  // (gene_flags_hc_kernel); those are computed by the general fp64 kernel in the same batch, through a conditional launch
  // that follows the hard-call launches on the same stream.  The engine's own decoders say what they wrote (hint per
  // gene: 1 hard calls / imputed, 0 dosages); blocks of unknown content (fp64 from the caller) start on the hard-call
  // kernel unless the caller has said they hold dosages (rvt_set_content_hint).  No history: the kernel a block runs on
  // — and with it the last bits of its records — depends on the block and the hint alone.
  int content_hint = -1;
  // rvt_host_register: host ranges of the caller that are page-locked — copies out of them are DMA straight from the
  // caller's memory (no staging copy by the CPU); `reg_pending`: such a copy has been enqueued and not yet waited for
  std::vector<std::pair<const char*, size_t>> host_reg;
  std::vector<char> host_reg_owned;  // (1: this context called hipHostRegister; 0: adopted from another member of a group)
  hipEvent_t ev_reg = nullptr;
  hipStream_t reg_stream = nullptr;  // the stream ev_reg was last recorded on
  bool reg_pending = false;
  int lattice_den = 0;        // rvt_set_dosage_lattice: dosage doubles are multiples of 1 / lattice_den (0: not stated)
  DevBuf<int> d_kind;      // device flag of rvt_block_classify (a stateless query)
  bool hc_enabled = true;     // RVT_HARDCALL=0 forces the general kernel (experiments)
  double null_beta[RVT_MAX_COV] = {};  // estimates of the model rvt_fit_null fitted
  bool have_null_beta = false;
  DevBuf<double> d_null_y;  // rvt_fit_null with a binary trait: y (ld doubles, zero-padded) for the per-variant Wald fits
  // rvt_wald_block's work space (wald_logistic.hip.h): one grow-only allocation, never touched inside the round loop
  DevBuf<char> d_wald_ws;
  // single-variant tests for related samples (fam_single.hip.h): grow-only work spaces of rvt_lrt_block_fam and of
  // rvt_fit_grammar_null / rvt_grammar_block, their null constants, and the generation of the FastLMM null they belong to
  uint64_t fam_gen = 0;        // counts rvt_fit_fam_null
  double fam_sigma2 = 0.0;     // sigma2_g of the fitted FastLMM null
  DevBuf<char> d_lrt_ws;
  uint64_t lrt_gen = 0;        // fam_gen the famLRT constants were formed for (0: none)
  double lrt_ssr0 = 0.0, lrt_slog = 0.0;
  DevBuf<char> d_fam_bed_ws;   // the family tests over resident .bed rows: counts, fill values, sums and flags of a piece (grow-only)
  DevBuf<char> d_gg_ws;
  bool have_grammar = false;
  int64_t gg_N = 0;
  int gg_d = 0;
  double gg_delta = 0.0, gg_gamma = 0.0, gg_ysy = 0.0, gg_sumty = 0.0, gg_afden = 0.0;
  // famGrammarGamma from resident .bed rows (rvt_grammar_bed_dev): the int8 digit planes of ty with their exponent and totals,
  // formed at the first call after a fit (gg_gen counts rvt_fit_grammar_null, as fam_gen / lrt_gen), and the call's work space
  uint64_t gg_gen = 0;
  DevBuf<char> d_gg_planes;
  uint64_t gg_planes_gen = 0;  // gg_gen the planes were formed for (0: none)
  int gg_exp = 0;
  long long gg_totals[8] = {};
  DevBuf<char> d_gg_bed_ws;
  // the multiple-trait score test (rvt_mtscore.hip): the centred [Yc | Zc] as kMtPlanes digit planes [plane][row][mt_ldk] (the A
  // operand of rot_gemm.hip.h, mt_plane bytes apart, per-row exponents mt_row_exp), the distinct indModel patterns as one 0 / 1
  // plane, the row sums of the stored values, the MtTest constants of the mt_T tests — resident from rvt_mt_fit_null to
  // rvt_mt_clear, in buffers of their own (d_rotA / d_rotB are rewritten by every integer-plane product) — and the grow-only
  // work space of rvt_mt_score_block (d_mt_B: the int8 copy of a piece's columns)
  bool have_mt = false;
  int64_t mt_N = 0, mt_ld = 0, mt_ldk = 0;
  int mt_R = 0, mt_K = 0, mt_T = 0;
  size_t mt_plane = 0;
  DevBuf<signed char> d_mt_planes, d_mt_pat, d_mt_B;
  DevBuf<double> d_mt_rowsum;
  DevBuf<char> d_mt_tests, d_mt_ws;
  std::vector<int> mt_row_exp;
  double mt_ms[3] = {0.0, 0.0, 0.0};  // rvt_mt_last_timing
  // streaming interface
  struct Pending {
    int64_t id;
    int M;
    double* dG;
    size_t bytes;  // capacity of dG
    std::vector<double> af;
    uint32_t tests;
    rvt_params prm;
    rvt_gene_result res;  // filled by the batch this gene was launched in (the queue is a deque: stable addresses)
    bool launched;
    int af_slot = -1;     // >= 0: the allele frequencies are still on their way back from the device (af_ring slot)
    int io_error = 0;     // != 0: the gene's VCF text / BGEN blocks were malformed (h_io_err): its record is void
    int decoded = 0;      // 1: VCF text, 2: BGEN blocks (the submission has an input-error word in its ring slot)
    bool planes = false;  // kind 3 only: G'[X | rr] on the int8 matrix cores from the null tile's digit planes (resident .bed genes)
    int kind = kKindUnknown;  // what the engine's decoder wrote (a BlockKind)
    // the fields every route sets; the block, the frequencies and the kind follow
    Pending(int64_t id_, int M_, uint32_t tests_, const rvt_params* prm_)
        : id(id_), M(M_), dG(nullptr), bytes(0), tests(tests_), prm(prm_ ? *prm_ : kDefaultParams), launched(false) {
      std::memset(&res, 0, sizeof(res));
    }
  };
  std::deque<Pending> queue;
  // free device blocks of the streaming interface (block_pool.h; taken through a BlockLease): fp64 blocks, and PACKED blocks
  // (2-bit rows), which are never handed out as fp64 blocks, whose pad rows must be zero
  BlockPool block_pool, pk_pool;
  // results of launched sub-batches land in contiguous arrays, then move into Pending::res at collect time
  struct Launched {
    size_t first;  // index into the queue at launch time (adjusted when the queue is popped)
    int n;
    std::vector<rvt_gene_result> res;
    bool done = false;  // the batch has finished and `res` is filled (set by finish_slot)
  };
  bool* next_done_flag = nullptr;  // handed to the slot of the next run_batch call (launch_group)
  std::deque<Launched> launched;
  // profiling
  bool profiling = false;
  std::vector<ProfEvent> events;
  std::vector<hipEvent_t> event_pool;
  rvt_timing timing;
  size_t eigen_lds_max = 48 * 1024;
};

// N and ld of the layout that blocks (rvt_block_alloc) have under the installed model: the null model's, else the family
// model's, else the multiple-trait model's
struct BlockDims {
  int64_t N, ld;
};
inline BlockDims block_dims(const rvt_ctx* c) {
  if (c->have_null) return {c->nc.N, c->null_ld};
  return c->have_fam ? BlockDims{c->fam_nc.N, c->fam_nc.ld} : BlockDims{c->mt_N, c->mt_ld};
}

namespace {

int fail(rvt_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define HIP_TRY(ctx, call)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return fail(ctx, RVT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// a slot's work space and pinned staging: grow-only, the old block freed once the slot's last batch has finished with it
int ensure_arena(rvt_ctx* c, Slot& sl, size_t bytes) {
  HIP_TRY(c, sl.arena.grow(bytes, bytes + bytes / 4, sl.stream, true, 0, "arena"));
  return RVT_OK;
}
int ensure_stage(rvt_ctx* c, Slot& sl, size_t bytes) {
  HIP_TRY(c, sl.h_stage.grow(bytes, bytes * 2, sl.stream));
  return RVT_OK;
}

// wait for one slot's batch and hand its records to the caller
int finish_slot(rvt_ctx* c, Slot& sl) {
  HIP_TRY(c, sync_stream(sl.stream));
  if (sl.pending_out) {
    // (kStatusHandedBack is bookkeeping: the gene started on the hard-call kernel and was computed by the fp64 kernel)
    bool any_back = false;
    for (int g = 0; g < sl.pending_n; ++g) {
      if (sl.h_results[g].status & kStatusHandedBack) {
        sl.h_results[g].status &= ~kStatusHandedBack;
        any_back = true;
        if (c->profiling) ++c->timing.genes_handed_back;
      }
    }
    // how wide the NEXT batches launch the general kernel over their hand-back lists (launch_suffstat): a stream that has
    // handed nothing back for a while gets a grid of 32 waves instead of 1 024
    if (any_back) c->handed_back_recently = 16;
    else if (c->handed_back_recently > 0) --c->handed_back_recently;
    std::memcpy(sl.pending_out, sl.h_results, sizeof(rvt_gene_result) * sl.pending_n);
    if (sl.pending_done) *sl.pending_done = true;
    sl.pending_done = nullptr;
    sl.pending_out = nullptr;
    sl.pending_n = 0;
  }
  return RVT_OK;
}

hipEvent_t get_event(rvt_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

struct Scope {  // times one kernel launch with HIP events on the launching stream when profiling is on
  rvt_ctx* c;
  int fam;
  hipStream_t st;
  hipEvent_t a = nullptr;
  Scope(rvt_ctx* c_, int fam_, hipStream_t st_) : c(c_), fam(fam_), st(st_) {
    if (c->profiling) {
      a = get_event(c);
      hipEventRecord(a, st);
    }
  }
  ~Scope() {
    if (c->profiling) {
      hipEvent_t b = get_event(c);
      hipEventRecord(b, st);
      c->events.push_back({fam, a, b});
    }
  }
};

void drain_events(rvt_ctx* c) {
  for (auto& e : c->events) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, e.a, e.b);
    switch (e.family) {
      case 0: c->timing.ms_suffstat += ms; c->timing.n_suffstat_launches++; break;
      case 4:
        c->timing.ms_suffstat += ms;
        c->timing.n_suffstat_launches++;
        c->timing.ms_suffstat_hc += ms;
        c->timing.n_suffstat_hc_launches++;
        break;
      case 1: c->timing.ms_burden += ms; c->timing.n_burden_launches++; break;
      case 2: c->timing.ms_stats += ms; c->timing.n_stats_launches++; break;
      case 5: break;  // conditional launches of the general kernel over hard-call genes (mostly empty): not counted
      default: c->timing.ms_pvalue += ms; c->timing.n_pvalue_launches++; break;
    }
    c->event_pool.push_back(e.a);
    c->event_pool.push_back(e.b);
  }
  c->events.clear();
}

// genes [0, n) of one register-budget group (kernels.hip.h: suffstat_group)
// list != nullptr: the genes come from a device work list (handed-back hard-call genes, suffstat_kernels.hip.h); the
// launch is then a fixed small grid whose workgroups loop over the list — empty almost always.
void launch_suffstat(rvt_ctx* c, hipStream_t st, int group, const GeneDesc* d_desc, int n, int max_wparts,
                     const NullDev& nd, const int* list = nullptr) {
  Scope sc(c, list ? 5 : 0, st);
  // Waves are independent (no LDS, no barriers), so a workgroup is ONE wave: the dispatcher can then place the
  // wide classes (one wave fills a SIMD's register file) on any free SIMD, instead of needing four free SIMDs on
  // one CU at once — which a single long-lived p-value wave per CU would block for its whole lifetime.
  dim3 grid(max_wparts, n);
  // (the list is empty almost always, but every wave of these kernels needs a SIMD's whole register file before it can start
  //  and leave: 1 024 of them took 2 ms to trickle through a chip that is busy with the next batch's streaming kernel, and the
  //  batch's tail waited behind them.  While no batch has handed a gene back for 16 batches the grid is 32 waves; a stream that
  //  does hand genes back — dosages the caller did not announce — keeps the wide grid.)
  if (list) grid = dim3(c->handed_back_recently > 0 ? 1024 : 32, 1);
  const long long N = c->nc.N, ld = c->nc.ld;
  const int d = c->nc.d;
  if (c->nc.binary)
    k2_launch_group_w1(group, grid, st, d_desc, list, max_wparts, nd, N, ld, d);
  else
    k2_launch_group_w0(group, grid, st, d_desc, list, max_wparts, nd, N, ld, d);
}

// glibc srandom_r / random_r for the default TYPE_3 generator: r[i] = 16807 r[i-1] mod (2^31 - 1) for the first 31
// words, then 310 outputs are discarded.  The state is kept normalised (oldest word first): a draw is
// x' = (x[1..30], x[0] + x[28]).
void seed_rand_state(uint32_t* x, unsigned seed) {
  int32_t r[34];
  r[0] = (int32_t)(seed == 0 ? 1 : seed);
  for (int i = 1; i < 31; ++i) {
    int64_t v = (16807LL * r[i - 1]) % 2147483647;
    if (v < 0) v += 2147483647;
    r[i] = (int32_t)v;
  }
  std::vector<uint32_t> o(344);
  for (int i = 0; i < 31; ++i) o[i] = (uint32_t)r[i];
  for (int i = 31; i < 34; ++i) o[i] = o[i - 31];
  for (int i = 34; i < 344; ++i) o[i] = o[i - 31] + o[i - 3];
  for (int i = 0; i < 31; ++i) x[i] = o[344 - 31 + i];
}

// inverse of a small (n <= RVT_MAX_COV) nonsingular matrix, row-major, Gauss-Jordan with partial pivoting
bool invert_spd(const double* M, int n, double* Minv) {
  double A[RVT_MAX_COV][2 * RVT_MAX_COV];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      A[i][j] = M[i * n + j];
      A[i][n + j] = (i == j) ? 1.0 : 0.0;
    }
  for (int k = 0; k < n; ++k) {
    int piv = k;
    for (int i = k + 1; i < n; ++i)
      if (fabs(A[i][k]) > fabs(A[piv][k])) piv = i;
    if (A[piv][k] == 0.0) return false;
    if (piv != k)
      for (int j = 0; j < 2 * n; ++j) std::swap(A[k][j], A[piv][j]);
    const double pv = A[k][k];
    for (int j = 0; j < 2 * n; ++j) A[k][j] /= pv;
    for (int i = 0; i < n; ++i)
      if (i != k) {
        const double f = A[i][k];
        if (f != 0.0)
          for (int j = 0; j < 2 * n; ++j) A[i][j] -= f * A[k][j];
      }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Minv[i * n + j] = A[i][n + j];
  return true;
}

// 16-sample steps handled by one wave: large enough to amortise the partial-tile write, small enough
// that a gene still spreads over >= 32..128 waves
// n_genes: genes of the batch — a big batch fills the chip with fewer, longer waves per gene (half the partial tiles
// to write and to reduce: measured +2.7 % at 512 genes)
// hcx: the batch's hard-call genes take the workgroup-cooperative kernel (suffstat_hcx.hip.h): a part is worked by four loader
// waves, so a quarter of the parts gives as many waves per gene; its iteration is 16 steps
void choose_split(int64_t ld, int n_genes, bool weighted, int* n_wparts, int* steps_per, bool hcx = false, bool fdx = false) {
  const int64_t nsteps = ld >> 4;
  const char* fe = getenv("RVT_WPARTS");  // (experiments / tests)
  const int forced = fe ? atoi(fe) : 0;
  // (cooperative kernel: one workgroup per CU — about eight rounds of workgroups over the chip balance a launch; fewer, longer
  //  wave-parts measured better down to that: 47.8 k gene-sets/s with 16 parts, 49.6 k with 8, 50.4-50.9 k with 5-6 at N = 200 000)
  const int coop = std::min(32, std::max(4, (2048 + n_genes - 1) / std::max(n_genes, 1)));
  const int target = forced > 0 ? forced : (hcx ? coop : (n_genes >= 1024 ? 32 : (n_genes >= 128 ? 64 : 128)));
  int64_t spw = (nsteps + target - 1) / target;
  if (spw < 64) spw = 64;
  const int unit = hcx ? 3 * kHcxIterSteps : kHcStepUnit;     // (48: whole iterations of both kernels)
  spw = (spw + unit - 1) / unit * unit;                       // whole ring iterations of the hard-call kernel
  if (hcx && spw > kHcwMaxSteps) spw = kHcwMaxSteps / unit * unit;
  if (spw > kHcwMaxSteps) spw = kHcwMaxSteps;                   // (int32 range of the weighted hard-call kernel's tiles)
  if (!weighted && spw > kHcMaxSteps) spw = kHcMaxSteps;        // (16-bit range of the hard-call kernel's masked-tile counters)
  if (fdx && spw > kFdxMaxSteps / 24 * 24) spw = kFdxMaxSteps / 24 * 24;  // (int32 range of the float-digit kernel's order sums)
  int64_t nw = (nsteps + spw - 1) / spw;
  if (nw < 1) nw = 1;
  *n_wparts = (int)nw;
  *steps_per = (int)spw;
}

}  // namespace

// ---- defined in rvt_engine.hip, called from the other translation units (hidden: not part of the ABI) ------------------------
#define RVT_INTERNAL __attribute__((visibility("hidden")))
// ---- kernel families -----------------------------------------------------------------------------------------------------
// Every non-template kernel of the engine is `static` in a header that all rvt_*.hip units see through this file; until
// round 6 each unit therefore compiled and shipped its own copy of all of them (76 kernels x 5 code objects).  Now a unit
// defines RVT_K_SPLIT and ONE of RVT_K_ENGINE / RVT_K_STREAM / RVT_K_FAM / RVT_K_PERM / RVT_K_META before including this
// header and gets the bodies of that family alone (tools and the host harness define nothing and get everything).  The
// later units name a family no shared header knows — RVT_K_MT (rvt_mtscore.hip), RVT_K_KINSHIP (rvt_kinship.hip),
// RVT_K_DECOMPOSE (rvt_decompose.hip) — so they get none of those bodies, only the kernels of the headers each includes for
// itself (mtscore_kernels.hip.h; kinship_kernels.hip.h; jacobi_kernels.hip.h and tridiag_kernels.hip.h).  The few kernels that two units launch live in one of them; the other goes through these host
// launchers (tools/kernel_units.sh lists which object carries which kernel; it reads every .o it finds).
// the column blocks' bookkeeping (rvt_meta.hip): the queue of single columns, and a block that is new / goes away / is refilled
extern "C" RVT_INTERNAL int flush_col_queue(rvt_ctx* c);
extern "C" RVT_INTERNAL int flush_col_queue_wait(rvt_ctx* c, bool earlier_flushes_too);
RVT_INTERNAL void block_register(rvt_ctx* c, const double* dG, int cols);
RVT_INTERNAL int block_forget(rvt_ctx* c, const double* dG);
RVT_INTERNAL void block_replaced(rvt_ctx* c, const double* dG);
RVT_INTERNAL void k_lmm_sums(dim3 grid, hipStream_t st, const double* uxy, const double* lam, long long N, int d, double delta,
                             int take_abs, double* partial);                                                   // rvt_fam.hip
RVT_INTERNAL void k_fam_colstat(dim3 grid, hipStream_t st, const double* const* cols, long long N, int* flags);  // rvt_fam.hip
RVT_INTERNAL void k_fam_flip_compact(dim3 grid, hipStream_t st, const double* const* src_cols, const int* src_flip, long long N,
                                     long long ld, double* dst);                                               // rvt_fam.hip
RVT_INTERNAL void k_raw_colstat(dim3 grid, hipStream_t st, const double* G, long long N, long long ld, double* colsum, int* poly);  // rvt_fam.hip
RVT_INTERNAL void k_rot_reduce_slices(hipStream_t st, const double* part, long long ldc, long long M, long long N, long long stride,
                                      int slices, double* C, int accumulate);                                  // rvt_fam.hip
RVT_INTERNAL void k_vt_integrate(dim3 grid, hipStream_t st, const GeneDesc* genes, int stage);                  // rvt_engine.hip
RVT_INTERNAL void k_vt_finish(dim3 grid, hipStream_t st, const GeneDesc* genes, int n, int stage);              // rvt_engine.hip
extern "C" {
RVT_INTERNAL int stage_ready(rvt_ctx* c);
RVT_INTERNAL bool host_registered(const rvt_ctx* c, const void* src, size_t bytes);
RVT_INTERNAL int reg_wait(rvt_ctx* c);
RVT_INTERNAL int small_h2d(rvt_ctx* c, void* dst, const void* src, size_t bytes);
RVT_INTERNAL int staged_h2d(rvt_ctx* c, void* dst, const void* src, size_t bytes);
RVT_INTERNAL int staged_h2d_2d(rvt_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows,
                               bool pad_zero = false);
RVT_INTERNAL int upload_block_data(rvt_ctx* c, double* dG, int M, const double* G);
struct DebugOut;
struct CovOut;
// kind (optional, per gene): what the engine's own decoder wrote into the block — a BlockKind byte (encode_kind, above)
RVT_INTERNAL int run_batch(rvt_ctx* c, int n, const double* const* dG, const int* Ms, const double* af, const int64_t* ids,
                           uint32_t tests, const rvt_params* prm, rvt_gene_result* out, DebugOut* dbg, CovOut* cov = nullptr,
                           const signed char* kind = nullptr);
// ---- defined in rvt_fam.hip
RVT_INTERNAL int ensure_fam_cols(rvt_ctx* c, size_t T, int64_t ld);
RVT_INTERNAL int rotate_columns(rvt_ctx* c, const double* d_src, int64_t ld_src, int ncols, double* d_dst, int64_t ld_dst,
                                hipStream_t st);
RVT_INTERNAL int gemm_tn_planes(rvt_ctx* c, const double* dA, int64_t ldA, int nA, const double* dB, int64_t ldB, int nB,
                                int64_t n_rows, double* C, int64_t ldc, hipStream_t st);
RVT_INTERNAL int rvt_planes_gemm(rvt_ctx* c, const signed char* A, size_t a_stride, int PA, int nA, const int* row_exp, int a_exp,
                                 const signed char* B, size_t b_stride, int PB, int nB, const int* col_exp, int64_t n_rows,
                                 int64_t ldk, double* C, int64_t ldc, hipStream_t st, const int2* a_krange = nullptr);
// quantize_columns into the context's d_mt_B (rvt_mt_score_block's pieces that hold more than hard calls), zero columns up to a
// multiple of `pad`: the planes, the bytes between them, their number and the ncols column exponents
RVT_INTERNAL int quantize_columns_mt(rvt_ctx* c, const double* d_src, int64_t n_rows, int64_t ld_src, int ncols, int pad, int64_t ldk,
                                     hipStream_t st, signed char** planes, size_t* plane_stride, int* n_planes, int* col_exp);
// the family form of the kinship for rvt_kinship_decompose_families (rvt_decompose.hip): the descriptors checked (blk_off[f] =
// where family f's block starts), the blocks checked for non-finite entries, the installation itself
RVT_INTERNAL int check_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                                std::vector<long long>* blk_off);
RVT_INTERNAL int check_blocks_finite(rvt_ctx* c, int64_t n_fam, const int64_t* fam_ptr, const std::vector<long long>& blk_off,
                                     const float* blocks, const char* what);
RVT_INTERNAL int install_families(rvt_ctx* c, int64_t N, int64_t n_fam, const int64_t* fam_ptr, const int32_t* members,
                                  const std::vector<long long>& blk_off, const float* blocks, const float* S);
// ---- defined in rvt_meta.hip: C = A' D [B | B2] in fp64 on the matrix cores (gemm_f64.hip.h)
RVT_INTERNAL int gemm_tn_f64(rvt_ctx* c, const double* A, int64_t lda, int M, const double* B, int64_t ldb, int Nb, const double* B2,
                             int64_t ldb2, int Nb2, const double* w, int64_t N, double* C, int64_t ldc, bool symmetric,
                             hipStream_t st, bool subtract = false, int halo = -1, int ring = 0, int col0 = 0);
// the calls of 0 / 1 / 2 / missing of n_rows rows of a resident .bed matrix, added to d_cnt[4 r + k] (recode_bed_count_kernel)
RVT_INTERNAL void bed_row_counts(hipStream_t st, const unsigned char* d_rows, long long cb, long long N, int n_rows,
                                 unsigned long long* d_cnt);
// the same of any number of consecutive rows into d_cnt, zeroed first, in launches of at most 32 768 rows; with host or counts,
// bed_counts_host behind it
RVT_INTERNAL int bed_piece_counts(rvt_ctx* c, hipStream_t st, const unsigned char* d_rows, long long cb, long long N,
                                  long long n_rows, unsigned long long* d_cnt, std::vector<unsigned long long>* host,
                                  long long* counts);
// the counts of n_rows rows copied to the host and st waited for: into host (optional) and, as long long, into counts (optional)
RVT_INTERNAL int bed_counts_host(rvt_ctx* c, hipStream_t st, const unsigned long long* d_cnt, long long n_rows,
                                 std::vector<unsigned long long>* host, long long* counts);
// The one question every call over resident rows asks before any device work (check_columns' counterpart for rows): may
// `who`, which consumes null model `model`, read V rows at d_rows, and at what pitch?  Rows inside a matrix the
// engine knows (rvt_ctx::bed_mats): sized for the model's N, on a row boundary, inside the matrix; the pitch is the record's.
// A pointer it does not know (another context's matrix, a caller's allocation) is taken on trust at bed_pitch of the model's N,
// as check_columns takes a block.  d_rows == NULL, V = 0: the state alone.
enum class BedModel { kNull, kFam, kMt, kGrammar };  // the ordinary, family, multiple-trait, GrammarGamma null model
RVT_INTERNAL int bed_rows_span(rvt_ctx* c, const char* who, const unsigned char* d_rows, int64_t V, BedModel model, int64_t* pitch);
// n_rows rows of a resident .bed matrix as fp64 columns (leading dimension ld), missing -> d_mu[row] (bed_expand_columns_kernel)
RVT_INTERNAL void bed_rows_expand(hipStream_t st, const unsigned char* d_rows, long long cb, const double* d_mu, long long N,
                                  long long ld, int n_rows, double* G);
// ---- defined in rvt_perm.hip
RVT_INTERNAL int rvt_kbac_stage(rvt_ctx* c, const double* dG, int M, const double* af, const std::vector<unsigned char>& y,
                                int nPerm, double alpha, rvt_kbac_result* r);
// ---- defined in rvt_engine.hip (continued)
RVT_INTERNAL int enqueue_classify(rvt_ctx* c, const double* dG, int M, int64_t N, int64_t ld, hipStream_t st, int* d_flag);
RVT_INTERNAL int cov_constants(rvt_ctx* c, bool fam, CovConsts* ccp, std::vector<double>* zzp);
RVT_INTERNAL int ensure_hcp_planes(rvt_ctx* c);
RVT_INTERNAL int debug_suffstat_collect(rvt_ctx* c, GeneDesc g0, int M, double* S, double* T, double* u, double* colsum,
                                        double* cmin, double* cmax);
RVT_INTERNAL int run_blocks_with_perm(rvt_ctx* c, int n, const double* const* dG, const int* M, const double* af,
                                      const int64_t* ids, uint32_t tests, const rvt_params* prm, rvt_gene_result* out);
}

struct RegWait {  // every entry point that copies out of the caller's memory ends with the wait
  rvt_ctx* c;
  explicit RegWait(rvt_ctx* c_) : c(c_) {}
  ~RegWait() {
    if (c && !c->reg_defer) (void)reg_wait(c);  // (rvt_submit_genes waits ONCE, behind its last gene)
  }
};

static inline double now_s() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

struct TraceScope {  // RVT_TRACE_SUBMIT: adds the scope's host time to *acc
  double* acc;
  double t0;
  TraceScope(rvt_ctx* c, double* a) : acc(c->trace_submit ? a : nullptr), t0(acc ? now_s() : 0.0) {}
  ~TraceScope() {
    if (acc) *acc += now_s() - t0;
  }
};

struct DebugOut {
  int* flip = nullptr;
  int* kept = nullptr;
  double* cmc = nullptr;
  double* zeg = nullptr;
  GeneDesc* desc0 = nullptr;
  int* planes_used = nullptr;  // packed rows: 1 = gene_tnull_hcp formed the T columns from the digit planes, 0 = the fp64 product
};

struct CovOut {  // rvt_cov_block: host destinations
  double* cov = nullptr;   // V x V
  double* xz = nullptr;    // V x d
  double* zz = nullptr;    // d x d
  int* poly = nullptr;     // V
  bool fam = false;        // family mode: the block is already rotated; raw column sums / flags are supplied
  const double* d_raw_colsum = nullptr;
  const int* d_raw_poly = nullptr;
  // family burden tests: per-column U, V, GLS allele frequency, p-value (host, V entries each); cov/xz may be null
  double *ustat = nullptr, *vstat = nullptr, *af = nullptr, *pval = nullptr;
  // MetaScoreTest (unrelated samples): ustat / vstat / effect / se / pval / ok, V entries each; no covariance rows
  bool score = false;
  const unsigned char* slice_hc = nullptr;  // score mode: per slice, 1 = the slice holds hard calls only
  bool uncentred = false;  // family mode: FastLMM::disableCenterGenotype (MetaFamBinary)
  double *effect = nullptr, *se = nullptr;
  int* ok = nullptr;
  // rvt_wald_block, quantitative trait (score mode as well): the linear Wald fit of every column from the same partials
  // (wald_linear_finish_kernel); beta / se / pval are V x d (row of column h: g, then the covariates), ok as ok[h] of the ABI
  bool wald = false;
  double wald_beta0[RVT_MAX_COV] = {};
  double *wbeta = nullptr, *wse = nullptr, *wpval = nullptr;
};

