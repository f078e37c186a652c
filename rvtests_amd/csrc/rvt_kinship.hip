// rvtests_amd — rvt_kinship_from_bed: the empirical kinship of `vcf2kinship --ibs` / `--bn` (vcfUtils/vcf2kinship.cpp) from
// rows of a resident .bed matrix, the step in front of rvt_kinship_decompose.  Part of librvtests_amd.so.
// Three stages per call (kinship_kernels.hip.h): the site pass (counts, filter decision, BN's table), the Gram product over the
// tiles of the lower triangle, the finish (divide, mirror, copy to the host).  The sites go through in chunks of 32 768, so
// the site pass's work space stays a few MB whatever V is; a chunk's product adds to the N x N sums of the chunks before it.
// this unit compiles (and ships) the kinship kernels only: see "kernel families" in rvt_engine_int.h
#define RVT_K_SPLIT
#define RVT_K_KINSHIP
#include "rvt_engine_int.h"
#include "kinship_kernels.hip.h"

namespace {
constexpr int64_t kKinChunk = 32768;  // sites per chunk (the count kernel's gridDim.y); RVT_KINSHIP_CHUNK lowers it

struct KinEvents {  // the stage boundaries of one chunk: stats [0, 1), product [1, 2); finish [0, 1)
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  ~KinEvents() {
    for (hipEvent_t x : e)
      if (x) hipEventDestroy(x);
  }
};

template <class T>
int kin_alloc(rvt_ctx* c, DevBuf<T>* b, size_t bytes, const char* what) {
  if (b->alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, RVT_E_HIP, "rvt_kinship_from_bed: hipMalloc(%zu bytes) failed for %s", bytes, what);
  }
  return RVT_OK;
}
}  // namespace

extern "C" {

int rvt_kinship_from_bed(rvt_ctx* c, const unsigned char* d_rows, int64_t V, int method, double min_maf, double max_missing,
                         double* K_out, rvt_kinship_info* info) {
  if (!c || !d_rows || !K_out || !info) return fail(c, RVT_E_INVALID, "rvt_kinship_from_bed: null argument");
  if (V < 1) return fail(c, RVT_E_INVALID, "rvt_kinship_from_bed: V = %lld", (long long)V);
  if (method != RVT_KINSHIP_IBS && method != RVT_KINSHIP_BN)
    return fail(c, RVT_E_INVALID, "rvt_kinship_from_bed: method %d: 0 = IBS, 1 = Balding-Nichols", method);
  if (!(min_maf >= 0.0 && min_maf <= 0.5)) return fail(c, RVT_E_INVALID, "rvt_kinship_from_bed: min_maf %g outside [0, 0.5]", min_maf);
  if (!(max_missing >= 0.0 && max_missing <= 1.0))
    return fail(c, RVT_E_INVALID, "rvt_kinship_from_bed: max_missing %g outside [0, 1]", max_missing);
  if (!c->have_null) return fail(c, RVT_E_STATE, "no null model set");
  if (V > (int64_t)1 << 30) return fail(c, RVT_E_TOO_LARGE, "rvt_kinship_from_bed: %lld sites (the integer sums hold 2^30)", (long long)V);
  int64_t pitch = 0;
  if (int rc = bed_rows_span(c, "rvt_kinship_from_bed", d_rows, V, BedModel::kNull, &pitch)) return rc;
  hipSetDevice(c->device);
  const bool bn = method == RVT_KINSHIP_BN;
  const long long N = c->nc.N, cb = pitch, ld = N;
  const long long nblk = (N + kKinTile - 1) / kKinTile, tiles = nblk * (nblk + 1) / 2;
  // (RVT_KINSHIP_CHUNK, 1 .. 32 768 sites: tests lower it so that small matrices take the path of several chunks)
  const char* env_chunk = getenv("RVT_KINSHIP_CHUNK");
  const int64_t max_chunk = env_chunk ? std::max<int64_t>(1, std::min<int64_t>(kKinChunk, atoll(env_chunk))) : kKinChunk;
  const int64_t chunk = std::min(V, max_chunk);
  hipStream_t st = c->stream;

  Layout L;
  const size_t o_cnt = L.take(sizeof(unsigned long long) * 4 * (size_t)chunk), o_z = L.take(sizeof(double) * 4 * (size_t)chunk),
               o_drop = L.take((size_t)chunk), o_tot = L.take(sizeof(KinTotals));
  DevBuf<char> ws;
  DevBuf<int> d_cc, d_ce;
  DevBuf<double> d_sum, d_K;
  const size_t nn = (size_t)N * (size_t)N;
  if (int rc = kin_alloc(c, &ws, L.total, "the site pass")) return rc;
  if (bn) {
    if (int rc = kin_alloc(c, &d_sum, sizeof(double) * nn, "the N x N sums")) return rc;
  } else {
    if (int rc = kin_alloc(c, &d_cc, sizeof(int) * nn, "the N x N pair counts")) return rc;
    if (int rc = kin_alloc(c, &d_ce, sizeof(int) * nn, "the N x N sums")) return rc;
  }
  if (int rc = kin_alloc(c, &d_K, sizeof(double) * nn, "the N x N kinship")) return rc;
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(ws + o_cnt);
  double* d_z = reinterpret_cast<double*>(ws + o_z);
  unsigned char* d_drop = reinterpret_cast<unsigned char*>(ws + o_drop);
  KinTotals* d_tot = reinterpret_cast<KinTotals*>(ws + o_tot);
  KinEvents ev;
  for (hipEvent_t& x : ev.e) HIP_TRY(c, hipEventCreate(&x));
  HIP_TRY(c, hipMemsetAsync(d_tot, 0, sizeof(KinTotals), st));

  double ms_stats = 0.0, ms_product = 0.0;
  for (int64_t v0 = 0; v0 < V; v0 += chunk) {
    const long long nv = (long long)std::min(chunk, V - v0);
    const unsigned char* rows = d_rows + (size_t)v0 * (size_t)cb;
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 4 * (size_t)nv, st));
    HIP_TRY(c, hipEventRecord(ev.e[0], st));
    bed_row_counts(st, rows, cb, N, (int)nv, d_cnt);
    hipLaunchKernelGGL(kin_site_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, d_cnt, nv, N, bn ? 1 : 0, min_maf,
                       max_missing, d_drop, d_z, d_tot);
    HIP_TRY(c, hipEventRecord(ev.e[1], st));
    if (bn)
      hipLaunchKernelGGL(kin_bn_kernel, dim3((unsigned)tiles), dim3(kKinThreads), 0, st, rows, cb, N, nv, d_drop, d_z, d_sum.get(), ld,
                         v0 > 0 ? 1 : 0);
    else
      hipLaunchKernelGGL(kin_ibs_kernel, dim3((unsigned)tiles), dim3(kKinThreads), 0, st, rows, cb, N, nv, d_drop, d_cc.get(),
                         d_ce.get(), ld, v0 > 0 ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[2], st));
    HIP_TRY(c, sync_stream(st));  // (the next chunk reuses the site pass's work space)
    float a = 0.f, b = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
    HIP_TRY(c, hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
    ms_stats += a, ms_product += b;
  }

  HIP_TRY(c, hipEventRecord(ev.e[0], st));
  const unsigned fin_blocks = (unsigned)std::min<size_t>((nn + 255) / 256, (size_t)8192);
  if (bn)
    hipLaunchKernelGGL(kin_finish_bn_kernel, dim3(fin_blocks), dim3(256), 0, st, d_sum.get(), N, ld, d_tot, d_K.get());
  else
    hipLaunchKernelGGL(kin_finish_ibs_kernel, dim3(fin_blocks), dim3(256), 0, st, d_cc.get(), d_ce.get(), N, ld, d_K.get());
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(K_out, d_K.get(), sizeof(double) * nn, hipMemcpyDeviceToHost, st));
  KinTotals tot;
  HIP_TRY(c, hipMemcpyAsync(&tot, d_tot, sizeof(KinTotals), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipEventRecord(ev.e[1], st));
  HIP_TRY(c, sync_stream(st));
  float f = 0.f;
  HIP_TRY(c, hipEventElapsedTime(&f, ev.e[0], ev.e[1]));
  info->sites = V;
  info->sites_used = (int64_t)tot.used;
  info->filtered_missing = (int64_t)tot.filtered_missing;
  info->filtered_maf = (int64_t)tot.filtered_maf;
  info->monomorphic = (int64_t)tot.monomorphic;
  info->ms_stats = ms_stats, info->ms_product = ms_product, info->ms_finish = (double)f;
  return RVT_OK;
}

}  // extern "C"
