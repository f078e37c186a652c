// rvtests_amd — host side (C++): GPU-backed ModelFitter adapters, ModelParser, ModelManager::create.
// See ModelFitterGpu.h for the reference lines each class mirrors.
#include "ModelFitterGpu.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <mutex>
#include <thread>

namespace rvt_host {

std::string floatToString(double v) {
  std::stringstream ss;
  ss.precision(6);
  ss << std::noshowpoint << v;
  return ss.str();
}

// printf("%g") without printf: a row of MetaCov's window is a thousand of these, and glibc's conversion (arbitrary precision,
// locale, stream state) costs ~200 ns each — the formatting threads of the adapter spent more on a flush than the device.
// The six significant digits are round-to-nearest of v x 10^(5 - k) computed in double: v x 10^p is ONE rounding of an exact
// product for |p| <= 22 (10^p is a double), i.e. off by at most 1.2e-10 at 10^6, so the digits are those of the exact decimal
// expansion unless the fraction lies within 1e-7 of one half — those (and everything outside the range, infinities, NaN) go
// to snprintf.  Same characters as "%g" in the C locale: fixed notation for exponents -4 .. 5, otherwise d.ddddde+XX, trailing
// zeros and a trailing point removed, "-0" for a negative zero.  tests/test_host_format_cpu.py: 3 million values against printf.
size_t formatG(double v, char* out) {
  static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  char* o = out;
  double a = v;
  if (std::signbit(v)) {
    a = -v;
    *o++ = '-';
  }
  if (a == 0.0) {
    *o++ = '0';
    return (size_t)(o - out);
  }
  if (!(a >= 1e-17 && a < 1e22)) return (size_t)snprintf(out, 32, "%g", v);  // (also NaN, infinities)
  int ex;
  (void)std::frexp(a, &ex);                       // a in [2^(ex-1), 2^ex)
  int k = (int)std::floor((ex - 1) * 0.30102999566398120);  // floor(log10 a) or one less
  long long digits = 0;
  for (int attempt = 0; attempt < 3; ++attempt) {
    const int p = 5 - k;
    if (p > 22 || p < -22) return (size_t)snprintf(out, 32, "%g", v);
    const double x = p >= 0 ? a * p10[p] : a / p10[-p];
    if (x < 1e5) {
      --k;
      continue;
    }
    if (x >= 1e6) {
      ++k;
      continue;
    }
    const double r = std::floor(x), f = x - r;
    if (std::fabs(f - 0.5) < 1e-7) return (size_t)snprintf(out, 32, "%g", v);  // a tie, or too close to call in double
    digits = (long long)r + (f > 0.5 ? 1 : 0);
    if (digits == 1000000) {
      digits = 100000;
      ++k;
    }
    break;
  }
  if (digits == 0) return (size_t)snprintf(out, 32, "%g", v);
  char d[6];
  for (int i = 5; i >= 0; --i) {
    d[i] = (char)('0' + digits % 10);
    digits /= 10;
  }
  int nd = 6;
  while (nd > 1 && d[nd - 1] == '0') --nd;  // trailing zeros go
  if (k < -4 || k >= 6) {
    *o++ = d[0];
    if (nd > 1) {
      *o++ = '.';
      for (int i = 1; i < nd; ++i) *o++ = d[i];
    }
    *o++ = 'e';
    int e = k;
    if (e < 0) {
      *o++ = '-';
      e = -e;
    } else {
      *o++ = '+';
    }
    if (e >= 100) *o++ = (char)('0' + e / 100);
    *o++ = (char)('0' + (e / 10) % 10);
    *o++ = (char)('0' + e % 10);
  } else if (k >= 0) {
    for (int i = 0; i <= k; ++i) *o++ = i < nd ? d[i] : '0';
    if (nd > k + 1) {
      *o++ = '.';
      for (int i = k + 1; i < nd; ++i) *o++ = d[i];
    }
  } else {
    *o++ = '0';
    *o++ = '.';
    for (int i = 0; i < -k - 1; ++i) *o++ = '0';
    for (int i = 0; i < nd; ++i) *o++ = d[i];
  }
  return (size_t)(o - out);
}
std::string formatG(double v) {
  char buf[40];
  return std::string(buf, formatG(v, buf));
}

static std::string lower(std::string s) {
  for (auto& c : s) c = (char)std::tolower((unsigned char)c);
  return s;
}

// ---- ModelParser (src/ModelParser.cpp:10-42, 106-151) --------------------------------------------------------
int ModelParser::parse(const std::string& s) {
  std::string arg = lower(s);
  param.clear();
  size_t l = arg.find('[');
  if (l == std::string::npos) {
    name = arg;
    return 0;
  }
  name = arg.substr(0, l);
  if (arg[arg.size() - 1] != ']') return -1;  // "Please use this format: model(model_param1=v1)"
  std::string all = arg.substr(l + 1, arg.size() - 1 - 1 - l);
  size_t pos = 0;
  while (pos <= all.size()) {
    size_t e = all.find_first_of(":,", pos);
    if (e == std::string::npos) e = all.size();
    std::string tok = all.substr(pos, e - pos);
    {  // (empty pieces are kept, as stringTokenize keeps them, base/Utils.h:194-218: "cmc[]" has ONE parameter, the tag "")
      size_t q = tok.find('=');
      if (q == std::string::npos)
        param[tok] = "";
      else
        param[tok.substr(0, q)] = tok.substr(q + 1);
    }
    pos = e + 1;
  }
  return 0;
}
void ModelParser::set(const std::string& tag, const std::string& value) { param[lower(tag)] = value; }
bool ModelParser::hasTag(const std::string& tag) const { return param.find(lower(tag)) != param.end(); }
const char* ModelParser::value(const std::string& tag) const {
  auto it = param.find(lower(tag));
  return it == param.end() ? nullptr : it->second.c_str();
}
const ModelParser& ModelParser::assign(const std::string& tag, double* v, double def) const {
  *v = hasTag(tag) ? atof(value(tag)) : def;
  return *this;
}
const ModelParser& ModelParser::assign(const std::string& tag, int* v, int def) const {
  // (through a double, as src/ModelParser.cpp:130-146: "nPerm=1e4" is 10 000)
  *v = hasTag(tag) ? (int)atof(value(tag)) : def;
  return *this;
}
const ModelParser& ModelParser::assign(const std::string& tag, bool* v, bool def) const {
  *v = hasTag(tag) ? true : def;
  return *this;
}

// ---- pieces the models share --------------------------------------------------------------------------------------------
namespace {
const char* const kNoDevice = "no MI355X device: the GPU models have no CPU fallback";
const rvt_params kDefaultParams{1.0, 25.0, 1.0, 25.0, 0, 0.05};
const char* const kPermutationHeader = "NumPerm\tActualPerm\tStat\tNumGreater\tNumEqual\tPermPvalue";

// copyCovariateAndIntercept (src/ModelUtil.h:102-130): X = [1 | covariates], N x (1 + ncov) column-major
std::vector<double> interceptAndCovariates(const GeneData& gd) {
  std::vector<double> X((size_t)gd.N * (1 + gd.ncov));
  for (int64_t i = 0; i < gd.N; ++i) X[i] = 1.0;
  if (gd.ncov) std::memcpy(X.data() + gd.N, gd.covariate, sizeof(double) * (size_t)gd.N * gd.ncov);
  return X;
}

// the 1s and the 0s of the phenotype, for rvt_fam_binary_scale's alpha = log(nCase / nCtrl)
void caseControlCounts(const GeneData& gd, int64_t* nCase, int64_t* nCtrl) {
  *nCase = *nCtrl = 0;
  for (int64_t i = 0; i < gd.N; ++i) {
    if (gd.phenotype[i] == 1) ++*nCase;
    else if (gd.phenotype[i] == 0) ++*nCtrl;
  }
}
}  // namespace

// Permutation::updateValue + Result::writeValue: ints via toString, doubles via floatToString (src/Result.h:52-63); getPvalue :95-98
std::string PermutationState::fields(int nPerm) const {
  const double p = actualPerm == 0 ? 1.0 : 1.0 * (numX + 0.5 * numEqual) / actualPerm;
  return std::to_string(nPerm) + "\t" + std::to_string(actualPerm) + "\t" + floatToString(obs) + "\t" + std::to_string(numX) + "\t" +
         std::to_string(numEqual) + "\t" + floatToString(p);
}

// ---- GpuBroker ----------------------------------------------------------------------------------------------------
GpuBroker& GpuBroker::instance() {
  static GpuBroker b;
  static bool init = false;
  if (!init) {
    init = true;
    if (const char* e = getenv("RVT_ADAPTER_BATCH")) b.setBatchWindow(atoi(e));
    if (const char* e = getenv("RVT_ADAPTER_BATCH_GB")) b.setBatchBytes((size_t)std::max(1, atoi(e)) << 30);
    if (const char* e = getenv("RVT_DOSAGE")) {  // "1": dosages; "d3": dosages printed with three decimals
      if (e[0] == 'd')
        b.setDosage(atoi(e + 1));
      else if (atoi(e) != 0)
        b.setDosage(-1);
    }
  }
  return b;
}

int GpuBroker::ensureContext(int device) {
  if (ctx) return 0;
  std::vector<int> ids;
  if (const char* e = getenv("RVT_DEVICES")) {  // e.g. RVT_DEVICES=0,1,2,3
    for (const char* p = e; *p;) {
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p) break;
      ids.push_back((int)v);
      p = (*end == ',') ? end + 1 : end;
    }
  }
  if (ids.empty()) ids.push_back(device);
  const int rc = rvt_group_init(&grp, (int)ids.size(), ids.data());
  if (rc) return rc;
  ctx = rvt_group_member(grp, 0);
  if (dosage) {
    int den = 0;
    if (dosageDecimals >= 0 && dosageDecimals <= 3) {
      den = 1;
      for (int k = 0; k < dosageDecimals; ++k) den *= 10;
    }
    return rvt_group_set_content(grp, 0, den);
  }
  return 0;
}

void GpuBroker::registerTests(uint32_t mask, const rvt_params& p) {
  tests |= mask;
  if (mask & RVT_TEST_SKAT) {
    params.skat_beta1 = p.skat_beta1;
    params.skat_beta2 = p.skat_beta2;
    params.skat_nperm = p.skat_nperm;
    params.skat_alpha = p.skat_alpha;
  }
  if (mask & RVT_TEST_SKATO) {
    params.skato_beta1 = p.skato_beta1;
    params.skato_beta2 = p.skato_beta2;
  }
}

void GpuBroker::shutdown() {
  moreGenes.clear();  // frees their device blocks, while the group still exists
  moreRows.clear();
  moreReady.clear();
  moreY.clear();
  moreBytes = 0;
  moreSerial = -1;
  moreTests = 0;
  if (grp) rvt_group_destroy(grp);
  grp = nullptr;
  ctx = nullptr;
  rows.clear();
  pendingSerial.clear();
  pendingBytes = 0;
  recBytes.clear();
  ready.clear();
  failedSerial.clear();
  haveNull = false;
  haveFamNull = false;
  famSerial = -1;
  famTests = 0;
  kinU = nullptr;
  curSerial = -1;
  tests = 0;
}

// copyCovariateAndIntercept (src/ModelUtil.h:102-130) + the null fit SkatTest::fit caches (src/Model.h:2672-2699)
int GpuBroker::installNull(const GeneData& gd, bool binary, std::string* err) {
  flushBurdenMore();  // the analytic burden tests' pending genes belong to the null model installed so far
  const int d = 1 + gd.ncov;
  const std::vector<double> X = interceptAndCovariates(gd);
  const int trait = binary ? RVT_TRAIT_BINARY : RVT_TRAIT_QUANTITATIVE;
  int rc;
  if (!fitter) {
    // default: LinearRegression::FitLinearModel / LogisticRegression::FitLogisticModel(cov, y, 100) on the device
    rc = rvt_group_fit_null(grp, trait, gd.N, d, X.data(), gd.phenotype, nullptr, nullptr);
  } else {
    // a caller-supplied fitter (e.g. the reference's own regression classes inside the rvtests tree)
    std::vector<double> res(gd.N), v(gd.N);
    double sigma2 = 1.0;
    if (fitter(binary, gd.N, d, X.data(), gd.phenotype, res.data(), v.data(), &sigma2)) {
      *err = binary ? "failed in fitting null model (logistic model)." : "failed in fitting null model (linear model).";
      return -1;
    }
    rc = rvt_group_set_null(grp, trait, gd.N, d, X.data(), res.data(), v.data(), sigma2);
  }
  if (rc) {
    *err = binary ? "failed in fitting null model (logistic model)." : "failed in fitting null model (linear model).";
    *err += std::string(" [") + rvt_group_last_error(grp) + "]";
    return -1;
  }
  haveNull = true;
  return 0;
}

rvt_ctx* GpuBroker::contextWithNull(const GeneData& gd, bool binary, std::string* err) {
  if (!context(err)) return nullptr;
  if (!haveNull || gd.phenotypeUpdated || gd.covariateUpdated)
    if (installNull(gd, binary, err)) return nullptr;
  return ctx;
}

rvt_ctx* GpuBroker::context(std::string* err) {
  if (ensureContext(0)) {
    *err = kNoDevice;
    return nullptr;
  }
  return ctx;
}

rvt_ctx* GpuBroker::contextWithFamNull(const GeneData& gd, std::string* err) {
  if (!context(err)) return nullptr;
  if (kinU != gd.kinshipIdentity()) {  // a new decomposition (autosomes vs X region in the reference): install it once
    const GeneData::KinshipFamilies& kf = gd.kinshipFamilies;
    if (gd.hasDenseKinship() ? rvt_set_kinship(ctx, gd.N, gd.kinshipU, gd.kinshipS)
                             : rvt_set_kinship_families(ctx, gd.N, kf.nFam, kf.famPtr, kf.members, kf.blocks, kf.S)) {
      *err = rvt_last_error(ctx);
      return nullptr;
    }
    kinU = gd.kinshipIdentity();
    haveFamNull = false;
  }
  if (!haveFamNull || gd.phenotypeUpdated || gd.covariateUpdated) {
    if (rvt_fit_fam_null(ctx, gd.N, 1 + gd.ncov, interceptAndCovariates(gd).data(), gd.phenotype, &famNull)) {
      *err = "SKAT test (for related individuals) failed in fitting null model (SKAT)";
      return nullptr;
    }
    haveFamNull = true;
  }
  return ctx;
}

const rvt_gene_result* GpuBroker::famResultFor(const GeneData& gd, std::string* err) {
  if (gd.serial == famSerial) return famOk ? &famRec : nullptr;
  famSerial = gd.serial;
  famOk = false;
  rvt_ctx* cx = contextWithFamNull(gd, err);
  if (withGene(cx, gd, err, [&](const double* const* block, const int* M) {
        return rvt_run_fam_tests(cx, 1, block, M, &gd.serial, famTests, &famRec);
      }))
    return nullptr;
  famOk = true;
  return &famRec;
}

int GpuBroker::withGene(rvt_ctx* cx, const GeneData& gd, std::string* err, const GeneCall& call) {
  if (!cx) return -1;
  int rc;
  {
    DeviceBlock block;
    if (block.alloc(cx, gd.M, err) || block.upload(gd.M, gd.genotype, err)) return -1;
    const double* p = block.get();
    rc = call(&p, &gd.M);
  }  // (the block is freed before the call's error text is read)
  if (rc) *err = rvt_last_error(cx);
  return rc ? -1 : 0;
}

int GpuBroker::submit(const GeneData& gd, bool binary, std::string* err) {
  if (gd.serial == curSerial) return curOk ? 0 : -1;  // another model of the same gene already submitted it
  // genes in flight are bounded by count and by the bytes of their device blocks (a 1024-variant gene is 4 GB at
  // N = 500 000)
  const size_t geneBytes = sizeof(double) * (size_t)gd.N * (size_t)gd.M;
  // a full window first takes what has finished (no waiting: the device keeps its batches in flight); only when
  // nothing comes back and twice the window is pending does the caller wait
  if ((int)pendingSerial.size() >= window || (!pendingSerial.empty() && pendingBytes + geneBytes > windowBytes)) {
    drainReady();
    if ((int)pendingSerial.size() >= 2 * window || (!pendingSerial.empty() && pendingBytes + geneBytes > 2 * windowBytes))
      flush();
  }
  curSerial = gd.serial;
  curOk = false;
  auto failed = [&]() {
    failedSerial.push_back(gd.serial);
    return -1;
  };
  if (ensureContext(0)) {
    *err = kNoDevice;
    return failed();
  }
  if (!haveNull || gd.phenotypeUpdated || gd.covariateUpdated) {
    flush();  // pending genes belong to the previous null model
    if (installNull(gd, binary, err)) return failed();
  }
  if (gd.bed) {  // 2-bit rows before consolidation: frequencies and imputation happen on the device
    if (rvt_group_submit_gene_bed(grp, gd.serial, gd.M, gd.bed, tests, &params, nullptr)) {
      *err = rvt_group_last_error(grp);
      return failed();
    }
  } else {
    if ((int)gd.markerFrequency.size() < gd.M) {
      *err = "marker frequencies missing";
      return failed();
    }
    if (rvt_group_submit_gene(grp, gd.serial, gd.M, gd.genotype, gd.markerFrequency.data(), tests, &params)) {
      *err = rvt_group_last_error(grp);
      return failed();
    }
  }
  pendingSerial.push_back(gd.serial);
  pendingBytes += geneBytes;
  recBytes[gd.serial] = geneBytes;
  curOk = true;
  return 0;
}

void GpuBroker::enqueue(DeferredGeneTest* m, TextSink* fp, const std::string& siteTab, int64_t serial) {
  rows.push_back(Row{m, fp, siteTab, serial});
}

// Write every row whose gene has its record (or failed at submission), in enqueue order, and stop at the first row that
// has to wait — rows reach each file in the order the reference writes them.
void GpuBroker::writeReadyRows(bool all) {
  size_t k = 0;
  for (; k < rows.size(); ++k) {
    const Row& r = rows[k];
    auto it = ready.find(r.serial);
    const bool failed = std::find(failedSerial.begin(), failedSerial.end(), r.serial) != failedSerial.end();
    if (it == ready.end() && !failed && !all) break;
    r.fp->write(r.siteTab + r.model->formatRow(it == ready.end() ? nullptr : &it->second));
  }
  rows.erase(rows.begin(), rows.begin() + k);
  // records nobody waits for any more: every remaining row belongs to a later gene (serials only grow)
  const int64_t keep = rows.empty() ? (pendingSerial.empty() ? INT64_MAX : pendingSerial.front()) : rows.front().serial;
  for (auto it = ready.begin(); it != ready.end();) it = (it->first < keep) ? ready.erase(it) : std::next(it);
  failedSerial.erase(std::remove_if(failedSerial.begin(), failedSerial.end(), [&](int64_t s) { return s < keep; }),
                     failedSerial.end());
}

// take what the device has finished, without waiting (rvt_collect_ready): the pipeline keeps running
int GpuBroker::drainReady() {
  if (!grp || pendingSerial.empty()) return 0;
  std::vector<rvt_gene_result> recs(pendingSerial.size());
  int n = 0;
  const int rc = rvt_group_collect_ready(grp, recs.data(), (int)recs.size(), &n);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    ready[recs[i].gene_id] = recs[i];
    pendingBytes -= std::min(pendingBytes, recBytes[recs[i].gene_id]);
    recBytes.erase(recs[i].gene_id);
  }
  pendingSerial.erase(pendingSerial.begin(), pendingSerial.begin() + n);
  writeReadyRows(false);
  return 0;
}

int GpuBroker::flush() {
  int rc = 0;
  if (ctx && !pendingSerial.empty()) {
    std::vector<rvt_gene_result> recs(pendingSerial.size());
    int n = 0;
    rc = rvt_group_collect(grp, recs.data(), (int)recs.size(), &n);
    if (!rc)
      for (int i = 0; i < n; ++i) ready[recs[i].gene_id] = recs[i];
  }
  pendingSerial.clear();
  recBytes.clear();
  pendingBytes = 0;
  writeReadyRows(true);
  ready.clear();
  failedSerial.clear();
  const int rcMore = flushBurdenMore();
  return rc ? rc : rcMore;
}

// ---- DeferredGeneTest ------------------------------------------------------------------------------------------------------
DeferredGeneTest::DeferredGeneTest(const char* name, uint32_t test, const rvt_params& p, const std::string& header_)
    : header(header_) {
  modelName = name;
  if (test) GpuBroker::instance().registerTests(test, p);
}
int DeferredGeneTest::fit(GeneData* dc) {
  curSerial = dc->serial;
  return GpuBroker::instance().submit(*dc, isBinaryOutcome(), &lastError);
}
void DeferredGeneTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) { fp->write(siteInfo.headerTab() + header); }
void DeferredGeneTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  GpuBroker::instance().enqueue(this, fp, siteInfo.valueTab(), curSerial);
}
void DeferredGeneTest::writeFootnote(TextSink*) { GpuBroker::instance().flush(); }

// ---- SkatTest ----------------------------------------------------------------------------------------------------------
SkatTest::SkatTest(int nPerm, double alpha, double beta1, double beta2)
    : DeferredGeneTest("Skat", RVT_TEST_SKAT, rvt_params{beta1, beta2, 1.0, 25.0, nPerm, alpha},
                       // with permutations: Permutation::writeHeader (src/Permutation.h:51-56,99-104)
                       nPerm > 0 ? std::string("Q\tPvalue\t") + kPermutationHeader + "\n" : "Q\tPvalue\n"),
      usePermutation(nPerm > 0) {}
std::string SkatTest::formatRow(const rvt_gene_result* res) const {
  // fitOK: genotype.cols == 0 after filtering -> NA row (src/Model.h:2665-2668)
  if (!res || !res->skat_ok || (usePermutation && !res->perm_ok))
    return usePermutation ? "NA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n" : "NA\tNA\n";
  std::string line = formatG(res->skat_Q) + "\t" + formatG(res->skat_p);
  if (usePermutation)  // Permutation::updateValue: ints via toString, doubles via floatToString (src/Result.h:52-63)
    line += "\t" + std::to_string(res->perm_num_perm) + "\t" + std::to_string(res->perm_actual_perm) + "\t" +
            floatToString(res->skat_Q) + "\t" + std::to_string(res->perm_num_greater) + "\t" +
            std::to_string(res->perm_num_equal) + "\t" + floatToString(res->perm_pvalue);
  return line + "\n";
}

// ---- SkatOTest -----------------------------------------------------------------------------------------------------------
SkatOTest::SkatOTest(double beta1, double beta2)
    : DeferredGeneTest("SkatO", RVT_TEST_SKATO, rvt_params{1.0, 25.0, beta1, beta2, 0, 0.05}, "Q\trho\tPvalue\n") {}
std::string SkatOTest::formatRow(const rvt_gene_result* res) const {
  // fitOK = (skato.Fit(...) == 0) (src/Model.h:2853-2859)
  if (!res || res->n_poly == 0 || !res->skato_ok) return "NA\tNA\tNA\n";
  return formatG(res->skato_Q) + "\t" + formatG(res->skato_rho) + "\t" + formatG(res->skato_p) + "\n";
}

// ---- CMCTest / ZegginiTest -------------------------------------------------------------------------------------------------
CMCTest::CMCTest() : DeferredGeneTest("CMC", RVT_TEST_CMC, kDefaultParams, "NonRefSite\tPvalue\n") {}
std::string CMCTest::formatRow(const rvt_gene_result* res) const {
  if (!res || !res->cmc_ok) return "NA\tNA\n";
  return std::to_string(res->cmc_nonref) + "\t" + floatToString(res->cmc_p) + "\n";
}

ZegginiTest::ZegginiTest() : DeferredGeneTest("Zeggini", RVT_TEST_ZEGGINI, kDefaultParams, "Pvalue\n") {}
std::string ZegginiTest::formatRow(const rvt_gene_result* res) const {
  return (res && res->zeg_ok) ? floatToString(res->zeg_p) + "\n" : std::string("NA\n");
}

// ---- AnalyticVTTest ---------------------------------------------------------------------------------------------------------
AnalyticVTTest::AnalyticVTTest(bool related_)
    : DeferredGeneTest(related_ ? "FamAnalyticVT" : "AnalyticVT", related_ ? 0 : RVT_TEST_ANALYTICVT, kDefaultParams,
                       "MinMAF\tMaxMAF\tOptimMAF\tOptimNumVar\tU\tV\tStat\tPvalue\n"),  // result.addHeader order, src/Model.h:2123-2130
      related(related_) {}
int AnalyticVTTest::fit(GeneData* dc) {
  if (!related) return DeferredGeneTest::fit(dc);
  fitOK = false;
  if (isBinaryOutcome()) {  // src/Model.h:2143-2149
    lastError = "Analytic VT test does not support binary outcomes. Results will be all NAs.";
    return -1;
  }
  if (!dc->hasKinship()) {  // model and data do not match (src/Model.h:2156-2160)
    lastError = "Analytic VT test has internal error!";
    return -1;
  }
  rvt_ctx* ctx = GpuBroker::instance().contextWithFamNull(*dc, &lastError);
  if (GpuBroker::withGene(ctx, *dc, &lastError,
                          [&](const double* const* block, const int* M) { return rvt_fam_analytic_vt(ctx, 1, block, M, &rec); }))
    return -1;
  fitOK = rec.vt_ok != 0;
  return fitOK ? 0 : -1;
}
void AnalyticVTTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  if (!related) {
    DeferredGeneTest::writeOutput(fp, siteInfo);
    return;
  }
  fp->write(siteInfo.valueTab());
  fp->write(formatRow(fitOK ? &rec : nullptr));
}
void AnalyticVTTest::writeFootnote(TextSink* fp) {
  if (!related) DeferredGeneTest::writeFootnote(fp);
}
std::string AnalyticVTTest::formatRow(const rvt_gene_result* r) const {
  // not fitted (binary trait, no polymorphic site, no usable threshold, integral not converged to 1e-3): the Result keeps
  // its cleared values (src/Model.h:2233-2246 after ModelFitter::reset)
  if (!r || !r->vt_ok || r->vt_p_error > 1e-3) return "NA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n";
  return floatToString(r->vt_minmaf) + "\t" + floatToString(r->vt_maxmaf) + "\t" + floatToString(r->vt_optmaf) + "\t" +
         std::to_string(r->vt_optnum) + "\t" + floatToString(r->vt_U) + "\t" + floatToString(r->vt_V) + "\t" +
         floatToString(r->vt_stat) + "\t" + floatToString(r->vt_p) + "\n";
}

// ---- KbacTest ---------------------------------------------------------------------------------------------------------------
KbacTest::KbacTest(int nPerm_, double alpha_) : nPerm(nPerm_), alpha(alpha_) { modelName = "Kbac"; }
int KbacTest::fit(GeneData* dc) {
  fitOK = false;
  if (!isBinaryOutcome()) {  // src/Model.h:2930-2936
    lastError = "KBAC test does not support continuous outcomes. Results will be all NAs.";
    return -1;
  }
  if (dc->ncov != 0) {  // src/Model.h:2937-2942
    lastError = "KBAC test does not support covariates. Results will be all NAs.";
    return -1;
  }
  rvt_ctx* ctx = GpuBroker::instance().contextWithNull(*dc, true, &lastError);  // (the null model defines N on the device)
  if (GpuBroker::withGene(ctx, *dc, &lastError, [&](const double* const* block, const int* M) {
        return rvt_kbac_blocks(ctx, 1, block, M, dc->markerFrequency.data(), dc->phenotype, nPerm, alpha, &rec);
      }))
    return -1;
  fitOK = rec.fit_ok != 0;
  return fitOK ? 0 : -1;
}
void KbacTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) { fp->write(siteInfo.headerTab() + "Pvalue\n"); }
void KbacTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  if (!fitOK) {
    fp->write("NA\n");
  } else {
    char buf[64];
    snprintf(buf, sizeof(buf), "%f\n", rec.pvalue);  // fp->printf("%f\n", this->pValue), src/Model.h:3005
    fp->write(buf);
  }
}

// ---- VariableThresholdPrice ---------------------------------------------------------------------------------------------------
VariableThresholdPrice::VariableThresholdPrice(int nPerm_, double alpha_) : nPerm(nPerm_), alpha(alpha_) {
  modelName = "VariableThresholdPrice";
}
int VariableThresholdPrice::fit(GeneData* dc) {
  fitOK = false;
  rvt_ctx* ctx = GpuBroker::instance().contextWithNull(*dc, isBinaryOutcome(), &lastError);  // (the null model defines N on the device)
  if (GpuBroker::withGene(ctx, *dc, &lastError, [&](const double* const* block, const int* M) {
        return rvt_vtprice_blocks(ctx, 1, block, M, dc->markerFrequency.data(), dc->phenotype, nPerm, alpha, &rec);
      }))
    return -1;
  fitOK = rec.fit_ok != 0;
  if (!fitOK) return -1;  // genotype.cols == 0: nothing below was touched (src/Model.h:1758-1761)
  zmax = rec.zmax;
  optimalFreq = rec.opt_freq;
  perm.take(rec, rec.zmax);  // perm.init(fabs(zmax))
  return 0;
}
void VariableThresholdPrice::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  // (after writeHeaderTab's own tab: an empty column, src/Model.h:1808-1809)
  fp->write(siteInfo.headerTab() + "\tOptFreq\tZmax\t" + kPermutationHeader + "\n");
}
void VariableThresholdPrice::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  fp->write("\t" + formatG(optimalFreq) + "\t" + formatG(zmax) + "\t" + perm.fields(nPerm) + "\n");
}

// ---- RareCoverTest / MadsonBrowningTest -----------------------------------------------------------------------------------------
RareCoverTest::RareCoverTest(int nPerm_, double alpha_) : nPerm(nPerm_), alpha(alpha_) { modelName = "RareCover"; }
int RareCoverTest::fit(GeneData* dc) {
  fitOK = false;
  if (!isBinaryOutcome()) {  // src/Model.h:1432-1438
    lastError = "Rarecover test does not support continuous outcomes. Results will be all NAs.";
    return -1;
  }
  if (dc->ncov != 0) {  // src/Model.h:1439-1445
    lastError = "Rarecover test does not support covariates. Results will be all NAs.";
    return -1;
  }
  rvt_ctx* ctx = GpuBroker::instance().contextWithNull(*dc, true, &lastError);  // (the null model defines N on the device)
  if (GpuBroker::withGene(ctx, *dc, &lastError, [&](const double* const* block, const int* M) {
        return rvt_rarecover_blocks(ctx, 1, block, M, dc->phenotype, nPerm, alpha, &rec);
      }))
    return -1;
  fitOK = rec.fit_ok != 0;
  if (!fitOK) return -1;  // genotype.cols == 0: perm.init was not reached (src/Model.h:1448-1451)
  numSelected = rec.n_selected;
  perm.take(rec, rec.stat);
  return 0;
}
void RareCoverTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + "NumIncludeMarker\t" + kPermutationHeader + "\n");
}
void RareCoverTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  fp->write((fitOK ? std::to_string(numSelected) : std::string("NA")) + "\t" + perm.fields(nPerm) + "\n");
}

MadsonBrowningTest::MadsonBrowningTest(int nPerm_, double alpha_) : nPerm(nPerm_), alpha(alpha_) { modelName = "MadsonBrowning"; }
int MadsonBrowningTest::fit(GeneData* dc) {
  fitOK = false;
  if (!isBinaryOutcome()) {  // src/Model.h:1257-1263
    lastError = "Madsen-Browning test does not support continuous outcomes. Results will be all NAs.";
    return -1;
  }
  rvt_ctx* ctx = GpuBroker::instance().contextWithNull(*dc, true, &lastError);  // the logistic null model, covariates included
  if (GpuBroker::withGene(ctx, *dc, &lastError, [&](const double* const* block, const int* M) {
        return rvt_mb_blocks(ctx, 1, block, M, dc->phenotype, nPerm, alpha, &rec);
      }))
    return -1;
  if (rec.n_poly == 0 || (!rec.fit_ok && rec.actual_perm == 0 && rec.stat == 0.0)) return -1;  // perm.init was not reached
  fitOK = rec.fit_ok != 0;  // (0 here: the eleventh failed shuffle — the counters printed are those reached)
  perm.take(rec, rec.stat);
  return fitOK ? 0 : -1;
}
void MadsonBrowningTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab());
  if (isBinaryOutcome())
    fp->write(kPermutationHeader);  // perm.writeHeader: no line end of its own
  else
    fp->write("Pvalue\n");
  fp->write("\n");  // (src/Model.h:1319: after "Pvalue\n" this leaves an empty line under the header)
}
void MadsonBrowningTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  if (isBinaryOutcome())
    fp->write(perm.fields(nPerm) + "\n");
  else
    fp->write("NA\n");
}

// ---- CMCWaldTest / ZegginiWaldTest / FpTest / CMCFisherExactTest -------------------------------------------------------------------
namespace {
// src/ModelFitter.h warnOnce: the reference prints these messages to stderr the first time each is seen and goes on (the models
// above keep theirs in lastError, where the reference returns an error to its caller instead).  fit() runs on the caller's thread;
// the lock keeps the list whole should two model sets ever be driven from two threads.
void warnOnce(const std::string& msg) {
  static std::mutex mu;
  static std::vector<std::string> seen;
  std::lock_guard<std::mutex> lock(mu);
  if (std::find(seen.begin(), seen.end(), msg) != seen.end()) return;
  seen.push_back(msg);
  fprintf(stderr, "%s\n", msg.c_str());
}
}  // namespace

int GpuBroker::submitBurdenMore(const GeneData& gd, bool binary, std::string* err) {
  if (gd.serial == moreSerial) return moreOk ? 0 : -1;  // another of the four models already submitted this gene
  moreSerial = gd.serial;
  moreOk = false;
  const size_t geneBytes = sizeof(double) * (size_t)gd.N * (size_t)gd.M;
  if ((int)moreGenes.size() >= window || (!moreGenes.empty() && moreBytes + geneBytes > windowBytes)) flushBurdenMore();
  rvt_ctx* cx = contextWithNull(gd, binary, err);  // (a new null model runs the pending genes first: installNull)
  if (!cx) return -1;
  if ((int)gd.markerFrequency.size() < gd.M) {
    *err = "marker frequencies missing";
    return -1;
  }
  MoreGene g{gd.serial, DeviceBlock(), gd.M, 1 + gd.ncov, {}};
  if (g.block.alloc(cx, gd.M, err) || g.block.upload(gd.M, gd.genotype, err)) return -1;
  g.af.assign(gd.markerFrequency.begin(), gd.markerFrequency.begin() + gd.M);
  if (moreGenes.empty()) moreY.assign(gd.phenotype, gd.phenotype + gd.N);
  moreGenes.push_back(std::move(g));
  moreBytes += geneBytes;
  moreOk = true;
  return 0;
}

void GpuBroker::enqueueBurdenMore(BurdenMoreTest* m, TextSink* fp, const std::string& siteTab, int64_t serial) {
  moreRows.push_back(MoreRow{m, fp, siteTab, serial});
  writeReadyMoreRows();  // (a gene that was not submitted has nothing to wait for)
}

// rows in call order, up to the first whose gene is still waiting for its call
void GpuBroker::writeReadyMoreRows() {
  size_t k = 0;
  for (; k < moreRows.size(); ++k) {
    const MoreRow& r = moreRows[k];
    if (std::any_of(moreGenes.begin(), moreGenes.end(), [&](const MoreGene& g) { return g.serial == r.serial; })) break;
    auto it = moreReady.find(r.serial);
    const bool have = it != moreReady.end();
    r.fp->write(r.model->formatRows(r.siteTab, have ? &it->second.rec : nullptr, have ? it->second.d : 0));
  }
  moreRows.erase(moreRows.begin(), moreRows.begin() + k);
}

int GpuBroker::flushBurdenMore() {
  int rc = 0;
  // the last call's records served the rows of its genes; the current gene's stays for the models that have yet to see it
  for (auto it = moreReady.begin(); it != moreReady.end();) it = (it->first != moreSerial) ? moreReady.erase(it) : std::next(it);
  if (ctx && !moreGenes.empty()) {
    const int n = (int)moreGenes.size();
    std::vector<const double*> ptr((size_t)n);
    std::vector<int> Ms((size_t)n);
    std::vector<double> af;
    for (int g = 0; g < n; ++g) {
      ptr[g] = moreGenes[g].block.get();
      Ms[g] = moreGenes[g].M;
      af.insert(af.end(), moreGenes[g].af.begin(), moreGenes[g].af.end());
    }
    std::vector<rvt_burden_more_result> recs((size_t)n);
    rc = rvt_burden_blocks(ctx, n, ptr.data(), Ms.data(), af.data(), moreY.data(), moreTests, recs.data());
    if (rc)
      warnOnce(std::string("burden tests failed: ") + rvt_last_error(ctx) + ". Results will be all NAs.");
    else
      for (int g = 0; g < n; ++g) moreReady[moreGenes[g].serial] = MoreRecord{recs[g], moreGenes[g].d};
  }
  moreGenes.clear();  // frees their device blocks
  moreBytes = 0;
  writeReadyMoreRows();
  return rc;
}

BurdenMoreTest::BurdenMoreTest(uint32_t which) { GpuBroker::instance().registerBurdenMore(which); }
int BurdenMoreTest::fit(GeneData* dc) {
  curSerial = dc->serial;
  return GpuBroker::instance().submitBurdenMore(*dc, isBinaryOutcome(), &lastError);
}
void BurdenMoreTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  GpuBroker::instance().enqueueBurdenMore(this, fp, siteInfo.valueTab(), curSerial);
}
void BurdenMoreTest::writeFootnote(TextSink*) { GpuBroker::instance().flushBurdenMore(); }

BurdenWaldTest::BurdenWaldTest(const char* name, bool zeggini_)
    : BurdenMoreTest(zeggini_ ? RVT_BURDEN_ZEGGINIWALD : RVT_BURDEN_CMCWALD), zeggini(zeggini_) {
  modelName = name;
}
void BurdenWaldTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + (zeggini ? "Beta\tSE\tPvalue\n" : "NonRefSite\tBeta\tSE\tPvalue\n"));
}
std::string BurdenWaldTest::formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int d) {
  // genotype.cols == 0 fails BEFORE X is rebuilt: X keeps the previous gene's shape (src/Model.h:925-928)
  if (r && r->n_poly > 0) xCols = 1 + d;  // [1, collapsed, covariates]
  const rvt_burden_wald_fit* f = !r ? nullptr : zeggini ? &r->zeggini_wald : &r->cmc_wald;
  const bool ok = r && r->n_poly > 0 && f->ok;
  std::string rows;
  for (int i = 1; i < xCols; ++i) {  // src/Model.h:959-978, 1050-1069
    rows += siteTab;
    if (ok) {
      if (!zeggini) rows += std::to_string(r->nonref_site) + "\t";
      rows += floatToString(f->beta[i - 1]) + "\t" + floatToString(f->se[i - 1]) + "\t" + floatToString(f->pvalue[i - 1]);
    } else {
      rows += zeggini ? "NA\tNA\tNA" : "NA\tNA\tNA\tNA";
    }
    rows += "\n";
  }
  return rows;
}

void FpTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) { fp->write(siteInfo.headerTab() + "Pvalue\n"); }
std::string FpTest::formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int) {
  return siteTab + ((r && r->n_poly > 0 && r->fp_ok) ? floatToString(r->fp_pvalue) : std::string("NA")) + "\n";
}

int CMCFisherExactTest::fit(GeneData* dc) {
  curSerial = dc->serial;
  if (!isBinaryOutcome()) {  // src/Model.h:1099-1105
    warnOnce("Fisher's exact test does not support continuous outcomes. Results will be all NAs.");
    return -1;
  }
  if (dc->ncov != 0) {  // :1110-1116 (the reference tests genotype.cols == 0 first: the row is the same NA row either way)
    warnOnce("Fisher's exact test does not support covariates. Results will be all NAs.");
    return -1;
  }
  return BurdenMoreTest::fit(dc);
}
void CMCFisherExactTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + "N00\tN01\tN10\tN11\tPvalueTwoSide\tPvalueLess\tPvalueGreater\n");
}
// result.clearValue() first (:1147): nothing of an earlier gene survives.  (Another of the four models may have submitted a gene
// this one skipped: the engine gives exact_ok = 0 for a quantitative null model or one with covariates.)
std::string CMCFisherExactTest::formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int) {
  if (!r || r->n_poly == 0 || !r->exact_ok) return siteTab + "NA\tNA\tNA\tNA\tNA\tNA\tNA\n";
  return siteTab + std::to_string(r->n00) + "\t" + std::to_string(r->n01) + "\t" + std::to_string(r->n10) + "\t" +
         std::to_string(r->n11) + "\t" + floatToString(r->exact_p_two) + "\t" + floatToString(r->exact_p_less) + "\t" +
         floatToString(r->exact_p_greater) + "\n";
}

// ---- FamSkatTest ----------------------------------------------------------------------------------------------------------
FamSkatTest::FamSkatTest(double, double) {
  modelName = "FamSkat";
  GpuBroker::instance().registerFamTests(RVT_TEST_FAMSKAT);
}
int FamSkatTest::fit(GeneData* dc) {
  fitOK = false;
  if (isBinaryOutcome()) {  // src/Model.h:3071-3078
    lastError = "SKAT test (for related individuals) does not support binary outcomes. Results will be all NAs.";
    return -1;
  }
  if (!dc->hasKinship()) {  // src/Model.h:3079-3087
    lastError = "SKAT test (for related individuals) cannot find kinship. Results will be all NAs.";
    return -1;
  }
  const rvt_gene_result* r = GpuBroker::instance().famResultFor(*dc, &lastError);
  if (!r) return -1;
  rec = *r;
  if (!rec.famskat_ok) return -1;  // genotype.cols == 0 after filtering -> NA row (src/Model.h:3066-3069)
  fitOK = true;
  return 0;
}
void FamSkatTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) { fp->write(siteInfo.headerTab() + "Q\tPvalue\n"); }
void FamSkatTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  if (!fitOK)
    fp->write("NA\tNA\n");
  else
    fp->write(formatG(rec.famskat_Q) + "\t" + formatG(rec.famskat_p) + "\n");
}

// ---- FamCMC / FamZeggini ---------------------------------------------------------------------------------------------------
FamBurdenTest::FamBurdenTest(bool zeg) : zeggini(zeg) {
  modelName = zeg ? "FamZeggini" : "FamCMC";
  GpuBroker::instance().registerFamTests(zeg ? RVT_TEST_FAMZEGGINI : RVT_TEST_FAMCMC);
}
int FamBurdenTest::fit(GeneData* dc) {
  fitOK = false;
  if (isBinaryOutcome()) {  // src/Model.h:2284-2291
    lastError = "burden test (for related individuals) does not support binary outcomes. Results will be all NAs.";
    return -1;
  }
  if (!dc->hasKinship()) {
    lastError = "burden test (for related individuals) cannot find kinship.";
    return -1;
  }
  const rvt_gene_result* r = GpuBroker::instance().famResultFor(*dc, &lastError);
  if (!r) return -1;
  rec = *r;
  if (!(zeggini ? rec.famzeg_ok : rec.famcmc_ok)) return -1;  // genotype.cols == 0 (src/Model.h:2297-2301)
  const double u = zeggini ? rec.famzeg_U : rec.famcmc_U, v = zeggini ? rec.famzeg_V : rec.famcmc_V;
  if (v != 0) effect = u / v;
  fitOK = true;
  return 0;
}
void FamBurdenTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + (zeggini ? "NumSite\tMeanBurden\tU\tV\tEffect\tPvalue\n" : "NumSite\tAF\tU\tV\tEffect\tPvalue\n"));
}
void FamBurdenTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.valueTab());
  if (!fitOK) {  // Result keeps "NA" for values that were not updated (src/Model.h:2344-2357)
    fp->write("NA\tNA\tNA\tNA\tNA\tNA\n");
    return;
  }
  const double af = zeggini ? rec.famzeg_af : rec.famcmc_af, u = zeggini ? rec.famzeg_U : rec.famcmc_U,
               v = zeggini ? rec.famzeg_V : rec.famcmc_V, p = zeggini ? rec.famzeg_p : rec.famcmc_p;
  fp->write(std::to_string(rec.n_poly) + "\t" + floatToString(af) + "\t" + floatToString(u) + "\t" +
            floatToString(v) + "\t" + floatToString(effect) + "\t" + floatToString(p) + "\n");
}

// ---- ColumnBlockTest: one site per fit(), one device call per block of sites ------------------------------------------------
ColumnBlockTest::ColumnBlockTest(const char* capacityEnv) {
  if (const char* e = getenv(capacityEnv)) capacity = std::max(1, std::min(65536, atoi(e)));
}
int ColumnBlockTest::makeRoom(size_t pendingRows) {
  if ((int)pendingRows >= capacity && used > 0 && flush()) return -1;
  if (used >= capacity) {  // flush() could not run: no writeOutput() has named the output sink yet
    lastError = getModelName() + ": the device block is full and no output was requested for its sites";
    return -1;
  }
  return 0;
}
int ColumnBlockTest::sameSampleSize(const GeneData& dc) {
  if (nSample < 0 || nSample == dc.N) return 0;
  lastError = "Sample size changed";
  return -1;
}
int ColumnBlockTest::allocateOnFirstUse(const GeneData& dc) {
  if (nSample >= 0) return 0;
  nSample = dc.N;
  nCovariate = dc.ncov + 1;
  return block.alloc(ctx, capacity, &lastError);
}
void ColumnBlockTest::writeFootnote(TextSink* fp) {
  fout = fp;
  flush();
}

// ---- MetaScoreTest (src/Model.h:3155-3398), unrelated samples ------------------------------------------------------------
MetaScoreTest::MetaScoreTest() : ColumnBlockTest("RVT_METASCORE_BLOCK") { modelName = "MetaScore"; }
MetaScoreTest::~MetaScoreTest() {
  if (fout) flush();
}
int MetaScoreTest::setParameter(const ModelParser& parser) {
  outputSE = parser.hasTag("se");  // src/Model.h:3177-3182 ("gwama" / "bolt" are not provided)
  return 0;
}
int MetaScoreTest::beginRow(const GeneData& dc) {
  if (makeRoom(rows.size())) return -1;
  rows.emplace_back();
  Row& row = rows.back();
  row.all = dc.counter;  // site statistics are printed whether or not the test runs (src/Model.h:3211-3230)
  if (isBinaryOutcome()) {
    row.cases = dc.caseCounter;
    row.ctrls = dc.ctrlCounter;
  }
  return 0;
}
int MetaScoreTest::fit(GeneData* dc) {
  useFamilyModel = dc->hasKinship();  // dc->hasKinship(): MetaFamQtl / MetaFamBinary (src/Model.h:3398-3668)
  if (beginRow(*dc)) return -1;
  if (dc->N == 0) return -1;
  if (sameSampleSize(*dc)) return -1;
  if (flushBeforeNewNull(*dc, &rows)) return -1;
  ctx = useFamilyModel ? GpuBroker::instance().contextWithFamNull(*dc, &lastError)
                       : GpuBroker::instance().contextWithNull(*dc, isBinaryOutcome(), &lastError);
  if (!ctx) return -1;
  if (useFamilyModel && isBinaryOutcome() && (nSample < 0 || dc->phenotypeUpdated)) {
    // MetaFamBinary::FitNullModel (src/Model.h:3566-3581): alpha = log(nCase / nCtrl), b = calculateB()
    int64_t nCase, nCtrl;
    caseControlCounts(*dc, &nCase, &nCtrl);
    if (rvt_fam_binary_scale(ctx, nCase, nCtrl, nullptr, &famB)) {
      lastError = rvt_last_error(ctx);
      return -1;
    }
  }
  if (allocateOnFirstUse(*dc)) return -1;
  if (dc->M != 1) return -1;  // "sanity check, this should not happen" (src/Model.h:3241-3244)
  // the caller overwrites the genotype buffer for the next site: copy the column into the device block now; whether
  // the site is monomorphic (src/Model.h:3246-3250) is decided on the device when the block is processed
  if (putSiteColumn(dc, used)) return -1;
  rows.back().column = used++;
  rows.back().tested = true;
  return 0;
}
void MetaScoreTest::writeHeader(TextSink*, const SiteInfo&) {
  // the header is deferred until the null model is known and is printed with the site columns writeOutput is given
  // (src/Model.h:3262-3264, 3283-3303)
}
void MetaScoreTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fout = fp;
  if (siteHeaderTab.empty()) siteHeaderTab = siteInfo.headerTab();
  if (rows.empty() || rows.back().written) rows.emplace_back();  // writeOutput without a fit(): counters unknown
  rows.back().siteTab = siteInfo.valueTab();
  rows.back().written = true;
}

namespace {
std::string triple(const char* fmt, double a, double b, double c) {
  char buf[128];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return buf;
}
std::string tripleInt(int a, int b, int c) {
  char buf[128];
  snprintf(buf, sizeof(buf), "%d:%d:%d", a, b, c);
  return buf;
}
}  // namespace

int MetaScoreTest::flush() {
  if (!fout) return 0;
  std::vector<int> ok(std::max(used, 1));
  std::vector<double> u(ok.size()), v(ok.size()), eff(ok.size()), se(ok.size()), pv(ok.size());
  bool scored = false;
  std::vector<double> famAf(ok.size());
  if (used > 0 && columnsReady() == 0) {  // (a failed recoding has set lastError: NA rows)
    const int rc = useFamilyModel
                       ? rvt_score_block_fam(ctx, block.get(), used, isBinaryOutcome() ? 1 : 0, ok.data(), u.data(), v.data(),
                                             famAf.data(), pv.data())
                       : rvt_score_block(ctx, block.get(), used, ok.data(), u.data(), v.data(), eff.data(), se.data(),
                                         pv.data());
    if (rc) {
      lastError = rvt_last_error(ctx);
    } else {
      scored = true;
      if (useFamilyModel) {
        // MetaFamQtl::GetEffect / FastLMM::GetSE (src/Model.h:3491-3496, FastLMM.cpp:452-455); MetaFamBinary: U b and
        // V b^2 are returned, effect = U / V / b = (U b) / (V b^2), SE = 1 / sqrt(V b^2) / b (:3647-3662)
        const double bdiv = isBinaryOutcome() ? famB : 1.0;
        for (int k = 0; k < used; ++k) {
          const bool nz = v[k] != 0.0 && bdiv != 0.0;
          eff[k] = nz ? u[k] / v[k] : 0.0;
          se[k] = nz ? 1.0 / std::sqrt(v[k]) / bdiv : 0.0;
        }
      }
    }
  }
  if (!headerOutputted && (scored || used == 0)) {
    // writeSummaryAndHeader (src/Model.h:3283-3297): g_SummaryHeader->outputHeader is the caller's; PrintNullModel:
    if (scored) {
      std::vector<double> beta(nCovariate), covb(nCovariate);
      double sigma2 = 0.0;
      int rcs;
      const rvt_fam_null& fnull = GpuBroker::instance().familyNull();
      if (useFamilyModel) {
        rcs = rvt_fam_null_summary(ctx, covb.data());
        for (int k = 0; k < nCovariate; ++k) beta[k] = fnull.beta[k];
      } else {
        rcs = rvt_null_summary(ctx, beta.data(), covb.data(), &sigma2);
      }
      if (rcs == RVT_OK) {
        fout->write("##NullModelEstimates\n");
        fout->write("## - Name\tBeta\tSD\n");
        fout->write("## - Intercept\t" + formatG(beta[0]) + "\t" + formatG(covb[0]) + "\n");
        for (size_t i = 0; i < covLabel.size(); ++i) {
          if ((int)i + 1 >= nCovariate) break;
          fout->write("## - " + covLabel[i] + "\t" + formatG(beta[i + 1]) + "\t" + formatG(covb[i + 1]) + "\n");
        }
        if (useFamilyModel) {  // GetSigmaG2 = sigma2, GetSigmaE2 = sigma2 * delta (FastLMM.cpp:456-457)
          fout->write("## - SigmaG2\t" + formatG(fnull.sigma2_g) + "\tNA\n");
          fout->write("## - SigmaE2\t" + formatG(fnull.sigma2_g * fnull.delta) + "\tNA\n");
        } else if (isBinaryOutcome()) {  // MetaUnrelatedBinary::PrintNullModel (src/Model.h:3751)
          fout->write("## - Sigma2\tNA\tNA\n");
        } else {
          fout->write("## - Sigma2\t" + formatG(sigma2) + "\tNA\n");
        }
      }
    }
    fout->write(siteHeaderTab);
    fout->write(std::string("AF\tINFORMATIVE_ALT_AC\tCALL_RATE\tHWE_PVALUE\tN_REF\tN_HET\tN_ALT\tU_STAT\tSQRT_V_STAT\t"
                            "ALT_EFFSIZE\t") +
                (outputSE ? "ALT_EFFSIZE_SE\t" : "") + "PVALUE\n");
    headerOutputted = true;
  }
  for (const Row& r : rows) {
    if (!r.written) continue;  // main calls writeOutput after every fit(); a row never written is never printed
    std::string line = r.siteTab;
    const SiteCounts &a = r.all, &ca = r.cases, &ct = r.ctrls;
    if (!isBinaryOutcome()) {  // src/Model.h:3307-3325
      // with kinship a tested site prints FastGetAF instead of the counter's frequency (src/Model.h:3255-3257)
      const double afv = (useFamilyModel && r.tested && scored && r.column >= 0 && ok[r.column]) ? famAf[r.column] : a.af;
      line += (afv >= 0.0 ? floatToString(afv) : std::string("NA")) + "\t";
      line += floatToString(a.ac) + "\t" + floatToString(a.callRate) + "\t" + floatToString(a.hwe) + "\t";
      line += std::to_string(a.nHomRef) + "\t" + std::to_string(a.nHet) + "\t" + std::to_string(a.nHomAlt) + "\t";
    } else {  // src/Model.h:3310-3351
      const double afb = (useFamilyModel && r.tested && scored && r.column >= 0 && ok[r.column]) ? famAf[r.column] : a.af;
      line += (afb >= 0.0 ? triple("%g:%g:%g", afb, ca.af, ct.af) : std::string("NA")) + "\t";
      line += triple("%g:%g:%g", a.ac, ca.ac, ct.ac) + "\t";
      line += triple("%g:%g:%g", a.callRate, ca.callRate, ct.callRate) + "\t";
      line += triple("%g:%g:%g", a.hwe, ca.hwe, ct.hwe) + "\t";
      line += tripleInt(a.nHomRef, ca.nHomRef, ct.nHomRef) + "\t" + tripleInt(a.nHet, ca.nHet, ct.nHet) + "\t" +
              tripleInt(a.nHomAlt, ca.nHomAlt, ct.nHomAlt) + "\t";
    }
    const int k = r.column;
    if (r.tested && scored && k >= 0 && ok[k]) {  // src/Model.h:3353-3364
      line += floatToString(u[k]) + "\t" + floatToString(std::sqrt(v[k])) + "\t" + floatToString(eff[k]) + "\t";
      if (outputSE) line += (v[k] > 0.0 ? floatToString(se[k]) : std::string("NA")) + "\t";
      line += floatToString(pv[k]) + "\n";
    } else {
      line += std::string("NA\tNA\tNA\t") + (outputSE ? "NA\t" : "") + "NA\n";
    }
    fout->write(line);
  }
  rows.clear();
  used = 0;
  return scored || lastError.empty() ? 0 : -1;
}

// ---- SingleVariantWaldTest / SingleVariantScoreTest (src/Model.h:98-180, 259-377), unrelated samples ---------------------
std::string GeneData::columnLabel() const {
  if (!genotypeLabel.empty() || !site) return genotypeLabel;
  return site->get("CHROM") + ":" + site->get("POS");
}

int SingleVariantBlockTest::fit(GeneData* dc) {
  if (makeRoom(rows.size())) return -1;
  rows.emplace_back();
  Row& row = rows.back();
  // X = [1, g, cov] is built (and its labels with it) before the monomorphic check (src/Model.h:117-129)
  row.labels.push_back(dc->columnLabel());
  for (int k = 0; k < dc->ncov; ++k) row.labels.push_back(k < (int)covLabel.size() ? covLabel[k] : std::string());
  row.af = dc->M == 1 && dc->markerFrequency.size() == 1 ? dc->markerFrequency[0] : dc->counter.af;  // getMarkerFrequency(dc, 0)
  if (dc->M != 1 || dc->N == 0) return -1;  // genotype.cols != 1
  if (sameSampleSize(*dc)) return -1;
  if (flushBeforeNewNull(*dc, &rows)) return -1;
  ctx = acquireContext(dc);
  if (!ctx) return -1;
  if (allocateOnFirstUse(*dc)) return -1;
  // the caller overwrites the genotype buffer for the next site: copy the column into the device block now; whether the site
  // is monomorphic is decided on the device when the block is processed
  if (block.uploadColumn(used, dc->genotype, &lastError)) return -1;
  rows.back().column = used++;
  return 0;
}
rvt_ctx* SingleVariantBlockTest::acquireContext(GeneData* dc) {
  return GpuBroker::instance().contextWithNull(*dc, isBinaryOutcome(), &lastError);
}
void SingleVariantBlockTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fout = fp;
  if (rows.empty() || rows.back().written) rows.emplace_back();  // writeOutput without a fit()
  rows.back().siteTab = siteInfo.valueTab();
  rows.back().written = true;
}
int SingleVariantBlockTest::flush() {
  if (!fout) return 0;
  ok.assign(std::max(used, 1), 0);
  const bool ran = used > 0 && runBlock() == 0;
  if (used > 0 && !ran) lastError = rvt_last_error(ctx);
  if (!ran) std::fill(ok.begin(), ok.end(), 0);
  for (const Row& r : rows) {
    if (!r.written) continue;  // main calls writeOutput after every fit(); a row never written is never printed
    fout->write(formatSingleRow(r));
  }
  rows.clear();
  used = 0;
  return ran || lastError.empty() ? 0 : -1;
}

SingleVariantWaldTest::SingleVariantWaldTest() { modelName = "SingleWald"; }
SingleVariantWaldTest::~SingleVariantWaldTest() {
  if (fout) flush();
}
void SingleVariantWaldTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + "Test\tBeta\tSE\tPvalue\n");
}
int SingleVariantWaldTest::runBlock() {
  const size_t n = (size_t)used * (size_t)nCovariate;
  beta.assign(n, 0.0);
  se.assign(n, 0.0);
  pv.assign(n, 0.0);
  return rvt_wald_block(ctx, block.get(), used, ok.data(), beta.data(), se.data(), pv.data(), nullptr);
}
std::string SingleVariantWaldTest::formatSingleRow(const Row& r) {
  std::string out;
  const int k = r.column;
  const bool fitted = k >= 0 && ok[k] == 1;
  for (size_t i = 0; i < r.labels.size(); ++i) {  // columns 1 .. of X (the intercept is skipped)
    if (hideCovar && i > 0) continue;
    if (fitted) {  // (Result::updateValue; never cleared in between)
      const size_t o = (size_t)k * nCovariate + i;
      lastBeta = floatToString(beta[o]);
      lastSE = floatToString(se[o]);
      lastP = floatToString(pv[o]);
    }
    out += r.siteTab + r.labels[i] + "\t" + lastBeta + "\t" + lastSE + "\t" + lastP + "\n";
  }
  return out;
}

SingleVariantScoreTest::SingleVariantScoreTest() { modelName = "SingleScore"; }
SingleVariantScoreTest::~SingleVariantScoreTest() {
  if (fout) flush();
}
void SingleVariantScoreTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + "AF\tU\tV\tSTAT\tDIRECTION\tEFFECT\tSE\tPVALUE\n");
}
int SingleVariantScoreTest::runBlock() {
  const size_t n = (size_t)used;
  u.assign(n, 0.0);
  v.assign(n, 0.0);
  eff.assign(n, 0.0);
  se.assign(n, 0.0);
  pv.assign(n, 0.0);
  std::vector<double> beta0(nCovariate), covb(nCovariate);
  const int rc = rvt_score_block(ctx, block.get(), used, ok.data(), u.data(), v.data(), eff.data(), se.data(), pv.data());
  return rc ? rc : rvt_null_summary(ctx, beta0.data(), covb.data(), &sigma2);
}
std::string SingleVariantScoreTest::formatSingleRow(const Row& r) {
  const int k = r.column;
  std::string na = "NA";
  std::string U = na, V = na, STAT = na, DIR = na, EFF = na, SE = na, P = na;
  if (k >= 0 && ok[k]) {
    // rvt_score_block returns MetaScore's units: U_STAT = U / sigma2, V_STAT = SS / sigma2 (quantitative; the binary ones are
    // LogisticRegressionScoreTest's own)
    const bool bin = isBinaryOutcome();
    const double s2 = bin ? 1.0 : sigma2;
    const double uu = u[k] * s2, vv = bin ? v[k] : v[k] * s2 * s2;
    const double ss = bin ? v[k] : v[k] * s2;  // SS
    U = floatToString(uu);
    V = floatToString(vv);
    STAT = floatToString(bin ? uu * (1.0 / vv) * uu : uu * ((1.0 / ss) / s2) * uu);
    if (uu != 0.0) DIR = uu > 0 ? "+" : "-";
    if (vv > 0.0) {
      EFF = floatToString(bin ? uu / vv : eff[k]);
      SE = floatToString(bin ? 1.0 / std::sqrt(vv) : s2 / std::sqrt(vv));  // GetSEBeta (LinearRegressionScoreTest.cpp:365)
    }
    P = floatToString(pv[k]);
  }
  return r.siteTab + floatToString(r.af) + "\t" + U + "\t" + V + "\t" + STAT + "\t" + DIR + "\t" + EFF +
         "\t" + SE + "\t" + P + "\n";
}

// ---- FastMultipleTraitScoreTest (src/Model.h:4935-5125) ------------------------------------------------------------------------
FastMultipleTraitScoreTest::FastMultipleTraitScoreTest() : ColumnBlockTest("RVT_SINGLE_BLOCK") {
  modelName = "FastMultipleTraitScore";
}
FastMultipleTraitScoreTest::~FastMultipleTraitScoreTest() {
  if (fout) flush();
}
void FastMultipleTraitScoreTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + "U_STAT\tV_STAT\tPVALUE\n");
}
// FitNullModel's bookkeeping (regression/FastMultipleTraitLinearRegressionScoreTest.cpp:245-283): names to columns, "1" and
// "intercept" dropped; the arithmetic is rvt_mt_fit_null's
int FastMultipleTraitScoreTest::fitNull(GeneData* dc) {
  if (!dc->phenotypeMatrix || dc->nPheno < 1 || dc->formula.empty()) {
    lastError = "Multiple trait score test needs the phenotype matrix and the formulae";
    return -1;
  }
  auto find = [](const std::vector<std::string>& labels, const std::string& name) {
    for (size_t i = 0; i < labels.size(); ++i)
      if (labels[i] == name) return (int)i;
    return -1;
  };
  std::vector<int> pheno, ptr(1, 0), cov;
  for (const GeneData::Formula& f : dc->formula) {
    const int y = find(dc->phenotypeLabel, f.phenotype);
    if (y < 0 || y >= dc->nPheno) {
      lastError = "Multiple trait score test: unknown phenotype " + f.phenotype;
      return -1;
    }
    pheno.push_back(y);
    for (const std::string& name : f.covariate) {
      std::string low = name;
      for (char& ch : low) ch = (char)tolower((unsigned char)ch);
      if (name == "1" || low == "intercept") continue;
      const int z = find(dc->covariateLabel, name);
      if (z < 0 || z >= dc->ncov) {
        lastError = "Multiple trait score test: unknown covariate " + name;
        return -1;
      }
      cov.push_back(z);
    }
    ptr.push_back((int)cov.size());
  }
  cov.push_back(0);  // (never read: keeps the pointer valid for tests without covariates)
  if (rvt_mt_fit_null(ctx, dc->N, dc->nPheno, dc->phenotypeMatrix, dc->ncov, dc->covariate, (int)pheno.size(), pheno.data(),
                      ptr.data(), cov.data(), nullptr, nullptr, nullptr)) {
    lastError = rvt_last_error(ctx);
    return -1;
  }
  nTest = (int)pheno.size();
  haveNull = true;
  return 0;
}
int FastMultipleTraitScoreTest::fit(GeneData* dc) {
  fitOK = false;
  if (isBinaryOutcome()) {  // warnOnce (src/Model.h:4981-4983)
    lastError = "Multiple trait score test model does not support binary trait yet.";
    return -1;
  }
  if (dc->M != 1 || dc->N == 0) return -1;  // genotype.cols != 1
  if (sameSampleSize(*dc)) return -1;
  if (makeRoom(rows.size())) return -1;  // (one entry of `rows` per column in use)
  if (!ctx) ctx = GpuBroker::instance().context(&lastError);
  if (!ctx) return -1;
  if (!haveNull || dc->phenotypeUpdated || dc->covariateUpdated) {
    if (used > 0 && flush()) return -1;  // the columns so far belong to the previous null
    if (fitNull(dc)) return -1;
  }
  if (nSample < 0) {  // (N is fixed only once the block exists: a failed allocation is tried again by the next site)
    if (block.alloc(ctx, capacity, &lastError)) return -1;
    nSample = dc->N;
  }
  // the caller overwrites the genotype buffer for the next site: copy the column into the device block now.  Not
  // DeviceBlock::uploadColumn: rvt_block_upload_columns takes N from the score tests' null models, which this context
  // does not have (its null is rvt_mt_fit_null's)
  if (rvt_block_upload(ctx, block.get() + (size_t)used * (size_t)rvt_padded_ld(nSample), 1, dc->genotype)) {
    lastError = rvt_last_error(ctx);
    return -1;
  }
  rows.emplace_back();
  written.push_back(0);
  ++used;
  fitOK = true;
  return 0;
}
void FastMultipleTraitScoreTest::writeOutput(TextSink* fp, const SiteInfo& siteInfo) {
  fout = fp;
  if (!fitOK) return;  // a site whose fit() failed prints no row
  fitOK = false;
  rows.back() = siteInfo.valueTab();
  written.back() = 1;
  if (used >= capacity) flush();  // numResult == blockSize (src/Model.h:5033-5035)
}
int FastMultipleTraitScoreTest::flush() {
  if (!fout) return 0;
  if (used == 0) return 0;
  const size_t cells = (size_t)used * (size_t)nTest;
  u.assign(cells, NAN);
  v.assign(cells, NAN);
  pv.assign(cells, NAN);
  const bool ran = rvt_mt_score_block(ctx, block.get(), used, u.data(), v.data(), pv.data()) == 0;
  if (!ran) {
    lastError = rvt_last_error(ctx);
    std::fill(u.begin(), u.end(), NAN), std::fill(v.begin(), v.end(), NAN), std::fill(pv.begin(), pv.end(), NAN);
  }
  char num[32];
  auto join = [&](const std::vector<double>& m, int row, std::string* out) {  // formatValue (src/Model.h:5091-5100)
    for (int t = 0; t < nTest; ++t) {
      if (t) *out += ',';
      const double x = m[(size_t)row * nTest + t];
      if (std::isnan(x)) *out += "nan";
      else out->append(num, formatG(x, num));
    }
  };
  for (int k = 0; k < used; ++k) {
    if (!written[(size_t)k]) continue;  // main calls writeOutput after every fit(); a row never written is never printed
    std::string line = rows[(size_t)k];
    join(u, k, &line);
    line += '\t';
    join(v, k, &line);
    line += '\t';
    join(pv, k, &line);
    line += '\n';
    fout->write(line);
  }
  rows.clear();
  written.clear();
  used = 0;
  return ran ? 0 : -1;
}

// ---- SingleVariantFamilyScore / LRT / GrammarGamma (src/Model.h:525-805), related samples ------------------------------------
SingleVariantFamilyTest::SingleVariantFamilyTest(const char* name, const char* header_, const char* what_)
    : header(header_), what(what_) {
  modelName = name;
}
void SingleVariantFamilyTest::writeHeader(TextSink* fp, const SiteInfo& siteInfo) {
  fp->write(siteInfo.headerTab() + header + "\n");
}
rvt_ctx* SingleVariantFamilyTest::acquireContext(GeneData* dc) {
  if (isBinaryOutcome()) {  // warnOnce (src/Model.h:544-549, 640-645, 734-739)
    lastError = "Single variant " + what + " does not support binary outcomes. Results will be all NAs.";
    return nullptr;
  }
  if (!dc->hasKinship()) {  // as FamSkatTest
    lastError = "Single variant " + what + " cannot find kinship. Results will be all NAs.";
    return nullptr;
  }
  return GpuBroker::instance().contextWithFamNull(*dc, &lastError);
}
int SingleVariantFamilyTest::runBlock() {
  for (auto& v : col) v.assign((size_t)used, 0.0);
  return blockEntry();
}
std::string SingleVariantFamilyTest::formatSingleRow(const Row& r) {
  const int k = r.column;
  if (k >= 0 && ok[k] == 1)  // (Result::updateValue; never cleared in between)
    for (int q = 0; q < 4; ++q) last[q] = floatToString(col[q][k]);
  return r.siteTab + last[0] + "\t" + last[1] + "\t" + last[2] + "\t" + last[3] + "\n";
}

SingleVariantFamilyScore::SingleVariantFamilyScore()
    : SingleVariantFamilyTest("FamScore", "AF\tU.Stat\tV.Stat\tPvalue", "score test (related individual)") {}
SingleVariantFamilyScore::~SingleVariantFamilyScore() {
  if (fout) flush();
}
int SingleVariantFamilyScore::blockEntry() {  // (this entry returns U and V before AF, the first column printed)
  return rvt_score_block_fam(ctx, block.get(), used, 0, ok.data(), col[1].data(), col[2].data(), col[0].data(), col[3].data());
}

SingleVariantFamilyLRT::SingleVariantFamilyLRT()
    : SingleVariantFamilyTest("FamLRT", "AF\tNullLogLik\tAltLogLik\tPvalue", "likelihood ratio test (related individuals)") {}
SingleVariantFamilyLRT::~SingleVariantFamilyLRT() {
  if (fout) flush();
}
int SingleVariantFamilyLRT::blockEntry() {
  return rvt_lrt_block_fam(ctx, block.get(), used, ok.data(), col[0].data(), col[1].data(), col[2].data(), col[3].data());
}

SingleVariantFamilyGrammarGamma::SingleVariantFamilyGrammarGamma(bool afKinship_)
    : SingleVariantFamilyTest("FamGrammarGamma", "AF\tBeta\tBetaVar\tPvalue", "garmma-gamma test (related individuals)"),
      afKinship(afKinship_) {}
SingleVariantFamilyGrammarGamma::~SingleVariantFamilyGrammarGamma() {
  if (fout) flush();
}
rvt_ctx* SingleVariantFamilyGrammarGamma::acquireContext(GeneData* dc) {
  rvt_ctx* cx = SingleVariantFamilyTest::acquireContext(dc);
  if (!cx) return nullptr;
  if (!haveNull || nullKinship != dc->kinshipIdentity() || dc->phenotypeUpdated || dc->covariateUpdated) {
    rvt_grammar_null gn;
    haveNull = false;
    if (rvt_fit_grammar_null(cx, dc->N, 1 + dc->ncov, interceptAndCovariates(*dc).data(), dc->phenotype, &gn)) {
      lastError = rvt_last_error(cx);
      return nullptr;
    }
    haveNull = true;
    nullKinship = dc->kinshipIdentity();
  }
  return cx;
}
int SingleVariantFamilyGrammarGamma::blockEntry() {
  return rvt_grammar_block(ctx, block.get(), used, afKinship ? 1 : 0, ok.data(), col[0].data(), col[1].data(), col[2].data(),
                           col[3].data());
}

// ---- MetaCovTest ---------------------------------------------------------------------------------------------------------
MetaCovTest::MetaCovTest(int windowSize_) : windowSize(windowSize_) {
  modelName = "MetaCov";
  capacity = 4096;  // (columns; shrunk to the memory budget at the first fit(), when N is known)
  // columns of the device ring at the start; RVT_METACOV_BLOCK lowers it (tests exercise the mid-stream flush and the wrap with it)
  if (const char* e = getenv("RVT_METACOV_BLOCK")) capacity = std::max(2, std::min(65536, atoi(e)));
  if (const char* e = getenv("RVT_METACOV_MAX_COLUMNS")) maxColumns = std::max(capacity, atoi(e));
  formatThreads = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency() / 2));
  if (const char* e = getenv("RVT_METACOV_FORMAT_THREADS")) formatThreads = std::max(1, atoi(e));
}
MetaCovTest::~MetaCovTest() {
  if (fout) flush(true);
  if (ctx && bandReg) rvt_host_unregister(ctx, bandReg);  // (the ring is freed behind this, by its member's destructor)
}
int MetaCovTest::setParameter(const ModelParser& parser) {
  outputGwama = parser.hasTag("gwama");
  return 0;
}
int MetaCovTest::fit(GeneData* dc) {
  fitOK = false;
  if (dc->M != 1 || dc->N == 0) return -1;  // src/Model.cpp:851-858
  if (!dc->site) {
    lastError = "MetaCov needs the site's CHROM/POS";
    return -1;
  }
  if (nSample >= 0 && nSample != dc->N) {
    lastError = "Sample size changed at [ " + dc->site->get("CHROM") + ":" + dc->site->get("POS") + " ]";
    return -1;
  }
  useFamilyModel = dc->hasKinship();  // dc->hasKinship(): MetaCovFamQtl instead of MetaCovUnrelatedQtl
  ctx = useFamilyModel ? GpuBroker::instance().contextWithFamNull(*dc, &lastError)
                       : GpuBroker::instance().contextWithNull(*dc, isBinaryOutcome(), &lastError);
  if (!ctx) return -1;
  if (useFamilyModel && isBinaryOutcome() && (nSample < 0 || dc->phenotypeUpdated)) {
    // MetaCovFamBinary::FitNullModel (src/Model.cpp:598-640): alpha = log(nCase / nCtrl), b = obtainB(alpha)
    int64_t nCase, nCtrl;
    caseControlCounts(*dc, &nCase, &nCtrl);
    if (rvt_fam_binary_scale(ctx, nCase, nCtrl, nullptr, nullptr)) {
      lastError = rvt_last_error(ctx);
      return -1;
    }
  }
  if (nSample < 0) {
    nSample = dc->N;
    nCovariate = dc->ncov + 1;
    // the ring may grow to 96 GB of columns (RVT_METACOV_RING_GB; the int8 copy and the two 4-bit stores the engine keeps per
    // column counted in: 10 bytes per genotype): 19 000 columns at N = 500 000
    {
      double gb = 96.0;
      if (const char* e = getenv("RVT_METACOV_RING_GB")) gb = std::max(1.0, atof(e));
      const double cols = gb * 1e9 / (10.0 * (double)std::max<int64_t>(dc->N, 1));
      if (cols < (double)maxColumns) maxColumns = std::max(std::min(capacity, 1024), (int)cols);
      if (capacity > maxColumns) capacity = maxColumns;
    }
    if (block.alloc(ctx, capacity, &lastError)) return -1;
  }
  if ((int)sites.size() == capacity) {
    const int before = (int)sites.size();
    if (flush(false)) return -1;
    // One window holds more sites than the ring: enlarge it.  ALSO when the flush could emit less than three quarters of the
    // ring — a window of 1 000 markers in a ring of 1 024 would read 1 000 columns to write 24 rows; with a ring of at least
    // four windows every flush emits three quarters of what it reads and is long enough to hide its fixed cost (measured at
    // N = 500 000, windows of 200 / 1 000 / 3 000 markers: rings of 4 096 / 4 096 / 16 384 columns run 2.0 / 1.3 / 1.1 times
    // as fast as rings of two windows).
    const bool full = (int)sites.size() == capacity;
    if (full || (canGrow && 4 * (before - (int)sites.size()) < 3 * before)) {
      if (grow()) {
        if (full) return -1;
        canGrow = false;     // (a ring that cannot grow any further just stays as efficient as it was: do not retry every fill)
        lastError.clear();
      }
    }
  }
  // the caller overwrites the genotype buffer for the next site: copy the column into the device ring now — into the physical
  // column behind the tail; nothing in the ring ever moves (RingMemoryPool::allocate, base/RingMemoryPool.cpp:31-47)
  if (putSiteColumn(dc, (head + (int)sites.size()) % capacity)) return -1;
  sites.push_back(Site{dc->site->get("CHROM"), atoi(dc->site->get("POS").c_str())});
  fitOK = true;  // whether the site is monomorphic (and therefore skipped) is decided on the device at flush time
  return 0;
}
void MetaCovTest::writeHeader(TextSink* fp, const SiteInfo&) {
  fp->write("CHROM\tSTART_POS\tEND_POS\tNUM_MARKER\tMARKER_POS\tCOV\n");
}
void MetaCovTest::writeOutput(TextSink* fp, const SiteInfo&) { fout = fp; }
void MetaCovTest::writeFootnote(TextSink* fp) {
  fout = fp;
  flush(true);
}

// Double the device ring (a window can hold more sites than the current block): the one occasion on which columns are copied —
// the old ring's two runs, head first, to the front of the new one.
int MetaCovTest::grow() {
  const int want = std::min(maxColumns, capacity * 2);
  if (want <= capacity) {
    lastError = "MetaCov: one window holds more sites than RVT_METACOV_MAX_COLUMNS allows";
    return -1;
  }
  if (columnsReady()) return -1;  // (the columns are copied as the device calls will read them)
  DeviceBlock bigger;
  const int V = (int)sites.size(), first = std::min(V, capacity - head);
  if (bigger.alloc(ctx, want, &lastError)) return -1;
  if (rvt_block_copy_columns(ctx, bigger.get(), 0, block.get(), head, first) ||
      (V > first && rvt_block_copy_columns(ctx, bigger.get(), first, block.get(), 0, V - first))) {
    lastError = rvt_last_error(ctx);
    return -1;
  }
  block = std::move(bigger);  // frees the old ring
  capacity = want;
  head = 0;
  return 0;
}

// Emit the rows of every head whose window is complete (all of them when `final`) and drop those heads: the ring's head index
// advances, no column moves (RingMemoryPool::deallocate, base/RingMemoryPool.cpp:49-63).
int MetaCovTest::flush(bool final) {
  const int V = (int)sites.size();
  if (V == 0 || !fout) return 0;
  const int d = nCovariate;
  auto outOfWindow = [&](int h, int j) {  // getWindowSize(queue, loci) > windowSize, src/Model.h:3974-3990
    return sites[j].chrom != sites[h].chrom || std::abs(sites[j].pos - sites[h].pos) > windowSize;
  };
  int H = 0;  // heads [0, H) are complete
  for (; H < V; ++H) {
    bool complete = final;
    for (int j = H + 1; j < V && !complete; ++j) complete = outOfWindow(H, j);
    if (!complete) break;
  }
  if (H == 0) return 0;  // nothing can be written yet: the caller enlarges the ring
  if (columnsReady()) return -1;
  // whole row panels of the band kernel (256 heads): a panel of 24 heads costs the tiles of a full one; the rest waits in the
  // ring — nothing moves, so keeping them costs nothing
  if (!final && H > 256) H -= H % 256;
  const float scale = (float)(1.0 / (double)nSample);
  std::vector<double> zz((size_t)d * d);
  // last[h] = the last site printed in head h's row (the scan of printCovariance stops at the first site out of the window)
  std::vector<int> last((size_t)H);
  for (int h = 0; h < H; ++h) {
    int j = h;
    while (j + 1 < V && !outOfWindow(h, j + 1)) ++j;
    last[(size_t)h] = j;
  }
  // chunks of heads: one device call each — the band of the chunk's heads against everything up to the end of their windows,
  // read from the ring where it lies (the call addresses the columns modulo the capacity)
  const int Hc = 4096;
  std::vector<double> xz;
  std::vector<int> poly;
  for (int h0 = 0; h0 < H; h0 += Hc) {
    const int h1 = std::min(H, h0 + Hc), nh = h1 - h0;
    int halo = 0, jmax = h1 - 1;
    for (int h = h0; h < h1; ++h) {
      halo = std::max(halo, last[(size_t)h] - h);
      jmax = std::max(jmax, last[(size_t)h]);
    }
    const int W = jmax - h0 + 1;
    const size_t need = (size_t)nh * ((size_t)halo + 1);
    if (bandBuf.size() < need) {
      // the band lands by DMA in a page-locked buffer (a pageable target went through the runtime's staging copies: a third of
      // the device-side time of a flush)
      if (bandReg) rvt_host_unregister(ctx, bandReg);
      bandReg = nullptr;
      bandBuf.assign(need + need / 4, 0.0f);
      if (rvt_host_register(ctx, bandBuf.data(), sizeof(float) * bandBuf.size()) == 0) bandReg = bandBuf.data();
    }
    xz.assign((size_t)W * d, 0.0);
    poly.assign((size_t)W, 0);
    const int col0 = (head + h0) % capacity;
    if (useFamilyModel ? rvt_cov_band_fam(ctx, block.get(), capacity, col0, nh, W, halo, scale, bandBuf.data(), xz.data(), zz.data(), poly.data())
                       : rvt_cov_band(ctx, block.get(), capacity, col0, nh, W, halo, scale, bandBuf.data(), xz.data(), zz.data(), poly.data())) {
      lastError = rvt_last_error(ctx);
      return -1;
    }
    // the rows of the chunk as text: a row of a 1 000-marker window is 1 000 "%g" conversions (~0.2 ms on one core, more than
    // the device spends on it by two orders of magnitude), and rows are independent — formatted by a few threads, written in
    // order by this one
    std::vector<std::string> rowText((size_t)nh);
    auto formatRow = [&](int h) {
      if (!poly[(size_t)(h - h0)]) return;  // monomorphic sites never entered the reference's queue (src/Model.cpp:879-884)
      const float* row = bandBuf.data() + (size_t)(h - h0) * ((size_t)halo + 1);
      std::string positions, values;
      int lastPrinted = h, num = 0;
      for (int j = h; j <= last[(size_t)h]; ++j) {
        if (!poly[(size_t)(j - h0)]) continue;
        if (num) {
          positions += ',';
          values += ',';
        }
        positions += std::to_string(sites[j].pos);
        char num_buf[40];
        values.append(num_buf, formatG((double)row[j - h], num_buf));  // (the device applied the float cast and the float 1/N,
                                                                      //  src/Model.cpp:975-984)
        lastPrinted = j;
        ++num;
      }
      if (outputGwama || isBinaryOutcome()) {  // src/Model.cpp:992-1000
        const double* xzHead = xz.data() + (size_t)(h - h0) * d;
        values += ':';
        for (int k = 0; k < d; ++k) {
          if (k) values += ',';
          values += formatG((double)((float)xzHead[k] * scale));
        }
        values += ':';
        for (int a = 0; a < d; ++a)
          for (int b = 0; b <= a; ++b) {
            if (a || b) values += ',';
            values += floatToString(zz[(size_t)a * d + b] * (double)scale);
          }
      }
      rowText[(size_t)(h - h0)] = sites[h].chrom + "\t" + std::to_string(sites[h].pos) + "\t" + std::to_string(sites[lastPrinted].pos) +
                                  "\t" + std::to_string(num) + "\t" + positions + "\t" + values + "\n";
    };
    {
      const size_t work = (size_t)nh * ((size_t)halo + 1);
      int T = (int)std::min<size_t>(formatThreads, work / 20000 + 1);  // (a thread is worth its start from ~20 000 values on)
      if (T <= 1) {
        for (int h = h0; h < h1; ++h) formatRow(h);
      } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; ++t)
          pool.emplace_back([&, t] {
            for (int h = h0 + t; h < h1; h += T) formatRow(h);  // (interleaved: rows near the end of the ring are shorter)
          });
        for (auto& th : pool) th.join();
      }
    }
    for (int h = h0; h < h1; ++h)
      if (!rowText[(size_t)(h - h0)].empty()) fout->write(rowText[(size_t)(h - h0)]);
  }
  head = (head + H) % capacity;
  sites.erase(sites.begin(), sites.begin() + H);
  return 0;
}

// ---- the dominant / recessive meta models (src/Model.h:3880-3902, 4098-4124) -------------------------------------------------------
namespace {
// why a coded model cannot take this site (empty: it can)
std::string codedRefusal(const GeneData& dc, const std::string& modelName) {
  // the family score file's AF comes from the additive genotype (src/Model.h:3256-3258), which the recoded block does not hold
  if (dc.hasKinship()) return modelName + ": related samples (a kinship) are not supported by the dominant / recessive models";
  if (!dc.rawGenotype) return modelName + " needs the genotypes before imputation (GeneData::rawGenotype)";
  return "";
}
// the recoder's two device operations on a block
int putRaw(ColumnRecoder& r, DeviceBlock& block, const GeneData& dc, int c, int coding, std::string* err) {
  return r.put(c, [&](int col) { return block.uploadColumn(col, dc.rawGenotype, err); },
               [&](int start, int n) { return block.recodeColumns(start, n, coding, err); });
}
int recodePending(ColumnRecoder& r, DeviceBlock& block, int coding, std::string* err) {
  return r.ready([&](int start, int n) { return block.recodeColumns(start, n, coding, err); });
}
}  // namespace

MetaCodedScoreTest::MetaCodedScoreTest(int coding_, const char* name) : coding(coding_) { modelName = name; }
MetaCodedScoreTest::~MetaCodedScoreTest() {
  if (fout) flush();
}
int MetaCodedScoreTest::fit(GeneData* dc) {
  lastError = codedRefusal(*dc, modelName);
  if (!lastError.empty()) {  // the row keeps its counters and prints NA; no null model is fitted for it
    beginRow(*dc);
    return -1;
  }
  return MetaScoreTest::fit(dc);
}
int MetaCodedScoreTest::putSiteColumn(GeneData* dc, int c) { return putRaw(recoder, block, *dc, c, coding, &lastError); }
int MetaCodedScoreTest::columnsReady() { return recodePending(recoder, block, coding, &lastError); }

MetaCodedCovTest::MetaCodedCovTest(int windowSize, int coding_, const char* name) : MetaCovTest(windowSize), coding(coding_) {
  modelName = name;
}
MetaCodedCovTest::~MetaCodedCovTest() {
  if (fout) flush(true);
}
int MetaCodedCovTest::fit(GeneData* dc) {
  lastError = codedRefusal(*dc, modelName);
  return lastError.empty() ? MetaCovTest::fit(dc) : -1;
}
int MetaCodedCovTest::putSiteColumn(GeneData* dc, int c) { return putRaw(recoder, block, *dc, c, coding, &lastError); }
int MetaCodedCovTest::columnsReady() { return recodePending(recoder, block, coding, &lastError); }

// ---- ModelManager (src/ModelManager.cpp:26-44 tokeniser, :46-271 switch) --------------------------------------------------------
ModelManager::~ModelManager() {
  GpuBroker::instance().flush();  // rows still pending refer to the models
  for (auto* m : model) delete m;
}

int ModelManager::create(const std::string& type, const std::string& modelList) {
  if (modelList.empty()) return 0;
  std::string modelType = lower(type);
  // split on ',' outside []
  std::vector<std::string> argModelName;
  std::string s;
  int depth = 0;
  for (char c : modelList) {
    if (c == '[') depth++;
    if (c == ']') depth--;
    if (c == ',' && depth == 0) {
      argModelName.push_back(s);
      s.clear();
    } else
      s.push_back(c);
  }
  argModelName.push_back(s);
  for (auto& a : argModelName) {
    ModelParser parser;
    if (parser.parse(a)) {
      lastError = "Please use this format: model(model_param1=v1)";
      return -1;
    }
    const std::string modelName = parser.getName();
    int nPerm;
    double alpha;
    if (modelType == "burden") {
      if (modelName == "cmc")
        model.push_back(new CMCTest);
      else if (modelName == "zeggini")
        model.push_back(new ZegginiTest);
      else if (modelName == "famcmc")  // src/ModelManager.cpp:133-136
        model.push_back(new FamBurdenTest(false));
      else if (modelName == "famzeggini")
        model.push_back(new FamBurdenTest(true));
      else if (modelName == "cmcwald")  // src/ModelManager.cpp:99-142: the four analytic tests take no parameters
        model.push_back(new CMCWaldTest());
      else if (modelName == "zegginiwald")
        model.push_back(new ZegginiWaldTest());
      else if (modelName == "fp")
        model.push_back(new FpTest());
      else if (modelName == "exactcmc")
        model.push_back(new CMCFisherExactTest());
      else if (modelName == "rarecover") {  // src/ModelManager.cpp:115-121
        parser.assign("nPerm", &nPerm, 10000).assign("alpha", &alpha, 0.05);
        model.push_back(new RareCoverTest(nPerm, alpha));
      } else if (modelName == "mb") {  // src/ModelManager.cpp:104-110
        parser.assign("nPerm", &nPerm, 10000).assign("alpha", &alpha, 0.05);
        model.push_back(new MadsonBrowningTest(nPerm, alpha));
      } else {
        lastError = "Unknown model name: " + modelName + " .";
        return -1;
      }
    } else if (modelType == "kernel") {
      if (modelName == "skat") {
        double beta1, beta2;
        parser.assign("nPerm", &nPerm, 10000).assign("alpha", &alpha, 0.05).assign("beta1", &beta1, 1.0).assign(
            "beta2", &beta2, 25.0);
        model.push_back(new SkatTest(nPerm, alpha, beta1, beta2));
      } else if (modelName == "skato") {
        double beta1, beta2;
        parser.assign("beta1", &beta1, 1.0).assign("beta2", &beta2, 25.0);
        model.push_back(new SkatOTest(beta1, beta2));
      } else if (modelName == "kbac") {
        parser.assign("nPerm", &nPerm, 10000).assign("alpha", &alpha, 0.05);
        model.push_back(new KbacTest(nPerm, alpha));
      } else if (modelName == "famskat") {
        double beta1, beta2;
        parser.assign("beta1", &beta1, 1.0).assign("beta2", &beta2, 25.0);  // src/ModelManager.cpp:188-193
        model.push_back(new FamSkatTest(beta1, beta2));
      } else {
        lastError = "Unknown model name: " + modelName + " .";
        return -1;
      }
    } else if (modelType == "vt") {
      if (modelName == "analytic")  // src/ModelManager.cpp:158-161
        model.push_back(new AnalyticVTTest(false));
      else if (modelName == "famanalytic")
        model.push_back(new AnalyticVTTest(true));
      else if (modelName == "price") {  // src/ModelManager.cpp vt switch: nPerm = 10000, alpha = 0.05
        parser.assign("nPerm", &nPerm, 10000).assign("alpha", &alpha, 0.05);
        model.push_back(new VariableThresholdPrice(nPerm, alpha));
      } else {
        lastError = "Unknown model name: " + modelName + " .";
        return -1;
      }
    } else if (modelType == "meta") {
      if (modelName == "score") {  // src/ModelManager.cpp:209-210
        model.push_back(new MetaScoreTest());
      } else if (modelName == "cov") {
        int windowSize;
        parser.assign("windowSize", &windowSize, 1000000);  // src/ModelManager.cpp:227-233
        model.push_back(new MetaCovTest(windowSize));
      } else if (modelName == "dominant" || modelName == "recessive") {  // src/ModelManager.cpp:211-226: a score and a cov model
        int windowSize;
        parser.assign("windowSize", &windowSize, 1000000);
        if (modelName == "dominant") {
          model.push_back(new MetaDominantTest());
          model.back()->setParameter(parser);
          model.push_back(new MetaDominantCovTest(windowSize));
        } else {
          model.push_back(new MetaRecessiveTest());
          model.back()->setParameter(parser);
          model.push_back(new MetaRecessiveCovTest(windowSize));
        }
      } else {
        lastError = "Unknown model name: " + modelName + " .";
        return -1;
      }
    } else if (modelType == "single") {
      // src/ModelManager.cpp:54-98 (exact, dominantexact, firth and mtscore — the multiple-trait test that drops rows per
      // missingness group — are not provided)
      if (modelName == "fastmtscore")
        model.push_back(new FastMultipleTraitScoreTest());
      else if (modelName == "wald")
        model.push_back(new SingleVariantWaldTest());
      else if (modelName == "score")
        model.push_back(new SingleVariantScoreTest());
      else if (modelName == "famscore")
        model.push_back(new SingleVariantFamilyScore());
      else if (modelName == "famlrt")
        model.push_back(new SingleVariantFamilyLRT());
      else if (modelName == "famgrammargamma") {  // src/ModelManager.cpp:68-84
        const char* v = parser.value("af");
        const std::string afMethod = v ? v : "mean";
        if (afMethod == "kinship")
          model.push_back(new SingleVariantFamilyGrammarGamma(true));
        else if (afMethod == "mean")
          model.push_back(new SingleVariantFamilyGrammarGamma(false));
        else {
          lastError = "FamGrammarGamma cannot recoginized specified kinship calculation method [ " + afMethod + " ], exit...";
          return -1;
        }
      } else {
        lastError = "Unknown model name: " + modelName + " .";
        return -1;
      }
    } else {
      lastError = "Unrecognized model type: " + type;
      return -1;
    }
    model.back()->setParameter(parser);  // src/ModelManager.cpp:273-275
  }
  return 0;
}

void ModelManager::setBinaryOutcome() {
  for (auto* m : model) m->setBinaryOutcome();
}
void ModelManager::setQuantitativeOutcome() {
  for (auto* m : model) m->setQuantitativeOutcome();
}
std::vector<std::string> ModelManager::outputNames(const std::string& prefix) const {
  std::vector<std::string> v;
  for (auto* m : model) v.push_back(prefix + "." + m->getModelName() + ".assoc");
  return v;
}

}  // namespace rvt_host
