// rvtests_amd — host side (C++), mirror of the reference's plugin surface for the hot path.
//
// Same class names, constructor arguments, method names and output formats as the reference, so that these
// classes can be dropped into src/ModelManager.cpp in place of the CPU ones:
//   ModelFitter   src/ModelFitter.h:17-75     fit / writeHeader / writeOutput / writeFootnote / reset / setParameter
//   ModelParser   src/ModelParser.{h,cpp}     "name[k=v:k2=v2]", case-folded, ':' or ',' separated
//   ModelManager  src/ModelManager.cpp:26-44,99-103,168-198,273-297   create(type, "a[..],b")
//   SkatTest      src/Model.h:2612-2772       "Q\tPvalue"            %g
//   SkatOTest     src/Model.h:2774-2889       "Q\trho\tPvalue"       %g
//   CMCTest       src/Model.h:807-907         "NonRefSite\tPvalue"   Result / floatToString (6 significant digits)
//   ZegginiTest   src/Model.h:1170-1242       "Pvalue"
// Every fit() goes through the C ABI of include/rvtests_amd.h; nothing here computes statistics on the CPU.
//
// Inside the real rvtests tree the adapters read the reference's own `DataConsolidator`, `Matrix`, `FileWriter`
// and `Result`.  To keep this repository self-contained (and testable without Eigen) the few members the hot
// path touches are abstracted behind `GeneData` / `TextSink` below; INTEGRATION.md lists the one-line mapping
// of each onto the reference types.
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/rvtests_amd.h"

namespace rvt_host {

struct SiteInfo;

// ---- what fit() may read: DataConsolidator getters (src/DataConsolidator.h:126-137,223-224) -------------
// What MetaScoreTest reads from the caller's GenotypeCounter after dc->countRawGenotype(0, &counter)
// (src/Model.h:3211-3230; libsrc/GenotypeCounter.h): the counting and the exact HWE test stay with the caller
// (DataConsolidator / GenotypeCounter are not on the accelerated path), the adapter only prints them.
struct SiteCounts {
  double af = -1.0;       // getAF(); < 0 prints NA
  double ac = 0.0;        // getAC()
  double callRate = 0.0;  // getCallRate()
  double hwe = 0.0;       // getHWE()
  int nHomRef = 0, nHet = 0, nHomAlt = 0;
};

struct GeneData {
  int64_t N = 0;
  int M = 0;
  const double* genotype = nullptr;   // dc->getGenotype(): imputed, unflipped, N x M column-major
  // dc->getOriginalGenotype() (src/DataConsolidator.h:133): the calls BEFORE imputation, N x M column-major, negative =
  // missing.  Read by the dominant / recessive meta models only (DataConsolidator::codeGenotypeFor*Model read it).
  const double* rawGenotype = nullptr;
  // Optional, INSTEAD of `genotype` for the gene tests (SKAT / SKAT-O / CMC / Zeggini): the gene as the extractor of a PLINK
  // file holds it BEFORE consolidation — M rows of ceil(N / 4) bytes, SNP-major 2-bit codes (libVcf/PlinkInputFile.cpp:24-47;
  // 00 -> 0, 10 -> 1, 11 -> 2, 01 -> missing).  The device then does what DataConsolidator::consolidate does (allele
  // frequencies, mean imputation: rvt_submit_gene_bed); markerFrequency is not needed.  1/32 of the bytes of `genotype`.
  const unsigned char* bed = nullptr;
  const double* phenotype = nullptr;  // dc->getPhenotype(): N
  const double* covariate = nullptr;  // dc->getCovariate(): N x ncov column-major, NO intercept
  int ncov = 0;
  std::vector<double> markerFrequency;  // dc->getMarkerFrequency(col) for col < M
  bool phenotypeUpdated = false, covariateUpdated = false;  // dc->isPhenotypeUpdated() / isCovariateUpdated()
  int64_t serial = 0;                 // increases with every dc.consolidate() (new gene)
  const SiteInfo* site = nullptr;     // dc->getResult(): CHROM / POS of the current site (single-variant models)
  // the genotype column's label (genotype.GetColumnLabel(0), the "Test" column of SingleWald); empty: CHROM:POS of `site`
  std::string genotypeLabel;
  std::string columnLabel() const;
  // dc->hasKinship(), getKinshipUForAuto() / getKinshipSForAuto() (src/DataConsolidator.h:236-258): EigenMatrix holds
  // Eigen::MatrixXf, i.e. float, column-major N x N and N x 1
  const float* kinshipU = nullptr;
  const float* kinshipS = nullptr;
  // The same decomposition family by family, INSTEAD of the two dense matrices, for a pedigree kinship of separate families
  // of at most 64 samples (the layout: rvt_set_kinship_families in rvtests_amd.h).  The reference has no such form — its
  // DataConsolidator only ever holds the N x N matrices — so only a caller built on this library fills it.
  struct KinshipFamilies {
    int64_t nFam = 0;
    const int64_t* famPtr = nullptr;   // nFam + 1
    const int32_t* members = nullptr;  // N
    const float* blocks = nullptr;     // every family's k x k block of eigenvectors, column-major, concatenated
    const float* S = nullptr;          // N eigenvalues, family by family
  } kinshipFamilies;
  bool hasDenseKinship() const { return kinshipU && kinshipS; }
  bool hasFamilyKinship() const {
    return kinshipFamilies.nFam > 0 && kinshipFamilies.famPtr && kinshipFamilies.members && kinshipFamilies.blocks && kinshipFamilies.S;
  }
  bool hasKinship() const { return hasDenseKinship() || hasFamilyKinship(); }  // dc->hasKinship()
  // what tells one installed decomposition from the next (the broker installs once per decomposition, by pointer identity)
  const float* kinshipIdentity() const { return hasDenseKinship() ? kinshipU : hasFamilyKinship() ? kinshipFamilies.blocks : nullptr; }
  // MetaScoreTest: raw-genotype counters of the current site — all samples, cases, controls (binary traits only)
  SiteCounts counter, caseCounter, ctrlCounter;
  // FastMultipleTraitScoreTest (`--multiplePheno`): dc->getPhenotype() as the N x nPheno matrix it then is (column-major,
  // NaN = missing) with its column labels, the labels of dc->getCovariate()'s columns (`covariate` above, NaN = missing) and
  // dc->getFormula(): per test the phenotype's name and the covariates' names ("1" / "intercept" are dropped by the model)
  const double* phenotypeMatrix = nullptr;
  int nPheno = 0;
  std::vector<std::string> phenotypeLabel, covariateLabel;
  struct Formula {
    std::string phenotype;
    std::vector<std::string> covariate;
  };
  std::vector<Formula> formula;
};

// ---- FileWriter stand-in (base/IO.h FileWriter::write / printf) -------------------------------------------
struct TextSink {
  std::string text;
  virtual ~TextSink() {}
  virtual void write(const std::string& s) { text += s; }  // in_tree/GpuModelFitter.h forwards to FileWriter::write
  void write(const char* s) { write(std::string(s)); }
};

// site columns the caller passes to writeHeader/writeOutput (Result::writeHeaderTab / writeValueTab)
struct SiteInfo {
  std::vector<std::pair<std::string, std::string>> kv;
  // set by the in-tree binding, which takes both lines from the reference's Result (joinValue): used verbatim
  bool verbatim = false;
  std::string headerLine, valueLine;
  std::string headerTab() const {
    if (verbatim) return headerLine;
    std::string s;
    for (auto& p : kv) s += p.first + "\t";
    return s;
  }
  std::string valueTab() const {
    if (verbatim) return valueLine;
    std::string s;
    for (auto& p : kv) s += p.second + "\t";
    return s;
  }
  std::string get(const std::string& key) const {  // Result::operator[]
    for (auto& p : kv)
      if (p.first == key) return p.second;
    return "";
  }
};

std::string floatToString(double v);  // base/TypeConversion.h:100-105 (6 significant digits)
std::string formatG(double v);        // printf("%g")
size_t formatG(double v, char* out);  // the same characters into out (at least 32 bytes, not terminated); returns their number

// ---- ModelParser --------------------------------------------------------------------------------------------
class ModelParser {
 public:
  int parse(const std::string& s);
  const std::string& getName() const { return name; }
  bool hasTag(const std::string& tag) const;
  const char* value(const std::string& tag) const;
  size_t size() const { return param.size(); }
  const ModelParser& assign(const std::string& tag, double* v, double def) const;
  const ModelParser& assign(const std::string& tag, int* v, int def) const;
  const ModelParser& assign(const std::string& tag, bool* v, bool def) const;
  void set(const std::string& tag, const std::string& value);  // (in-tree binding: copy a tag of the reference's parser)

 private:
  std::string name;
  std::map<std::string, std::string> param;
};

class DeferredGeneTest;
class BurdenMoreTest;

// ---- a device block (rvt_block_alloc) and the context it lives on ------------------------------------------------------------
// Move-only, empty after a move.  The destructor frees the block it holds and does nothing else: a block must go out of scope,
// or its owner be cleared, before its context is destroyed.  alloc / upload / uploadColumn return 0, or -1 with the context's
// error text in *err.
class DeviceBlock {
 public:
  DeviceBlock() = default;
  DeviceBlock(DeviceBlock&& o) noexcept : ctx(o.ctx), ptr(o.release()) {}
  DeviceBlock& operator=(DeviceBlock&& o) noexcept {
    if (this != &o) {
      free();
      ctx = o.ctx;
      ptr = o.release();
    }
    return *this;
  }
  ~DeviceBlock() { free(); }
  int alloc(rvt_ctx* cx, int columns, std::string* err) {  // (whatever was held is freed first)
    free();
    ctx = cx;
    return done(rvt_block_alloc(ctx, columns, &ptr), err);
  }
  // the first M columns, complete on return
  int upload(int M, const double* host, std::string* err) { return done(rvt_block_upload(ctx, ptr, M, host), err); }
  // one column, through the engine's column queue
  int uploadColumn(int col, const double* host, std::string* err) { return done(rvt_block_upload_columns(ctx, ptr, col, 1, host), err); }
  // columns [col, col + n) recoded in place (RVT_CODING_*), queued uploads of them included
  int recodeColumns(int col, int n, int coding, std::string* err) {
    return done(rvt_block_recode(ctx, ptr, col, ptr, col, n, coding, nullptr), err);
  }
  double* get() const { return ptr; }
  double* release() {  // for a caller that frees the block itself, later
    double* p = ptr;
    ptr = nullptr;
    return p;
  }

 private:
  int done(int rc, std::string* err) const {
    if (rc) *err = rvt_last_error(ctx);
    return rc ? -1 : 0;
  }
  void free() {
    if (ptr) rvt_block_free(ctx, ptr);
    ptr = nullptr;
  }
  rvt_ctx* ctx = nullptr;
  double* ptr = nullptr;
};

// What the dominant / recessive meta models share: a site's RAW column goes into the block by rvt_block_upload_columns — the
// engine's column queue packs it, its negative missing code included, and keeps batching — and is remembered as pending; a
// pending run — consecutive physical columns — is recoded in place by ONE rvt_block_recode before any device call reads the
// block, before a column that does not continue it (the ring wrapping) and at the latest when it holds kMaxPending columns.
// The decisions are made here without a device: `upload(col)` and `recode(start, n)` are the caller's two device operations
// (0 = done), which a stand-alone program replaces by its own.
class ColumnRecoder {
 public:
  static constexpr int kMaxPending = 32;  // = the engine's column queue: one recoding per queue flush
  // the site's raw column into block column c
  template <class Upload, class Recode>
  int put(int c, Upload upload, Recode recode) {
    if (n > 0 && c != start + n && ready(recode)) return -1;  // (the ring wrapped)
    if (upload(c)) return -1;
    if (n == 0) start = c;
    ++n;
    return n >= kMaxPending ? ready(recode) : 0;
  }
  // recode what is pending
  template <class Recode>
  int ready(Recode recode) {
    if (n == 0) return 0;
    const int s = start, k = n;
    n = 0;  // (also after a failure: the columns are not recoded twice)
    return recode(s, k) ? -1 : 0;
  }
  int pending() const { return n; }

 private:
  int start = 0, n = 0;
};

// ---- the engine shared by all GPU-backed models of one run ---------------------------------------------------
// One device group per process (rvt_group_*: RVT_DEVICES=0,1,... lists the GPUs, default device 0): the gene tests'
// stream is dealt to the members and collected in submission order; the models that drive a context themselves
// (MetaCov, MetaScore, the related-sample tests) use member 0.  The null model is installed once on every member (and
// again when the caller flags an updated phenotype/covariate); each new gene is submitted ONCE with the union of the
// registered tests, whichever model's fit() sees it first.
class GpuBroker {
 public:
  static GpuBroker& instance();
  int ensureContext(int device);
  void registerTests(uint32_t mask, const rvt_params& p);
  // Deferred, batched execution.  fit() only SUBMITS the gene (rvt_submit_gene copies the caller's buffer, which
  // the next consolidate() overwrites); writeOutput() only records (sink, site columns); rows are written in call
  // order by flush(), which runs one rvt_collect over everything pending.  flush() is triggered when `window` genes
  // are pending and a new one arrives, by writeFootnote() and by ~ModelManager — the reference's own MetaCovTest
  // defers its rows the same way (src/Model.cpp:828-834), and `main` ignores fit()'s return value
  // (src/Main.cpp:1251).  Default window: 64 genes or 64 GB of genotype blocks, whichever fills first (RVT_ADAPTER_BATCH /
  // RVT_ADAPTER_BATCH_GB override; window = 1 keeps at most one gene in flight).
  void setBatchWindow(int k) { window = k < 1 ? 1 : k; }
  void setBatchBytes(size_t b) { windowBytes = b; }
  // `--dosage TAG` (src/Main.cpp FLAG_dosageTag): the blocks fit() receives hold dosages, not hard calls; `decimals` = the
  // number of decimals the tag is printed with (3 for an imputation server's DS; -1 = unknown / not decimal text, e.g.
  // BGEN): states the lattice 10^decimals to the engine (rvt_group_set_content).  Call before the first fit(); RVT_DOSAGE
  // (1 / the number of decimals as "d3") does the same from the environment.  Never affects the records.
  void setDosage(int decimals) {
    dosage = true;
    dosageDecimals = decimals;
  }
  int submit(const GeneData& gd, bool binary, std::string* err);
  void enqueue(DeferredGeneTest* m, TextSink* fp, const std::string& siteTab, int64_t serial);
  int flush();       // wait for everything pending and write all rows
  int drainReady();  // take the finished prefix without waiting (rvt_collect_ready) and write the rows it completes
  void shutdown();
  // context + null model for models that drive the C ABI themselves (MetaCovTest)
  rvt_ctx* contextWithNull(const GeneData& gd, bool binary, std::string* err);
  // the bare context, for a model that installs a null of its own kind (FastMultipleTraitScoreTest: rvt_mt_fit_null)
  rvt_ctx* context(std::string* err);
  // context + kinship + FastLMM null for FamSkatTest (refitted when the caller flags new phenotype / covariates)
  rvt_ctx* contextWithFamNull(const GeneData& gd, std::string* err);
  // The synchronous gene tests: upload the gene's N x M block to `cx`, run one rvt_* entry on it (`call`: one gene, its block
  // pointer and its M), free the block.  -1 with *err set when the upload or the call fails, and when `cx` is null (*err is then
  // what the context* call above left).
  typedef std::function<int(const double* const* block, const int* M)> GeneCall;
  static int withGene(rvt_ctx* cx, const GeneData& gd, std::string* err, const GeneCall& call);
  // the related-sample gene tests (FamSkat, FamCMC, FamZeggini) share one rotation per gene: the first model whose
  // fit() sees a gene runs the union of the registered tests, the others read the cached record
  void registerFamTests(uint32_t mask) { famTests |= mask; }
  const rvt_gene_result* famResultFor(const GeneData& gd, std::string* err);
  // the analytic burden tests (CMCWald, ZegginiWald, Fp, CMCFisherExact) share one device copy of each gene and one
  // rvt_burden_blocks call per window of genes, with the union of the registered tests: the first model whose fit() sees a gene
  // uploads it, writeOutput() only records (model, sink, site columns), and the rows are written in call order when the window
  // (the one of the gene tests above: genes or bytes) is full, when a new null model is about to be installed, at writeFootnote()
  // and at flush().  A gene that could not be submitted, or whose call failed, prints NA rows.
  void registerBurdenMore(uint32_t mask) { moreTests |= mask; }
  int submitBurdenMore(const GeneData& gd, bool binary, std::string* err);
  void enqueueBurdenMore(BurdenMoreTest* m, TextSink* fp, const std::string& siteTab, int64_t serial);
  int flushBurdenMore();
  // null model: fitted on the device (rvt_fit_null) unless the caller installs its own routine (e.g. the
  // reference's LinearRegression / LogisticRegression inside the rvtests tree); see INTEGRATION.md
  typedef int (*NullFitter)(bool binary, int64_t N, int d, const double* X, const double* y, double* res, double* v,
                            double* sigma2);
  void setNullFitter(NullFitter f) { fitter = f; }
  const rvt_fam_null& familyNull() const { return famNull; }  // estimates of the FastLMM null last fitted

 private:
  rvt_group* grp = nullptr;
  rvt_ctx* ctx = nullptr;  // member 0
  bool dosage = false;
  int dosageDecimals = -1;
  uint32_t tests = 0;
  rvt_params params{1.0, 25.0, 1.0, 25.0, 0, 0.05};
  bool haveNull = false;
  rvt_fam_null famNull{};
  int64_t curSerial = -1;
  bool curOk = false;
  int window = 64;                              // genes in flight (RVT_ADAPTER_BATCH)
  size_t windowBytes = (size_t)64 << 30;        // ... and the bytes of their device blocks (RVT_ADAPTER_BATCH_GB)
  size_t pendingBytes = 0;
  struct Row {
    DeferredGeneTest* model;
    TextSink* fp;
    std::string siteTab;
    int64_t serial;
  };
  std::vector<Row> rows;               // in writeOutput() order
  std::vector<int64_t> pendingSerial;  // genes submitted and not yet collected, submission order
  std::map<int64_t, rvt_gene_result> ready;  // records collected, waiting for their rows to be written
  std::map<int64_t, size_t> recBytes;        // device bytes of each pending gene
  void writeReadyRows(bool all);
  std::vector<int64_t> failedSerial;   // genes whose submission failed: NA rows
  NullFitter fitter = nullptr;
  const float* kinU = nullptr;
  bool haveFamNull = false;
  uint32_t famTests = 0;
  int64_t famSerial = -1;
  bool famOk = false;
  rvt_gene_result famRec{};
  uint32_t moreTests = 0;
  struct MoreGene {
    int64_t serial;
    DeviceBlock block;  // on member 0; freed when flushBurdenMore() / shutdown() clear the vector
    int M, d;
    std::vector<double> af;
  };
  struct MoreRecord {
    rvt_burden_more_result rec;
    int d;  // 1 + the covariates of the gene's null model: the Wald tests print d rows
  };
  struct MoreRow {
    BurdenMoreTest* model;
    TextSink* fp;
    std::string siteTab;
    int64_t serial;
  };
  std::vector<MoreGene> moreGenes;           // uploaded and not yet run, submission order
  std::vector<double> moreY;                 // the phenotype of the pending genes (exactCMC's table)
  size_t moreBytes = 0;
  std::map<int64_t, MoreRecord> moreReady;   // records of the last call, waiting for their rows
  std::vector<MoreRow> moreRows;             // in writeOutput() order
  int64_t moreSerial = -1;
  bool moreOk = false;
  void writeReadyMoreRows();
  int installNull(const GeneData& gd, bool binary, std::string* err);
};

// ---- ModelFitter ---------------------------------------------------------------------------------------------------
class ModelFitter {
 public:
  virtual int fit(GeneData* dc) = 0;
  virtual void writeHeader(TextSink* fp, const SiteInfo& siteInfo) = 0;
  virtual void writeOutput(TextSink* fp, const SiteInfo& siteInfo) = 0;
  virtual void writeFootnote(TextSink*) {}
  virtual int setParameter(const ModelParser&) { return 0; }
  virtual void reset() {}
  virtual ~ModelFitter() {}
  const std::string& getModelName() const { return modelName; }
  bool isBinaryOutcome() const { return binaryOutcome; }
  void setBinaryOutcome() { binaryOutcome = true; }
  void setQuantitativeOutcome() { binaryOutcome = false; }

 protected:
  std::string modelName = "UninitializedModel";
  bool binaryOutcome = false;
  int64_t curSerial = -1;  // gene handed to the last fit()
  std::string lastError;
};

// The gene tests that run batched through GpuBroker: fit() = submit, writeOutput() = enqueue, writeFootnote() = flush.  A model
// is its registration (test bit and parameters), the header text after the site columns, and formatRow.
class DeferredGeneTest : public ModelFitter {
 public:
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeFootnote(TextSink* fp) override;
  // one output row (without the site columns, with the newline) from a collected record; r == nullptr -> NA row
  virtual std::string formatRow(const rvt_gene_result* r) const = 0;

 protected:
  // test == 0 registers nothing (AnalyticVTTest for related samples, which runs synchronously)
  DeferredGeneTest(const char* name, uint32_t test, const rvt_params& p, const std::string& header);
  std::string header;  // the column names after the site columns, with the newline
};

class SkatTest : public DeferredGeneTest {
 public:
  SkatTest(int nPerm, double alpha, double beta1, double beta2);
  std::string formatRow(const rvt_gene_result* r) const override;

 private:
  bool usePermutation;
};

class SkatOTest : public DeferredGeneTest {
 public:
  SkatOTest(double beta1, double beta2);
  std::string formatRow(const rvt_gene_result* r) const override;
};

class CMCTest : public DeferredGeneTest {
 public:
  CMCTest();
  std::string formatRow(const rvt_gene_result* r) const override;
};

class ZegginiTest : public DeferredGeneTest {
 public:
  ZegginiTest();
  std::string formatRow(const rvt_gene_result* r) const override;
};

// `--vt analytic` (src/ModelManager.cpp:158-159; AnalyticVT(UNRELATED), src/Model.h:2105-2259): quantitative traits only,
// columns MinMAF MaxMAF OptimMAF OptimNumVar U V Stat Pvalue.  The reference's p-value comes from a randomised rule at
// absolute accuracy 1e-3 and the row is NA when that rule's error estimate exceeds it (MvtNorm::compute_Band); here the
// integral is evaluated deterministically and the row is NA when ITS error estimate exceeds 1e-3.
// `--vt famanalytic` (AnalyticVT(RELATED), :160-161): the same columns from FastLMM's frequencies, scores and variances
// (rvt_fam_analytic_vt); synchronous, one gene per call.
class AnalyticVTTest : public DeferredGeneTest {
 public:
  explicit AnalyticVTTest(bool related = false);
  std::string formatRow(const rvt_gene_result* r) const override;
  int fit(GeneData* dc) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeFootnote(TextSink* fp) override;

 private:
  bool related;
  bool fitOK = false;
  rvt_gene_result rec{};
};

// `--kernel kbac[nPerm=10000:alpha=0.05]` (src/ModelManager.cpp kernel switch; KBACTest, src/Model.h:2891-3045): binary
// traits without covariates, one column "Pvalue" printed with %f.  Synchronous: the permutations consume the process-wide
// random stream gene by gene.
class KbacTest : public ModelFitter {
 public:
  KbacTest(int nPerm, double alpha);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;

 private:
  int nPerm;
  double alpha;
  bool fitOK = false;
  rvt_kbac_result rec{};
};

// Permutation's members (src/Permutation.h:150-156) as its constructor leaves them; reset() zeroes all but numPerm (:99-105),
// which the models keep themselves
struct PermutationState {
  double obs = -1.0;
  int actualPerm = -1, numX = -1, numEqual = -1;
  void reset() {
    obs = 0.0;
    actualPerm = numX = numEqual = 0;
  }
  template <class Rec>
  void take(const Rec& r, double stat) {  // perm.init(stat), then the counters of a permutation entry's record
    obs = stat;
    actualPerm = r.actual_perm;
    numX = r.num_greater;
    numEqual = r.num_equal;
  }
  std::string fields(int nPerm) const;  // NumPerm ActualPerm Stat NumGreater NumEqual PermPvalue, tab-separated
};

// `--vt price[nPerm=10000,alpha=0.05]` (src/ModelManager.cpp vt switch; VariableThresholdPrice, src/Model.h:1745-1882): Price's
// variable-threshold permutation test for quantitative and binary traits (covariates are ignored, as the reference does
// after its warning).  Columns: an EMPTY one (writeHeaderTab's tab followed by "\tOptFreq", src/Model.h:1807-1812), OptFreq,
// Zmax with %g, then Permutation's NumPerm ActualPerm Stat NumGreater NumEqual PermPvalue.  A gene whose fit failed still
// prints a row (:1814-1819 has no fitOK test): the Permutation fields as reset() leaves them and the OptFreq / Zmax of the
// last successful fit (-1 before the first).  Synchronous: in exact mode the shuffles consume the process-wide random
// stream gene by gene.
class VariableThresholdPrice : public ModelFitter {
 public:
  VariableThresholdPrice(int nPerm, double alpha);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void reset() override {  // src/Model.h:1820-1824 over Permutation::reset (src/Permutation.h:99-105)
    fitOK = false;
    perm.reset();
  }

 private:
  int nPerm;
  double alpha;
  bool fitOK = false;
  double zmax = -1.0, optimalFreq = -1.0;  // members of the reference's class: they survive reset()
  PermutationState perm;
  rvt_vtprice_result rec{};
};

// `--burden rarecover[nPerm=10000,alpha=0.05]` (src/ModelManager.cpp:115-121; RareCoverTest, src/Model.h:1419-1590): the greedy
// cover's largest genotype-phenotype correlation under shuffles of a 0 / 1 phenotype.  Columns: NumIncludeMarker (NA unless the
// fit succeeded), then Permutation's six.  A quantitative trait or covariates fail the fit after a warning; the row still prints
// (:1488-1497 has no fitOK test around the Permutation fields).  Synchronous: in exact mode the shuffles consume the process-wide
// random stream gene by gene.
class RareCoverTest : public ModelFitter {
 public:
  RareCoverTest(int nPerm, double alpha);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void reset() override { perm.reset(); }  // src/Model.h:1477-1480 over Permutation::reset (src/Permutation.h:99-105)

 private:
  int nPerm;
  double alpha;
  bool fitOK = false;
  int numSelected = 0;
  PermutationState perm;
  rvt_rarecover_result rec{};
};

// `--burden mb[nPerm=10000,alpha=0.05]` (src/ModelManager.cpp:104-110; MadsonBrowningTest, src/Model.h:1244-1340).  Binary trait:
// the header is Permutation's six names and one "\n", a row its six values and "\n" (no fitOK test); quantitative trait: the header
// is "Pvalue\n" followed by a second "\n" — an empty line — and every row is "NA" (:1311-1331).  Synchronous, as RareCoverTest.
class MadsonBrowningTest : public ModelFitter {
 public:
  MadsonBrowningTest(int nPerm, double alpha);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void reset() override { perm.reset(); }  // src/Model.h:1306-1309

 private:
  int nPerm;
  double alpha;
  bool fitOK = false;
  PermutationState perm;
  rvt_mb_result rec{};
};

// `--burden cmcWald`, `zegginiWald`, `fp`, `exactCMC` (src/ModelManager.cpp:99-142; CMCWaldTest, ZegginiWaldTest, CMCFisherExactTest
// src/Model.h:909-1168, FpTest :1344-1417): the analytic burden tests of rvt_burden_blocks.  No name takes parameters.  Batched
// through GpuBroker like CMC and Zeggini: fit() submits the gene once for all four, writeOutput() records the row, the rows are
// formatted from the records in call order (GpuBroker::submitBurdenMore).  Rows are the reference's:
//   CMCWald / ZegginiWald  one row per column 1 .. X.cols - 1 of X = [1, collapsed, covariates] (site columns repeated), "NonRefSite
//                          Beta SE Pvalue" / "Beta SE Pvalue"; NA fields when the fit failed.  A gene without polymorphic column
//                          fails BEFORE X is rebuilt: it prints as many NA rows as the previous gene's X had columns, less one —
//                          none when no gene has built X yet.
//   Fp                     "Pvalue"
//   CMCFisherExact         "N00 N01 N10 N11 PvalueTwoSide PvalueLess PvalueGreater"; a quantitative trait or covariates warn once
//                          and print NA rows
class BurdenMoreTest : public ModelFitter {
 public:
  int fit(GeneData* dc) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeFootnote(TextSink* fp) override;
  // the gene's rows, site columns and line ends included, from its record (r == nullptr: the gene was not run) and the d of its
  // null model; called once per writeOutput(), in call order
  virtual std::string formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int d) = 0;

 protected:
  explicit BurdenMoreTest(uint32_t which);
};
class BurdenWaldTest : public BurdenMoreTest {
 public:
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  std::string formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int d) override;

 protected:
  BurdenWaldTest(const char* name, bool zeggini);

 private:
  bool zeggini;
  int xCols = 0;  // this->X.cols as the last gene with a polymorphic column left it
};
class CMCWaldTest : public BurdenWaldTest {
 public:
  CMCWaldTest() : BurdenWaldTest("CMCWald", false) {}
};
class ZegginiWaldTest : public BurdenWaldTest {
 public:
  ZegginiWaldTest() : BurdenWaldTest("ZegginiWald", true) {}
};
class FpTest : public BurdenMoreTest {
 public:
  FpTest() : BurdenMoreTest(RVT_BURDEN_FP) { modelName = "Fp"; }
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  std::string formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int d) override;
};
class CMCFisherExactTest : public BurdenMoreTest {
 public:
  CMCFisherExactTest() : BurdenMoreTest(RVT_BURDEN_EXACTCMC) { modelName = "CMCFisherExact"; }
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  std::string formatRows(const std::string& siteTab, const rvt_burden_more_result* r, int d) override;
};

// `--kernel famSkat[beta1:beta2]` (src/Model.h:3048-3145).  The reference ignores beta1 / beta2 for this model
// (FamSkat.cpp:129-137 always uses Beta(1, 25)); so does this adapter.
class FamSkatTest : public ModelFitter {
 public:
  FamSkatTest(double beta1, double beta2);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;

 private:
  bool fitOK = false;
  rvt_gene_result rec{};
};

// `--burden famcmc` / `--burden famzeggini` (src/Model.h:2261-2492): collapse + FastLMM score test.
class FamBurdenTest : public ModelFitter {
 public:
  explicit FamBurdenTest(bool zeggini);
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;

 private:
  bool zeggini;
  bool fitOK = false;
  double effect = -1.0;  // the reference leaves the previous value when V == 0 (src/Model.h:2338-2340)
  rvt_gene_result rec{};
};

// `--meta cov[windowSize=..:gwama]` for unrelated samples.  fit() is called once per variant (genotype.cols == 1,
// src/Model.cpp:844-858) and only copies the column into a device-resident ring; covariance rows are produced block
// by block on the GPU (rvt_cov_block) and written in the reference's order and format when their window is complete
// — the reference itself defers each row until its head is evicted (src/Model.h:3956-3968), so deferring changes
// when a row reaches the file, not what the file holds.  A window that holds more sites than the ring — and, since round 5,
// a flush that could emit less than half of the ring — makes the ring grow (up to RVT_METACOV_MAX_COLUMNS and 96 GB of columns,
// RVT_METACOV_RING_GB): with at least two windows in the ring every flush emits half of what it reads.  Rings wider than one
// block of the symmetric kernel are processed as heads-by-window rectangles of up to 1 024 heads (rvt_cov_rect; the exact int8
// product for hard calls like the symmetric block).  Rows still pending are flushed by writeFootnote() / the
// destructor, as the reference's destructor does (src/Model.cpp:828-834).
class MetaCovTest : public ModelFitter {
 public:
  explicit MetaCovTest(int windowSize);
  ~MetaCovTest() override;
  int setParameter(const ModelParser& parser) override;
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeFootnote(TextSink* fp) override;

 protected:
  // put this site's column into column c of the ring (the coded models upload the raw calls and recode them on the device)
  virtual int putSiteColumn(GeneData* dc, int c) { return block.uploadColumn(c, dc->genotype, &lastError); }
  // called before any device call on the ring (flush, grow)
  virtual int columnsReady() { return 0; }
  int flush(bool final);
  TextSink* fout = nullptr;
  DeviceBlock block;         // the device ring: `capacity` columns, never compacted

 private:
  struct Site {
    std::string chrom;
    int pos;
  };
  int grow();
  int windowSize;
  int capacity = 4096;                 // columns of the device ring (grows until it holds four windows)
  int head = 0;                        // physical column of sites[0]: site k lives in column (head + k) mod capacity
  int maxColumns = 65536;              // RVT_METACOV_MAX_COLUMNS
  bool canGrow = true;                 // false once a non-mandatory grow() failed (not retried on every fill)
  int formatThreads = 1;               // threads that turn the band of a flush into text (RVT_METACOV_FORMAT_THREADS; default up to 8)
  std::vector<float> bandBuf;          // where the band of a flush lands (page-locked: rvt_host_register)
  float* bandReg = nullptr;
  bool outputGwama = false;
  bool fitOK = false;
  bool useFamilyModel = false;
  int64_t nSample = -1;
  int nCovariate = 0;
  rvt_ctx* ctx = nullptr;
  std::vector<Site> sites;   // variants currently in the ring, file order
};

// What the models that test one site per fit() share (MetaScoreTest, the single-variant tests, FastMultipleTraitScoreTest):
// fit() copies the site's column into a device block of `capacity` columns; a full block, writeFootnote() and the destructor
// of the concrete class run flush(): ONE device call over the `used` columns, whose rows are then written in file order.
// The head of fit() is offered as steps: each model runs them in its own order, which decides what row a failing site prints.
class ColumnBlockTest : public ModelFitter {
 public:
  void writeFootnote(TextSink* fp) override;

 protected:
  explicit ColumnBlockTest(const char* capacityEnv);  // the environment variable that overrides `capacity`
  // Rows still pending are written by the destructors of the concrete classes (flush() is theirs: a base destructor could no
  // longer reach it); the block is freed behind them, by its member's destructor.
  virtual int flush() = 0;
  int makeRoom(size_t pendingRows);        // flush a full block; -1 also when it stays full (no sink named yet)
  int sameSampleSize(const GeneData& dc);  // -1: "Sample size changed"
  // the rows tested so far belong to the previous null model: finish them before a new one replaces it (the current site's
  // row, already the last of `rows`, stays)
  template <class Row>
  int flushBeforeNewNull(const GeneData& dc, std::vector<Row>* rows) {
    if (nSample < 0 || !(dc.phenotypeUpdated || dc.covariateUpdated) || used == 0) return 0;
    Row keep = rows->back();
    rows->pop_back();
    if (flush()) return -1;
    rows->push_back(keep);
    return 0;
  }
  int allocateOnFirstUse(const GeneData& dc);  // the first site that gets this far fixes N and the null's columns
  int capacity = 1024;
  int64_t nSample = -1;
  int nCovariate = 0;  // columns of the null X, intercept included
  int used = 0;        // columns of the block in use
  rvt_ctx* ctx = nullptr;
  DeviceBlock block;
  TextSink* fout = nullptr;
};

// `--meta score` (src/Model.h:3155-3398): MetaUnrelatedQtl / MetaUnrelatedBinary, and MetaFamQtl / MetaFamBinary when the
// caller hands over a kinship decomposition (the BOLT variants are not provided).  Sites are copied
// into a device block as fit() sees them; a full block (or writeFootnote / the destructor) runs ONE rvt_score_block
// over all of them and writes their rows in file order, after the summary header with the null-model estimates.
class MetaScoreTest : public ColumnBlockTest {
 public:
  MetaScoreTest();
  ~MetaScoreTest() override;
  int setParameter(const ModelParser& parser) override;
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  std::vector<std::string> covLabel;  // g_SummaryHeader->getCovLabel() (src/Model.h:3287-3289): set by the caller

 protected:
  // put this site's column into column c of the block (the coded models upload the raw calls and recode them on the device)
  virtual int putSiteColumn(GeneData* dc, int c) { return block.uploadColumn(c, dc->genotype, &lastError); }
  // called before the device call of flush()
  virtual int columnsReady() { return 0; }
  int flush() override;             // capacity: RVT_METASCORE_BLOCK
  int beginRow(const GeneData& dc);  // the site's row with its counters (printed whether or not the test runs); -1: no room

 private:
  struct Row {
    std::string siteTab;            // filled by writeOutput
    SiteCounts all, cases, ctrls;
    bool tested = false;            // fit() reached the score test (false: the row prints the counters only)
    bool written = false;           // writeOutput was called for this site
    int column = -1;                // column in the device block
  };
  bool outputSE = false;
  bool useFamilyModel = false;
  double famB = 1.0;                // MetaFamBinary: b
  bool headerOutputted = false;
  std::string siteHeaderTab;
  std::vector<Row> rows;
};

// `--meta dominant` / `--meta recessive` (src/ModelManager.cpp:211-226): the score file and the covariance file of the
// RAREMETAL dominant / recessive models (MetaDominantTest / MetaRecessiveTest src/Model.h:3880-3902, MetaDominantCovTest /
// MetaRecessiveCovTest :4098-4124) — MetaScoreTest / MetaCovTest on the column DataConsolidator::codeGenotypeForDominantModel /
// ...RecessiveModel make of the site's calls before imputation (src/DataConsolidator.cpp:390-472), recoded on the device
// (rvt_block_recode).  The site counters stay those of the raw additive calls (fitWithGivenGenotype, src/Model.h:3211-3230).
// Not carried: the reference's DROP branch (missing calls are always imputed to the recoded mean), and related samples — with a
// kinship the fit fails with a message and the rows print NA.
class MetaCodedScoreTest : public MetaScoreTest {
 public:
  ~MetaCodedScoreTest() override;  // (the pending rows are written here: the base's destructor no longer reaches the hooks)
  int fit(GeneData* dc) override;  // refuses a kinship and a site without raw calls before anything is fitted

 protected:
  MetaCodedScoreTest(int coding, const char* name);
  int putSiteColumn(GeneData* dc, int c) override;
  int columnsReady() override;

 private:
  int coding;
  ColumnRecoder recoder;
};
class MetaDominantTest final : public MetaCodedScoreTest {
 public:
  MetaDominantTest() : MetaCodedScoreTest(RVT_CODING_DOMINANT, "MetaDominant") {}
};
class MetaRecessiveTest final : public MetaCodedScoreTest {
 public:
  MetaRecessiveTest() : MetaCodedScoreTest(RVT_CODING_RECESSIVE, "MetaRecessive") {}
};
class MetaCodedCovTest : public MetaCovTest {
 public:
  ~MetaCodedCovTest() override;
  int fit(GeneData* dc) override;

 protected:
  MetaCodedCovTest(int windowSize, int coding, const char* name);
  int putSiteColumn(GeneData* dc, int c) override;
  int columnsReady() override;

 private:
  int coding;
  ColumnRecoder recoder;
};
class MetaDominantCovTest final : public MetaCodedCovTest {
 public:
  explicit MetaDominantCovTest(int windowSize) : MetaCodedCovTest(windowSize, RVT_CODING_DOMINANT, "MetaDominantCov") {}
};
class MetaRecessiveCovTest final : public MetaCodedCovTest {
 public:
  explicit MetaRecessiveCovTest(int windowSize) : MetaCodedCovTest(windowSize, RVT_CODING_RECESSIVE, "MetaRecessiveCov") {}
};

// `--single wald,score` for unrelated samples.  fit() is called once per variant (genotype.cols == 1) and copies the column
// into a device block; a full block (or writeFootnote / the destructor) runs ONE device call over all of them and writes their
// rows in file order, as MetaScoreTest does.  The null model is the device fit of rvt_fit_null.
class SingleVariantBlockTest : public ColumnBlockTest {
 public:
  int fit(GeneData* dc) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;
  std::vector<std::string> covLabel;  // covariate column labels (cov.GetColumnLabel(k)): set by the caller

 protected:
  struct Row {
    std::string siteTab;
    std::vector<std::string> labels;  // X.GetColumnLabel(1 ..): the genotype, then the covariates
    double af = -1.0;
    int column = -1;       // column in the device block; -1: not tested (fit() failed before the test)
    bool written = false;  // writeOutput was called for this site
  };
  SingleVariantBlockTest() : ColumnBlockTest("RVT_SINGLE_BLOCK") {}
  // the device call over the first `used` columns; its return code (not 0: the block's rows print NA)
  virtual int runBlock() = 0;
  virtual std::string formatSingleRow(const Row& r) = 0;
  // the context with this model's null installed (default: rvt_fit_null's); nullptr with lastError set when the site
  // cannot be tested
  virtual rvt_ctx* acquireContext(GeneData* dc);
  int flush() override;
  std::vector<Row> rows;
  std::vector<int> ok;
};

// SingleVariantWaldTest (src/Model.h:98-180): "Test Beta SE Pvalue", one row per column of X after the intercept (only the
// genotype's with hideCovar = FLAG_hideCovar).  Like the reference's writeOutput this never clears its Result: a failed or
// monomorphic site prints the Beta / SE / Pvalue the previous row left (NA before the first fitted row).
class SingleVariantWaldTest final : public SingleVariantBlockTest {
 public:
  SingleVariantWaldTest();
  ~SingleVariantWaldTest() override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  bool hideCovar = false;

 private:
  int runBlock() override;
  std::string formatSingleRow(const Row& r) override;
  std::vector<double> beta, se, pv;
  std::string lastBeta = "NA", lastSE = "NA", lastP = "NA";
};

// SingleVariantScoreTest (src/Model.h:259-377): "AF U V STAT DIRECTION EFFECT SE PVALUE" in LinearRegressionScoreTest's units
// (U = g'res, V = SS sigma2, EFFECT = U / SS, SE = GetSEBeta) or LogisticRegressionScoreTest's (U, V, EFFECT = U / V,
// SE = 1 / sqrt(V)), from rvt_score_block.
class SingleVariantScoreTest final : public SingleVariantBlockTest {
 public:
  SingleVariantScoreTest();
  ~SingleVariantScoreTest() override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;

 private:
  int runBlock() override;
  std::string formatSingleRow(const Row& r) override;
  std::vector<double> u, v, eff, se, pv;
  double sigma2 = 1.0;
};

// The single-variant tests for related samples (src/Model.h:525-805): FamScore "AF U.Stat V.Stat Pvalue" (rvt_score_block_fam),
// FamLRT "AF NullLogLik AltLogLik Pvalue" (rvt_lrt_block_fam) and FamGrammarGamma "AF Beta BetaVar Pvalue"
// (rvt_grammar_block).  The kinship is GeneData's (either form) through the broker's install; a binary trait or a missing
// kinship fails every fit().  Like the reference's writeOutput these never clear their Result: a failed or monomorphic site
// prints the values the previous row left (NA before the first fitted row).
class SingleVariantFamilyTest : public SingleVariantBlockTest {
 public:
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;

 protected:
  SingleVariantFamilyTest(const char* name, const char* header, const char* what);
  rvt_ctx* acquireContext(GeneData* dc) override;
  int runBlock() override;
  virtual int blockEntry() = 0;  // the model's rvt_*_block entry over the first `used` columns, into ok and col
  std::string formatSingleRow(const Row& r) override;
  std::vector<double> col[4];  // the four printed values per column of the block
  std::string last[4] = {"NA", "NA", "NA", "NA"};
  std::string header;
  std::string what;  // the model's words in the reference's warnings
};

class SingleVariantFamilyScore final : public SingleVariantFamilyTest {
 public:
  SingleVariantFamilyScore();
  ~SingleVariantFamilyScore() override;

 private:
  int blockEntry() override;
};

class SingleVariantFamilyLRT final : public SingleVariantFamilyTest {
 public:
  SingleVariantFamilyLRT();
  ~SingleVariantFamilyLRT() override;

 private:
  int blockEntry() override;
};

class SingleVariantFamilyGrammarGamma final : public SingleVariantFamilyTest {
 public:
  explicit SingleVariantFamilyGrammarGamma(bool afKinship);
  ~SingleVariantFamilyGrammarGamma() override;

 private:
  rvt_ctx* acquireContext(GeneData* dc) override;
  int blockEntry() override;
  bool afKinship = false;
  bool haveNull = false;
  const float* nullKinship = nullptr;  // the decomposition the GrammarGamma null was fitted on
};

// FastMultipleTraitScoreTest (src/Model.h:4935-5125, `--single fastmtscore` under --multiplePheno): every site against the T
// tests of GeneData::formula, "U_STAT V_STAT PVALUE" with the T numbers of a site joined by ",", each printed as the reference's
// toString(double) prints it (%g; NaN as "nan").  The block pattern of SingleVariantBlockTest: fit() copies the site's column
// into a device ring of `capacity` columns (1024, RVT_SINGLE_BLOCK), a full block — and writeFootnote / the destructor — runs ONE
// rvt_mt_score_block and writes the rows in file order.  The null (rvt_mt_fit_null) is made by the first fit() and again when the
// caller flags an updated phenotype / covariate.  fit() fails on a binary trait (the reference's warnOnce) and on a genotype
// with other than one column; such a site prints NO row (the reference counts it into its block without a genotype column).
class FastMultipleTraitScoreTest final : public ColumnBlockTest {
 public:
  FastMultipleTraitScoreTest();
  ~FastMultipleTraitScoreTest() override;
  int fit(GeneData* dc) override;
  void writeHeader(TextSink* fp, const SiteInfo& siteInfo) override;
  void writeOutput(TextSink* fp, const SiteInfo& siteInfo) override;

 private:
  int fitNull(GeneData* dc);
  int flush() override;
  int nTest = 0;
  bool haveNull = false, fitOK = false;
  std::vector<std::string> rows;  // the site columns of the block's columns, in file order ("" until writeOutput names them)
  std::vector<char> written;
  std::vector<double> u, v, pv;
};

// ---- ModelManager::create -----------------------------------------------------------------------------------------
class ModelManager {
 public:
  ~ModelManager();
  // type: "burden" | "kernel" | "vt" | "meta" | "single"; modelList: "cmc,zeggini", "skat[nPerm=0:beta1=1],skato" or "cov[windowSize=500000]"
  int create(const std::string& type, const std::string& modelList);
  const std::vector<ModelFitter*>& getModel() const { return model; }
  void setBinaryOutcome();
  void setQuantitativeOutcome();
  // "<prefix>.<ModelName>.assoc" names (src/ModelManager.cpp:285-297)
  std::vector<std::string> outputNames(const std::string& prefix) const;
  std::string lastError;

 private:
  std::vector<ModelFitter*> model;
};

}  // namespace rvt_host
