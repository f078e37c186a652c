// rvtests_amd — the multiple-trait score test (`--single fastmtscore`): the arithmetic of ONE (variant, test) cell.
//
// `RVT_HD`, as rvt_special.h: the SAME source is compiled by hipcc into the finishing kernel (mtscore_kernels.hip.h) and by g++
// into the host test harness (hostcheck.cpp: hc_mt_cell), where the CPU tests compare it with the numpy statement.
//
// Replaces the per-test, per-variant body of FastMultipleTraitLinearRegressionScoreTest::TestCovariateBlock
// (regression/FastMultipleTraitLinearRegressionScoreTest.cpp:391-470) in fp64, in the reference's order of operations:
// the rare-allele correction from the UNCENTRED g'indModel (:398-412), u and v from the centred products (:419-433), the
// covariate terms (:435-445), sigma2 and the correction (:446-449), p = chisq_Q(u^2 / v, 1) or NaN when v == 0 (:461-466).
#pragma once
#include "rvt_special.h"

namespace rvt {

constexpr int kMtMaxCov = 15;  // covariates per test (RVT_MAX_COV - 1: the intercept is the centring)

// The constants of one test, as rvt_mt_fit_null leaves them (FitNullModel, :332-368).  ok = 0: a test without observations or
// with a covariate matrix that is not positive definite — every cell of it is NaN.
struct MtTest {
  int y;                // resident row of the phenotype
  int ncov;             // covariates (<= kMtMaxCov)
  int pattern;          // row of the test's indModel among the distinct patterns
  int ok;
  int z[kMtMaxCov + 1]; // resident rows of the covariates
  double obs;           // OBS = sum indModel
  double scale_xy;      // OBS / sum indY
  double scale_xx;      // OBS / N
  double sigma2;
  double scale_xz[kMtMaxCov];
  double zy[kMtMaxCov];
  double zz_inv[kMtMaxCov * kMtMaxCov];  // row-major ncov x ncov
};

// n: samples; nm = g'indModel (g as stored, not centred); gy = gc'Yc[:, y]; gz[c] = gc'Zc[:, z_c]; gg = |gc|^2.
RVT_HD void mt_cell(double n, double nm, double gy, const double* gz, double gg, const MtTest& t, double* u_out, double* v_out,
                    double* p_out) {
  if (!t.ok) {
    *u_out = *v_out = *p_out = NAN;
    return;
  }
  const double thr = (double)(float)sqrt(2.0 * n);  // const float thresholdAC = sqrt(2.0 * g.rows())
  const double af = nm / (2.0 * t.obs);
  double corr = nm < thr ? 2.0 * af * (1.0 - 2.0 * af) * t.obs : -1.0;  // (the 1 - 2 af is the reference's)
  double u = gy * t.scale_xy;
  double v = gg * t.scale_xx;
  corr = corr > 0.0 ? corr / v : 1.0;  // divides by v as it stands here
  const int C = t.ncov;
  if (C > 0) {
    double xz[kMtMaxCov];
    for (int a = 0; a < C; ++a) xz[a] = gz[a] * t.scale_xz[a];
    double du = 0.0, dv = 0.0;
    for (int a = 0; a < C; ++a) {
      double w = 0.0, q = 0.0;
      for (int b = 0; b < C; ++b) {
        w += t.zz_inv[a * C + b] * t.zy[b];
        q += t.zz_inv[a * C + b] * xz[b];
      }
      du += xz[a] * w;
      dv += xz[a] * q;
    }
    u -= du;
    v -= dv;
  }
  v *= t.sigma2;
  v *= corr;
  *u_out = u;
  *v_out = v;
  *p_out = (v == 0.0) ? NAN : chisq_Q(u * u / v, 1.0);
}

}  // namespace rvt
