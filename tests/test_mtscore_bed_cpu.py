"""rvt_mt_score_bed_dev without a GPU: its C ABI and binding, and the identities of its front stage (mtscore_kernels.hip.h, second
half) in numpy — the column moments follow from the four counts of a row, and the statement of c + mu m is the statement of the
imputed column."""
import os
import re
from fractions import Fraction

import numpy as np

import fam_bed_cases
import mtscore_bed_cases as cases
import mtscore_ref as mt
import rvtests_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_header_declares_documents_and_the_library_exports():
    src = open(os.path.join(ROOT, "include", "rvtests_amd.h")).read()
    decl = ("int rvt_mt_score_bed_dev(rvt_ctx* ctx, const unsigned char* d_rows, int64_t V, double* ustat, double* vstat, "
            "double* pvalue,\n                         long long* counts);")
    assert decl in src
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\nint rvt_mt_score_bed_dev\(", src, flags=re.S)
    assert doc
    for cited in ("regression/FastMultipleTraitLinearRegressionScoreTest.cpp:391-470", "src/DataConsolidator.cpp:217-245",
                  "RVT_E_INVALID", "RVT_E_STATE", "counts", "Exact", "Rounded", "rvt_mt_last_timing", "Not covered from resident rows",
                  "FastMultipleTraitScoreTest", "rvt_group_"):
        assert cited in doc.group(1), cited
    rvtests_amd.build_library()
    lib = rvtests_amd.load_library()
    assert hasattr(lib, "rvt_mt_score_bed_dev")
    assert callable(getattr(rvtests_amd.Engine, "mt_score_bed_dev"))


def test_the_counts_give_the_centred_moment():
    """gg = (n1 + 4 n2) - a a / called against (1) the same in rational arithmetic: a a is an exact double (a < 2^26), so two
    roundings — the quotient and the difference — of quantities no larger than n1 + 4 n2, i.e. within eps (n1 + 4 n2); and (2)
    sum (g - gbar)^2 of the imputed fp64 column in numpy, whose N squares and N - 1 additions each round once: within N eps of the
    sum in the worst order (measured: 3e-14 relative and below).  Monomorphic rows: exactly 0."""
    for N in (1497, 1502, 20000):
        raw = fam_bed_cases.calls(N, 30, seed=cases.SEED)
        assert raw.shape == (N, cases.ROWS)
        G = fam_bed_cases.imputed(raw)
        c, m, cnt, mu = cases.split(raw)
        mu_c, gg = cases.moments(cnt)
        assert np.array_equal(mu_c, mu)
        mono = G.min(0) == G.max(0)
        assert mono.any() and (gg[mono] == 0.0).all()
        worst = 0.0
        for v in range(raw.shape[1]):
            n0, n1, n2 = (int(x) for x in cnt[v, :3])
            called, a, s2 = n0 + n1 + n2, n1 + 2 * n2, n1 + 4 * n2
            exact = Fraction(s2) - Fraction(a * a, called) if called else Fraction(0)
            assert abs(Fraction(float(gg[v])) - exact) <= Fraction(float(EPS)) * s2, v
            col = float(((G[:, v] - G[:, v].mean()) ** 2).sum())
            assert abs(col - gg[v]) <= N * EPS * max(col, gg[v]) + EPS * s2, (N, v, col, gg[v])
            if col > 0:
                worst = max(worst, abs(col - gg[v]) / col)
        print("N=%d: counts against the column, worst relative difference %.3g" % (N, worst))


def test_the_statement_of_c_plus_mu_m_is_the_statement_of_the_imputed_column():
    N = 1497
    Y, Z, tests, _ = mt.base_input(N)
    raw = fam_bed_cases.calls(N, 30, seed=cases.SEED)
    c, m, cnt, mu = cases.split(raw)
    nul = mt.fit_null(Y, Z, tests)
    got = mt.score(Y, Z, tests, c + mu[None, :] * m, null=nul)
    ref = mt.score(Y, Z, tests, fam_bed_cases.imputed(raw), null=nul)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isfinite(ref[0]).any() and np.isnan(ref[2]).any()
