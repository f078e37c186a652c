"""CPU: numpy statements of the analytic burden tests --burden cmcWald, zegginiWald, fp, exactCMC (CMCWaldTest, ZegginiWaldTest,
CMCFisherExactTest src/Model.h:909-1168, FpTest :1344-1417) that tests/test_gpu_burden_wald.py holds the engine to:

  fp_collapse    fpCollapse (src/Model.cpp:177-197) of the flipped, polymorphic block
  fisher_2x2     Table2by2::FullFastFisherExactTest (regression/Table2by2.cpp:316-357) with its table of cumulative log sums,
                 term by term in the reference's order; pinned on tests/golden/fisher_2x2.json (recorded from the reference's own
                 class) and checked against exact rational arithmetic on small tables
  table_2x2      the 2 x 2 table of CMCFisherExactTest::fit
  *_rows         the text rows the four classes print

The Wald and score statements are wald_linear / wald_logistic of tests/test_single_cpu.py and orc.metascore, applied to orc.collapse
columns."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import orc
import synth
from test_single_cpu import wald_linear, wald_logistic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fisher_2x2.json")
SITE_HEADER = "Range\tN_INFORMATIVE\tNumVar\tNumPolyVar\t"


# ---- statements ------------------------------------------------------------------------------------------------------------------
def fp_collapse(Gf, af):
    """Gf: the flipped, polymorphic N x m block; af: the gene's frequencies, read by the FILTERED column's index (quirk #3)."""
    out = np.zeros(Gf.shape[0])
    for m in range(Gf.shape[1]):
        f = af[m]
        if f <= 0.0 or f >= 1.0:
            continue
        w = 1.0 / math.sqrt(f * (1.0 - f))
        out = out + Gf[:, m] * w
    return out


def table_2x2(cmc, y):
    """[N00, N01, N10, N11], indexed [geno][pheno]; geno = (int)cmc, pheno = (int)y, samples outside 0 .. 1 skipped"""
    g, p = np.trunc(cmc).astype(np.int64), np.trunc(y).astype(np.int64)
    keep = (g >= 0) & (g <= 1) & (p >= 0) & (p <= 1)
    g, p = g[keep], p[keep]
    return [int(((g == a) & (p == b)).sum()) for a in (0, 1) for b in (0, 1)]


def _log_facs(n):
    lf = [0.0] * (n + 1)
    for i in range(1, n + 1):
        lf[i] = lf[i - 1] + math.log(float(i))
    return np.array(lf)


def fisher_terms(n00, n01, n10, n11):
    """(logp of every admissible i, the admissible i, logpCutoff) as FullFastFisherExactTest forms them"""
    row0, row1, col0, total = n00 + n01, n10 + n11, n00 + n10, n00 + n01 + n10 + n11
    lf = _log_facs(total)

    def logp(a, b, c, d):  # Table2by2::logHypergeometricProb, the reference's order of operations
        return (lf[a + b] + lf[c + d] + lf[a + c] + lf[b + d] - lf[a] - lf[b] - lf[c] - lf[d] - lf[a + b + c + d])
    cutoff = float(logp(n00, n01, n10, n11))
    upper = min(row0, col0)
    lower = max(0, row0 + col0 - total)
    i = np.arange(lower, upper + 1)
    return logp(i, row0 - i, col0 - i, row1 + i - col0), i, cutoff


def _seq_sum(x):
    return float(np.cumsum(x)[-1]) if len(x) else 0.0      # a running sum, as the reference's += in ascending i


def fisher_2x2(n00, n01, n10, n11):
    """(PvalueTwoSide, PvalueLess, PvalueGreater)"""
    lp, i, cutoff = fisher_terms(n00, n01, n10, n11)
    with np.errstate(over="ignore", divide="ignore"):
        e = np.exp(lp - cutoff)
        sums = (_seq_sum(e[lp <= cutoff]), _seq_sum(e[i <= n00]), _seq_sum(e[i >= n00]))
        return tuple(float(np.exp(cutoff + np.log(s))) for s in sums)


def fisher_near_tie(n00, n01, n10, n11, rel=1e-9):
    """Does a term other than the observed one lie within rel of the cutoff?  (Such a term can fall on either side of `<=` when
    lgamma stands for the cumulative log sums.)"""
    lp, i, cutoff = fisher_terms(n00, n01, n10, n11)
    other = i != n00
    return bool((np.abs(lp[other] - cutoff) <= rel * abs(cutoff)).any())


def fisher_exact_rational(n00, n01, n10, n11):
    row0, col0, total = n00 + n01, n00 + n10, n00 + n01 + n10 + n11
    den = math.comb(total, col0)

    def prob(i):
        return Fraction(math.comb(row0, i) * math.comb(total - row0, col0 - i), den)
    lo, hi = max(0, row0 + col0 - total), min(row0, col0)
    p0 = prob(n00)
    two = sum(prob(i) for i in range(lo, hi + 1) if prob(i) <= p0)
    return float(two), float(sum(prob(i) for i in range(lo, n00 + 1))), float(sum(prob(i) for i in range(n00, hi + 1)))


def fmt(x):
    """floatToString (base/TypeConversion.h): %g"""
    return "%g" % x


def burden_statement(G, af, X, y, binary):
    """What the four classes compute for one gene (G imputed, unflipped): a dict of the record's fields."""
    Gf, fl, kp = orc.flip_poly(G)
    d = X.shape[1]
    r = dict(n_poly=Gf.shape[1], cmc=np.zeros(len(y)), zeg=np.zeros(len(y)), fp=np.zeros(len(y)), nonref=0,
             wald=[(0, 0, None, None, None)] * 2, fp_ok=0, exact_ok=0)
    if Gf.shape[1] == 0:
        return r
    r["cmc"], r["zeg"], r["fp"] = orc.collapse(Gf, 0), orc.collapse(Gf, 1), fp_collapse(Gf, af)
    r["nonref"] = int((r["cmc"] != 0.0).sum())
    wald = wald_logistic if binary else wald_linear
    r["wald"] = []
    for col in (r["cmc"], r["zeg"]):
        ok, rounds, beta, se, p = wald(col, X, y)
        r["wald"].append((1 if ok == 1 else 0, rounds, beta, se, p))
    rc, o = orc.metascore(r["fp"][:, None], X, y, binary)
    assert rc == 0
    r["fp_ok"] = int(o["ok"][0])
    r["fp_u"], r["fp_v"], r["fp_p"] = float(o["U"][0]), float(o["V"][0]), float(o["p"][0])
    if binary and d == 1:
        r["exact_ok"] = 1
        r["table"] = table_2x2(r["cmc"], y)
        r["exact_p"] = fisher_2x2(*r["table"])
    return r


# ---- the rows the classes print ------------------------------------------------------------------------------------------------------
WALD_HEADER = {"CMCWald": "NonRefSite\tBeta\tSE\tPvalue", "ZegginiWald": "Beta\tSE\tPvalue"}
FP_HEADER = "Pvalue"
EXACT_HEADER = "N00\tN01\tN10\tN11\tPvalueTwoSide\tPvalueLess\tPvalueGreater"


def wald_rows(site, name, fit, nonref, d, prev_cols):
    """CMCWaldTest / ZegginiWaldTest::writeOutput: one row per column 1 .. X.cols - 1.  fit = None: the gene failed before X was
    rebuilt — as many NA rows as the previous gene's X had columns, less one (prev_cols; none when no gene has built X yet)."""
    lead = ["NA"] if name == "CMCWald" else []
    if fit is None:
        return [site + "\t".join(lead + ["NA"] * 3)] * max(prev_cols - 1, 0)
    ok, rounds, beta, se, p = fit
    rows = []
    for k in range(d):
        if ok:
            f = ([str(nonref)] if name == "CMCWald" else []) + [fmt(beta[k]), fmt(se[k]), fmt(p[k])]
        else:
            f = lead + ["NA"] * 3
        rows.append(site + "\t".join(f))
    return rows


def fp_row(site, ok, p):
    return site + (fmt(p) if ok else "NA")


def exact_row(site, ok, table=None, pv=None):
    return site + ("\t".join([str(t) for t in table] + [fmt(x) for x in pv]) if ok else "\t".join(["NA"] * 7))


# ---- tests ---------------------------------------------------------------------------------------------------------------------
def golden_tables():
    doc = json.load(open(GOLDEN))
    assert "Table2by2" in doc["how"]
    return doc["tables"]


def test_fisher_statement_reproduces_the_reference_s_recorded_p_values():
    tabs = golden_tables()
    assert len(tabs) >= 40
    assert any(sum(t["n"]) == 500000 for t in tabs) and any(0 < t["two"] < 1e-100 for t in tabs)
    assert any(min(t["n"][0] + t["n"][1], t["n"][2] + t["n"][3]) == 0 for t in tabs)          # degenerate margins
    for t in tabs:
        got = fisher_2x2(*t["n"])
        for g, k in zip(got, ("two", "less", "greater")):
            # the same operations in the same order; numpy's exp / log may round differently from libm's in the last place,
            # which a cutoff of magnitude <= 2e3 turns into at most a few 1e-13 relative
            assert abs(g - t[k]) <= 1e-11 * abs(t[k]), (t["n"], k, g, t[k])


@pytest.mark.parametrize("tab", [(3, 1, 1, 3), (8, 2, 1, 5), (2, 7, 8, 2), (12, 5, 7, 7), (20, 3, 4, 15), (1, 9, 11, 3), (6, 6, 6, 7),
                                 (100, 50, 40, 90), (30, 1, 25, 9), (5, 0, 0, 0), (0, 0, 3, 4), (10, 0, 0, 10)])
def test_fisher_statement_against_exact_rational_arithmetic(tab):
    got, want = fisher_2x2(*tab), fisher_exact_rational(*tab)
    if fisher_near_tie(*tab):     # symmetric tables: the mirror term ties with the observed one and may fall on either side
        got, want = got[1:], want[1:]
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-10 * w, (tab, got, want)


def test_fp_collapse_reads_af_by_the_filtered_index_and_counts_imputed_fractions():
    N = 50
    G = np.zeros((N, 4))
    G[:5, 0] = 1.0
    G[:, 1] = 0.0                      # monomorphic: dropped, the columns behind it move up
    G[5:9, 2] = 2.0
    G[9, 2] = 0.37                     # an imputed fraction counts in Fp, not in CMC
    G[10:12, 3] = 1.0
    af = np.array([0.05, 0.2, 1.0, 0.3])   # af[2] = 1 is the THIRD FILTERED column's (original column 3): skipped
    Gf, fl, kp = orc.flip_poly(G)
    assert Gf.shape[1] == 3
    fp = fp_collapse(Gf, af)
    w0, w1 = 1 / math.sqrt(0.05 * 0.95), 1 / math.sqrt(0.2 * 0.8)
    assert fp[0] == 1.0 * w0 and fp[5] == 2.0 * w1 and fp[9] == 0.37 * w1 and fp[10] == 0.0
    assert orc.collapse(Gf, 0)[9] == 0.0 and orc.collapse(Gf, 1)[5] == 1.0


def test_table_and_rows():
    cmc = np.array([0, 1, 1, 0, 1, 0.0])
    y = np.array([0, 0, 1, 1, 1, 2.0])          # the last sample is outside 0 .. 1: skipped
    assert table_2x2(cmc, y) == [1, 1, 1, 2]
    site = "gene0\t6\t3\t\t"
    assert exact_row(site, 0) == site + "NA\tNA\tNA\tNA\tNA\tNA\tNA"
    assert exact_row(site, 1, [1, 1, 1, 2], (1.0, 0.5, 0.25)) == site + "1\t1\t1\t2\t1\t0.5\t0.25"
    fit = (1, 4, np.array([0.5, -1e-7]), np.array([0.25, 3.0]), np.array([0.045, 1.0]))
    assert wald_rows(site, "CMCWald", fit, 3, 2, 0) == [site + "3\t0.5\t0.25\t0.045", site + "3\t-1e-07\t3\t1"]
    assert wald_rows(site, "ZegginiWald", fit, 3, 2, 0) == [site + "0.5\t0.25\t0.045", site + "-1e-07\t3\t1"]
    assert wald_rows(site, "CMCWald", None, 0, 2, 0) == [] and wald_rows(site, "ZegginiWald", None, 0, 2, 3) == [site + "NA\tNA\tNA"] * 2
    assert fp_row(site, 1, 0.125) == site + "0.125" and fp_row(site, 0, 0.0) == site + "NA"


def test_statement_of_one_gene_is_consistent():
    N, d = 400, 2
    Graw, G, af = synth.make_gene(N, 9, seed=3, missing=0.02, common=True, mono=True, maf_lo=-2.0, maf_hi=-1.0)
    X, y, res, v, s2 = synth.make_null(N, 1, 1, seed=5)
    r = burden_statement(G, af, X, y, 1)
    assert r["n_poly"] > 0 and r["exact_ok"] == 1 and sum(r["table"]) == N
    assert r["table"][2] + r["table"][3] == r["nonref"]
    assert r["wald"][0][0] == 1 and r["fp_ok"] == 1
    assert abs(sum(fisher_2x2(*r["table"])[1:]) - 1.0 - math.exp(fisher_terms(*r["table"])[2]) ) < 1e-9   # less + greater = 1 + p(obs)


def test_model_manager_accepts_the_four_names_and_exactcmc_prints_na_for_a_quantitative_trait(tmp_path):
    """`--burden exactcmc` on a quantitative trait warns and prints NA rows without touching a device (src/Model.h:1099-1105);
    an unknown name is still refused; the four names parse (no model takes parameters)."""
    import test_vtprice_cpu as vt
    from test_burdenperm_cpu import write_input, run_burden_driver, split_outputs
    vt._ensure_driver()
    rng = np.random.default_rng(2)
    G = (rng.random((60, 4)) < 0.2).astype(np.float64)
    path = str(tmp_path / "in.bin")
    write_input(path, rng.normal(size=60), 0, [G, G])
    rc, out, err = run_burden_driver(path, "exactcmc")
    assert rc == 0, err
    f = split_outputs(out)
    assert f["out.CMCFisherExact.assoc"] == [SITE_HEADER + EXACT_HEADER] + [exact_row("gene%d\t60\t4\t\t" % g, 0) for g in (0, 1)]
    assert err.count("Fisher's exact test does not support continuous outcomes") == 1        # warnOnce
    # no gene in the file: the four models are created and write their headers, nothing is fitted
    write_input(path, (rng.random(60) < 0.5).astype(np.float64), 1, [])
    rc, out, err = run_burden_driver(path, "cmcwald,zegginiwald,fp,exactcmc")
    assert rc == 0, err
    f = split_outputs(out)
    assert f == {"out.CMCWald.assoc": [SITE_HEADER + WALD_HEADER["CMCWald"]], "out.ZegginiWald.assoc": [SITE_HEADER + WALD_HEADER["ZegginiWald"]],
                 "out.Fp.assoc": [SITE_HEADER + FP_HEADER], "out.CMCFisherExact.assoc": [SITE_HEADER + EXACT_HEADER]}
    rc, out, err = run_burden_driver(path, "cmat")
    assert rc == 1 and "Unknown model name: cmat" in err


def fisher_2x2_lgamma(a, b, c, d):
    """The engine's formulation (fisher_2x2_kernel): lgamma(n + 1) for the cumulative log sums, the margin terms formed once"""
    def lg(n):
        return math.lgamma(n + 1.0)
    row0, row1, col0, total = a + b, c + d, a + c, a + b + c + d
    margins = lg(row0) + lg(row1) + lg(col0) + lg(b + d) - lg(total)

    def lp(i, j, k, m):
        return margins - lg(i) - lg(j) - lg(k) - lg(m)
    cutoff = lp(a, b, c, d)
    s = [0.0, 0.0, 0.0]
    for i in range(max(0, row0 + col0 - total), min(row0, col0) + 1):
        v = lp(i, row0 - i, col0 - i, row1 + i - col0)
        e = math.exp(v - cutoff)
        s[0] += e if v <= cutoff else 0.0
        s[1] += e if i <= a else 0.0
        s[2] += e if i >= a else 0.0
    return [math.exp(cutoff + math.log(x)) for x in s]


def test_lgamma_formulation_is_within_the_north_star_tolerance_of_the_reference():
    """The documented difference: apart from exact ties of the two-sided sum, lgamma in the place of the reference's
    cumulative log sums moves no recorded p-value by more than 1e-6 relative — N = 500 000 and p < 1e-100 included."""
    ties = 0
    for t in golden_tables():
        tie = fisher_near_tie(*t["n"])
        ties += tie
        for g, k in zip(fisher_2x2_lgamma(*t["n"]), ("two", "less", "greater")):
            if tie and k == "two":
                continue
            assert abs(g - t[k]) <= 1e-6 * t[k], (t["n"], k, g, t[k])
    assert 0 < ties < len(golden_tables()) // 2
