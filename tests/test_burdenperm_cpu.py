"""CPU: plain numpy statements of the reference's RareCoverTest::fit (src/Model.h:1419-1590) and MadsonBrowningTest::fit
(src/Model.h:1244-1340 over madsonBrowningCollapse / getMarkerFrequencyFromControl, src/Model.cpp:47-66,155-175 and the
two-argument TestCovariate, regression/LogisticRegressionScoreTest.cpp:310-373) in fp64, driven by the glibc stream the oracle
exports — the yardsticks of tests/test_gpu_burdenperm.py — beside the forms the kernels use (bitsets and popcounts; integer case
sums and the Gram matrix), and the checks that need no GPU: the forms against the statements, the ABI entries and their records,
the `--burden rarecover[...],mb` parser entries and the two header lines."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import orc
import test_vtprice_cpu as vt

ROOT = vt.ROOT
DRIVER = vt.DRIVER
PERM_HEADER = vt.PERM_HEADER
SITE_HEADER = "Range\tN_INFORMATIVE\tNumVar\tNumPolyVar\t"


def valid_phenotype(y):
    """the engine's rule: 0 / 1 with both classes present"""
    y = np.asarray(y, dtype=np.float64)
    return bool(np.isin(y, (0.0, 1.0)).all() and 0 < (y == 1.0).sum() < len(y))


def popcount(x):
    return bin(x).count("1")


# ---- RareCover: the literal statement ----------------------------------------------------------------------------------------
def rc_correlation_loop(g, collapsed, pheno):
    """calculateCorrelation (src/Model.h:1544-1573) word for word, one sample at a time"""
    sum_g = sum_g2 = sum_p = sum_p2 = sum_gp = 0.0
    n = len(pheno)
    for i in range(n):
        geno = 1.0 if g[i] + collapsed[i] > 0 else 0.0
        if geno > 0.0:
            sum_g += geno
            sum_g2 += geno * geno
            sum_gp += geno * pheno[i]
        sum_p += pheno[i]
        sum_p2 += pheno[i] * pheno[i]
    return rc_correlation_tail(sum_g, sum_g2, sum_p, sum_p2, sum_gp, n)


def rc_correlation_tail(sum_g, sum_g2, sum_p, sum_p2, sum_gp, n):
    cov_gp = sum_gp - sum_g * sum_p / n
    var_g = sum_g2 - sum_g * sum_g / n
    var_p = sum_p2 - sum_p * sum_p / n
    v = var_g * var_p
    if v < 1e-10:
        return 0.0
    return cov_gp / math.sqrt(v)


def rc_correlation_literal(g, collapsed, pheno):
    """the same over whole vectors: for a 0 / 1 phenotype every summand of the five sums is 0 or 1, so each sum is an exact integer
    in any order (checked against the loop below)"""
    geno = ((g + collapsed) > 0).astype(np.float64)
    return rc_correlation_tail(float(geno.sum()), float((geno * geno).sum()), float(pheno.sum()), float((pheno * pheno).sum()),
                               float((geno * pheno).sum()), len(pheno))


def rc_stat_literal(Gf, pheno, corr=rc_correlation_literal):
    """calculateStat (src/Model.h:1503-1539) on the flipped, polymorphic block: (stat, selected columns in selection order)"""
    N, m = Gf.shape
    c = np.zeros(N)
    selected, stat = [], -1.0
    while len(selected) < m:
        max_idx, max_corr = -1, -1.0
        for i in range(m):
            if i in selected:
                continue
            r = corr(Gf[:, i], c, pheno)
            if r > max_corr:
                max_corr, max_idx = r, i
        if max_idx < 0:
            break
        if max_corr > stat:
            stat = max_corr
            selected.append(max_idx)
            c = np.where(c + Gf[:, max_idx] > 0, 1.0, c)          # combine()
        else:
            break
    return stat, selected


# ---- RareCover: the form the kernel uses --------------------------------------------------------------------------------------
def rc_bitsets(Gf):
    """the K samples that carry any column (g > 0), numbered in sample order, and every column as a bitset over them"""
    carr = Gf > 0
    samp = np.nonzero(carr.any(1))[0]
    bits = []
    for j in range(Gf.shape[1]):
        b = 0
        for k in np.nonzero(carr[samp, j])[0]:
            b |= 1 << int(k)
        bits.append(b)
    return samp, bits


def rc_stat_bitset(bits, Y, cases, N):
    """the greedy cover from n_g = popc(c | B_j), n_gp = popc((c | B_j) & Y), cases and N"""
    m = len(bits)
    c, selected, stat = 0, [], -1.0
    while len(selected) < m:
        max_idx, max_corr = -1, -1.0
        for j in range(m):
            if j in selected:
                continue
            u = c | bits[j]
            n_g, n_gp = float(popcount(u)), float(popcount(u & Y))
            r = rc_correlation_tail(n_g, n_g, float(cases), float(cases), n_gp, N)
            if r > max_corr:
                max_corr, max_idx = r, j
        if max_idx < 0 or not max_corr > stat:
            break
        stat = max_corr
        selected.append(max_idx)
        c |= bits[max_idx]
    return stat, selected


def y_bits(samp, pheno):
    Y = 0
    for k in np.nonzero(pheno[samp] == 1.0)[0]:
        Y |= 1 << int(k)
    return Y


def rarecover_statement(G, y, nperm, alpha, rand=vt.orc_rand, form="bitset", shuffles=True):
    """RareCoverTest::fit on the unflipped block G.  form: "literal" (dense vectors) or "bitset"; both give the same bits
    (test_rarecover_bitset_form_equals_the_literal_statement_bit_for_bit)."""
    Gf = orc.flip_poly(np.asfortranarray(G, dtype=np.float64))[0]
    if Gf.shape[1] == 0 or not valid_phenotype(y):
        return {"fit_ok": False, "n_poly": Gf.shape[1]}
    pheno = np.asarray(y, dtype=np.float64).copy()
    N = len(pheno)
    cases = int(pheno.sum())
    samp, bits = rc_bitsets(Gf)
    if form == "bitset":
        stat_of = lambda p: rc_stat_bitset(bits, y_bits(samp, p), cases, N)
    else:
        stat_of = lambda p: rc_stat_literal(Gf, p)
    stat, selected = stat_of(pheno)
    st = vt.Stop(nperm, alpha, stat)
    perms = []
    while shuffles and st.next():
        vt.permute(pheno, rand)
        s = stat_of(pheno)[0]
        st.add(s)
        perms.append(s)
    return {"fit_ok": True, "n_poly": Gf.shape[1], "n_carrier": len(samp), "n_selected": len(selected), "selected": selected,
            "stat": stat, "actual": st.actual, "num_x": int(st.num_x), "num_eq": int(st.num_eq), "pvalue": st.pvalue(),
            "perms": perms}


# ---- Madsen-Browning: the literal statement --------------------------------------------------------------------------------------
def mb_weights_literal(Gf, pheno):
    """madsonBrowningCollapse's weights (src/Model.cpp:155-175): the frequency among the controls, sums in sample order; 0 = skipped"""
    N, m = Gf.shape
    ctrl = pheno != 1.0
    w = np.zeros(m)
    for j in range(m):
        g = Gf[ctrl, j]
        g = g[g >= 0]
        freq = 1.0 * (vt.seq_sum(g) + 1) / (2 * len(g) + 2)
        if freq <= 0.0 or freq >= 1.0:
            continue
        w[j] = 1.0 / math.sqrt(freq * (1.0 - freq) * N)
    return w


def mb_collapse_literal(Gf, w):
    out = np.zeros(Gf.shape[0])
    for j in range(Gf.shape[1]):
        if w[j] != 0.0:
            out = out + Gf[:, j] * w[j]
    return out


def mb_stat_literal(Gf, pheno):
    """the collapsed column under this phenotype through the two-argument TestCovariate with m = 1 (sums in sample order; the 1 x 1
    LLT solve is 1 / l / l with l = sqrt(V)); None where the reference returns false (stat < 0)"""
    N = Gf.shape[0]
    X = mb_collapse_literal(Gf, mb_weights_literal(Gf, pheno))
    y_mean = vt.seq_sum(pheno) / N
    y_var = y_mean * (1.0 - y_mean)
    U = vt.seq_sum(X * (pheno - y_mean))
    SS = (vt.seq_sum(X * X) - vt.seq_sum(X) * vt.seq_sum(X) / N) * y_var
    ell = math.sqrt(SS) if SS > 0 else float("nan")
    S = (U * (1.0 / ell / ell)) * U
    return None if S < 0 else S


# ---- Madsen-Browning: the form the kernels use -----------------------------------------------------------------------------------
def mb_gram_parts(Gf):
    """per gene: the entry lists, the column sums and K = G'G"""
    ent = [np.nonzero(Gf[:, j])[0] for j in range(Gf.shape[1])]
    val = [Gf[e, j] for j, e in enumerate(ent)]
    AC = np.array([vt.seq_sum(v) for v in val])
    return ent, val, AC, Gf.T @ Gf


def mb_stat_gram(parts, pheno, N, detail=False):
    ent, val, AC, K = parts
    m = len(ent)
    cases = float((pheno == 1.0).sum())
    ybar = cases / N
    A = np.array([vt.seq_sum(val[j] * pheno[ent[j]]) for j in range(m)])
    w = np.zeros(m)
    for j in range(m):
        f = ((AC[j] - A[j]) + 1.0) / (2.0 * (N - cases) + 2.0)
        if not (f <= 0.0 or f >= 1.0):
            w[j] = 1.0 / math.sqrt(f * (1.0 - f) * N)
    S1 = float(w @ AC)
    U = float(w @ A) - ybar * S1
    S2 = float(w @ K @ w)
    V = ybar * (1.0 - ybar) * (S2 - S1 / N * S1)
    stat = U * U / V
    if detail:
        return stat, dict(A=A, AC=AC, w=w, S1=S1, S2=S2, U=U, V=V, ybar=ybar, cases=cases)
    return stat


def mb_bound(Gf, parts, pheno):
    """Forward bound on |Gram form - literal statement| for one phenotype, to first order in u = 2^-53.  Both forms evaluate the same
    real number from the same data; they differ in the order of their sums and in forming the controls' allele count as AC_j - A_j.
      * no sum of either form has more non-zero terms than n = nnz + m^2 + 16 (a zero term adds no error), so a sum of terms t_i is
        off by at most e sum |t_i|, e = n u / (1 - n u);
      * the controls' count: off by e (AC_j + A_j) where it is a difference, so f_j by the relative e_f = e (AC_j + A_j + 1) /
        (AC_j - A_j + 1) + 4 u, and w_j = 1 / sqrt(f (1 - f) N) by e_w = e_f (1 + f / (1 - f)) / 2 + 4 u (the largest over j is used);
      * U = sum_j w_j (A_j - ybar AC_j): off by (e_w + e + 4 u) T, T = sum_j w_j (A_j (1 - ybar) + ybar (AC_j - A_j)) the sum of the
        absolute terms;
      * S2 (non-negative terms, two weights each) by the relative 2 e_w + e + 4 u, S1 by e_w + e + 4 u, so V = ybar (1 - ybar) (S2 -
        S1^2 / N) by the relative e_V = ((2 e_w + e + 4 u) S2 + 2 (e_w + e + 4 u) S1^2 / N) / (S2 - S1^2 / N) + 4 u;
      * stat = U^2 / V: |d stat| <= stat e_V + (2 |U| dU + dU^2) / V + 4 u stat per form; twice that for the two forms, and 1 % on
        top for the second-order terms."""
    stat, d = mb_stat_gram(parts, pheno, Gf.shape[0], detail=True)
    N, m = Gf.shape
    u = 2.0 ** -53
    n = int(np.count_nonzero(Gf)) + m * m + 16
    e = n * u / (1 - n * u)
    used = d["w"] != 0
    A, AC, w = d["A"][used], d["AC"][used], d["w"][used]
    f = ((AC - A) + 1.0) / (2.0 * (N - d["cases"]) + 2.0)
    e_f = e * (AC + A + 1.0) / (AC - A + 1.0) + 4 * u
    e_w = float(np.max(e_f * (1.0 + f / (1.0 - f)) / 2.0 + 4 * u)) if used.any() else 0.0
    T = float(np.sum(w * (A * (1.0 - d["ybar"]) + d["ybar"] * (AC - A))))
    dU = (e_w + e + 4 * u) * T
    D = d["S2"] - d["S1"] * d["S1"] / N
    e_V = ((2 * e_w + e + 4 * u) * d["S2"] + 2 * (e_w + e + 4 * u) * d["S1"] * d["S1"] / N) / D + 4 * u
    one = stat * e_V + (2 * abs(d["U"]) * dU + dU * dU) / d["V"] + 4 * u * stat
    return 2.02 * one


def mb_observed(Gf, X, y):
    """the observed statistic: the binary score test of the logistic null model y ~ X on the observed collapsed column, what
    TestCovariate(cov, pheno, collapsed) intends (regression/LogisticRegressionScoreTest.cpp:220-302; DESIGN.md on quirk #15)"""
    y = np.asarray(y, dtype=np.float64)
    rc, beta, p, v = orc.fit_logistic(X, y)
    if rc != 0:
        return None
    x = mb_collapse_literal(Gf, mb_weights_literal(Gf, y))
    U = vt.seq_sum(x * (y - p))
    xv = x * v
    t = X.T @ xv
    V = float(x @ xv) - float(t @ np.linalg.solve(X.T @ (X * v[:, None]), t))
    return U * U / V if V > 0 else None


def mb_statement(G, X, y, nperm, alpha, rand=vt.orc_rand, form="gram", obs=None, keep=False):
    """MadsonBrowningTest::fit on the unflipped block G under the null model y ~ X.  obs: compare the permuted statistics with this
    observed value instead (the device's).  form: "gram" or "literal"."""
    Gf = orc.flip_poly(np.asfortranarray(G, dtype=np.float64))[0]
    if Gf.shape[1] == 0 or not valid_phenotype(y):
        return {"fit_ok": False, "n_poly": Gf.shape[1]}
    pheno = np.asarray(y, dtype=np.float64).copy()
    N = len(pheno)
    stat = mb_observed(Gf, X, pheno)
    if stat is None:
        return {"fit_ok": False, "n_poly": Gf.shape[1]}
    parts = mb_gram_parts(Gf)
    st = vt.Stop(nperm, alpha, stat if obs is None else obs)
    perms, bounds, failed, ok = [], [], 0, True
    while st.next():
        vt.permute(pheno, rand)
        s = mb_stat_gram(parts, pheno, N) if form == "gram" else mb_stat_literal(Gf, pheno)
        if s is None or s < 0:                                     # src/Model.h:1291-1299
            if failed < 10:
                failed += 1
                continue
            ok = False
            break
        st.add(s)
        if keep:
            perms.append(s)
            bounds.append(mb_bound(Gf, parts, pheno))
    return {"fit_ok": ok, "n_poly": Gf.shape[1], "n_entries": int(np.count_nonzero(Gf)), "stat": stat, "actual": st.actual,
            "num_x": int(st.num_x), "num_eq": int(st.num_eq), "pvalue": st.pvalue(), "perms": perms, "bounds": bounds}


# ---- the rows the reference prints ------------------------------------------------------------------------------------------------
def perm_fields(nperm, res):
    if not res["fit_ok"]:                                           # the Permutation fields after reset()
        return "%d\t0\t%s\t0\t0\t%s" % (nperm, vt.float_to_string(0.0), vt.float_to_string(1.0))
    return "%d\t%d\t%s\t%d\t%d\t%s" % (nperm, res["actual"], vt.float_to_string(res["stat"]), res["num_x"], res["num_eq"],
                                       vt.float_to_string(res["pvalue"]))


def rarecover_row(nperm, res):
    return ("%d" % res["n_selected"] if res["fit_ok"] else "NA") + "\t" + perm_fields(nperm, res)


# ---- genes ------------------------------------------------------------------------------------------------------------------------
def gene(rng, N, M, lo=-2.2, hi=-1.0, ties=False, flip=False, imputed=False):
    maf = 10 ** rng.uniform(lo, hi, M)
    G = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    if ties:
        G[:, 1::3] = G[:, 0::3][:, :G[:, 1::3].shape[1]]           # duplicated columns: equal correlations, the first one wins
    if flip:
        G[:, 0] = 2.0 - G[:, 0]
    if imputed:
        G[rng.random(N) < 0.02, M - 1] = 0.37                      # a carrier here (g > 0), not in --vt price ((int)g > 0)
    return np.asfortranarray(G)


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_rarecover_vector_sums_equal_the_sample_loop():
    rng = np.random.default_rng(2)
    G = gene(rng, 90, 5, lo=-1.5, hi=-0.8, imputed=True)
    y = (rng.random(90) < 0.4).astype(np.float64)
    Gf = orc.flip_poly(G)[0]
    a = rc_stat_literal(Gf, y, corr=rc_correlation_loop)
    assert a == rc_stat_literal(Gf, y) and a[0] > 0


def test_rarecover_bitset_form_equals_the_literal_statement_bit_for_bit():
    rng = np.random.default_rng(11)
    cases = ((300, 12, dict(ties=True)), (257, 9, dict(flip=True, imputed=True)), (120, 1, {}), (400, 40, dict(ties=True, imputed=True)),
             (64, 3, dict(lo=-1.0, hi=-0.5)))
    seen_tie = seen_zero = False
    for N, M, kw in cases:
        G = gene(rng, N, M, **kw)
        Gf, fl, kp = orc.flip_poly(G)
        if kw.get("flip"):
            assert fl[0] == 1
        samp, bits = rc_bitsets(Gf)
        if kw.get("imputed"):
            j = Gf.shape[1] - 1
            rows = np.nonzero(Gf[:, j] == 0.37)[0]
            assert len(rows) and all(bits[j] >> int(np.searchsorted(samp, i)) & 1 for i in rows)     # 0.37 counts as a carrier
        for trial in range(6):
            y = (rng.random(N) < (0.5 if trial else 0.3)).astype(np.float64)
            lit = rc_stat_literal(Gf, y)
            bit = rc_stat_bitset(bits, y_bits(samp, y), int(y.sum()), N)
            assert lit == bit, (N, M, trial, lit, bit)                                              # statistic AND selected set
            for j in lit[1]:                                  # of identical columns (equal correlations) the first one is taken
                twins = [k for k in range(Gf.shape[1]) if k != j and (Gf[:, k] == Gf[:, j]).all()]
                assert all(k > j for k in twins)
                seen_tie = seen_tie or bool(twins)
    # v < 1e-10: a column every sample carries gives var_g = 0, its correlation is 0.0 and a later column can still win or tie
    N = 50
    Gf = np.zeros((N, 2), order="F")
    Gf[:, 0] = 1.0
    Gf[::5, 1] = 1.0
    y = np.zeros(N)
    y[::5] = 1.0
    assert rc_correlation_literal(Gf[:, 0], np.zeros(N), y) == 0.0
    samp, bits = rc_bitsets(Gf)
    lit, bit = rc_stat_literal(Gf, y), rc_stat_bitset(bits, y_bits(samp, y), int(y.sum()), N)
    assert lit == bit and lit[1] == [1] and lit[0] == 1.0
    seen_zero = True
    assert seen_tie and seen_zero
    # whole fits, shuffles included, from one stream position
    G = gene(rng, 150, 6, ties=True)
    y = (rng.random(150) < 0.4).astype(np.float64)
    orc.rand_seed(5)
    a = rarecover_statement(G, y, 60, 0.2, form="literal")
    orc.rand_seed(5)
    b = rarecover_statement(G, y, 60, 0.2, form="bitset")
    orc.rand_seed(1)
    assert a == b and a["actual"] > 0
    assert rarecover_statement(np.zeros((50, 3)), y[:50], 10, 0.5)["fit_ok"] is False
    assert rarecover_statement(G, rng.normal(size=150), 10, 0.5)["fit_ok"] is False


def test_madsen_browning_gram_form_agrees_with_the_literal_statement_within_the_forward_bound():
    rng = np.random.default_rng(21)
    worst = 0.0
    for N, M, kw in ((300, 12, {}), (257, 9, dict(flip=True, imputed=True)), (120, 1, {}), (500, 40, dict(ties=True))):
        G = gene(rng, N, M, **kw)
        Gf = orc.flip_poly(G)[0]
        parts = mb_gram_parts(Gf)
        for trial in range(8):
            y = (rng.random(N) < 0.4).astype(np.float64)
            lit, gram, bound = mb_stat_literal(Gf, y), mb_stat_gram(parts, y, N), mb_bound(Gf, parts, y)
            assert lit is not None and abs(gram - lit) <= bound, (N, M, trial, lit, gram, bound)
            assert bound <= 1e-9 * max(lit, 1e-3)                    # (the bound is not vacuous)
            worst = max(worst, abs(gram - lit) / bound)
    print("largest |gram - literal| / bound", worst)
    # hard calls: A_j and AC_j are exact integers, equal configurations give bit-equal statistics
    G = gene(rng, 200, 5)
    Gf = orc.flip_poly(G)[0]
    parts = mb_gram_parts(Gf)
    y = (rng.random(200) < 0.5).astype(np.float64)
    y2 = y.copy()
    free = np.nonzero((Gf == 0).all(1))[0]
    i, j = free[y[free] == 1][0], free[y[free] == 0][0]              # swap a case and a control who carry nothing
    y2[i], y2[j] = 0.0, 1.0
    assert mb_stat_gram(parts, y, 200) == mb_stat_gram(parts, y2, 200)


def test_madsen_browning_observed_statistic_is_the_score_test_of_the_oracle():
    """U^2 / V of the statement = the statistic behind the oracle's MetaScore p-value of the collapsed column (two covariates)"""
    from scipy import stats as sps
    rng = np.random.default_rng(4)
    N = 600
    G = gene(rng, N, 8, lo=-1.8, hi=-1.0)
    X = np.asfortranarray(np.column_stack([np.ones(N), rng.normal(size=(N, 2))]))
    y = (rng.random(N) < 1 / (1 + np.exp(-(0.3 * X[:, 1] - 0.4)))).astype(np.float64)
    Gf = orc.flip_poly(G)[0]
    stat = mb_observed(Gf, X, y)
    x = mb_collapse_literal(Gf, mb_weights_literal(Gf, y))
    rc, o = orc.metascore(np.asfortranarray(x.reshape(-1, 1)), X, y, 1)
    assert rc == 0 and o["ok"][0]
    assert abs(o["U"][0] ** 2 / o["V"][0] - stat) <= 1e-9 * stat
    assert abs(sps.chi2.sf(stat, 1) - o["p"][0]) <= 1e-9 * o["p"][0]


def _layout(rec_name, R, names):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rvtests_amd.h"\nint main(void) {\n  printf("%%zu", sizeof(%s));\n' % rec_name
    assert [f[0] for f in R._fields_] == names
    for n in names:
        src += '  printf(" %%zu", offsetof(%s, %s));\n' % (rec_name, n)
    src += "  return 0;\n}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(R)] + [getattr(R, n).offset for n in names]


def test_library_exports_both_entries_and_the_record_layouts_match_the_header():
    import rvtests_amd
    L = rvtests_amd.load_library()
    assert hasattr(L, "rvt_rarecover_blocks") and hasattr(L, "rvt_mb_blocks")
    perm = ["num_perm", "actual_perm", "num_greater", "num_equal", "perm_pvalue"]
    _layout("rvt_rarecover_result", rvtests_amd.RareCoverResult, ["fit_ok", "n_poly", "n_carrier", "n_selected", "stat"] + perm)
    _layout("rvt_mb_result", rvtests_amd.MbResult, ["fit_ok", "n_poly", "n_entries", "stat"] + perm)


def write_input(path, y, binary, genes, cov=None):
    import struct
    ncov = 0 if cov is None else cov.shape[1]
    with open(path, "wb") as f:
        f.write(struct.pack("<qiii", len(y), ncov, int(binary), len(genes)))
        f.write(np.ascontiguousarray(y, dtype="<f8").tobytes())
        if ncov:
            f.write(np.asfortranarray(cov, dtype="<f8").tobytes(order="F"))
        for G in genes:
            f.write(struct.pack("<i", G.shape[1]))
            f.write(np.ascontiguousarray(G.sum(0) / (2.0 * len(y)), dtype="<f8").tobytes())
            f.write(np.asfortranarray(G, dtype="<f8").tobytes(order="F"))


def run_burden_driver(path, spec, perm_exact=None):
    env = dict(os.environ)
    env.pop("RVT_PERM_EXACT", None)
    env.pop("RVT_DRIVER_VT", None)
    if perm_exact is not None:
        env["RVT_PERM_EXACT"] = "1" if perm_exact else "0"
    p = subprocess.run([DRIVER, path, "-", spec], capture_output=True, text=True, timeout=900, env=env)
    return p.returncode, p.stdout, p.stderr


def split_outputs(out):
    """{file name: its lines} of the driver's "== name" sections"""
    files, cur = {}, None
    for ln in out.split("\n")[:-1]:
        if ln.startswith("== "):
            cur = files.setdefault(ln[3:], [])
        else:
            cur.append(ln)
    return files


def test_model_manager_accepts_rarecover_and_mb_and_the_headers_are_the_reference_s(tmp_path):
    vt._ensure_driver()
    rng = np.random.default_rng(1)
    G = gene(rng, 60, 4)
    path = str(tmp_path / "in.bin")
    # quantitative trait: RareCover's header as ever, Madsen-Browning's is "Pvalue\n" + "\n" (src/Model.h:1311-1320): an empty line
    write_input(path, rng.normal(size=60), 0, [G])
    rc, out, err = run_burden_driver(path, "rarecover[nPerm=200,alpha=0.1],mb")
    assert rc == 0, err
    assert out.startswith("== out.RareCover.assoc\n")
    f = split_outputs(out)
    assert f["out.RareCover.assoc"][0] == SITE_HEADER + "NumIncludeMarker\t" + PERM_HEADER
    assert f["out.RareCover.assoc"][1] == "gene0\t60\t4\t\tNA\t200\t0\t0\t0\t0\t1"          # NumPerm from the parsed nPerm
    assert f["out.MadsonBrowning.assoc"] == [SITE_HEADER + "Pvalue", "", "gene0\t60\t4\t\tNA"]
    # binary trait: perm.writeHeader writes no line end, the "\n" that follows is the only one (src/Model.h:1314-1319)
    write_input(path, (rng.random(60) < 0.5).astype(np.float64), 1, [G])
    rc, out, err = run_burden_driver(path, "rarecover,mb")
    assert rc == 0, err
    f = split_outputs(out)
    assert f["out.MadsonBrowning.assoc"][0] == SITE_HEADER + PERM_HEADER and len(f["out.MadsonBrowning.assoc"]) == 2
    assert f["out.MadsonBrowning.assoc"][1].split("\t")[4] == "10000"                       # default nPerm
    assert f["out.RareCover.assoc"][1].split("\t")[5] == "10000"
    rc, out, err = run_burden_driver(path, "nosuch")
    assert rc == 1 and "Unknown model name: nosuch" in err
