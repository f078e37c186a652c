"""CPU: `--single famscore,famlrt,famgrammargamma` — numpy statements of the three single-variant tests for related samples
(src/Model.h:525-805) held to the oracle where it has the quantity, the driver's registry, headers and NA rows.  The statements
are what tests/test_gpu_single_fam.py holds the device to."""
import struct
import subprocess

import numpy as np
import pytest

import orc
import synth
from test_fam_cpu import make_family_case
from test_host_driver import DRIVER, _ensure_driver, write_input

PI = 3.1415926535897  # regression/FastLMM.cpp:18, GrammarGamma.cpp:22
GRID = np.exp(-10 + 0.2 * np.arange(101))


def chisq_Q(x):
    return orc.lib().orc_chisq_Q(float(x), 1.0)


def is_monomorphic(g):
    return bool((g == g[0]).all())


def fam_score(g, ux, uy, U, S, delta, sigma2, beta):
    """FastLMM(SCORE, MLE)::TestCovariate + GetAF: (U, V, p, af) of one raw column."""
    lam = np.abs(S)
    w = 1.0 / (lam + delta)
    ug = U.T @ (g - g.mean())
    r = uy - ux @ beta
    Ust = np.sum(ug * r * w) / sigma2
    A = ux.T @ (ux * w[:, None])
    wx = ux * w[:, None]
    V = (ug * w) @ ug - (ug @ wx) @ np.linalg.solve(A, wx.T @ ug)
    V /= sigma2
    p = chisq_Q(Ust * Ust / V) if V > 0 else 1.0
    return Ust, V, p, fam_af(g, U, S)


def fam_af(g, U, S):
    u1 = U.T @ np.ones(len(g))
    u1s = u1 / np.abs(S)
    return 0.5 * (u1s @ (U.T @ g)) / (u1s @ u1)


def lrt_null(ux, uy, S, delta):
    """Null constants of famLRT at delta: A, beta*, r*, SSR*, sum log(|lambda| + delta)."""
    lam = np.abs(S)
    w = 1.0 / (lam + delta)
    A = ux.T @ (ux * w[:, None])
    beta = np.linalg.solve(A, ux.T @ (uy * w))
    r = uy - ux @ beta
    return A, beta, r, np.sum(w * r * r), np.sum(np.log(lam + delta))


def fam_lrt(g, ux, uy, U, S, delta, sigma2):
    """FastLMM(LRT, MLE)::TestCovariate in the Schur form: (ok, null_ll, alt_ll, p, af)."""
    N = len(g)
    if is_monomorphic(g):
        return 0, None, None, None, fam_af(g, U, S)
    lam = np.abs(S)
    w = 1.0 / (lam + delta)
    A, beta, r, ssr0, slog = lrt_null(ux, uy, S, delta)
    ug = U.T @ g
    b = ux.T @ (ug * w)
    sgg = ug @ (ug * w)
    s = sgg - b @ np.linalg.solve(A, b)
    if not s > 1e-12 * sgg:
        return -1, None, None, None, fam_af(g, U, S)
    t = ug @ (w * r)
    alt_s2 = (ssr0 - t * t / s) / N
    null_ll = -0.5 * (N * np.log(2 * PI) + slog + N + N * np.log(sigma2))
    alt_ll = -0.5 * (N * np.log(2 * PI) + slog + N + N * np.log(alt_s2))
    return 1, null_ll, alt_ll, chisq_Q(N * np.log(sigma2 / alt_s2)), fam_af(g, U, S)


def fam_lrt_literal(g, ux, uy, U, S, delta):
    """The reference's own steps: scaled [ux | ug] system, its normal equations, altSSR (FastLMM.cpp:160-190)."""
    lam = np.abs(S)
    ug = U.T @ g
    ax = np.column_stack([ux, ug])
    sc = 1.0 / np.sqrt(lam + delta)
    x, y = ax * sc[:, None], uy * sc
    bet = np.linalg.solve(x.T @ x, x.T @ y)
    return np.sum((uy - ax @ bet) ** 2 / (lam + delta))


def grammar_objective(delta, ux, uy, S):
    """GrammarGamma getBetaSigma2 + getLogLikelihood (GrammarGamma.cpp:159-197): (ll, SSR)."""
    t = S + delta
    if (t < 0).any():
        return np.nan, np.nan
    x, y = ux * np.sqrt(t)[:, None], uy * np.sqrt(t)
    beta = np.linalg.solve(x.T @ x, x.T @ y)
    ssr = np.sum((uy - ux @ beta) ** 2 / t)
    N = len(uy)
    return -0.5 * (N * np.log(2 * PI) + np.sum(np.log(np.abs(t))) + N + N * np.log(ssr)), ssr


def grammar_null_given_delta(X, y, U, S, delta, sigma2_g):
    """gamma, ty, ySigmaY of GrammarGamma::FitNullModel (GrammarGamma.cpp:96-121) for a given delta and sigma2_g."""
    N = len(y)
    gamma = np.sum(S / (S + delta)) / sigma2_g / (N - 1)
    resid = y - X @ np.linalg.solve(X.T @ X, X.T @ y)
    ty = U @ ((U.T @ resid) / (S + delta)) / sigma2_g
    return gamma, ty, resid @ ty


def grammar_test(g, gamma, ty, ysy, U=None, S=None, delta=None):
    """GrammarGamma::TestCovariate + GetAF: (ok, af, beta, beta_var, p); U given: af=kinship."""
    if U is not None:
        u1 = U.T @ np.ones(len(g))
        t = S + delta
        af = 0.5 * np.sum(t * u1 * (U.T @ g)) / np.sum(t * u1 * u1)
    else:
        af = 0.5 * g.mean()
    if is_monomorphic(g):
        return 0, af, None, None, None
    gc = g - g.mean()
    gg = gc @ gc
    gty = gc @ ty
    return 1, af, gty / gg / gamma, ysy / gg / gamma, chisq_Q(gty * gty / gg / gamma)


def grammar_grid(ux, uy, S):
    lls = np.array([grammar_objective(t, ux, uy, S)[0] for t in GRID])
    return lls, int(np.nanargmax(lls))


def _null(X, y, U, S):
    rc, nul = orc.fastlmm_null(X, y, U, S)
    assert rc == 0 and nul.ok
    return nul


@pytest.mark.parametrize("d", [1, 3])
def test_famscore_statement_matches_oracle(d):
    N, K, U, S, X, y = make_family_case(40, d, 11 + d)
    nul = _null(X, y, U, S)
    beta = np.array([nul.beta[k] for k in range(d)])
    G = synth.make_gene(N, 12, seed=5 + d, missing=0.02, common=True, mono=True)[1]
    ux, uy = U.T @ X, U.T @ y
    tested = 0
    for h in range(G.shape[1]):
        rc, o = orc.fam_burden(G[:, [h]], X, y, U, S, nul, 2)
        if rc:
            assert is_monomorphic(G[:, h])
            continue
        tested += 1
        Ust, V, p, af = fam_score(G[:, h], ux, uy, U, S, nul.delta, nul.sigma2, beta)
        assert Ust == pytest.approx(o.U, rel=1e-8, abs=1e-12)
        assert V == pytest.approx(o.V, rel=1e-8)
        assert p == pytest.approx(o.pvalue, rel=1e-6)
        assert af == pytest.approx(o.af, rel=1e-9)
    assert tested >= 4


@pytest.mark.parametrize("d", [1, 2, 4])
def test_famlrt_schur_form_matches_literal_fit(d):
    N, K, U, S, X, y = make_family_case(50, d, 21 + d)
    nul = _null(X, y, U, S)
    ux, uy = U.T @ X, U.T @ y
    G = synth.make_gene(N, 10, seed=31 + d, missing=0.02, common=True, mono=True)[1]
    for h in range(G.shape[1]):
        g = G[:, h]
        ok, null_ll, alt_ll, p, af = fam_lrt(g, ux, uy, U, S, nul.delta, nul.sigma2)
        if ok != 1:
            continue
        ssr = fam_lrt_literal(g, ux, uy, U, S, nul.delta)
        assert alt_ll == pytest.approx(-0.5 * (N * np.log(2 * PI) + np.sum(np.log(np.abs(S) + nul.delta)) + N +
                                               N * np.log(ssr / N)), rel=1e-10)
        assert p == pytest.approx(chisq_Q(2 * (alt_ll - null_ll)), rel=1e-6, abs=1e-300)
    # g in the span of X (a covariate as the genotype) is a failed fit
    if d > 1:
        assert fam_lrt(X[:, 1].copy(), ux, uy, U, S, nul.delta, nul.sigma2)[0] == -1


def test_fastlmm_null_sigma2_is_the_oracles():
    N, K, U, S, X, y = make_family_case(40, 2, 5)
    nul = _null(X, y, U, S)
    ux, uy = U.T @ X, U.T @ y
    A, beta, r, ssr0, slog = lrt_null(ux, uy, S, nul.delta)
    # sigma2 of the null belongs to the last Brent evaluation: close to, not equal to, SSR*/N at the final delta
    assert ssr0 / N == pytest.approx(nul.sigma2, rel=1e-3)


@pytest.mark.parametrize("d", [1, 3])
def test_grammar_grid_and_bracket_optimum(d):
    N, K, U, S, X, y = make_family_case(60, d, 41 + d)
    ux, uy = U.T @ X, U.T @ y
    lls, mi = grammar_grid(ux, uy, S)
    assert 0 < mi < 100
    lo, hi = GRID[mi - 1], GRID[mi + 1]
    fine = np.linspace(lo, hi, 801)
    best = fine[int(np.argmax([grammar_objective(t, ux, uy, S)[0] for t in fine]))]
    assert lo < best < hi
    # the objective uses log SSR: sigma2_g = SSR / N of the optimum
    ll, ssr = grammar_objective(best, ux, uy, S)
    assert np.isfinite(ll) and ssr > 0


def test_grammar_statement_given_delta():
    N, K, U, S, X, y = make_family_case(50, 2, 77)
    delta, s2 = 0.7, 0.9
    gamma, ty, ysy = grammar_null_given_delta(X, y, U, S, delta, s2)
    G = synth.make_gene(N, 8, seed=3, missing=0.0, common=True, mono=True)[1]
    # ty = Sigma^-1 resid with Sigma = sigma2_g U (S + delta) U' = sigma2_g (K + delta I)
    resid = y - X @ np.linalg.solve(X.T @ X, X.T @ y)
    ref = np.linalg.solve(s2 * (K + delta * np.eye(N)), resid)      # (U holds floats: equal to ~1e-7)
    assert np.allclose(ty, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    for h in range(G.shape[1]):
        ok, af, b, bv, p = grammar_test(G[:, h], gamma, ty, ysy)
        assert af == pytest.approx(0.5 * G[:, h].mean())
        if ok:
            assert p == pytest.approx(chisq_Q(b * b / bv * ysy), rel=1e-9)
        ok2, afk, *_ = grammar_test(G[:, h], gamma, ty, ysy, U, S, delta)
        # all eigenvalues of the nuclear-family kinship are positive: the kinship AF is the GLS mean under K + delta I
        V = K + delta * np.eye(N)
        one = np.ones(N)
        assert afk == pytest.approx(0.5 * (one @ V @ G[:, h]) / (one @ V @ one), rel=1e-5)


# ---- driver --------------------------------------------------------------------------------------------------------------
def write_kinship(path, U, S):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", U.shape[0]))
        f.write(np.asfortranarray(U, dtype="<f4").tobytes(order="F"))
        f.write(np.ascontiguousarray(S, dtype="<f4").tobytes())


def run_single_fam(path, sites, single, kin=None):
    args = [DRIVER, path, "-", "-", "-", sites] + ([kin] if kin else []) + ["--single", single]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    sections, cur = {}, None
    for line in p.stdout.splitlines():
        if line.startswith("== "):
            cur = line[3:]
            sections[cur] = []
        elif cur is not None:
            sections[cur].append(line)
    return p.returncode, sections, p.stderr


def fam_driver_case(tmp_path, binary=0, n_fam=30, d=2, seed=9):
    N, K, U, S, X, y = make_family_case(n_fam, d, seed)
    if binary:
        y = (y > np.median(y)).astype(float)
    _, G, af = synth.make_gene(N, 10, seed=seed, missing=0.0, common=True, mono=True)
    G[:, 3] = 1.0                                   # a monomorphic site in the middle
    path = str(tmp_path / "in.bin")
    write_input(path, y, X[:, 1:], binary, [(G[:, :6], af[:6]), (G[:, 6:], af[6:])])
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        for j in range(G.shape[1]):
            f.write("1 %d\n" % (500 + j))
    kin = str(tmp_path / "kin.bin")
    write_kinship(kin, U, S)
    return path, sites, kin, N, U, S, X, y, G


HEADERS = {"out.FamScore.assoc": "CHROM\tPOS\tAF\tU.Stat\tV.Stat\tPvalue",
           "out.FamLRT.assoc": "CHROM\tPOS\tAF\tNullLogLik\tAltLogLik\tPvalue",
           "out.FamGrammarGamma.assoc": "CHROM\tPOS\tAF\tBeta\tBetaVar\tPvalue"}


def test_fam_single_registry_and_headers(tmp_path):
    _ensure_driver()
    path, sites, kin, N, U, S, X, y, G = fam_driver_case(tmp_path)
    rc, sec, err = run_single_fam(path, sites, "famscore,famlrt,famgrammargamma", kin)
    assert rc == 0, err
    assert list(sec) == list(HEADERS)
    for name, h in HEADERS.items():
        assert sec[name][0] == h
        assert len(sec[name]) == 1 + G.shape[1]
        assert [r.split("\t")[1] for r in sec[name][1:]] == [str(500 + j) for j in range(G.shape[1])]
    rc, sec, err = run_single_fam(path, sites, "famGrammarGamma[af=kinship]", kin)
    assert rc == 0, err
    assert list(sec) == ["out.FamGrammarGamma.assoc"]
    assert sec["out.FamGrammarGamma.assoc"][0] == HEADERS["out.FamGrammarGamma.assoc"]


def test_fam_grammar_bad_af_method(tmp_path):
    _ensure_driver()
    path, sites, kin, *_ = fam_driver_case(tmp_path)
    rc, sec, err = run_single_fam(path, sites, "famgrammargamma[af=bogus]", kin)
    assert rc == 1
    assert "FamGrammarGamma cannot recoginized specified kinship calculation method [ bogus ], exit..." in err


def test_fam_single_binary_trait_rows_are_na(tmp_path):
    _ensure_driver()
    path, sites, kin, N, U, S, X, y, G = fam_driver_case(tmp_path, binary=1)
    rc, sec, err = run_single_fam(path, sites, "famscore,famlrt,famgrammargamma", kin)
    assert rc == 0, err
    for name in HEADERS:
        for row in sec[name][1:]:
            assert row.split("\t")[2:] == ["NA"] * 4


def test_fam_single_without_kinship_rows_are_na(tmp_path):
    _ensure_driver()
    path, sites, kin, N, U, S, X, y, G = fam_driver_case(tmp_path)
    rc, sec, err = run_single_fam(path, sites, "famscore,famlrt")
    assert rc == 0, err
    for name in ("out.FamScore.assoc", "out.FamLRT.assoc"):
        for row in sec[name][1:]:
            assert row.split("\t")[2:] == ["NA"] * 4


def test_fam_single_na_rows_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_single_fam.py")
    _ensure_driver()
    path, sites, kin, *_ = fam_driver_case(tmp_path)
    rc, sec, err = run_single_fam(path, sites, "famscore,famlrt,famgrammargamma", kin)
    assert rc == 0, err
    for name in HEADERS:
        for row in sec[name][1:]:
            assert row.split("\t")[2:] == ["NA"] * 4
