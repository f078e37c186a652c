"""GPU: the single-variant tests for related samples — rvt_score_block_fam as famScore, rvt_lrt_block_fam, rvt_fit_grammar_null
and rvt_grammar_block — held to the numpy statements of tests/test_single_fam_cpu.py, and the driver's rows."""
import numpy as np
import pytest

import synth
from test_fam_cpu import make_family_case
from test_single_fam_cpu import (HEADERS, GRID, fam_driver_case, fam_lrt, fam_score, grammar_null_given_delta,
                                 grammar_objective, grammar_test, is_monomorphic, run_single_fam)
from test_host_driver import _ensure_driver

pytestmark = pytest.mark.gpu
MAXV = 1024  # RVT_MAX_VARIANTS


@pytest.fixture
def engine_factory():
    import rvtests_amd
    made = []

    def make():
        e = rvtests_amd.Engine(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


def columns(N, seed):
    """Hard calls, mean-imputed, dosage, monomorphic and rare columns."""
    rng = np.random.default_rng(seed)
    G = synth.make_gene(N, 10, seed=seed, missing=0.02, common=True, mono=True)[1]
    dos = np.clip(rng.binomial(2, 0.3, (N, 4)) + rng.normal(0, 0.15, (N, 4)), 0, 2)
    rare = np.zeros((N, 2))
    rare[rng.integers(0, N, 2), 0] = 1.0
    rare[rng.integers(0, N, 1), 1] = 2.0
    mono = np.full((N, 2), 1.0)
    return np.column_stack([G, dos, rare, mono])


def grm_case(N, d, seed):
    """A dense kinship: the GRM of random genotypes (U dense, small eigenvalues)."""
    rng = np.random.default_rng(seed)
    m = 3 * N
    Z = rng.binomial(2, rng.uniform(0.05, 0.5, m), (N, m)).astype(float)
    Z = (Z - Z.mean(0)) / np.maximum(Z.std(0), 1e-9)
    K = Z @ Z.T / m
    S, U = np.linalg.eigh(K)
    U = U.astype(np.float32).astype(np.float64)
    S = S.astype(np.float32).astype(np.float64)
    X = np.column_stack([np.ones(N)] + [rng.standard_normal(N) for _ in range(d - 1)])
    L = np.linalg.cholesky(K + 1e-6 * np.eye(N))
    y = X @ rng.standard_normal(d) * 0.3 + np.sqrt(0.5) * (L @ rng.standard_normal(N)) + np.sqrt(0.5) * rng.standard_normal(N)
    return N, K, U, S, X, y


def rel(a, b, tol):
    return abs(a - b) <= tol * abs(b) + 1e-300


def check_lrt(r, G, U, S, X, y, nul):
    ux, uy = U.T @ X, U.T @ y
    fitted = 0
    for h in range(G.shape[1]):
        ok, nll, all_, p, af = fam_lrt(G[:, h], ux, uy, U, S, nul.delta, nul.sigma2_g)
        assert r["ok"][h] == ok, h
        assert rel(r["af"][h], af, 1e-8), h
        if ok != 1:
            continue
        fitted += 1
        assert rel(r["null_ll"][h], nll, 1e-8)
        assert rel(r["alt_ll"][h], all_, 1e-8), (h, r["alt_ll"][h], all_)
        assert rel(r["p"][h], p, 1e-6), (h, r["p"][h], p)
    return fitted


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_lrt_and_score_block_fam_match_statements(engine_factory, d):
    N, K, U, S, X, y = make_family_case(60, d, 300 + d)
    eng = engine_factory()
    eng.set_kinship(U, S)
    nul = eng.fit_fam_null(X, y)
    G = columns(N, 7 + d)
    ptr = eng.upload_block(G)
    assert check_lrt(eng.lrt_block_fam(ptr, G.shape[1]), G, U, S, X, y, nul) >= 8
    r = eng.score_block_fam(ptr, G.shape[1], 0)
    beta = np.array([nul.beta[k] for k in range(d)])
    ux, uy = U.T @ X, U.T @ y
    for h in range(G.shape[1]):
        assert r["ok"][h] == (0 if is_monomorphic(G[:, h]) else 1)
        if not r["ok"][h]:
            continue
        Ust, V, p, af = fam_score(G[:, h], ux, uy, U, S, nul.delta, nul.sigma2_g, beta)
        assert rel(r["U"][h], Ust, 1e-8) and rel(r["V"][h], V, 1e-8) and rel(r["p"][h], p, 1e-6)
        assert rel(r["af"][h], af, 1e-8)
    eng.free_block(ptr)


def check_grammar(eng, G, U, S, X, y, af_kinship=0):
    N = len(y)
    gn = eng.fit_grammar_null(X, y)
    ux, uy = U.T @ X, U.T @ y
    lls = np.array([grammar_objective(t, ux, uy, S)[0] for t in GRID])
    assert gn.max_index == int(np.nanargmax(lls))
    mi = gn.max_index
    if 0 < mi < 100:
        lo, hi = GRID[mi - 1], GRID[mi + 1]
        assert lo < gn.delta < hi
        fine = np.linspace(lo, hi, 2001)
        best = max(grammar_objective(t, ux, uy, S)[0] for t in fine)
        assert grammar_objective(gn.delta, ux, uy, S)[0] >= best - 1e-3   # Brent stops at a 1e-3 bracket
        ssr = grammar_objective(gn.delta, ux, uy, S)[1]
        assert gn.sigma2_g == pytest.approx(ssr / N, rel=1e-2)           # the last evaluation's, near the optimum
    gamma, ty, ysy = grammar_null_given_delta(X, y, U, S, gn.delta, gn.sigma2_g)
    assert rel(gn.gamma, gamma, 1e-8) and rel(gn.ySigmaY, ysy, 1e-7)
    ptr = eng.upload_block(G)
    r = eng.grammar_block(ptr, G.shape[1], af_kinship)
    for h in range(G.shape[1]):
        kin = (U, S, gn.delta) if af_kinship else ()
        ok, af, b, bv, p = grammar_test(G[:, h], gamma, ty, ysy, *kin)
        assert r["ok"][h] == ok
        assert rel(r["af"][h], af, 1e-8), (h, r["af"][h], af)
        if ok:
            assert rel(r["beta"][h], b, 1e-7), (h, r["beta"][h], b)
            assert rel(r["beta_var"][h], bv, 1e-7)
            assert rel(r["p"][h], p, 1e-6), (h, r["p"][h], p)
    eng.free_block(ptr)
    return r


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("af_kinship", [0, 1])
def test_grammar_matches_statement(engine_factory, d, af_kinship):
    N, K, U, S, X, y = make_family_case(60, d, 400 + d)
    eng = engine_factory()
    eng.set_kinship(U, S)
    eng.fit_fam_null(X, y)
    check_grammar(eng, columns(N, 17 + d), U, S, X, y, af_kinship)


def test_dense_kinship_case(engine_factory):
    N, K, U, S, X, y = grm_case(1200, 3, 5)
    eng = engine_factory()
    eng.set_kinship(U, S)
    nul = eng.fit_fam_null(X, y)
    G = columns(N, 3)
    ptr = eng.upload_block(G)
    assert check_lrt(eng.lrt_block_fam(ptr, G.shape[1]), G, U, S, X, y, nul) >= 8
    eng.free_block(ptr)
    check_grammar(eng, G, U, S, X, y, 0)
    check_grammar(eng, G, U, S, X, y, 1)


def test_block_wider_than_max_variants(engine_factory):
    N, K, U, S, X, y = make_family_case(50, 2, 91)
    eng = engine_factory()
    eng.set_kinship(U, S)
    nul = eng.fit_fam_null(X, y)
    eng.fit_grammar_null(X, y)
    rng = np.random.default_rng(4)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, MAXV + 77), (N, MAXV + 77)).astype(float)
    ptr = eng.upload_block(G)
    big = eng.lrt_block_fam(ptr, G.shape[1])
    bigg = eng.grammar_block(ptr, G.shape[1], 0)
    eng.free_block(ptr)
    sub = np.ascontiguousarray(G[:, MAXV - 3:MAXV + 5])
    ptr = eng.upload_block(sub)
    small = eng.lrt_block_fam(ptr, sub.shape[1])
    smallg = eng.grammar_block(ptr, sub.shape[1], 0)
    eng.free_block(ptr)
    for k in ("ok", "af", "alt_ll", "p"):    # a variant's numbers do not depend on the block it is in
        assert np.array_equal(big[k][MAXV - 3:MAXV + 5], small[k])
    for k in ("ok", "af", "beta", "beta_var", "p"):
        assert np.array_equal(bigg[k][MAXV - 3:MAXV + 5], smallg[k])
    idx = list(range(0, G.shape[1], 97)) + [G.shape[1] - 1]
    check_lrt({k: v[idx] for k, v in big.items()}, G[:, idx], U, S, X, y, nul)


def test_poisoned_work_spaces(engine_factory, monkeypatch):
    N, K, U, S, X, y = make_family_case(40, 3, 55)
    G = columns(N, 12)
    out = []
    for poison in (None, "255"):
        if poison:
            monkeypatch.setenv("RVT_POISON", poison)
        eng = engine_factory()
        eng.set_kinship(U, S)
        eng.fit_fam_null(X, y)
        eng.fit_grammar_null(X, y)
        ptr = eng.upload_block(G)
        out.append((eng.lrt_block_fam(ptr, G.shape[1]), eng.grammar_block(ptr, G.shape[1], 1)))
        eng.free_block(ptr)
    for a, b in zip(out[0], out[1]):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_driver_rows(tmp_path):
    _ensure_driver()
    path, sites, kin, N, U, S, X, y, G = fam_driver_case(tmp_path)
    rc, sec, err = run_single_fam(path, sites, "famscore,famlrt,famgrammargamma", kin)
    assert rc == 0, err
    import rvtests_amd
    eng = rvtests_amd.Engine(0)
    try:
        eng.set_kinship(U, S)
        nul = eng.fit_fam_null(X, y)
        gn = eng.fit_grammar_null(X, y)
    finally:
        eng.close()
    ux, uy = U.T @ X, U.T @ y
    beta = np.array([nul.beta[k] for k in range(X.shape[1])])
    gamma, ty, ysy = grammar_null_given_delta(X, y, U, S, gn.delta, gn.sigma2_g)
    V = G.shape[1]
    rows = {k: [r.split("\t")[2:] for r in sec[k][1:]] for k in HEADERS}
    for h in range(V):
        g = G[:, h]
        if is_monomorphic(g):                     # fit() failed: the previous row's values again
            assert h > 0
            for k in HEADERS:
                assert rows[k][h] == rows[k][h - 1]
            continue
        Ust, Vs, p, af = fam_score(g, ux, uy, U, S, nul.delta, nul.sigma2_g, beta)
        ok, nll, all_, pl, afl = fam_lrt(g, ux, uy, U, S, nul.delta, nul.sigma2_g)
        okg, afg, bg, bvg, pg = grammar_test(g, gamma, ty, ysy)
        want = {"out.FamScore.assoc": [af, Ust, Vs, p], "out.FamLRT.assoc": [afl, nll, all_, pl],
                "out.FamGrammarGamma.assoc": [afg, bg, bvg, pg]}
        for k, vals in want.items():
            got = [float(x) for x in rows[k][h]]
            for a, b in zip(got, vals):
                assert abs(a - b) <= 1e-5 * abs(b) + 1e-12, (k, h, got, vals)


def large_family_case(n_fam, d, seed):
    """Nuclear families of 4 in sample order, U block diagonal with its eigenpairs sorted by eigenvalue (as an
    eigensolver of the whole kinship returns them): rvt_set_kinship re-orders them by family and reads only the panels
    of U that hold a family's samples."""
    rng = np.random.default_rng(seed)
    N = 4 * n_fam
    blk = np.array([[1, 0, .5, .5], [0, 1, .5, .5], [.5, .5, 1, .5], [.5, .5, .5, 1]])
    s4, u4 = np.linalg.eigh(blk)
    u4 = u4.astype(np.float32).astype(np.float64)
    S = np.tile(s4.astype(np.float32).astype(np.float64), n_fam)
    U = np.zeros((N, N))
    for f in range(n_fam):
        U[4 * f:4 * f + 4, 4 * f:4 * f + 4] = u4
    order = np.argsort(S, kind="stable")
    U, S = np.asfortranarray(U[:, order]), S[order]
    X = np.column_stack([np.ones(N)] + [rng.standard_normal(N) for _ in range(d - 1)])
    fam = np.repeat(rng.standard_normal(n_fam), 4)
    y = X @ rng.standard_normal(d) * 0.3 + np.sqrt(0.4) * fam + np.sqrt(0.6) * rng.standard_normal(N)
    return N, U, S, X, y


def test_large_family_case_structured_path(engine_factory):
    N, U, S, X, y = large_family_case(2000, 3, 17)
    eng = engine_factory()
    eng.set_kinship(U, S)
    assert eng.kinship_structure() < 0.5          # the family-panel path of the rotation and of U v
    nul = eng.fit_fam_null(X, y)
    G = columns(N, 29)
    ptr = eng.upload_block(G)
    assert check_lrt(eng.lrt_block_fam(ptr, G.shape[1]), G, U, S, X, y, nul) >= 8
    eng.free_block(ptr)
    check_grammar(eng, G, U, S, X, y, 0)
    check_grammar(eng, G, U, S, X, y, 1)
