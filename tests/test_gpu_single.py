"""GPU: rvt_wald_block (SingleVariantWaldTest on [1, g, cov]) against the numpy statements of tests/test_single_cpu.py (which are
checked against the oracle's regressions there), and `host_driver --single wald,score` rows against the oracle's numbers."""
import os

import numpy as np
import pytest

import orc
import synth
from test_gpu_metacov import engine_factory  # noqa: F401  (fixture)
from test_host_driver import write_input
from test_single_cpu import wald_linear, wald_logistic, design, run_single, write_sites

pytestmark = pytest.mark.gpu

REL = 1e-6   # BASELINE.json north_star tolerance for statistics and p-values


def columns(N, rng, y=None):
    """hard calls, a mean-imputed column, a dosage column, a monomorphic column and a rare variant carried by cases only"""
    maf = rng.uniform(0.02, 0.5, 5)
    G = (rng.random((N, 5, 2)) < maf[None, :, None]).sum(2).astype(float)
    G[:, 1] = np.where(rng.random(N) < 0.05, G[:, 1].mean(), G[:, 1])
    G[:, 2] = np.round(rng.uniform(0, 2, N), 3)
    G[:, 3] = 1.0
    rare = np.zeros(N)
    carriers = np.flatnonzero(y == 1) if y is not None else np.arange(N)
    rare[carriers[:3]] = 1.0
    G[:, 4] = rare
    return G


def statement(binary, g, X, y):
    return wald_logistic(g, X, y) if binary else wald_linear(g, X, y)


def check_against_statement(r, G, X, y, binary, cols):
    for j in cols:
        ok, rounds, beta, se, p = statement(binary, G[:, j], X, y)
        assert r["ok"][j] == ok, j
        assert r["rounds"][j] == rounds, j
        if ok != 1:
            continue
        # beta: relative, with an absolute floor far below the row's largest estimate (a covariate's estimate can be ~0);
        # SE and p: relative alone, element by element (a p of 1e-12 is held to 1e-6 of itself)
        assert np.allclose(r["beta"][j], beta, rtol=REL, atol=1e-9 * np.abs(beta).max()), (j, r["beta"][j], beta)
        for got, want in ((r["se"][j], se), (r["p"][j], p)):
            assert (np.abs(got - want) <= REL * np.abs(want)).all(), (j, got, want)


@pytest.mark.parametrize("binary", [0, 1])
@pytest.mark.parametrize("N,d", [(1500, 1), (1500, 3), (20000, 5), (1500, 16)])
def test_wald_block_matches_statement(engine_factory, binary, N, d):
    rng = np.random.default_rng(1000 * binary + N + d)
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=N + d + binary)
    G = columns(N, rng, y if binary else None)
    eng = engine_factory()
    eng.fit_null(binary, X, y)
    ptr = eng.upload_block(G)
    r = eng.wald_block(ptr, G.shape[1])
    assert r["beta"].shape == (G.shape[1], d)
    check_against_statement(r, G, X, y, binary, range(G.shape[1]))
    assert r["ok"][3] == 0                              # monomorphic
    r2 = eng.wald_block(ptr, G.shape[1])                # the same bits again
    for k in ("ok", "rounds", "beta", "se", "p"):
        assert np.array_equal(r[k], r2[k]), k
    eng.free_block(ptr)


@pytest.mark.parametrize("binary", [0, 1])
def test_wald_block_more_than_one_launch_chunk(engine_factory, binary):
    """V > 4 096: every column's fit depends on the column alone, so copies of a column give the same bits wherever they lie."""
    N, d = 1500, 3
    rng = np.random.default_rng(77 + binary)
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=5 + binary)
    base = columns(N, rng, y if binary else None)
    reps = 4150 // base.shape[1] + 1
    G = np.tile(base, (1, reps))[:, :4150].copy(order="F")
    eng = engine_factory()
    eng.fit_null(binary, X, y)
    ptr = eng.upload_block(G)
    r = eng.wald_block(ptr, G.shape[1])
    check_against_statement(r, G, X, y, binary, range(base.shape[1]))
    for j in range(G.shape[1]):
        b = j % base.shape[1]
        for k in ("ok", "rounds", "beta", "se", "p"):
            assert np.array_equal(r[k][j], r[k][b]), (j, k)
    eng.free_block(ptr)


def test_wald_block_large_binary_small_p(engine_factory):
    N, d = 200000, 4
    rng = np.random.default_rng(9)
    X, y, res, v, s2 = synth.make_null(N, d, 1, seed=21)
    G = (rng.random((N, 3, 2)) < np.array([0.3, 0.05, 0.01])[None, :, None]).sum(2).astype(float)
    G[:, 0] += (y == 1) * (rng.random(N) < 0.15)            # strongly associated: p < 1e-10
    eng = engine_factory()
    eng.fit_null(1, X, y)
    ptr = eng.upload_block(G)
    r = eng.wald_block(ptr, G.shape[1])
    check_against_statement(r, G, X, y, 1, range(G.shape[1]))
    assert r["p"][0, 0] < 1e-10
    A = design(G[:, 0], X)
    rc, b, p, vv = orc.fit_logistic(A, y)
    assert rc == 0 and np.allclose(r["beta"][0], b[1:], rtol=REL)
    eng.free_block(ptr)


@pytest.mark.parametrize("binary", [0, 1])
def test_wald_block_poisoned_work_spaces(monkeypatch, engine_factory, binary):
    """RVT_POISON=255 before the context exists: the slot arenas and the Wald work space start as 0xff bytes; the
    results are the statement's and the same bits as from a context without poison."""
    N, d = 1500, 3
    rng = np.random.default_rng(202 + binary)
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=17 + binary)
    G = columns(N, rng, y if binary else None)
    out = []
    for poison in ("255", None):
        if poison:
            monkeypatch.setenv("RVT_POISON", poison)
        else:
            monkeypatch.delenv("RVT_POISON", raising=False)
        eng = engine_factory()
        eng.fit_null(binary, X, y)
        ptr = eng.upload_block(G)
        out.append(eng.wald_block(ptr, G.shape[1]))
        eng.free_block(ptr)
    check_against_statement(out[0], G, X, y, binary, range(G.shape[1]))
    for k in ("ok", "rounds", "beta", "se", "p"):
        assert np.array_equal(out[0][k], out[1][k]), k


def test_wald_block_needs_fit_null(engine_factory):
    import rvtests_amd
    N, d = 500, 2
    X, y, res, v, s2 = synth.make_null(N, d, 1, seed=3)
    eng = engine_factory()
    with pytest.raises(rvtests_amd.RvtError):
        eng.wald_block(1, 4)
    eng.set_null(1, X, res, v)                  # a caller's null model: no estimates, no y
    G = np.random.default_rng(1).integers(0, 3, (N, 4)).astype(float)
    ptr = eng.upload_block(G)
    with pytest.raises(rvtests_amd.RvtError, match="rvt_fit_null"):
        eng.wald_block(ptr, 4)
    eng.free_block(ptr)


def _f6(x):
    return float("%.6g" % x)


@pytest.mark.parametrize("binary", [0, 1])
def test_driver_single_rows_match_oracle(tmp_path, binary):
    N, d = 1500, 3
    rng = np.random.default_rng(31 + binary)
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=41 + binary)
    G = columns(N, rng, y if binary else None)[:, [0, 3, 1, 2]]   # the monomorphic site follows a fitted one
    path = str(tmp_path / "in.bin")
    write_input(path, y, X[:, 1:], binary, [(G, np.full(G.shape[1], 0.1))])
    sites = str(tmp_path / "sites.txt")
    write_sites(sites, G.shape[1])
    rc, sec, err = run_single(path, sites, "wald,score")
    assert rc == 0, err
    rows = [r.split("\t") for r in sec["out.SingleWald.assoc"][1:]]
    assert len(rows) == G.shape[1] * d
    prev = ["NA"] * 3
    for j in range(G.shape[1]):
        ok, rounds, beta, se, p = statement(binary, G[:, j], X, y)
        for k in range(d):
            f = rows[j * d + k]
            assert f[:3] == ["1", str(1000 + j), "1:%d" % (1000 + j) if k == 0 else "cov%d" % k]
            if ok == 1:
                for s, want in zip(f[3:], (beta[k], se[k], p[k])):
                    assert abs(float(s) - _f6(want)) <= 2e-6 * abs(_f6(want)) + 1e-300, (j, k, s, want)
            else:                                    # Result never cleared: the previous row's values again
                assert f[3:] == prev
            prev = f[3:]
    # score rows: LinearRegressionScoreTest / LogisticRegressionScoreTest units from the MetaScore oracle
    rcs, o = orc.metascore(G, X, y, binary)
    assert rcs == 0
    srows = [r.split("\t") for r in sec["out.SingleScore.assoc"][1:]]
    for j, f in enumerate(srows):
        if not o["ok"][j]:
            assert f[3:] == ["NA"] * 7
            continue
        sig2 = 1.0 if binary else o["sigma2"]
        U = o["U"][j] * sig2
        V = o["V"][j] * sig2 * sig2
        want = [U, V, U * U / V]
        for s, w in zip(f[3:6], want):
            assert abs(float(s) - _f6(w)) <= 2e-6 * abs(_f6(w)), (j, s, w)
        assert f[6] == ("+" if U > 0 else "-")
        eff, sev = (U / V, 1.0 / np.sqrt(V)) if binary else (o["effect"][j], sig2 / np.sqrt(V))
        assert abs(float(f[7]) - _f6(eff)) <= 2e-6 * abs(_f6(eff))
        assert abs(float(f[8]) - _f6(sev)) <= 2e-6 * abs(_f6(sev))
        assert abs(float(f[9]) - _f6(o["p"][j])) <= 2e-6 * abs(_f6(o["p"][j]))
    rc, sec, err = run_single(path, sites, "wald", ["--hide-covar"])
    assert rc == 0, err
    hrows = [r.split("\t") for r in sec["out.SingleWald.assoc"][1:]]
    assert len(hrows) == G.shape[1]
    assert hrows[0][3:] == rows[0][3:]
    assert hrows[1][3:] == rows[0][3:]             # the stale values of the genotype row before it
