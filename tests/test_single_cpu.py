"""CPU: `--single wald,score` — registry, output headers, NA rows without a device — and numpy statements of the two Wald fits
(SingleVariantWaldTest on A = [1, g, cov], src/Model.h:98-180) checked against the oracle's LinearRegression / LogisticRegression.
The statements are what tests/test_gpu_single.py holds the device to."""
import subprocess

import numpy as np
import pytest

import orc
import synth
from test_host_driver import DRIVER, _ensure_driver, write_input


def chisq_Q(x):
    return orc.lib().orc_chisq_Q(float(x), 1.0)


def design(g, X):
    """The reference's copyGenotypeWithCovariateAndIntercept: [1, g, X_1 ..] (X holds the intercept in column 0)."""
    return np.column_stack([X[:, :1], g, X[:, 1:]])


def wald_linear(g, X, y):
    """LinearRegression::FitLinearModel on A = [1, g, cov]: (ok, rounds, beta, se, p) of columns 1 .. d of A."""
    d = X.shape[1]
    if is_monomorphic(g):
        return 0, 0, np.zeros(d), np.zeros(d), np.ones(d)
    A = design(g, X)
    Ci = np.linalg.inv(A.T @ A)
    beta = Ci @ (A.T @ y)
    r = y - A @ beta
    s2 = r @ r / len(y)
    se = np.sqrt(np.diag(Ci) * s2)
    p = np.array([chisq_Q(b * b / (s * s)) for b, s in zip(beta, se)])
    return 1, 0, beta[1:], se[1:], p[1:]


def is_monomorphic(g):
    """isMonomorphicMarker (src/DataConsolidator.cpp:94-116): every non-missing value equals the first."""
    nm = g[g >= 0]
    return nm.size == 0 or bool((nm == nm[0]).all())


def wald_logistic(g, X, y, nrrounds=100):
    """LogisticRegression::FitLogisticModel(A, y, 100) on A = [1, g, cov] (regression/LogisticRegression.cpp:279-336): the
    deviance on the round's p (before the update) summed as safeSum (non-finite terms dropped).  rounds = rounds executed.
    A D that is not positive definite is a failed fit (-1)."""
    d = X.shape[1]
    zero = (np.zeros(d), np.zeros(d), np.ones(d))
    if is_monomorphic(g):
        return (0, 0) + zero
    A = design(g, X)
    beta = np.zeros(d + 1)
    last = -99999.0
    for it in range(nrrounds):
        p = 1.0 / (1.0 + np.exp(-(A @ beta)))
        v = p * (1.0 - p)
        D = A.T @ (A * v[:, None])
        try:
            L = np.linalg.cholesky(D)
        except np.linalg.LinAlgError:
            return (-1, it + 1) + zero
        beta = beta + np.linalg.solve(L.T, np.linalg.solve(L, A.T @ (y - p)))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = y * np.log(p) + (1.0 - y) * np.log(1.0 - p)
        dev = -2.0 * t[np.isfinite(t)].sum()
        if it > 1 and abs(dev - last) < 1e-3:
            se = np.sqrt(np.diag(np.linalg.inv(D)))
            pv = np.array([chisq_Q(b * b / (s * s)) for b, s in zip(beta, se)])
            return 1, it + 1, beta[1:], se[1:], pv[1:]
        if not np.isfinite(dev) or abs(dev) < np.finfo(float).tiny:
            return (-1, it + 1) + zero
        last = dev
    return (-1, nrrounds) + zero


def case(N, d, binary, seed):
    rng = np.random.default_rng(seed)
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=seed)
    maf = rng.uniform(0.05, 0.5, 6)
    G = (rng.random((N, 6, 2)) < maf[None, :, None]).sum(2).astype(float)
    G[:, 2] = np.where(rng.random(N) < 0.1, G[:, 2].mean(), G[:, 2])   # mean-imputed entries
    G[:, 4] = rng.uniform(0, 2, N)                                       # dosage
    if binary:
        G[:, 5] += 0.5 * y                                               # an associated column
    return X, y, G


@pytest.mark.parametrize("d", [1, 3])
def test_linear_statement_matches_oracle(d):
    X, y, G = case(800, d, 0, 31 + d)
    for j in range(G.shape[1]):
        ok, rounds, beta, se, p = wald_linear(G[:, j], X, y)
        assert ok == 1 and rounds == 0
        A = design(G[:, j], X)
        rc, b, pred, resid, s2 = orc.fit_linear(A, y)
        assert rc == 0
        covb = np.linalg.inv(A.T @ A) * s2
        assert np.allclose(beta, b[1:], rtol=1e-9, atol=1e-12)
        assert np.allclose(se, np.sqrt(np.diag(covb))[1:], rtol=1e-9)
        assert np.allclose(p, [chisq_Q(bb * bb / c) for bb, c in zip(b[1:], np.diag(covb)[1:])], rtol=1e-8, atol=1e-300)


@pytest.mark.parametrize("d", [1, 3])
def test_logistic_statement_matches_oracle(d):
    X, y, G = case(900, d, 1, 51 + d)
    for j in range(G.shape[1]):
        ok, rounds, beta, se, p = wald_logistic(G[:, j], X, y)
        assert ok == 1 and rounds > 2
        A = design(G[:, j], X)
        rc, b, pp, v = orc.fit_logistic(A, y)
        assert rc == 0
        assert np.allclose(beta, b[1:], rtol=1e-9, atol=1e-12)
        covb = np.linalg.inv(A.T @ (A * v[:, None]))   # covB = D^-1 of the last executed round
        assert np.allclose(se, np.sqrt(np.diag(covb))[1:], rtol=1e-9)
        # the round count: the fit ends inside `rounds` rounds and not inside one fewer
        assert orc.fit_logistic(A, y, rounds)[0] == 0
        assert orc.fit_logistic(A, y, rounds - 1)[0] == -1


def test_monomorphic_statement():
    X, y, G = case(300, 2, 1, 7)
    assert wald_logistic(np.full(300, 1.0), X, y)[:2] == (0, 0)
    g = np.full(300, 2.0)
    g[:5] = -9.0                                    # missing entries do not make a site polymorphic
    assert wald_linear(g, X, y)[0] == 0


def write_sites(path, n):
    with open(path, "w") as f:
        for j in range(n):
            f.write("1 %d\n" % (1000 + j))


def run_single(path, sites, single, extra=(), env=None):
    p = subprocess.run([DRIVER, path, "-", "-", "-", sites, "--single", single] + list(extra), capture_output=True, text=True,
                       timeout=300, env=env)
    sections, cur = {}, None
    for line in p.stdout.splitlines():
        if line.startswith("== "):
            cur = line[3:]
            sections[cur] = []
        elif cur is not None:
            sections[cur].append(line)
    return p.returncode, sections, p.stderr


def _driver_case(tmp_path, binary=0, d=3, N=600):
    X, y, G = case(N, d, binary, 71 + d)
    genes = [(G[:, :4], np.full(4, 0.1)), (G[:, 4:], np.full(2, 0.2))]
    path = str(tmp_path / "in.bin")
    write_input(path, y, X[:, 1:], binary, genes)
    sites = str(tmp_path / "sites.txt")
    write_sites(sites, G.shape[1])
    return path, sites, X, y, G


def test_single_registry_and_headers(tmp_path):
    _ensure_driver()
    path, sites, X, y, G = _driver_case(tmp_path)
    rc, sec, err = run_single(path, sites, "firth")
    assert rc == 1 and "Unknown model name: firth" in err
    rc, sec, err = run_single(path, sites, "exact")
    assert rc == 1 and "Unknown model name: exact" in err
    rc, sec, err = run_single(path, sites, "wald,score")
    assert rc == 0, err
    assert list(sec) == ["out.SingleWald.assoc", "out.SingleScore.assoc"]
    assert sec["out.SingleWald.assoc"][0] == "CHROM\tPOS\tTest\tBeta\tSE\tPvalue"
    assert sec["out.SingleScore.assoc"][0] == "CHROM\tPOS\tAF\tU\tV\tSTAT\tDIRECTION\tEFFECT\tSE\tPVALUE"
    V, d = G.shape[1], X.shape[1]
    assert len(sec["out.SingleWald.assoc"]) == 1 + V * d        # one row per column of X after the intercept
    assert len(sec["out.SingleScore.assoc"]) == 1 + V
    rc, sec, err = run_single(path, sites, "wald", ["--hide-covar"])
    assert rc == 0, err
    rows = sec["out.SingleWald.assoc"][1:]
    assert len(rows) == V and [r.split("\t")[2] for r in rows] == ["1:%d" % (1000 + j) for j in range(V)]


def test_single_na_rows_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_single.py")
    _ensure_driver()
    path, sites, X, y, G = _driver_case(tmp_path)
    rc, sec, err = run_single(path, sites, "wald,score")
    assert rc == 0, err
    d = X.shape[1]
    for j, row in enumerate(sec["out.SingleWald.assoc"][1:]):
        f = row.split("\t")
        label = "1:%d" % (1000 + j // d) if j % d == 0 else "cov%d" % (j % d)
        assert f[:3] == ["1", str(1000 + j // d), label]
        assert f[3:] == ["NA"] * 3                  # no device => fit() fails => NA, never a CPU result
    for row in sec["out.SingleScore.assoc"][1:]:
        assert row.split("\t")[3:] == ["NA"] * 7    # (AF is the caller's)


def test_driver_bad_input_after_pending_rows(tmp_path):
    """A sites file one line short: the driver stops with status 2 after some sites were fitted and written; the models
    still hold those rows when they are destroyed (each concrete model writes them in its own destructor)."""
    _ensure_driver()
    path, sites, X, y, G = _driver_case(tmp_path)
    write_sites(sites, G.shape[1] - 1)
    for single in ("wald", "score", "wald,score"):
        rc, sec, err = run_single(path, sites, single)
        assert rc == 2, (single, rc, err[-500:])
