"""The identities behind rvt_score_bed_dev under a binary trait, stated in numpy and checked against the oracle's MetaScore on
the imputed matrix: from the 2-bit codes of a row — H in {0, 1, 2} (0 where missing), m = [missing], D2 = [H = 2] and the imputed
value mu — and the weighted null tile Z = [v X_0 .. v X_{d-1} | res | v]:

    t_k = H'Z_k + mu m'Z_k        u = H'Z_res + mu m'Z_res        s = H'Z_v + 2 D2'Z_v + mu^2 m'Z_v        SS = s - t'C^-1 t

This pins the mu^2 and 2 D2 terms independently of the device (tests/test_gpu_score_bed_binary.py has the kernel)."""
import math

import numpy as np

import orc


def score_from_codes(raw, X, y):
    """raw: N x V hard calls, negative = missing.  dict of ok, U, V, effect, se, p as orc.metascore returns them."""
    raw = np.asarray(raw, dtype=np.float64)
    X = np.asfortranarray(X, dtype=np.float64)
    N, V = raw.shape
    d = X.shape[1]
    rc, beta, p, v = orc.fit_logistic(X, y)
    assert rc == 0
    res = y - p
    Z = np.column_stack([v[:, None] * X, res, v])                # N x (d + 2)
    Cinv = np.linalg.inv(X.T @ (v[:, None] * X))
    m = (raw < 0).astype(np.float64)
    H = np.where(raw < 0, 0.0, raw)
    D2 = (H == 2).astype(np.float64)
    imputed = orc.impute_mean(np.asfortranarray(raw))
    mu = np.zeros(V)                                             # the value imputeGenotypeToMean wrote, 0 without a missing call
    for h in range(V):
        miss = np.flatnonzero(raw[:, h] < 0)
        if miss.size:
            mu[h] = imputed[miss[0], h]
    HZ, mZ, DZ = H.T @ Z, m.T @ Z, D2.T @ Z                      # V x (d + 2) each
    t = HZ[:, :d] + mu[:, None] * mZ[:, :d]
    u = HZ[:, d] + mu * mZ[:, d]
    s = HZ[:, d + 1] + 2.0 * DZ[:, d + 1] + mu * mu * mZ[:, d + 1]
    SS = s - np.einsum("hk,kl,hl->h", t, Cinv, t)
    # polymorphic: the imputed column takes two values — unweighted, from the counts and mu alone
    g = H + mu[None, :] * m
    ok = (g.min(0) != g.max(0)) & (SS > 0)
    out = dict(ok=ok.astype(np.int32), U=np.zeros(V), V=np.zeros(V), effect=np.zeros(V), se=np.zeros(V), p=np.ones(V))
    for h in np.flatnonzero(ok):
        out["U"][h] = u[h]
        out["V"][h] = SS[h]
        out["effect"][h] = u[h] / SS[h] if u[h] != 0.0 else 0.0
        out["se"][h] = 1.0 / math.sqrt(SS[h])
        out["p"][h] = math.erfc(math.sqrt(0.5 * u[h] * u[h] / SS[h]))   # chi-square tail, one degree of freedom
    return out


def make_raw(N, V, seed):
    rng = np.random.default_rng(seed)
    maf = 10 ** rng.uniform(-2.0, -0.4, V)
    raw = rng.binomial(2, maf, size=(N, V)).astype(np.float64)
    raw[rng.random((N, V)) < 0.02] = -9.0
    raw[:, 2] = 0.0                                              # all 0
    raw[:, 4] = np.where(raw[:, 4] < 0, -9.0, 2.0)               # all 2 apart from its missing calls
    raw[:, 6] = -9.0                                             # nothing but missing calls
    hi = rng.binomial(2, 0.8, N).astype(np.float64)              # allele frequency above 0.5: mu > 1
    hi[rng.random(N) < 0.05] = -9.0
    raw[:, 9] = hi
    return raw


def test_the_identities_of_the_codes_match_the_oracle():
    N, V, d = 1203, 40, 3
    raw = make_raw(N, V, 20)
    rng = np.random.default_rng(21)
    X = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(d - 1)]))
    lin = -0.5 + 0.4 * X[:, 1] - 0.3 * X[:, 2] + 0.5 * np.maximum(raw[:, 9], 0)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    G = orc.impute_mean(np.asfortranarray(raw))
    assert (raw[:, 4] < 0).any() and G[:, 9].mean() > 1.0 and G[raw[:, 9] < 0, 9].min() > 1.0
    rc, o = orc.metascore(G, X, y, 1)
    assert rc == 0
    r = score_from_codes(raw, X, y)
    assert np.array_equal(r["ok"], o["ok"])
    assert not o["ok"][[2, 4, 6]].any() and o["ok"][9] and o["ok"].sum() >= V - 6
    for f in ("U", "V", "effect", "se", "p"):
        assert np.allclose(r[f], o[f], rtol=1e-10, atol=0), f


def test_the_two_weighted_terms_are_needed():
    """Without 2 D2'Z_v, or with mu in place of mu^2, the statement misses the oracle: the check above can see both terms."""
    N, V, d = 1203, 40, 3
    raw = make_raw(N, V, 20)
    rng = np.random.default_rng(21)
    X = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(d - 1)]))
    y = (rng.random(N) < 0.4).astype(np.float64)
    rc, o = orc.metascore(orc.impute_mean(np.asfortranarray(raw)), X, y, 1)
    assert rc == 0
    rc, beta, p, v = orc.fit_logistic(X, y)
    h = 9
    g = orc.impute_mean(np.asfortranarray(raw))[:, h]
    H = np.where(raw[:, h] < 0, 0.0, raw[:, h])
    m = (raw[:, h] < 0).astype(np.float64)
    mu = g[raw[:, h] < 0][0]
    s = g @ (v * g)
    full = H @ v + 2.0 * ((H == 2) @ v) + mu * mu * (m @ v)
    assert abs(full - s) <= 1e-12 * s
    assert abs(H @ v + mu * mu * (m @ v) - s) > 1e-3 * s          # no 2 D2 term
    assert abs(H @ v + 2.0 * ((H == 2) @ v) + mu * (m @ v) - s) > 1e-4 * s   # mu, not mu^2
