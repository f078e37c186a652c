"""The multiple-trait score test (`--single fastmtscore`) as a numpy statement, parameterised by dtype.

Written from the text of regression/FastMultipleTraitLinearRegressionScoreTest.cpp (FitNullModel, TestCovariateBlock); it holds
none of it.  fp64 is the yardstick of the device tests; float32 is the reference's own precision (Eigen MatrixXf) up to the order
of its sums, which is numpy's here."""
import numpy as np

from orc import lib as _orc_lib


def chisq_Q1(x):
    return _orc_lib().orc_chisq_Q(float(x), 1.0)


def fit_null(Y, Z, tests, dtype=np.float64):
    """Per-analysis part.  Y: N x P, Z: N x Q (or None), NaN = missing; tests: [(y, [z, ..]), ..].  Returns a dict."""
    dt = np.dtype(dtype).type
    Y = np.asarray(Y, dtype=dtype)
    N, P = Y.shape
    Z = np.zeros((N, 0), dtype=dtype) if Z is None else np.asarray(Z, dtype=dtype)
    YZ = np.concatenate([Y, Z], axis=1)
    ind = (~np.isnan(YZ)).astype(dtype)
    cnt = ind.sum(axis=0)
    C = np.where(np.isnan(YZ), dt(0), YZ)
    mean = np.where(cnt > 0, C.sum(axis=0) / np.maximum(cnt, dt(1)), dt(0)).astype(dtype)
    C = ((C - mean) * ind).astype(dtype)
    T = len(tests)
    out = dict(N=N, P=P, C=C, ind=ind, tests=[], ok=np.zeros(T, dtype=np.int32), obs=np.zeros(T), sigma2=np.full(T, np.nan))
    for t, (y, zs) in enumerate(tests):
        zc = [P + int(z) for z in zs]
        ind_model = ind[:, y].copy()
        for z in zc:
            ind_model = ind_model * ind[:, z]
        OBS = dt(ind_model.sum())
        rec = dict(y=int(y), z=zc, ind_model=ind_model, obs=OBS, ok=False)
        out["obs"][t] = float(OBS)
        out["tests"].append(rec)
        if OBS == 0 or cnt[y] == 0 or any(cnt[z] == 0 for z in zc):
            continue
        rec["scale_xy"] = dt(OBS / cnt[y])
        rec["scale_xx"] = dt(OBS / dt(N))
        rec["scale_xz"] = (OBS / cnt[zc]).astype(dtype) if zc else np.zeros(0, dtype=dtype)
        sigma2 = dt((C[:, y] ** 2).sum() * OBS / cnt[y])
        if zc:
            Zc = C[:, zc]
            iz = ind[:, zc]
            with np.errstate(divide="ignore", invalid="ignore"):
                A = ((Zc.T @ Zc) * OBS / (iz.T @ iz)).astype(dtype)
                zy = ((Zc.T @ C[:, y]) * OBS / (iz.T @ ind[:, y])).astype(dtype)
            if not (np.all(np.isfinite(A)) and np.all(np.isfinite(zy))):
                continue
            try:
                np.linalg.cholesky(A.astype(np.float64))
            except np.linalg.LinAlgError:
                continue
            rec["zz_inv"] = np.linalg.inv(A.astype(np.float64)).astype(dtype)
            rec["zy"] = zy
            sigma2 = dt(sigma2 - zy @ rec["zz_inv"] @ zy)
        rec["sigma2"] = dt(sigma2 / OBS)
        rec["ok"] = True
        out["ok"][t] = 1
        out["sigma2"][t] = float(rec["sigma2"])
    return out


def score(Y, Z, tests, G, dtype=np.float64, want_terms=False, null=None):
    """U, V, P (V x T each) of the columns of G (N x V: raw, imputed) — and, with want_terms, the largest |term| of every U cell
    (|GYZ[:, y] scale_xy| or |xz zz_inv zy|) and the branch flags of every cell."""
    dt = np.dtype(dtype).type
    nul = fit_null(Y, Z, tests, dtype) if null is None else null
    G = np.asarray(G, dtype=dtype)
    N, nv = G.shape
    T = len(tests)
    C = nul["C"]
    thr = float(np.float32(np.sqrt(2.0 * N)))
    gc = (G - G.mean(axis=0)).astype(dtype)
    GYZ = (gc.T @ C).astype(dtype)                    # nv x (P + Q)
    gg = (gc * gc).sum(axis=0).astype(dtype)
    U = np.full((nv, T), np.nan)
    V = np.full((nv, T), np.nan)
    Pv = np.full((nv, T), np.nan)
    terms = np.zeros((nv, T))
    flags = dict(rare=np.zeros((nv, T), bool), corr_nonpos=np.zeros((nv, T), bool), v_zero=np.zeros((nv, T), bool),
                 nan_test=np.zeros((nv, T), bool))
    for t, rec in enumerate(nul["tests"]):
        if not rec["ok"]:
            flags["nan_test"][:, t] = True
            continue
        OBS = rec["obs"]
        nm = (G.T @ rec["ind_model"]).astype(dtype)
        af = nm / (dt(2) * OBS)
        rare = nm < thr
        corr = np.where(rare, dt(2) * af * (dt(1) - dt(2) * af) * OBS, dt(-1)).astype(dtype)
        u = (GYZ[:, rec["y"]] * rec["scale_xy"]).astype(dtype)
        v = (gg * rec["scale_xx"]).astype(dtype)
        pos = corr > 0
        flags["rare"][:, t] = rare
        flags["corr_nonpos"][:, t] = rare & ~pos
        with np.errstate(divide="ignore", invalid="ignore"):
            corr = np.where(pos, corr / v, dt(1)).astype(dtype)
        big = np.abs(u).astype(np.float64)
        if rec["z"]:
            xz = (GYZ[:, rec["z"]] * rec["scale_xz"]).astype(dtype)
            du = (xz @ (rec["zz_inv"] @ rec["zy"])).astype(dtype)
            dv = np.einsum("ia,ab,ib->i", xz, rec["zz_inv"], xz).astype(dtype)
            big = np.maximum(big, np.abs(du).astype(np.float64))
            u = u - du
            v = v - dv
        v = v * rec["sigma2"]
        v = (v * corr).astype(dtype)
        U[:, t] = u
        V[:, t] = v
        terms[:, t] = big
        flags["v_zero"][:, t] = v == 0
        for i in range(nv):
            if v[i] != 0:
                Pv[i, t] = chisq_Q1(float(u[i]) * float(u[i]) / float(v[i])) if dtype == np.float64 else \
                    chisq_Q1(float(np.float32(u[i] * u[i] / v[i])))
    if want_terms:
        return U, V, Pv, terms, flags
    return U, V, Pv


# ---- the seeded inputs of the CPU and GPU tests -----------------------------------------------------------------------------------
BASE_TESTS = [(0, []), (1, [0]), (1, [1, 2]), (2, [0, 3]), (3, [0, 3]), (5, [0, 1, 2, 3]), (3, [3, 0]), (4, [2])]
RARE_MAF = (0.002, 0.003, 0.004, 0.008, 0.012)


def base_input(N, seed=7):
    """Y (N x 6: scales 0.1 .. 100, offsets up to 1e4), Z (N x 4: offsets up to 1000), missing rates 0 - 50 % per column, the 8
    tests above (one without covariates, two sharing y, two sharing a covariate set AND a missing pattern, all four covariates,
    a swapped covariate order, one whose y and z are never observed together) and 14 variants: five common hard calls, five
    rare ones, a mean-imputed column, a three-decimal dosage, all-zero, all-one.  Trait 0 carries variant 0 with an effect
    ~ 1 / sqrt(N) (smallest p between 1e-20 and 1e-8)."""
    rng = np.random.default_rng(seed + N)
    Zs = rng.standard_normal((N, 4))
    Z = Zs * np.array([1.0, 5.0, 0.5, 20.0]) + np.array([0.0, 1000.0, -30.0, 250.0])
    maf = [0.3, 0.12, 0.45, 0.2, 0.07]
    G = np.zeros((N, 14))
    for j, f in enumerate(maf):
        G[:, j] = rng.binomial(2, f, N)
    for j, f in enumerate(RARE_MAF):
        k = max(1, int(round(2 * N * f)))
        G[rng.choice(N, k, replace=False), 5 + j] = 1.0
    g = rng.binomial(2, 0.25, N).astype(float)
    miss = rng.random(N) < 0.03
    g[miss] = g[~miss].mean()
    G[:, 10] = g
    G[:, 11] = np.round(np.clip(rng.binomial(2, 0.35, N) + 0.15 * rng.standard_normal(N), 0.0, 2.0), 3)
    G[:, 12] = 0.0
    G[:, 13] = 1.0
    scale = np.array([1.0, 0.1, 100.0, 7.0, 30.0, 0.5])
    offset = np.array([0.0, 1e4, -500.0, 3.0, 2500.0, 0.02])
    E = rng.standard_normal((N, 6)) + 0.5 * Zs[:, [0]] + 0.3 * Zs[:, [3]]
    E[:, 0] += (12.5 / np.sqrt(N)) * np.std(E[:, 0]) * (G[:, 0] - G[:, 0].mean())
    Y = E * scale + offset
    ymiss = [0.0, 0.05, 0.2, None, None, 0.3]
    for j, r in enumerate(ymiss):
        if r:
            Y[rng.random(N) < r, j] = np.nan
    Y[np.isnan(Y[:, 2]), 3] = np.nan          # traits 2 and 3: the same pattern
    Y[: N // 2, 4] = np.nan                   # trait 4 and covariate 2 are never observed together
    Z[N // 2:, 2] = np.nan
    Z[rng.random(N) < 0.1, 1] = np.nan
    Z[rng.random(N) < 0.02, 3] = np.nan
    return Y, Z, list(BASE_TESTS), G


def close_cells(got, ref, rel, floor=None):
    """Element-wise |got - ref| <= rel |ref| (+ floor), NaN exactly where ref is NaN; returns (ok, worst relative excess)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return False, np.inf
    m = ~np.isnan(ref)
    tol = rel * np.abs(ref[m]) + (0.0 if floor is None else np.asarray(floor)[m])
    err = np.abs(got[m] - ref[m])
    bad = err > tol
    worst = float(np.max(err / np.maximum(tol, 1e-300))) if err.size and np.any(err > 0) else 0.0
    return not np.any(bad), worst
