"""CPU: the numpy statement of the multiple-trait score test (tests/mtscore_ref.py) against the oracle's linear score test, its
invariances and branches on the seeded inputs, and the shared cell arithmetic of the device (rvt_mtscore.h, built into the host
harness as hc_mt_cell) against the statement.  Also writes the float32-vs-fp64 deviation table INTEGRATION.md quotes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hc
import mtscore_ref as mt
import orc
import rvtests_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1500, 20000)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for N in SIZES:
        Y, Z, tests, G = mt.base_input(N)
        nul = mt.fit_null(Y, Z, tests)
        out[N] = (Y, Z, tests, G, nul) + tuple(mt.score(Y, Z, tests, G, want_terms=True, null=nul))
    return out


def test_statement_matches_oracle_linear_score():
    """Complete data, common variants: U is the oracle's LinearRegressionScoreTest U, V its V times the ratio of the variance
    estimators.  Both estimate sigma2 as RSS / N (LinearRegression: sigma2 = RSS / N; here (sum Yc^2 - zy' zz_inv zy) / OBS with
    OBS = N), so the ratio is 1."""
    RATIO = 1.0
    rng = np.random.default_rng(11)
    N = 800
    Z = rng.standard_normal((N, 3)) * [1.0, 4.0, 0.3] + [0.0, 50.0, -2.0]
    G = rng.binomial(2, [0.2, 0.35, 0.5, 0.1], (N, 4)).astype(float)
    Y = np.stack([rng.standard_normal(N) + Z[:, 0], 3.0 * rng.standard_normal(N) + 0.2 * G[:, 1] + 10.0], axis=1)
    tests = [(0, [0, 1, 2]), (1, [0, 1, 2]), (1, [])]
    U, V, P = mt.score(Y, Z, tests, G)
    for t, (y, zs) in enumerate(tests):
        X = np.column_stack([np.ones(N)] + [Z[:, z] for z in zs])
        rc, o = orc.metascore(G, X, Y[:, y], 0)
        assert rc == 0 and np.all(o["ok"] == 1)
        s2 = o["sigma2"]
        np.testing.assert_allclose(U[:, t], o["U"] * s2, rtol=1e-10)             # (the oracle prints U / sigma2 and SS / sigma2)
        np.testing.assert_allclose(V[:, t], o["V"] * s2 * s2 * RATIO, rtol=1e-10)
        np.testing.assert_allclose(P[:, t], o["p"], rtol=1e-8)


def test_covariate_order_and_pattern_sharing(cases):
    Y, Z, tests, G, nul, U, V, P, terms, flags = cases[1500]
    a, b = tests.index((3, [0, 3])), tests.index((3, [3, 0]))
    for M in (U, V, P):
        np.testing.assert_allclose(M[:, b], M[:, a], rtol=1e-12, atol=0.0)
    # tests 3 and 4: the same covariates and the same observed pattern, another y — each alone gives the same numbers
    a, b = tests.index((2, [0, 3])), tests.index((3, [0, 3]))
    assert np.array_equal(nul["tests"][a]["ind_model"], nul["tests"][b]["ind_model"])
    for k in (a, b):
        U1, V1, P1 = mt.score(Y, Z, [tests[k]], G)
        for M, M1 in ((U, U1), (V, V1), (P, P1)):
            assert np.array_equal(M[:, k], M1[:, 0], equal_nan=True)
    assert not np.allclose(U[:10, a], U[:10, b])


@pytest.mark.parametrize("N", SIZES)
def test_branches_are_hit(cases, N):
    Y, Z, tests, G, nul, U, V, P, terms, flags = cases[N]
    live = ~flags["nan_test"]
    assert np.any(flags["rare"] & live) and np.any(~flags["rare"] & live)
    assert np.any(flags["corr_nonpos"] & live)                        # af = 0: the all-zero column
    assert np.any(flags["v_zero"] & live) and np.all(np.isnan(P[flags["v_zero"] & live]))   # constant columns
    assert np.any(flags["nan_test"]) and nul["ok"].tolist() == [1] * 7 + [0]
    assert np.all(np.isnan(U[:, 7])) and nul["obs"][7] == 0
    rare_cols = [5 + j for j, f in enumerate(mt.RARE_MAF) if 2 * N * f < np.sqrt(2 * N)]
    assert len(rare_cols) >= 3 and all(np.all(flags["rare"][j, :7]) for j in rare_cols)
    assert 1e-20 < np.nanmin(P) < 1e-8 and np.nanargmin(P) == 0     # the causal pair: variant 0, test 0


def _hc_cell():
    L = hc.lib()
    dp = C.POINTER(C.c_double)
    L.hc_mt_cell.restype = None
    L.hc_mt_cell.argtypes = [C.c_double, C.c_double, C.c_double, dp, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double,
                             C.c_double, C.c_double, dp, dp, dp, dp]
    return L.hc_mt_cell


def test_exports():
    """The host harness has the cell function, the library the new entry points."""
    assert hasattr(hc.lib(), "hc_mt_cell")
    rvtests_amd.build_library()
    L = rvtests_amd.load_library()
    for n in ("rvt_mt_fit_null", "rvt_mt_score_block", "rvt_mt_clear"):
        assert hasattr(L, n), n


@pytest.mark.parametrize("N", SIZES)
def test_hc_mt_cell_matches_statement(cases, N):
    """The shared header's cell arithmetic, fed the fp64 products numpy forms, against the statement cell by cell."""
    Y, Z, tests, G, nul, U, V, P, terms, flags = cases[N]
    cell = _hc_cell()
    dp = C.POINTER(C.c_double)
    Cm = nul["C"]
    gc = G - G.mean(axis=0)
    GYZ = gc.T @ Cm
    gg = (gc * gc).sum(axis=0)
    zero = np.zeros(16)
    worst = 0.0
    for t, rec in enumerate(nul["tests"]):
        nm = G.T @ rec["ind_model"]
        nc = len(rec["z"])
        sxz = np.ascontiguousarray(rec.get("scale_xz", zero), dtype=np.float64)
        zy = np.ascontiguousarray(rec.get("zy", zero), dtype=np.float64)
        zzi = np.ascontiguousarray(rec.get("zz_inv", zero), dtype=np.float64)
        for v in range(G.shape[1]):
            gz = np.ascontiguousarray(GYZ[v, rec["z"]] if nc else zero, dtype=np.float64)
            out = np.zeros(3)
            cell(float(N), float(nm[v]), float(GYZ[v, rec["y"]]), gz.ctypes.data_as(dp), float(gg[v]), nc, int(rec["ok"]),
                 float(rec["obs"]), float(rec.get("scale_xy", 0.0)), float(rec.get("scale_xx", 0.0)), float(rec.get("sigma2", 0.0)),
                 sxz.ctypes.data_as(dp), zy.ctypes.data_as(dp), zzi.ctypes.data_as(dp), out.ctypes.data_as(dp))
            for got, ref, fl in ((out[0], U[v, t], 1e-12 * terms[v, t]), (out[1], V[v, t], 0.0), (out[2], P[v, t], 0.0)):
                assert np.isnan(got) == np.isnan(ref), (t, v)
                if not np.isnan(ref):
                    assert abs(got - ref) <= 1e-12 * abs(ref) + fl, (t, v, got, ref)
                    if ref != 0:
                        worst = max(worst, abs(got - ref) / abs(ref))
    print("hc_mt_cell vs statement: worst relative difference %.3g" % worst)


def test_write_f32_deviation_table(cases):
    """float32 restatement (the reference's precision, numpy's summation order) against fp64 on the two GPU test inputs: a record
    for INTEGRATION.md, nothing is asserted on the figures."""
    table = {}
    for N in SIZES:
        Y, Z, tests, G, nul, U, V, P, terms, flags = cases[N]
        U32, V32, P32 = mt.score(Y, Z, tests, G, dtype=np.float32)
        row = {}
        for name, a, b in (("U", U32, U), ("V", V32, V), ("P", P32, P)):
            m = ~np.isnan(b) & ~np.isnan(a) & (b != 0)
            r = np.abs(a[m] - b[m]) / np.abs(b[m])
            row[name] = {"max_rel": float(r.max()), "median_rel": float(np.median(r))}
        table["N=%d" % N] = row
    path = os.path.join(ROOT, "profiles", "mtscore_f32_deviation.json")
    with open(path, "w") as f:
        json.dump({"what": "float32 vs fp64 numpy statement of fastmtscore, 14 variants x 8 tests (tests/mtscore_ref.py base_input)",
                   "deviation": table}, f, indent=1, sort_keys=True)
        f.write("\n")
    assert os.path.getsize(path) > 0
