"""CPU: the models, routes, references and bounds of test_gpu_null_width.py (null_width_cases.py) checked without a GPU — every
model the GPU file installs fits and stays on the route the GPU file asserts (no column the digit planes would refuse, no
weight beyond the weighted kernel's range), the restated shift rule decrements exactly where the model builder means it to,
and the long-double reference together with an exact-integer emulation of the digit planes stays inside every bound."""
import numpy as np
import pytest

import null_width_cases as nw


@pytest.fixture(scope="module")
def models(oracle_lib):
    return {key: nw.case_model(*key) for key in nw.MODELS}


def test_every_model_fits_and_stays_on_its_route(models):
    assert len(models) == len(nw.MODELS)
    for (N, d, binary), (X, y, res, v, s2) in models.items():
        assert X.shape == (N, d) and np.all(X[:, 0] == 1.0)
        assert np.all(np.isfinite(res)) and np.all(np.isfinite(v)) and s2 > 0
        C = X.T @ ((v[:, None] if binary else 1.0) * X)
        assert np.linalg.cond(C) < 1e8, (N, d, binary, np.linalg.cond(C))
        for b in (0, 1) if binary else (0,):
            ratio = nw.column_scale_ratio(nw.null_tile(X, res, v, b))
            assert np.all(ratio <= 2.0 ** 16), (N, d, binary, b, ratio)          # the planes' rule (ensure_hcp_planes)
            if b or d <= nw.FDX_MAX_D:
                assert np.all(ratio <= 4096.0), (N, d, binary, b, ratio)         # the hcx rule; the float-digit kernel's too
        if binary:
            assert np.all(v >= 0.0) and np.all(v <= 0.49)                        # gene_suffstat_hcw's digit range
            assert set(np.unique(y)) == {0.0, 1.0}


def test_the_columns_do_not_look_alike(models):
    """The shifts of one model's columns differ — a kernel that took scale[k] of a neighbour column is off by a power of two —
    and the two columns at the decrement point behave as built: largest entry 4 (1 - 2^-30): decremented; exactly 8: not."""
    X, y, res, v, s2 = models[(2003, 13, 0)]
    for B in (nw.B_HCX, nw.B_PLANES):
        shifts = [nw.quantise(X[:, k], B)[1] for k in range(13)]
        assert len(set(shifts[1:6])) == 5 and shifts[0] == shifts[1], shifts   # (intercept and indicator: both end at 1)
        assert np.max(np.abs(X[:, 4])) == 4.0 * (1.0 - 2.0 ** -30) and np.max(np.abs(X[:, 5])) == 8.0
        assert shifts[4] == B - 4      # e = 2: B - 3, decremented
        assert shifts[5] == B - 5      # e = 4: B - 5, kept
        assert shifts[0] == B - 2      # the intercept: e = 1, 2^(B-2) is under the cut
        for k in range(13):
            q, s = nw.quantise(X[:, k], B)
            top = np.max(np.abs(q))
            assert 2.0 ** (B - 3) * 0.98 <= top <= 0.98 * 2.0 ** (B - 1) + 1, (B, k, top)


def test_expected_route_restates_the_table():
    r = nw.expected_route
    assert [r(d, 0, "block") for d in (1, 13, 14)] == ["gene_suffstat_hc", "gene_suffstat_hc", "fp64"]
    assert [r(d, 1, "block") for d in (1, 6, 7, 13, 14)] == ["gene_suffstat_hcx"] * 2 + ["gene_suffstat_hcw"] * 2 + ["fp64"]
    assert [r(d, 0, "bed") for d in (13, 14)] == ["gene_suffstat_hcp", "expanded"]
    assert [r(d, 0, "bed_dev") for d in (13, 14)] == ["gene_tnull_hcp", "expanded"] and r(2, 1, "bed_dev") == "expanded"
    assert [r(d, 0, "score_bed_dev") for d in (13, 14)] == ["planes", "refused"]
    assert [r(d, 0, "lattice") for d in (13, 14)] == ["gene_suffstat_lat", "fp64"]
    assert [r(d, 0, "float") for d in (6, 7)] == ["gene_suffstat_fdx", "fp64"]


def test_column_scale_ratio_is_the_engines_quantity():
    col = np.array([0.0, 1.0, -2.0, 3.0, 0.0, -40.0])        # non-zero magnitudes 1 2 3 40: the upper median is 3
    assert nw.column_scale_ratio(col[:, None])[0] == 40.0 / 3.0
    assert nw.column_scale_ratio(np.zeros((5, 1)))[0] == 0.0


@pytest.mark.parametrize("B,d,binary,route", [(nw.B_HCX, 6, 1, "gene_suffstat_hcx"), (nw.B_PLANES, 13, 0, "gene_tnull_hcp")])
def test_the_reference_stays_inside_the_digit_plane_bound(models, B, d, binary, route):
    """The digit planes' T in exact integers against the long-double reference: inside t_bound (ratio <= 1), and well above
    zero — the bound is about the quantisation, not slack (0.04 with a fifth of the calls imputed at B = 42, d = 6; 0.15 at
    B = 56, d = 13: the half-unit errors of c_j entries add like a random walk, the bound adds them in full)."""
    N, M = 2003, 33
    X, y, res, v, s2 = models[(N, d, binary)]
    tile = nw.null_tile(X, res, v, binary)
    raw = (nw.masked_gene(N, M) if binary else nw.gene(N, M))[0]
    G, T = nw.emulate_planes(raw, tile, B)
    S0, T0 = nw.ref_suffstat(G, v if binary else np.ones(N), tile)
    bound = nw.t_bound(G, tile, route)
    err = np.abs((T.astype(np.longdouble) - T0).astype(np.float64))
    assert np.all(err[bound == 0] == 0)
    ratio = np.max(err[bound > 0] / bound[bound > 0])
    print("B = %d, d = %d: worst |T - ref| / bound = %.3g" % (B, d, ratio))
    assert 1e-3 < ratio <= 1.0, ratio
    # a lost lowest plane pair (the digits below 2^14 of the integer) misses the bound by orders of magnitude
    k = 2
    q, shift = nw.quantise(tile[:, k], B)
    lost = np.ldexp(np.abs(raw.clip(0)).T @ np.abs((q & 0x3FFF).astype(np.float64)), -shift)
    assert np.max(lost[bound[:, k] > 0] / bound[bound[:, k] > 0, k]) > 100.0


def test_fp64_and_gram_bounds_hold_for_plain_fp64(oracle_lib):
    """numpy's fp64 products (some order of N multiply-adds) against the long-double reference: inside the fp64-route bound and
    the Gram bounds; zero-bound entries are exactly zero."""
    N, M, d = 2003, 33, 14
    X, y, res, v, s2 = nw.case_model(N, d, 1)
    raw, G, af = nw.gene(N, M)
    tile = nw.null_tile(X, res, v, 1)
    S0, T0 = nw.ref_suffstat(G, v, tile)
    T = G.T @ tile
    S = (G * v[:, None]).T @ G
    bt, bs = nw.t_bound(G, tile, "fp64"), nw.s_bound(G, v, 1, True)
    et = np.abs((T.astype(np.longdouble) - T0).astype(np.float64))
    es = np.abs((S.astype(np.longdouble) - S0).astype(np.float64))
    assert np.all(et <= bt) and np.all(es <= bs)
    assert np.all(bt[7] == 0) and np.all(et[7] == 0)        # the all-zero column
    H = np.where(raw < 0, 0.0, raw)
    Sq, _ = nw.ref_suffstat(H, np.ones(N), tile)
    assert np.all(nw.s_bound(H, np.ones(N), 0, False) == 0) and np.array_equal((H.T @ H).astype(np.longdouble), Sq)
