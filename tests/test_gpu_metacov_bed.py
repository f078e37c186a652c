"""GPU: MetaCov's band from rows of a resident .bed matrix (rvt_cov_band_bed_dev) against the CPU oracle on the mean-imputed
columns, against the ring route on the same columns (rvt_cov_band), across its own paths (one product, four products, the
fp64 band), and for independence of pass and slice splits, of the window a row is called in and of what the context ran
before.

Base case: N = 6 105 (ceil(N / 4) = 1 527 is odd: every second row starts on an odd address, the last byte carries three
padding pairs, all set), d = 3, 700 rows with 2 % missing and the hand-made rows of tests/metacov_bed_cases.py, halo = 300,
H = W = 700 (three 256-head panels)."""
import ctypes as C
import os

import numpy as np
import pytest

import metacov_bed_cases as cases
import orc

pytestmark = pytest.mark.gpu

N0, D0, V0, HALO0 = 6105, 3, 700, 300
FLOAT_BAND = 2e-7    # of the largest covariance: the band is float32 (2^-24 = 6e-8 per rounding, the cast and the scaling)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        u = "u%d" % a.dtype.itemsize
        return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def _engine():
    import rvtests_amd
    return rvtests_amd.Engine(0)


class _Resident:
    """raw calls as a resident matrix behind one other row (so that the window's first row is misaligned too)"""

    def __init__(self, eng, raw):
        self.eng = eng
        self.cb = (raw.shape[0] + 3) // 4
        self.d_bed = eng.bed_alloc(raw.shape[1] + 1)
        eng.bed_upload(self.d_bed, 0, np.full((1, self.cb), 0x55, dtype=np.uint8))
        eng.bed_upload(self.d_bed, 1, cases.pack(raw))

    def row(self, j):
        return self.d_bed + (1 + j) * self.cb

    def free(self):
        self.eng.bed_free(self.d_bed)


def _ring_band(eng, G, H, W, halo):
    """the same columns uploaded one by one into a ring block and run through rvt_cov_band"""
    V = G.shape[1]
    ring = eng.alloc_block(V)
    for j in range(V):
        eng.upload_columns(ring, j, G[:, j])
    out = eng.cov_band(ring, V, 0, H, W, halo)
    path = eng.cov_band_last_path()
    eng.free_block(ring)
    return out, path


def _oracle(G, X, y, binary, halo):
    V = G.shape[1]
    rc, kept, ocov, row_end, oxz, ozz = orc.metacov(G, np.ones(V, dtype=np.int32), np.arange(V, dtype=np.int32), X, y, binary, halo)
    assert rc == 0
    return kept, ocov, oxz, ozz


def _check_against_oracle(band, xz, zz, poly, oracle, halo):
    """band within FLOAT_BAND x max|cov| on the pairs the reference prints, xz / zz to 1e-9; returns the scale"""
    kept, ocov, oxz, ozz = oracle
    V = len(kept)
    assert np.array_equal(poly, kept)
    scale = np.nanmax(np.abs(ocov))
    worst, checked = 0.0, 0
    for h in range(V):
        if not kept[h]:
            continue
        js = np.arange(h, min(V, h + halo + 1))
        js = js[kept[js].astype(bool)]
        worst = max(worst, np.abs(band[h, js - h].astype(np.float64) - ocov[h, js]).max())
        checked += len(js)
        if h + halo + 1 > V:
            assert np.isnan(band[h, V - h:]).all()
    print("band against the oracle: worst %.3g of bound %.3g over %d pairs" % (worst, FLOAT_BAND * scale, checked))
    assert checked > V and worst <= FLOAT_BAND * scale
    kk = kept.astype(bool)
    assert np.allclose(xz[kk], oxz[kk], rtol=1e-9, atol=1e-9 * max(np.abs(oxz[kk]).max(), 1.0))
    assert np.allclose(zz, ozz, rtol=1e-9, atol=1e-9 * max(np.abs(ozz).max(), 1.0))
    return scale


@pytest.fixture(scope="module")
def base():
    """the base case on one engine, its default call and the oracle's scale — computed once, never changed"""
    raw = cases.calls(N0, V0, seed=2024, missing=0.02)
    G = cases.imputed(raw)
    X, y, res, v, s2 = cases.null_model(N0, D0, 0, seed=7)
    eng = _engine()
    eng.set_null(0, X, res, v, s2)
    rows = _Resident(eng, raw)
    out = eng.cov_band_bed(rows.row(0), V0, V0, HALO0)
    oracle = _oracle(G, X, y, 0, HALO0)
    b = dict(raw=raw, G=G, X=X, y=y, eng=eng, rows=rows, out=out, path=eng.cov_band_last_path(), oracle=oracle,
             scale=float(np.nanmax(np.abs(oracle[1]))))
    for a in out:
        a.setflags(write=False)
    yield b
    rows.free()
    eng.close()


def test_against_the_oracle_on_the_mean_imputed_columns(base):
    band, xz, zz, poly, cnt = base["out"]
    assert base["path"] == 24
    assert band.shape == (V0, HALO0 + 1) and band.dtype == np.float32
    _check_against_oracle(band, xz, zz, poly, base["oracle"], HALO0)
    assert np.array_equal(poly, cases.polymorphic(base["G"]))
    assert cnt.dtype == np.int64 and np.array_equal(cnt, cases.counts(base["raw"]))
    k = V0 - len(cases.SPECIAL)
    assert poly[k:].tolist() == [0, 0, 0, 1, 1]


def _compare_with_ring(bed_out, ring_out, scale):
    band, xz, zz, poly = bed_out[:4]
    rband, rxz, rzz, rpoly = ring_out
    assert np.array_equal(poly, rpoly)
    assert np.array_equal(np.isnan(band), np.isnan(rband))
    m = ~np.isnan(rband)
    worst = np.abs(band[m].astype(np.float64) - rband[m].astype(np.float64)).max()
    wxz = np.abs(xz - rxz).max()
    print("band against the ring: worst %.3g of bound %.3g; xz worst %.3g of bound %.3g"
          % (worst, FLOAT_BAND * scale, wxz, 1e-11 * np.abs(rxz).max()))
    assert worst <= FLOAT_BAND * scale
    assert wxz <= 1e-11 * np.abs(rxz).max()
    assert np.array_equal(zz, rzz)


def test_against_the_ring_route_on_the_same_columns(base):
    ring_out, path = _ring_band(base["eng"], base["G"], V0, V0, HALO0)
    assert path == 4
    _compare_with_ring(base["out"], ring_out, base["scale"])


def test_rows_without_a_missing_call_take_one_product(base):
    raw = cases.without_missing(base["raw"])
    eng = base["eng"]
    rows = _Resident(eng, raw)
    try:
        out = eng.cov_band_bed(rows.row(0), V0, V0, HALO0)
        assert eng.cov_band_last_path() == 21
    finally:
        rows.free()
    band, xz, zz, poly, cnt = out
    assert np.array_equal(cnt, cases.counts(raw)) and (cnt[:, 3] == 0).all()
    scale = _check_against_oracle(band, xz, zz, poly, _oracle(raw, base["X"], base["y"], 0, HALO0), HALO0)
    ring_out, path = _ring_band(eng, raw, V0, V0, HALO0)
    assert path == 1
    _compare_with_ring(out, ring_out, scale)


def test_a_window_that_is_the_whole_matrix_at_every_row_alignment():
    """N = 515 (pitch 129: consecutive rows start at all four byte alignments), the window is the whole matrix — its first row is
    the allocation's first bytes, its last row ends at the matrix's last byte and holds a missing call in sample N - 1: the
    front stage's loads of four bytes at the edges of what it may touch."""
    N, d, V, halo = 515, 2, 37, 8
    raw = cases.calls(N, V, seed=515, missing=0.02)
    raw[N - 1, V - 1] = -9.0
    X, y, res, v, s2 = cases.null_model(N, d, 0, seed=516)
    eng = _engine()
    try:
        eng.set_null(0, X, res, v, s2)
        d_bed = eng.bed_alloc(V)
        eng.bed_upload(d_bed, 0, cases.pack(raw))
        band, xz, zz, poly, cnt = eng.cov_band_bed(d_bed, V, V, halo)
        assert eng.cov_band_last_path() == 24
        eng.bed_free(d_bed)
    finally:
        eng.close()
    G = cases.imputed(raw)
    assert np.array_equal(cnt, cases.counts(raw)) and cnt[V - 1, 3] == 1
    assert np.array_equal(poly, cases.polymorphic(G))
    _check_against_oracle(band, xz, zz, poly, _oracle(G, X, y, 0, halo), halo)


@pytest.mark.parametrize("var, value", [("RVT_BAND_PASS", "256"), ("RVT_BAND_SLICES", "3")])
def test_pass_and_slice_splits_give_the_same_bits(base, monkeypatch, var, value):
    monkeypatch.setenv(var, value)
    out = base["eng"].cov_band_bed(base["rows"].row(0), V0, V0, HALO0)
    assert base["eng"].cov_band_last_path() == 24
    for got, want in zip(out, base["out"]):
        assert _same_bits(got, want)


def test_a_rows_numbers_do_not_depend_on_the_window(base):
    eng, rows = base["eng"], base["rows"]
    band, xz, zz, poly, cnt = base["out"]
    again = eng.cov_band_bed(rows.row(0), V0, V0, HALO0)
    for got, want in zip(again, base["out"]):
        assert _same_bits(got, want)
    s = 100
    sband, sxz, szz, spoly, scnt = eng.cov_band_bed(rows.row(s), V0 - s, V0 - s, HALO0)
    assert eng.cov_band_last_path() == 24
    assert _same_bits(sxz, xz[s:]) and np.array_equal(spoly, poly[s:]) and np.array_equal(scnt, cnt[s:])
    # both windows end at row 700: every shared head sees the same markers
    assert _same_bits(sband, band[s:])
    # heads [100, 400) with their full halo as a window that ends earlier: their rows again
    hband = eng.cov_band_bed(rows.row(s), 300, V0 - s, HALO0)[0]
    assert _same_bits(hband, band[s:s + 300])


def test_binary_null_model_takes_the_fp64_band(base):
    X, y, res, v, s2 = cases.null_model(N0, D0, 1, seed=9)
    eng = _engine()
    try:
        eng.set_null(1, X, res, v, s2)
        rows = _Resident(eng, base["raw"])
        out = eng.cov_band_bed(rows.row(0), V0, V0, HALO0)
        assert eng.cov_band_last_path() == 20
        rows.free()
        band, xz, zz, poly, cnt = out
        assert np.array_equal(cnt, cases.counts(base["raw"]))
        scale = _check_against_oracle(band, xz, zz, poly, _oracle(base["G"], X, y, 1, HALO0), HALO0)
        ring_out, path = _ring_band(eng, base["G"], V0, V0, HALO0)
        assert path == 0
        _compare_with_ring(out, ring_out, scale)
    finally:
        eng.close()


def test_fp64_band_under_the_quantitative_model_agrees_with_four_products(base, monkeypatch):
    monkeypatch.setenv("RVT_METACOV_FP64", "1")
    out = base["eng"].cov_band_bed(base["rows"].row(0), V0, V0, HALO0)
    assert base["eng"].cov_band_last_path() == 20
    band, xz, zz, poly, cnt = base["out"]
    b64 = out[0]
    assert np.array_equal(np.isnan(band), np.isnan(b64))
    m = ~np.isnan(band)
    scale = base["scale"]
    worst = np.abs(band[m].astype(np.float64) - b64[m].astype(np.float64)).max()
    print("four products against the fp64 band: worst %.3g of bound %.3g" % (worst, FLOAT_BAND * scale))
    assert worst <= FLOAT_BAND * scale
    assert np.array_equal(out[3], poly) and np.array_equal(out[4], cnt)
    assert np.allclose(out[1], xz, rtol=1e-9, atol=1e-9 * np.abs(xz).max())


def test_longer_sample_axis_and_wide_model(monkeypatch):
    """N = 70 001 (16 row slices, several K chunks per band slice, N mod 4 = 1), d = 9: the widest instantiation of the front stage"""
    N, V, halo, d = 70001, 300, 64, 9
    raw = cases.calls(N, V, seed=99, missing=0.02)
    X, y, res, v, s2 = cases.null_model(N, d, 0, seed=5)
    eng = _engine()
    try:
        eng.set_null(0, X, res, v, s2)
        rows = _Resident(eng, raw)
        band, xz, zz, poly, cnt = eng.cov_band_bed(rows.row(0), V, V, halo)
        assert eng.cov_band_last_path() == 24
        monkeypatch.setenv("RVT_METACOV_FP64", "1")
        b64, xz64, _, poly64, cnt64 = eng.cov_band_bed(rows.row(0), V, V, halo)
        assert eng.cov_band_last_path() == 20
        rows.free()
    finally:
        eng.close()
    assert np.array_equal(cnt, cases.counts(raw)) and np.array_equal(cnt64, cnt)
    G = cases.imputed(raw)
    assert np.array_equal(poly, cases.polymorphic(G)) and np.array_equal(poly64, poly)
    assert np.array_equal(np.isnan(band), np.isnan(b64))
    m = ~np.isnan(band)
    scale = float(np.abs(b64[m]).max())                      # max |cov|: a diagonal entry, which the band holds
    worst = np.abs(band[m].astype(np.float64) - b64[m].astype(np.float64)).max()
    print("N = 70 001: four products against the fp64 band: worst %.3g of bound %.3g" % (worst, FLOAT_BAND * scale))
    assert worst <= FLOAT_BAND * scale
    # covXZ in numpy: (G'X - colsum(G) colsum(X) / N) / sigma2
    want = (G.T @ X - np.outer(G.sum(0), X.sum(0)) / N) / s2
    assert np.allclose(xz, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_refusals_write_nothing():
    import rvtests_amd
    N, d, V, halo = 515, 2, 12, 4
    raw = cases.calls(N, V, seed=3)
    X, y, res, v, s2 = cases.null_model(N, d, 0, seed=4)
    eng = _engine()
    try:
        L = eng.L
        band = np.full((V, halo + 1), 7.0, dtype=np.float32)
        xz, zz = np.full((V, d), 7.0), np.full((d, d), 7.0)
        poly = np.full(V, 7, dtype=np.int32)
        cnt = np.full((V, 4), 7, dtype=np.int64)

        def call(rows, H, W, band=band, xz=xz, poly=poly):
            p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            L.rvt_cov_band_bed_dev.restype = C.c_int     # (Engine.cov_band_bed sets its own argument types: set per call)
            L.rvt_cov_band_bed_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 5
            return L.rvt_cov_band_bed_dev(eng.ctx, C.c_void_p(rows), H, W, halo, 1.0, p(band), p(xz), p(zz), p(poly), p(cnt))

        def untouched():
            return (band == 7).all() and (xz == 7).all() and (zz == 7).all() and (poly == 7).all() and (cnt == 7).all()

        assert call(0x1000, V, V) == -4 and untouched()                 # RVT_E_STATE: no null model (checked before any read)
        eng.set_null(0, X, res, v, s2)
        rows = _Resident(eng, raw)
        r0 = rows.row(0)
        assert call(r0, 0, V) == -1 and untouched()                     # RVT_E_INVALID: H < 1
        assert call(r0, V, V - 1) == -1 and untouched()                 # W < H
        assert call(None, V, V) == -1 and untouched()                   # no rows
        assert call(r0, V, V, band=None) == -1 and untouched()
        assert call(r0, V, V, xz=None) == -1 and untouched()
        assert call(r0, V, V, poly=None) == -1 and untouched()
        with pytest.raises(rvtests_amd.RvtError, match="error -1:"):
            eng.cov_band_bed(r0, 3, 2, halo)
        assert call(r0, V, V) == 0 and not untouched()                  # (and the call the refusals stood in for runs)
        assert np.array_equal(cnt, cases.counts(raw))
        rows.free()
    finally:
        eng.close()


@pytest.mark.parametrize("var", ["RVT_HARDCALL", "RVT_PACKED"])
def test_switched_off_paths_are_refused_by_name(monkeypatch, var):
    import rvtests_amd
    N, d, V = 515, 2, 12
    raw = cases.calls(N, V, seed=3)
    X, y, res, v, s2 = cases.null_model(N, d, 0, seed=4)
    monkeypatch.setenv(var, "0")
    eng = _engine()
    try:
        eng.set_null(0, X, res, v, s2)
        rows = _Resident(eng, raw)
        with pytest.raises(rvtests_amd.RvtError, match=r"error -4:.*%s=0" % var):
            eng.cov_band_bed(rows.row(0), V, V, 4)
        with pytest.raises(rvtests_amd.RvtError, match=r"error -4:.*%s=0" % var):
            eng.score_bed_dev(rows.row(0), V)
        rows.free()
    finally:
        eng.close()


# ---- context reuse: the arrangement of tests/test_gpu_context_reuse.py --------------------------------------------------------------
REUSE_SHAPES = (dict(N=6105, d=3, V=150, halo=40, seed=31), dict(N=4099, d=5, V=90, halo=20, seed=32))
_reuse_inputs = {}


def _reuse_case(k):
    if k not in _reuse_inputs:
        sh = REUSE_SHAPES[k]
        raw = cases.calls(sh["N"], sh["V"], seed=sh["seed"])
        _reuse_inputs[k] = (raw, cases.imputed(raw), cases.null_model(sh["N"], sh["d"], 0, seed=sh["seed"] + 100))
    return _reuse_inputs[k]


def _reuse_steps(eng, k, everything):
    """shape k on engine eng: (score_bed_dev, cov_band on a ring,) cov_band_bed"""
    sh = REUSE_SHAPES[k]
    raw, G, (X, y, res, v, s2) = _reuse_case(k)
    eng.set_null(0, X, res, v, s2)
    rows = _Resident(eng, raw)
    try:
        if everything:
            eng.score_bed_dev(rows.row(0), sh["V"])
            _ring_band(eng, G, sh["V"], sh["V"], sh["halo"])
        return eng.cov_band_bed(rows.row(0), sh["V"] - 7, sh["V"], sh["halo"]), eng.cov_band_last_path()
    finally:
        rows.free()


def _set_env(values):
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


def test_the_result_does_not_depend_on_what_the_context_ran_before():
    env = ("RVT_POISON", "RVT_SCRIBBLE")
    fresh = []
    old = _set_env({k: None for k in env})
    try:
        for k in range(len(REUSE_SHAPES)):
            eng = _engine()
            try:
                fresh.append(_reuse_steps(eng, k, everything=False))
            finally:
                eng.close()
    finally:
        _set_env(old)
    old = _set_env({k: "255" for k in env})
    try:
        eng = _engine()
        try:
            got = [_reuse_steps(eng, k, everything=True) for k in (0, 1, 0, 1)]
        finally:
            eng.close()
    finally:
        _set_env(old)
    for k, ((out, path), i) in enumerate(zip(got, (0, 1, 0, 1))):
        assert path == fresh[i][1] == 24
        for a, b in zip(out, fresh[i][0]):
            assert _same_bits(a, b), (k, i)
