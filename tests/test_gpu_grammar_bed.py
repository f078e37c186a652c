"""GPU: famGrammarGamma from rows of a resident .bed matrix (rvt_grammar_bed_dev, rvt_debug_grammar_bed) — the integer product
against numpy with no tolerance, the five columns against the fp64 block route on the uploaded imputed columns of the same calls
and against GrammarGamma's numpy statement, independence of the launch plan, of the piece and of what the context ran before,
the chain from a resident matrix to the scan, and the refusals.  The rows hold every row kind of fam_bed_cases.HAND_ROWS, carry
set padding bits and lie behind one other row (odd row addresses at N = 515: 129 bytes)."""
import ctypes as C

import numpy as np
import pytest

import fam_bed_cases
import grammar_bed_cases as gb
from test_fam_cpu import make_family_case
from test_gpu_fam_bed import dense_case, family_case, resident
from test_gpu_kinship_bed import calls as kinship_calls, with_null
from test_gpu_kinship_families import blocks_of, null_for_layout
from test_gpu_single_fam import MAXV
from test_single_fam_cpu import grammar_null_given_delta, grammar_test

pytestmark = pytest.mark.gpu

FIELDS = ("af", "beta", "beta_var", "p")
PIECE = 8192                                              # rows of one launch of the product (af=mean)


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


def install(eng, shape):
    """The kinship of the shape on eng, an ordinary null model for the rows' pitch, and NO family null model:
    (N, U, S, X, y, raw), U and S as numpy's statements take them."""
    if shape == "family":                                 # N = 237, the family form
        c, X, y, raw = family_case()
        null_for_layout(eng, c.N)
        U_flat, S, _ = eng.kinship_decompose_families(c.fam_ptr, c.members, c.flat(c.K), install=True)
        return c.N, c.dense(blocks_of(c, U_flat)).astype(np.float64), S.astype(np.float64), X, y, raw
    N, U, S, X, y, raw = dense_case()                     # N = 515, dense digit planes
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    assert eng.kinship_structure() == 1.0
    return N, U, S, X, y, raw


def same_bits(a, b, fields=FIELDS):
    if not (np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["counts"], b["counts"])):
        return False
    return all(np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)) for f in fields)


def cut(r, lo, hi):
    return {k: v[lo:hi] for k, v in r.items()}


# ---- 1. the integer product ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["family", "dense"])
def test_exact_sums(engine_factory, shape):
    eng = engine_factory()
    N, U, S, X, y, raw = install(eng, shape)
    V = raw.shape[1]
    gn = eng.fit_grammar_null(X, y)
    gamma, ty, ysy = grammar_null_given_delta(X, y, U, S, gn.delta, gn.sigma2_g)
    d_bed, d_rows = resident(eng, raw)
    dbg = eng.debug_grammar_bed(d_rows, V)
    planes, e = dbg["planes"], dbg["exp2"]
    err = np.abs(gb.planes_value(planes, e) - ty).max()
    print("planes against numpy's ty: worst difference %.3g of max|ty| (allowed 1e-9), e = %d" % (err / np.abs(ty).max(), e))
    assert err <= 1e-9 * np.abs(ty).max()
    assert (planes[1:] >= 0).all() and np.array_equal(dbg["totals"], planes.astype(np.int64).sum(1))
    want = gb.integer_sums(fam_bed_cases.pack(raw), N, planes)
    assert np.array_equal(dbg["sums"], want)              # no tolerance
    cnt = fam_bed_cases.site_pass(raw)[0]
    n1, n2, nm = gb.counts_of(dbg["sums"])
    assert np.array_equal(np.stack([N - n1 - n2 - nm, n1, n2, nm], axis=1), cnt)
    eng.bed_free(d_bed)


# ---- 2. the five columns -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["family", "dense"])
def test_against_the_block_route_and_the_statement(engine_factory, shape):
    eng = engine_factory()
    N, U, S, X, y, raw = install(eng, shape)
    V = raw.shape[1]
    gn = eng.fit_grammar_null(X, y)
    gamma, ty, ysy = grammar_null_given_delta(X, y, U, S, gn.delta, gn.sigma2_g)
    cnt = fam_bed_cases.site_pass(raw)[0]
    d_bed, d_rows = resident(eng, raw)
    lone = eng.grammar_bed_dev(d_rows, V, 0)              # af=mean with NO family null model on the context
    assert np.array_equal(lone["counts"], cnt)
    tested, refused = gb.check_against_statement(lone, raw, ty, gamma, ysy, grammar_test, what=shape + " af=mean, statement")
    assert tested >= 10 and refused >= 4
    eng.fit_fam_null(X, y)                                # the block route and af=kinship need its layout
    ptr = eng.upload_block(fam_bed_cases.imputed(raw))
    for kin in (0, 1):
        bed = eng.grammar_bed_dev(d_rows, V, kin)
        blk = eng.grammar_block(ptr, V, kin)
        assert np.array_equal(bed["ok"], blk["ok"]) and np.array_equal(bed["counts"], cnt)
        k = blk["ok"] == 1
        assert k.sum() >= 10
        floor = (cnt[:, 1] + 2 * cnt[:, 2] + fam_bed_cases.site_pass(raw)[1] * cnt[:, 3]) * np.abs(ty).max() * 2.0 ** -50
        G = fam_bed_cases.imputed(raw)
        gg = ((G - G.mean(0)) ** 2).sum(0)
        for f, tol in (("af", 1e-8), ("beta", 1e-7), ("beta_var", 1e-7), ("p", 1e-6)):
            sel = k if f != "af" else np.ones(V, dtype=bool)
            allowed = tol * np.abs(blk[f][sel]) + 1e-300
            if f == "beta":
                allowed = allowed + floor[sel] / (gg[sel] * gamma)
            ratio = np.abs(bed[f][sel] - blk[f][sel]) / allowed
            print("%s af_kinship=%d %s: worst difference between the routes / allowed %.3g" % (shape, kin, f, ratio.max()))
            assert (ratio <= 1.0).all(), (f, kin)
        kin_args = (U, S, gn.delta) if kin else ()
        gb.check_against_statement(bed, raw, ty, gamma, ysy, grammar_test, kin_args, what="%s af_kinship=%d, statement" % (shape, kin))
        if not kin:
            assert same_bits(bed, lone)
    eng.free_block(ptr)
    eng.bed_free(d_bed)


# ---- 3. the split ----------------------------------------------------------------------------------------------------------------------
def test_independence_of_the_split(engine_factory, monkeypatch):
    eng = engine_factory()
    N, U, S, X, y, raw = install(eng, "dense")
    V = raw.shape[1]
    eng.fit_fam_null(X, y)
    eng.fit_grammar_null(X, y)
    d_bed, d_rows = resident(eng, raw)
    cb = (N + 3) // 4
    assert gb.plan(N, V, 256, 64)["slices"] == 9 and N - 8 * 64 == 3      # nine slices, the last with 3 live samples
    runs = []
    for env in ({}, {"RVT_GG_BED_SLICE": "64"}, {"RVT_GG_BED_SLICE": "128"}, {"RVT_GG_BED_TILES": "1"},
                {"RVT_GG_BED_SLICE": "64", "RVT_GG_BED_TILES": "1"}):
        for k in ("RVT_GG_BED_SLICE", "RVT_GG_BED_TILES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        runs.append((eng.grammar_bed_dev(d_rows, V, 0), eng.grammar_bed_dev(d_rows, V, 1), eng.debug_grammar_bed(d_rows, V)["sums"]))
        sub = eng.grammar_bed_dev(d_rows + 5 * cb, 39, 0), eng.grammar_bed_dev(d_rows + 5 * cb, 39, 1)
        assert same_bits(sub[0], cut(runs[-1][0], 5, 44)) and same_bits(sub[1], cut(runs[-1][1], 5, 44)), env
    assert (runs[0][0]["ok"] == 1).sum() >= 10
    for r in runs[1:]:
        assert same_bits(r[0], runs[0][0]) and same_bits(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
    eng.bed_free(d_bed)


# ---- 4. more rows than one piece -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece,kins", [(MAXV, (0, 1)), (PIECE, (0,))])
def test_rows_beyond_one_piece(engine_factory, piece, kins):
    """V = piece + 77 at N = 100: af=kinship walks the front stage's pieces of RVT_MAX_VARIANTS rows, the product its own of
    8192; a row's columns are the bits of a separate call on the rows around the seam."""
    N, K, U, S, X, y = make_family_case(25, 2, 91)
    assert N == 100
    eng = engine_factory()
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    eng.fit_fam_null(X, y)
    eng.fit_grammar_null(X, y)
    V = piece + 77
    raw = fam_bed_cases.calls(N, V - len(fam_bed_cases.HAND_ROWS), seed=99, maf_hi=-0.7)
    d_bed, d_rows = resident(eng, raw)
    cb = (N + 3) // 4
    cnt = fam_bed_cases.site_pass(raw)[0]
    for kin in kins:
        whole = eng.grammar_bed_dev(d_rows, V, kin)
        assert np.array_equal(whole["counts"], cnt)
        for lo, hi in ((piece - 3, piece + 5), (V - 40, V)):
            part = eng.grammar_bed_dev(d_rows + lo * cb, hi - lo, kin)
            assert same_bits(part, cut(whole, lo, hi)), (kin, lo)
        assert (whole["ok"][piece - 3:piece + 5] == 1).sum() >= 4
    eng.bed_free(d_bed)


# ---- 5. the chain -------------------------------------------------------------------------------------------------------------------------
def test_chain_from_resident_rows_to_the_scan(engine_factory):
    """bed upload -> kinship_from_bed(install=True) -> fit_fam_null -> fit_grammar_null -> grammar_bed_dev of 200 of the same
    rows: nothing crosses the link as fp64.  Equal to the fp64 block route within the route tolerances."""
    eng = engine_factory()
    N, V, n = 300, 2000, 200
    X, y = with_null(eng, N)
    G = kinship_calls(N, V, 0.05, special=False)
    d_bed = eng.bed_alloc(V)
    eng.bed_upload(d_bed, 0, eng.pack_bed(G))
    eng.kinship_from_bed(d_bed, V, method="bn", install=True)
    eng.fit_fam_null(X, y)
    gn = eng.fit_grammar_null(X, y)
    assert np.isfinite(gn.delta)
    raw = G[:, :n].astype(np.float64)
    ptr = eng.upload_block(fam_bed_cases.imputed(raw))
    for kin in (0, 1):
        bed, blk = eng.grammar_bed_dev(d_bed, n, kin), eng.grammar_block(ptr, n, kin)
        assert np.array_equal(bed["ok"], blk["ok"])
        k = blk["ok"] == 1
        assert k.sum() > 100
        for f, tol in (("af", 1e-8), ("beta", 1e-7), ("beta_var", 1e-7), ("p", 1e-6)):
            worst = np.max(np.abs(bed[f][k] - blk[f][k]) / np.maximum(np.abs(blk[f][k]), 1e-300))
            print("af_kinship=%d %s: worst relative difference between the routes %.3g (allowed %.0e)" % (kin, f, worst, tol))
            assert worst <= tol, (f, kin)
    eng.free_block(ptr)
    eng.bed_free(d_bed)


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------------
def test_reuse_under_scribble_and_a_second_fit(engine_factory, monkeypatch):
    def fresh(y_):
        e = engine_factory()
        N, U, S, X, y, raw = install(e, "dense")
        e.fit_fam_null(X, y)
        e.fit_grammar_null(X, y_ if y_ is not None else y)
        d_bed, d_rows = resident(e, raw)
        return e, d_bed, d_rows, raw.shape[1], X, y

    e0, bed0, rows0, V, X, y = fresh(None)
    ref = e0.grammar_bed_dev(rows0, V, 0), e0.grammar_bed_dev(rows0, V, 1)
    y2 = y[::-1].copy() + 0.25 * X[:, 1]
    e2, bed2, rows2, _, _, _ = fresh(y2)
    ref2 = e2.grammar_bed_dev(rows2, V, 0), e2.grammar_bed_dev(rows2, V, 1)
    assert not np.array_equal(ref[0]["beta"], ref2[0]["beta"], equal_nan=True)
    monkeypatch.setenv("RVT_SCRIBBLE", "165")
    e1, bed1, rows1, _, _, _ = fresh(None)
    for _ in range(2):                                    # the same call twice on one context, every work space refilled
        assert same_bits(e1.grammar_bed_dev(rows1, V, 0), ref[0]) and same_bits(e1.grammar_bed_dev(rows1, V, 1), ref[1])
    monkeypatch.delenv("RVT_SCRIBBLE")
    e1.fit_grammar_null(X, y2)                            # another fit: the planes are rebuilt
    assert same_bits(e1.grammar_bed_dev(rows1, V, 0), ref2[0]) and same_bits(e1.grammar_bed_dev(rows1, V, 1), ref2[1])
    for e, b in ((e0, bed0), (e1, bed1), (e2, bed2)):
        e.bed_free(b)


def test_refusals_write_nothing(engine_factory):
    SENT = -7.5
    e = engine_factory()
    N, U, S, X, y, raw = install(e, "dense")
    V = raw.shape[1]
    d_bed, d_rows = resident(e, raw)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    e.L.rvt_grammar_bed_dev.restype = C.c_int
    e.L.rvt_grammar_bed_dev.argtypes = [vp, vp, C.c_int64, C.c_int, ip] + [dp] * 4 + [vp]

    def call(ctx, rows, v, kin, drop=None):
        """(return code, whether every output array still holds its sentinel); drop: the index of an output passed as null"""
        ok = np.full(V, -77, dtype=np.int32)
        outs = [np.full(V, SENT) for _ in range(4)]
        cnt = np.full((V, 4), -77, dtype=np.int64)
        args = [ok.ctypes.data_as(ip)] + [o.ctypes.data_as(dp) for o in outs]
        if drop is not None:
            args[drop] = None
        rc = e.L.rvt_grammar_bed_dev(ctx, vp(rows) if rows else None, v, kin, *args, cnt.ctypes.data_as(vp))
        return rc, (ok == -77).all() and (cnt == -77).all() and all((o == SENT).all() for o in outs)

    # no rvt_fit_grammar_null yet
    assert call(e.ctx, d_rows, V, 0) == (-4, True)
    e.fit_grammar_null(X, y)
    # null arguments, V < 1
    for ctx, rows, v in ((None, d_rows, V), (e.ctx, None, V), (e.ctx, d_rows, 0)):
        assert call(ctx, rows, v, 0) == (-1, True)
    for drop in range(5):
        assert call(e.ctx, d_rows, V, 0, drop) == (-1, True)
    # af=kinship without a family null model; af=mean runs
    assert call(e.ctx, d_rows, V, 1) == (-4, True)
    rc, untouched = call(e.ctx, d_rows, V, 0)
    assert rc == 0 and not untouched
    # an ordinary null model of another N: the rows would have another pitch
    null_for_layout(e, N + 10)
    assert call(e.ctx, d_rows, V, 0) == (-4, True)
    null_for_layout(e, N)
    assert call(e.ctx, d_rows, V, 0)[0] == 0
    # a ty that is not finite: a trait so small that its residual sum of squares underflows to 0, sigma2_g = 0 and ty = x / 0;
    # should the fit itself refuse such a trait, there is no GrammarGamma null model — the same code
    import rvtests_amd
    try:
        e.fit_grammar_null(X, y * 1e-200)
        print("the fit took the trait: the call has to find ty not finite")
    except rvtests_amd.RvtError as err:
        print("the fit refused the trait:", err)
    assert call(e.ctx, d_rows, V, 0) == (-4, True)
    e.bed_free(d_bed)
