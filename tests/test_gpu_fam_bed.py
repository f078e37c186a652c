"""GPU: famScore and famLRT from rows of a resident .bed matrix (rvt_score_bed_dev_fam, rvt_lrt_bed_dev_fam, and their front
stage through rvt_debug_rotate_bed) under the three installed forms of U — the family form, dense digit planes, the
column-compressed gather — against numpy, against the fp64 block route on the uploaded imputed columns of the same calls, and
against the oracle.  The rows hold every row kind of fam_bed_cases.HAND_ROWS, carry set padding bits, and lie behind an odd
number of other rows (odd row addresses when the pitch is odd, N = 515: 129 bytes)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fam_bed_cases
import orc
import rotref
from test_fam_cpu import make_family_case
from test_gpu_kinship_bed import calls as kinship_calls, with_null
from test_gpu_kinship_families import blocks_of, null_for_layout, p_close, rel, spd_cohort
from test_gpu_single_fam import grm_case

pytestmark = pytest.mark.gpu

N_HAND = len(fam_bed_cases.HAND_ROWS)


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


def resident(eng, raw, lead=1):
    """The packed rows behind `lead` other rows of one allocation: (d_bed, device address of the first of them)."""
    rows = fam_bed_cases.pack(raw)
    V, cb = rows.shape
    d_bed = eng.bed_alloc(lead + V)
    eng.bed_upload(d_bed, 0, np.full((lead, cb), 0xE4, dtype=np.uint8))
    eng.bed_upload(d_bed, lead, rows)
    return d_bed, d_bed + lead * cb


def both_routes(eng, raw, binary):
    """(score, lrt) of the resident rows and of the uploaded imputed columns of the same calls."""
    V = raw.shape[1]
    d_bed, d_rows = resident(eng, raw)
    bed = eng.score_bed_dev_fam(d_rows, V, binary), eng.lrt_bed_dev_fam(d_rows, V)
    eng.bed_free(d_bed)
    ptr = eng.upload_block(fam_bed_cases.imputed(raw))
    blk = eng.score_block_fam(ptr, V, binary), eng.lrt_block_fam(ptr, V)
    eng.free_block(ptr)
    return bed, blk


SCORE, LRT = ("U", "V", "af", "p"), ("af", "null_ll", "alt_ll", "p")


def check_routes(raw, bed, blk):
    """ok equal everywhere; where ok: U, V within 1e-8 relative, af 1e-9, p within p_close, log-likelihoods 1e-9 relative — the
    figures between routes of test_gpu_kinship_families.py and test_gpu_metascore.py.  The counts are numpy's."""
    cnt = fam_bed_cases.site_pass(raw)[0]
    for got, want, tol in ((bed[0], blk[0], dict(U=1e-8, V=1e-8, af=1e-9)), (bed[1], blk[1], dict(af=1e-9, null_ll=1e-9, alt_ll=1e-9))):
        assert np.array_equal(got["ok"], want["ok"])
        assert np.array_equal(got["counts"], cnt)
        k = want["ok"] == 1
        assert k.sum() >= 10
        for f, t in tol.items():
            worst = np.max(np.abs(got[f][k] - want[f][k]) / np.maximum(np.abs(want[f][k]), 1e-300))
            print("%s: worst relative difference between the routes %.3g (allowed %.0e)" % (f, worst, t))
            assert rel(got[f][k], want[f][k], t), f
        assert p_close(got["p"][k], want["p"][k])
    assert bed[0]["ok"][-N_HAND + 3] == 0 and bed[1]["ok"][-N_HAND + 3] == 0      # the row with no called sample


def bit_equal(bed, blk):
    for got, want, fields in ((bed[0], blk[0], SCORE), (bed[1], blk[1], LRT)):
        if not np.array_equal(got["ok"], want["ok"]):
            return False
        for f in fields:
            if not np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64)):
                return False
    return True


def check_oracle(eng, raw, X, y, U, S, nul, binary, r):
    """score_bed_dev_fam against orc.fam_burden per column, as test_score_block_fam_matches_oracle holds score_block_fam."""
    d = X.shape[1]
    b = 1.0
    if binary:
        alpha, b = eng.fam_binary_scale(int((y == 1).sum()), int((y == 0).sum()))
    onul = orc.FamNull()
    onul.ok = 1
    onul.delta, onul.sigma2 = nul.delta, nul.sigma2_g
    for k in range(d):
        onul.beta[k] = nul.beta[k]
    G = fam_bed_cases.imputed(raw)
    tested = refused = 0
    for h in range(G.shape[1]):
        rc, o = orc.fam_burden(G[:, [h]], X, y, U, S, onul, 3 if binary else 2)
        assert r["ok"][h] == (1 if rc == 0 else 0), h
        if rc:
            refused += 1
            continue
        tested += 1
        assert abs(r["U"][h] - o.U * b) <= 1e-8 * abs(o.U * b) + 1e-12
        assert abs(r["V"][h] - o.V * b * b) <= 1e-8 * o.V * b * b
        assert abs(r["af"][h] - o.af) <= 1e-9 * abs(o.af) + 1e-15
        assert abs(r["p"][h] - o.pvalue) <= 1e-6 * o.pvalue
    assert tested >= 10 and refused >= 4, (tested, refused)


# ---- 1. the family form ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_case():
    """Families of 64, 33, 5, 3 and singletons, members interleaved; one more singleton makes N = 237 = 4 * 59 + 1."""
    c = spd_cohort([64, 1, 1, 5, 33, 1, 64, 3, 64, 1], 51)
    assert c.N == 237
    rng = np.random.default_rng(52)
    X = np.column_stack([np.ones(c.N), rng.standard_normal(c.N), rng.standard_normal(c.N)])
    fam_effect = np.concatenate([np.full(sz, rng.standard_normal()) for sz in c.sizes])
    y = np.empty(c.N)
    y[c.members] = fam_effect
    y += 0.3 * X[:, 1] + rng.standard_normal(c.N)
    raw = fam_bed_cases.calls(c.N, 37, seed=1234)
    raw.setflags(write=False)
    return c, X, y, raw


def install_family(eng, binary):
    c, X, y, raw = family_case()
    if binary:
        y = (y > np.median(y)).astype(float)
    null_for_layout(eng, c.N)                                 # (the .bed calls take the rows' pitch from it)
    U_flat, S, _ = eng.kinship_decompose_families(c.fam_ptr, c.members, c.flat(c.K), install=True)
    nul = eng.fit_fam_null(X, y)
    if binary:
        eng.fam_binary_scale(int((y == 1).sum()), int((y == 0).sum()))
    return c, X, y, raw, blocks_of(c, U_flat), S, nul


def test_family_form_rotation_against_numpy(eng):
    """debug_rotate_bed against numpy's fp64 U'G of the imputed columns within SpdCohort's 2 k 2^-53 sum |u_r g_r|; two calls
    agree bit for bit; and so does the fp64 route on the uploaded imputed columns (the tile holds the same doubles)."""
    c, X, y, raw, Ub, S, nul = install_family(eng, 0)
    V = raw.shape[1]
    G = fam_bed_cases.imputed(raw)
    want, bound = c.rotate(Ub, G)
    d_bed, d_rows = resident(eng, raw)
    for ncols in (1, 17, V):
        got = eng.debug_rotate_bed(d_rows, ncols)
        err = np.abs(got - want[:, :ncols])
        print("ncols %d: worst error / bound %.3g" % (ncols, (err / np.maximum(bound[:, :ncols], 1e-300)).max()))
        assert np.isfinite(got).all() and (err <= bound[:, :ncols]).all()
        assert np.array_equal(got.view(np.uint64), eng.debug_rotate_bed(d_rows, ncols).view(np.uint64))
    ptr = eng.upload_block(G)
    assert np.array_equal(got.view(np.uint64), eng.debug_rotate(ptr, V).view(np.uint64))
    eng.free_block(ptr)
    eng.bed_free(d_bed)


@pytest.mark.parametrize("binary", [0, 1])
def test_family_form_routes_bits_and_oracle(eng, binary):
    c, X, y, raw, Ub, S, nul = install_family(eng, binary)
    bed, blk = both_routes(eng, raw, binary)
    check_routes(raw, bed, blk)
    full = raw[:, (raw >= 0).all(0)]                          # the rows without a missing call: bit for bit
    assert full.shape[1] >= 5
    assert bit_equal(*both_routes(eng, full, binary))
    check_oracle(eng, raw, X, y, c.dense(Ub).astype(np.float64), S.astype(np.float64), nul, binary, bed[0])


# ---- 2. dense U on digit planes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case():
    """N = 515: pitch 129, K padded to 640 bytes, three row panels."""
    N, K, U, S, X, y = grm_case(515, 3, 120 + 515)
    raw = fam_bed_cases.calls(N, 64, seed=4321)
    raw.setflags(write=False)
    return N, U, S, X, y, raw


def install_dense(eng, binary):
    N, U, S, X, y, raw = dense_case()
    if binary:
        y = (y > np.median(y)).astype(float)
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    assert eng.kinship_structure() == 1.0
    nul = eng.fit_fam_null(X, y)
    if binary:
        eng.fam_binary_scale(int((y == 1).sum()), int((y == 0).sum()))
    return N, U, S, X, y, raw, nul


def test_dense_rotation_against_the_integer_statement(eng):
    """debug_rotate_bed against tests/rotref.py's statement of the quantised product of the imputed columns (six planes: the
    batch holds non-integer fill values), within the accumulation bound that tests/test_gpu_rotate.py holds the dense kernel to
    for such a batch (rotref.rotation_bounds' acc).  The device forms U'c + mu U'm from two exact single-plane products with mu
    in the statement's fixed point, i.e. the statement's integer sum split in two: 6 + 6 plane additions and one fma, fewer
    roundings of smaller partial sums than the 36 plane pairs acc allows for.  (With the unrounded mu a rare column — small
    sum |g|, hence a small acc — misses this bound by the statement's own 2^-39 rounding of mu: 43 x acc in numpy.)"""
    N, U, S, X, y, raw, nul = install_dense(eng, 0)
    V = raw.shape[1]
    G = fam_bed_cases.imputed(raw)
    U32 = np.asfortranarray(U.astype(np.float32))
    ref, planes = rotref.exact_rotation(U32, G)
    assert planes == rotref.PLANES_G
    slices = rotref.k_slices(N, V, planes)
    acc, uq, gq = rotref.rotation_bounds(N, planes, slices, np.abs(G).sum(0), float(np.abs(U32).max()), np.abs(G).max(0))
    d_bed, d_rows = resident(eng, raw)
    got = eng.debug_rotate_bed(d_rows, V)
    err = np.abs(got - ref)
    print("worst error / bound %.3g (bound %.3g .. %.3g)" % ((err / np.maximum(acc[None, :], 1e-300)).max(), acc.min(), acc.max()))
    assert np.isfinite(got).all() and (err <= acc[None, :]).all()
    assert np.array_equal(got.view(np.uint64), eng.debug_rotate_bed(d_rows, V).view(np.uint64))
    eng.bed_free(d_bed)


@pytest.mark.parametrize("binary", [0, 1])
def test_dense_routes_no_missing_subset_and_oracle(eng, binary):
    """The rows without a missing call are ONE exact plane on both routes — the same integer product, the same sums from the
    counts as from the doubles — so they are held to bit equality, not to the 1e-11 the two routes would otherwise owe."""
    N, U, S, X, y, raw, nul = install_dense(eng, binary)
    bed, blk = both_routes(eng, raw, binary)
    check_routes(raw, bed, blk)
    full = raw[:, (raw >= 0).all(0)]
    assert full.shape[1] >= 5
    assert bit_equal(*both_routes(eng, full, binary))
    check_oracle(eng, raw, X, y, U, S, nul, binary, bed[0])


# ---- 3. more rows than one piece ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "gather"])
def test_pieces_beyond_one_block(eng, monkeypatch, form):
    """V = 1100: two pieces, the second of 76 rows (no multiple of 16 or 256); columns equal what separate calls on their row
    ranges return — the contract of test_score_block_fam_chunks_beyond_one_block.  Nuclear families as rvt_set_kinship takes them
    at N = 160 go to the column-compressed gather (the piece is expanded on the device); RVT_KINSHIP_DENSE keeps the planes."""
    if form == "dense":
        monkeypatch.setenv("RVT_KINSHIP_DENSE", "1")
    N, K, U, S, X, y = make_family_case(40, 2, 77)
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    assert (eng.kinship_structure() == 1.0) == (form == "dense")
    eng.fit_fam_null(X, y)
    V = 1100
    raw = fam_bed_cases.calls(N, V - N_HAND, seed=99, maf_hi=-0.7)
    d_bed, d_rows = resident(eng, raw)
    cb = (N + 3) // 4
    whole = eng.score_bed_dev_fam(d_rows, V), eng.lrt_bed_dev_fam(d_rows, V)
    for lo, hi in ((0, 40), (1000, 1060), (1060, 1100)):
        part = eng.score_bed_dev_fam(d_rows + lo * cb, hi - lo), eng.lrt_bed_dev_fam(d_rows + lo * cb, hi - lo)
        for w, p, fields in zip(whole, part, (SCORE, LRT)):
            assert np.array_equal(p["ok"], w["ok"][lo:hi]) and (p["ok"] == 1).sum() > 5
            assert np.array_equal(p["counts"], w["counts"][lo:hi])
            k = p["ok"] == 1
            for f in fields:
                assert np.allclose(p[f][k], w[f][lo:hi][k], rtol=1e-9, atol=1e-12), f
    ptr = eng.upload_block(fam_bed_cases.imputed(raw))
    check_routes(raw, whole, (eng.score_block_fam(ptr, V), eng.lrt_block_fam(ptr, V)))
    eng.free_block(ptr)
    eng.bed_free(d_bed)


# ---- 4. the chain, and the refusals ----------------------------------------------------------------------------------------------
def test_chain_from_resident_rows_to_the_scan(eng):
    """bed upload -> kinship_from_bed(install=True) -> fit_fam_null -> score_bed_dev_fam / lrt_bed_dev_fam of 200 of the same
    rows: nothing crosses the link as fp64.  Equal to the fp64 route within the route tolerances."""
    N, V = 300, 2000
    X, y = with_null(eng, N)
    G = kinship_calls(N, V, 0.05, special=False)
    rows = eng.pack_bed(G)
    d_bed = eng.bed_alloc(V)
    eng.bed_upload(d_bed, 0, rows)
    K, info, (U, S, dinfo) = eng.kinship_from_bed(d_bed, V, method="bn", install=True)
    nul = eng.fit_fam_null(X, y)
    assert np.isfinite(nul.delta)
    n = 200
    bed = eng.score_bed_dev_fam(d_bed, n), eng.lrt_bed_dev_fam(d_bed, n)
    raw = G[:, :n].astype(np.float64)
    ptr = eng.upload_block(fam_bed_cases.imputed(raw))
    blk = eng.score_block_fam(ptr, n), eng.lrt_block_fam(ptr, n)
    for got, want, tol in ((bed[0], blk[0], dict(U=1e-8, V=1e-8, af=1e-9)), (bed[1], blk[1], dict(af=1e-9, null_ll=1e-9, alt_ll=1e-9))):
        assert np.array_equal(got["ok"], want["ok"])
        k = want["ok"] == 1
        assert k.sum() > 100
        for f, t in tol.items():
            assert rel(got[f][k], want[f][k], t), f
        assert p_close(got["p"][k], want["p"][k])
    eng.free_block(ptr)
    eng.bed_free(d_bed)


def test_refusals_write_nothing_and_singletons_are_a_scaled_copy():
    import rvtests_amd
    N = 50
    raw = fam_bed_cases.calls(N, 9, seed=3)
    V = raw.shape[1]
    SENT = -7.5

    def raw_calls(e, ctx, d_rows, v):
        """(return codes, every output array) of the three C calls with sentinel-filled outputs"""
        L = e.L
        vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.rvt_score_bed_dev_fam.restype = L.rvt_lrt_bed_dev_fam.restype = L.rvt_debug_rotate_bed.restype = C.c_int
        L.rvt_score_bed_dev_fam.argtypes = [vp, vp, C.c_int64, C.c_int, ip] + [dp] * 4 + [vp]
        L.rvt_lrt_bed_dev_fam.argtypes = [vp, vp, C.c_int64, ip] + [dp] * 4 + [vp]
        L.rvt_debug_rotate_bed.argtypes = [vp, vp, C.c_int, dp]
        ok = np.full(V, -77, dtype=np.int32)
        outs = [np.full(V, SENT) for _ in range(4)]
        cnt = np.full((V, 4), -77, dtype=np.int64)
        rot = np.full((N, V), SENT, order="F")
        okp, outp = ok.ctypes.data_as(ip), [o.ctypes.data_as(dp) for o in outs]
        rcs = (L.rvt_score_bed_dev_fam(ctx, vp(d_rows), v, 0, okp, *outp, cnt.ctypes.data_as(vp)),
               L.rvt_lrt_bed_dev_fam(ctx, vp(d_rows), v, okp, *outp, cnt.ctypes.data_as(vp)),
               L.rvt_debug_rotate_bed(ctx, vp(d_rows), int(v), rot.ctypes.data_as(dp)))
        return rcs, [ok, cnt, rot] + outs

    def untouched(arrays):
        return all((a == (SENT if a.dtype == np.float64 else -77)).all() for a in arrays)

    e = rvtests_amd.Engine(0)
    try:
        null_for_layout(e, N)
        d_bed, d_rows = resident(e, raw)
        # no family null model yet
        rcs, arrays = raw_calls(e, e.ctx, d_rows, V)
        assert rcs == (-4, -4, -4) and untouched(arrays)
        # singletons only, through the family form: U = 1 per sample, in the members' order
        members = np.random.default_rng(4).permutation(N).astype(np.int32)
        e.set_kinship_families(np.arange(N + 1, dtype=np.int64), members, np.ones(N, dtype=np.float32), np.ones(N, dtype=np.float32))
        rng = np.random.default_rng(5)
        X = np.column_stack([np.ones(N), rng.standard_normal(N)])
        e.fit_fam_null(X, rng.standard_normal(N))
        # null arguments, V = 0
        for ctx, rows, v in ((None, d_rows, V), (e.ctx, None, V), (e.ctx, d_rows, 0)):
            rcs, arrays = raw_calls(e, ctx, rows, v)
            assert rcs == (-1, -1, -1) and untouched(arrays)
        # the unrelated-looking scaled copy, and both calls run
        G = fam_bed_cases.imputed(raw)
        assert np.array_equal(e.debug_rotate_bed(d_rows, V), G[members])
        bed = e.score_bed_dev_fam(d_rows, V), e.lrt_bed_dev_fam(d_rows, V)
        ptr = e.upload_block(G)
        blk = e.score_block_fam(ptr, V), e.lrt_block_fam(ptr, V)
        e.free_block(ptr)
        assert np.array_equal(bed[0]["ok"], blk[0]["ok"]) and np.array_equal(bed[1]["ok"], blk[1]["ok"])
        k = blk[0]["ok"] == 1
        assert k.sum() >= 5 and rel(bed[0]["U"][k], blk[0]["U"][k], 1e-8) and rel(bed[0]["V"][k], blk[0]["V"][k], 1e-8)
        # an ordinary null model of another N beside the family null: the rows would have another pitch
        null_for_layout(e, N + 10)
        rcs, arrays = raw_calls(e, e.ctx, d_rows, V)
        assert rcs == (-4, -4, -4) and untouched(arrays)
        null_for_layout(e, N)
        assert np.array_equal(e.score_bed_dev_fam(d_rows, V)["U"].view(np.uint64), bed[0]["U"].view(np.uint64))
        e.bed_free(d_bed)
    finally:
        e.close()
