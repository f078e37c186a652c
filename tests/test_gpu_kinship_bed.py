"""GPU: rvt_kinship_from_bed — the empirical kinship of `vcf2kinship --ibs` / `--bn` from rows of a resident .bed matrix —
against the numpy restatement of the reference (tests/kinship_ref.py).
IBS divides the same exact integers on both sides: bit-equal.  BN: both sides sum V products z_i z_j in fp64, each in its own
order; a sum's error is at most V 2^-53 sum |z_i z_j| / n, and sum |z_i z_j| / n <= sqrt(K_ii K_jj) (Cauchy-Schwarz), so
|K_ij - ref_ij| <= (V_used + 16) 2^-52 sqrt(ref_ii ref_jj), the 16 for the roundings of mean, scale and z.
Shapes: N = 203, 515, 1027 — ceil(N/4) = 51, 129, 257, all odd, so every row after the first starts misaligned; each N is
3 past a multiple of 4 (padding pairs in the last byte) and past a power of two (a partial last tile of 128; two, five and
nine sample blocks: off-diagonal tiles too).  V = 1, 67, 1000: one site, a partial slab of 128, several slabs with a partial
last one."""
import functools

import numpy as np
import pytest

import kinship_ref
import rvtests_amd

pytestmark = pytest.mark.gpu

SHAPES_N = (203, 515, 1027)
SHAPES_V = (1, 67, 1000)
EPS = 2.0 ** -52


@pytest.fixture
def engine_factory():
    made = []

    def make():
        e = rvtests_amd.Engine(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


def with_null(eng, N):
    """any quantitative null model of N samples (the .bed calls take N from it)"""
    rng = np.random.default_rng(N)
    X = np.asfortranarray(np.column_stack([np.ones(N), rng.normal(size=N)]))
    y = rng.normal(size=N)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)
    return X, y


@functools.lru_cache(maxsize=None)
def calls(N, V, missing, special=True):
    """(N, V) hard calls, -9 = missing: per-site frequencies in [0.01, 0.5], `missing` of the calls missing, and
    sites (V >= 7)  1 missing everywhere, 2 and 3 monomorphic, 4 all het, 5 all hom-alt;
    samples         N - 2 missing at every site; 1 and 2 never called together (1 is missing at the even sites, 2 is called
                    exactly where 1 is missing): c_12 = 0."""
    rng = np.random.default_rng(1000 * N + V + int(100 * missing))
    f = rng.uniform(0.01, 0.5, V)
    G = rng.binomial(2, f, size=(N, V)).astype(np.int8)
    if missing > 0:
        G[rng.random((N, V)) < missing] = -9
    if special:
        G[N - 2, :] = -9
        G[1, (np.arange(V) % 2) == 0] = -9
        G[2, :] = np.where(G[1, :] < 0, np.maximum(G[2, :], 0), -9)   # called exactly where sample 1 is not
        if V >= 7:   # (the special sites keep the pattern of missing calls)
            G[:, 1] = -9
            for site, call in ((2, 0), (3, 0), (4, 1), (5, 2)):
                G[:, site] = np.where(G[:, site] < 0, -9, call)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def reference(N, V, missing, method, min_maf=0.0, max_missing=1.0, special=True):
    K, info = kinship_ref.kinship(calls(N, V, missing, special), method, min_maf, max_missing)
    K.setflags(write=False)
    return K, info


def upload(eng, rows, lead=0, tail=0):
    """the rows at row `lead` of an allocation of lead + V + tail rows (the others hold 0xE4 bytes: calls 0, missing, 1, 2);
    returns (d_bed, d_rows)"""
    V, cb = rows.shape
    d_bed = eng.bed_alloc(lead + V + tail)
    if lead:
        eng.bed_upload(d_bed, 0, np.full((lead, cb), 0xE4, dtype=np.uint8))
    eng.bed_upload(d_bed, lead, rows)
    if tail:
        eng.bed_upload(d_bed, lead + V, np.full((tail, cb), 0xE4, dtype=np.uint8))
    return d_bed, d_bed + lead * cb


def run(eng, rows, method, lead=0, tail=0, **kw):
    d_bed, d_rows = upload(eng, rows, lead, tail)
    try:
        return eng.kinship_from_bed(d_rows, rows.shape[0], method=method, **kw)
    finally:
        eng.bed_free(d_bed)


def counts_of(info):
    return dict(sites=info.sites, sites_used=info.sites_used, filtered_missing=info.filtered_missing,
                filtered_maf=info.filtered_maf, monomorphic=info.monomorphic)


def check_ibs(K, info, G, ref, ref_info, min_maf=0.0, max_missing=1.0):
    assert counts_of(info) == ref_info
    assert K.shape == ref.shape and (K == ref).all()
    assert (K == K.T).all()
    used = [v for v in range(G.shape[1]) if kinship_ref.site_filter(G[:, v].astype(np.int64), min_maf, max_missing) is None]
    has_call = (G[:, used] >= 0).any(axis=1)
    assert (np.diag(K)[has_call] == 2.0).all() and (np.diag(K)[~has_call] == 0.0).all()


def check_bn(K, info, ref, ref_info):
    assert counts_of(info) == ref_info
    assert (K == K.T).all()
    d = np.sqrt(np.diag(ref))
    bound = (ref_info["sites_used"] + 16) * EPS * np.outer(d, d)
    err = np.abs(K - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("BN: max |K - ref| / bound = %.3g (max |err| %.3g)" % (worst, err.max()))
    assert (err <= bound).all(), worst
    assert (K[np.diag(ref) == 0.0, :] == 0.0).all()   # a sample without a call: its row is exactly zero


@pytest.mark.parametrize("missing", [0.0, 0.05])
@pytest.mark.parametrize("V", SHAPES_V)
@pytest.mark.parametrize("N", SHAPES_N)
def test_ibs_is_bit_equal_to_the_restatement(engine_factory, N, V, missing):
    eng = engine_factory()
    with_null(eng, N)
    G = calls(N, V, missing)
    K, info = run(eng, eng.pack_bed(G), "ibs")
    ref, ref_info = reference(N, V, missing, "ibs")
    check_ibs(K, info, G, ref, ref_info)
    assert K[1, 2] == 0.0 and K[N - 2, 0] == 0.0    # never called together; never called


@pytest.mark.parametrize("missing", [0.0, 0.05])
@pytest.mark.parametrize("V", SHAPES_V)
@pytest.mark.parametrize("N", SHAPES_N)
def test_bn_within_the_summation_bound(engine_factory, N, V, missing):
    eng = engine_factory()
    with_null(eng, N)
    G = calls(N, V, missing)
    K, info = run(eng, eng.pack_bed(G), "bn")
    ref, ref_info = reference(N, V, missing, "bn")
    check_bn(K, info, ref, ref_info)
    if V >= 7:
        assert info.monomorphic >= 4    # the uncalled site, the two monomorphic ones and the all-hom-alt one


def check(method, K, info, G, ref, ref_info, **flt):
    check_ibs(K, info, G, ref, ref_info, **flt) if method == "ibs" else check_bn(K, info, ref, ref_info)


@pytest.mark.parametrize("method", ["ibs", "bn"])
def test_sites_past_one_chunk(engine_factory, method):
    """The driver takes the sites in chunks of 32 768: V = 32 768 + 67 is one full chunk and a partial second one, which starts
    at a row offset, adds to the N x N sums in device memory, reuses the site pass's work space and adds to its totals.
    N = 67 (one partial tile) keeps the restatement's 32 835 sites at about a second."""
    N, V = 67, 32768 + 67
    eng = engine_factory()
    with_null(eng, N)
    G = calls(N, V, 0.05)
    K, info = run(eng, eng.pack_bed(G), method)
    ref, ref_info = reference(N, V, 0.05, method)
    check(method, K, info, G, ref, ref_info)


@pytest.mark.parametrize("method", ["ibs", "bn"])
@pytest.mark.parametrize("N,V,chunk", [(203, 1000, 256), (515, 1000, 200), (1027, 1000, 333), (203, 67, 1)])
def test_small_chunks_give_the_same_kinship(engine_factory, monkeypatch, N, V, chunk, method):
    """RVT_KINSHIP_CHUNK lowers the chunk, so that matrices with several sample blocks (diagonal and off-diagonal tiles) take
    the path of many chunks: 256 = two slabs of 128 sites per chunk, 200 and 333 = chunks that end inside a slab, 1 = a chunk
    per site; the last chunk is partial in each.  The same checks as for one chunk — IBS bit-equal (so also equal to the
    one-chunk result), BN within its bound, the counts summed over the chunks — without and with the filters, whose dropped
    sites differ from chunk to chunk (the drop flags and tables of a chunk must not leak into the next)."""
    monkeypatch.setenv("RVT_KINSHIP_CHUNK", str(chunk))
    eng = engine_factory()
    with_null(eng, N)
    G = calls(N, V, 0.05)
    rows = eng.pack_bed(G)
    for flt in ({}, dict(min_maf=0.05, max_missing=0.06)):
        if flt and N > 515:     # (the filtered restatement of the largest shape is left out: seconds of numpy)
            continue
        ref, ref_info = reference(N, V, 0.05, method, **flt)
        if flt and V == 1000:
            assert 0 < ref_info["sites_used"] < V - 100
        K, info = run(eng, rows, method, **flt)
        check(method, K, info, G, ref, ref_info, **flt)


@pytest.mark.parametrize("method", ["ibs", "bn"])
def test_padding_pairs_contribute_nothing(engine_factory, method):
    """the unused pairs of each row's last byte set to 11 (a call of 2), then to 01 (missing): K and every count as from clean rows"""
    N, V = 203, 67
    eng = engine_factory()
    with_null(eng, N)
    clean = eng.pack_bed(calls(N, V, 0.05))
    high = (0xFF << (2 * (N % 4))) & 0xFF
    K0, info0 = run(eng, clean, method)
    for fill in (0xFF, 0x55):
        dirty = clean.copy()
        dirty[:, -1] = (dirty[:, -1] & ~np.uint8(high)) | np.uint8(fill & high)
        assert (dirty[:, -1] != clean[:, -1]).all()
        K1, info1 = run(eng, dirty, method)
        assert counts_of(info1) == counts_of(info0)
        assert np.array_equal(K1, K0)


@pytest.mark.parametrize("N,V,missing", [(203, 1000, 0.05), (515, 67, 0.0)])
def test_filters(engine_factory, N, V, missing):
    eng = engine_factory()
    with_null(eng, N)
    G = calls(N, V, missing)
    rows = eng.pack_bed(G)
    flt = dict(min_maf=0.05, max_missing=0.03)
    ref, ref_info = reference(N, V, missing, "ibs", **flt)
    assert 0 < ref_info["sites_used"] < V and ref_info["filtered_missing"] > 0 and ref_info["filtered_maf"] > 0
    K, info = run(eng, rows, "ibs", **flt)
    check_ibs(K, info, G, ref, ref_info, **flt)
    ref, ref_info = reference(N, V, missing, "bn", **flt)
    K, info = run(eng, rows, "bn", **flt)
    check_bn(K, info, ref, ref_info)
    # min_maf = 0.5 drops every site but those with af = 0.5 exactly (af < 0.5 || af > 0.5 is false there: the all-het site and
    # whatever the draw made so) — as in the restatement; without those sites everything is dropped and K is all zero
    called = (G >= 0).sum(axis=0)
    half = np.where(G >= 0, G, 0).sum(axis=0) == called     # ac == 2 nonmissing / 2, nothing called included
    assert half[4] and half.sum() < V
    for method in ("ibs", "bn"):
        ref, ref_info = reference(N, V, missing, method, 0.5, 1.0)
        K, info = run(eng, rows, method, min_maf=0.5)
        assert counts_of(info) == ref_info and ref_info["sites_used"] >= 1
        check_ibs(K, info, G, ref, ref_info, min_maf=0.5) if method == "ibs" else check_bn(K, info, ref, ref_info)
        K, info = run(eng, rows[~half], method, min_maf=0.5)
        assert info.sites_used == 0 and info.sites == V - half.sum() and info.filtered_maf == info.sites and (K == 0.0).all()


@pytest.mark.parametrize("method", ["ibs", "bn"])
def test_rows_inside_a_larger_allocation(engine_factory, method):
    """d_rows at row 5 of a larger allocation, other rows behind: the same numbers as the same rows uploaded at row 0"""
    N, V = 515, 67
    eng = engine_factory()
    with_null(eng, N)
    rows = eng.pack_bed(calls(N, V, 0.05))
    K0, info0 = run(eng, rows, method)
    K1, info1 = run(eng, rows, method, lead=5, tail=3)
    assert counts_of(info1) == counts_of(info0) and np.array_equal(K1, K0)


def test_errors(engine_factory):
    N, V = 203, 3
    eng = engine_factory()
    with_null(eng, N)
    d_bed, d_rows = upload(eng, eng.pack_bed(calls(N, V, 0.0)))
    K = np.zeros((N, N))
    Kp = K.ctypes.data_as(rvtests_amd.engine.c_double_p)
    info = rvtests_amd.KinshipInfo()
    f = eng.L.rvt_kinship_from_bed
    INVALID, STATE, TOO_LARGE = -1, -4, -5
    assert f(None, d_rows, V, 1, 0.0, 1.0, Kp, info) == INVALID
    assert f(eng.ctx, None, V, 1, 0.0, 1.0, Kp, info) == INVALID
    assert f(eng.ctx, d_rows, V, 1, 0.0, 1.0, None, info) == INVALID
    assert f(eng.ctx, d_rows, V, 1, 0.0, 1.0, Kp, None) == INVALID
    assert f(eng.ctx, d_rows, 0, 1, 0.0, 1.0, Kp, info) == INVALID
    assert f(eng.ctx, d_rows, V, 2, 0.0, 1.0, Kp, info) == INVALID
    assert f(eng.ctx, d_rows, V, -1, 0.0, 1.0, Kp, info) == INVALID
    for maf in (-0.01, 0.51, float("nan")):
        assert f(eng.ctx, d_rows, V, 0, maf, 1.0, Kp, info) == INVALID
    for mm in (-0.01, 1.01, float("nan")):
        assert f(eng.ctx, d_rows, V, 0, 0.0, mm, Kp, info) == INVALID
    assert f(eng.ctx, d_rows, (1 << 30) + 1, 0, 0.0, 1.0, Kp, info) == TOO_LARGE
    with pytest.raises(ValueError):
        eng.kinship_from_bed(d_rows, V, method="king")
    # no null model: another context (the rows are those of the first, on the same device; the call refuses before it reads them)
    bare = engine_factory()
    assert f(bare.ctx, d_rows, V, 1, 0.0, 1.0, Kp, info) == STATE
    with pytest.raises(rvtests_amd.RvtError, match="-4"):
        bare.kinship_from_bed(d_rows, V)
    assert (K == 0.0).all()     # no refused call wrote anything
    # ... and the accepted call at the limits of the two ranges still works
    K1, info1 = eng.kinship_from_bed(d_rows, V, method="ibs", min_maf=0.0, max_missing=1.0)
    assert info1.sites == V and (np.diag(K1)[0] == 2.0)
    eng.bed_free(d_bed)


def test_chain_to_the_decomposition_and_the_family_null(engine_factory):
    """BN with install=True: the kinship goes through float into rvt_kinship_decompose; the eigenvalues are LAPACK's of the same
    float matrix within tests/test_gpu_decompose.py's bound for its grm case (3e-7 of the largest: float storage of S), and the
    family null model can be fitted on the installed kinship."""
    N, V = 300, 2000
    eng = engine_factory()
    X, y = with_null(eng, N)
    G = calls(N, V, 0.05, special=False)
    K, info, (U, S, dinfo) = run(eng, eng.pack_bed(G), "bn", install=True)
    ref, ref_info = reference(N, V, 0.05, "bn", special=False)
    check_bn(K, info, ref, ref_info)
    lam = np.linalg.eigvalsh(K.astype(np.float32).astype(np.float64))
    assert (np.diff(S) >= 0).all()
    assert np.abs(S - lam).max() <= 3e-7 * np.abs(lam).max()
    assert U.shape == (N, N)
    nul = eng.fit_fam_null(X, y)
    assert np.isfinite(nul.delta) and np.isfinite(nul.sigma2_g)
