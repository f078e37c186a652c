"""rvt_score_bed_dev under a binary trait: the single-variant score test of a case-control cohort straight from the 2-bit rows of a
resident .bed matrix (three int8 passes over the planes of [v X | res | v], a finisher that takes the weighted diagonal as it
stands) — against the oracle's MetaScore on the imputed matrix, against rvt_score_block on the same matrix as doubles, for both
ways of installing the null model, on a used context, and where the call has to refuse.  tests/test_score_bed_binary_cpu.py
states the arithmetic in numpy."""
import numpy as np
import pytest

import orc
import synth
from test_gpu_metascore import check, engine_factory  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FIELDS = ("U", "V", "effect", "se", "p")
SHARED = (10007, 1000, 4)          # the case the oracle parity and the fp64 comparison both use: built once
_shared = {}


@pytest.fixture(autouse=True)
def poisoned_work_spaces(monkeypatch):
    monkeypatch.setenv("RVT_POISON", "255")   # fresh work spaces hold 0xff bytes: nothing may be read unwritten


def make_case(N, V, d):
    """The generator of test_score_of_resident_bed_rows_matches_the_oracle (1 % missing; columns 3, 5 and 40 special), a
    case-control phenotype from a logistic model in X and column 7, and the oracle's MetaScore of the imputed matrix."""
    if (N, V, d) in _shared:
        return _shared[(N, V, d)]
    rng = np.random.default_rng(N + V)
    maf = 10 ** rng.uniform(-2.5, -0.4, V)
    raw = rng.binomial(2, maf, size=(N, V)).astype(np.float64)
    raw[rng.random((N, V)) < 0.01] = -9.0
    raw[:, 3] = np.where(raw[:, 3] < 0, -9.0, 2.0)            # monomorphic apart from its missing calls
    raw[:, 5] = 0.0
    if V > 40:
        raw[:, 40] = -9.0                                     # nothing but missing calls
    X = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(d - 1)]))
    beta = np.concatenate([[-0.7], 0.3 * rng.normal(size=d - 1)])
    lin = X @ beta + 0.4 * np.maximum(raw[:, 7], 0)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    G = orc.impute_mean(np.asfortranarray(raw))
    rc, o = orc.metascore(G, X, y, 1)
    assert rc == 0
    case = (raw, X, y, G, o)
    if (N, V, d) == SHARED:
        _shared[(N, V, d)] = case
    return case


def resident(eng, raw, dirty_pad=False):
    """The rows of raw in device memory, two rows into the allocation; returns (allocation, address of the first row)."""
    N, V = raw.shape
    cb = (N + 3) // 4
    rows = eng.pack_bed(raw)
    if dirty_pad and N % 4:
        rows[:, -1] |= np.uint8((0xFF << (2 * (N % 4))) & 0xFF)   # 1-bits in the code positions behind sample N - 1
    d_bed = eng.bed_alloc(V + 2)
    eng.bed_upload(d_bed, 0, np.zeros((2, cb), dtype=np.uint8))
    eng.bed_upload(d_bed, 2, rows)
    return d_bed, d_bed + 2 * cb


def as_dict(out):
    return dict(ok=out[0], U=out[1], V=out[2], effect=out[3], se=out[4], p=out[5])


def assert_same_fields(a, b, label):
    """The bound of the quantitative resident test against rvt_score_block (test_gpu_metascore.py): rtol 1e-9, atol 1e-12 max."""
    assert (a["ok"] == b["ok"]).all()
    k = b["ok"].astype(bool)
    worst = {}
    for f in FIELDS:
        x, y = a[f][k], b[f][k]
        worst[f] = float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))
    print(label, "worst relative deviation per field:", worst)
    for f in FIELDS:
        x, y = a[f][k], b[f][k]
        assert np.allclose(x, y, rtol=1e-9, atol=1e-12 * max(np.abs(y).max(), 1e-300)), (f, worst[f])


@pytest.mark.parametrize("N,V,d", [(4099, 70, 2), (4110, 33, 1), SHARED, (3001, 8300, 1), (2003, 40, 13)])
def test_binary_score_of_resident_rows_matches_the_oracle(engine_factory, N, V, d):
    """N = 4099: the byte path of the copy pass; N = 4110: its dword path, with 1-bits behind the last sample of every row;
    V = 8300: more than one chunk of 256 slices and a short last slice; d = 13: the widest tile (15 columns)."""
    raw, X, y, G, o = make_case(N, V, d)
    eng = engine_factory()
    eng.fit_null(1, X, y)
    d_bed, rows = resident(eng, raw, dirty_pad=(N == 4110))
    out = eng.score_bed_dev(rows, V)
    assert o["ok"].sum() > V // 2
    check(o, as_dict(out))
    want_cnt = np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1)
    assert np.array_equal(out[6], want_cnt)
    eng.bed_free(d_bed)


def test_binary_score_across_a_wave_part_boundary(engine_factory):
    """More samples than the 131 072 one wave-part's int32 sums may hold."""
    N, V, d = 140003, 40, 2
    raw, X, y, G, o = make_case(N, V, d)
    eng = engine_factory()
    eng.fit_null(1, X, y)
    d_bed, rows = resident(eng, raw)
    out = eng.score_bed_dev(rows, V)
    check(o, as_dict(out))
    want_cnt = np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1)
    assert np.array_equal(out[6], want_cnt)
    eng.bed_free(d_bed)


def test_binary_score_of_resident_rows_matches_the_fp64_kernel(engine_factory, monkeypatch):
    """The same imputed matrix as doubles through rvt_score_block on a context without the integer kernels."""
    N, V, d = SHARED
    raw, X, y, G, o = make_case(N, V, d)
    eng = engine_factory()
    eng.fit_null(1, X, y)
    d_bed, rows = resident(eng, raw)
    r = as_dict(eng.score_bed_dev(rows, V, want_counts=False))
    eng.bed_free(d_bed)
    monkeypatch.setenv("RVT_HARDCALL", "0")
    ref = engine_factory()
    ref.fit_null(1, X, y)
    ptr = ref.upload_block(G)
    f = ref.score_block(ptr, V)
    ref.free_block(ptr)
    assert_same_fields(r, f, "packed rows against fp64 blocks")


def test_binary_score_after_fit_null_and_after_set_null(engine_factory):
    """The null model fitted on the device, and the caller's residuals and weights: the same statistics."""
    N, V, d = 4099, 70, 3
    X, y, res, v, s2 = synth.make_null(N, d, 1, 11)
    rng = np.random.default_rng(5)
    raw = rng.binomial(2, 10 ** rng.uniform(-2.3, -0.4, V), size=(N, V)).astype(np.float64)
    raw[rng.random((N, V)) < 0.01] = -9.0
    outs = []
    for fitted in (True, False):
        eng = engine_factory()
        if fitted:
            eng.fit_null(1, np.asfortranarray(X), y)
        else:
            eng.set_null(1, np.asfortranarray(X), res, v)
        d_bed, rows = resident(eng, raw)
        outs.append(as_dict(eng.score_bed_dev(rows, V, want_counts=False)))
        eng.bed_free(d_bed)
    assert outs[0]["ok"].sum() > V // 2
    assert_same_fields(outs[0], outs[1], "fit_null against set_null")


def test_binary_score_after_gene_batches_used_the_work_space(engine_factory):
    """As test_score_of_resident_rows_after_gene_batches_used_the_work_space: 2 048 genes first (under a binary null they take
    the expanded route), then the score test of the same matrix — equal to that of a fresh context, and to a second call."""
    N, V = 20011, 4096
    rng = np.random.default_rng(78)
    raw = rng.binomial(2, 10 ** rng.uniform(-2.3, -0.5, V), size=(N, V)).astype(np.float64)
    raw[rng.random((N, V)) < 0.02] = -9.0
    X = np.asfortranarray(np.column_stack([np.ones(N), rng.normal(size=N)]))
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(0.8 - 0.3 * X[:, 1]))).astype(np.float64)
    outs = []
    for dirty in (True, False):
        eng = engine_factory()
        eng.fit_null(1, X, y)
        cb = (N + 3) // 4
        d_bed = eng.bed_alloc(V)
        eng.bed_upload(d_bed, 0, eng.pack_bed(raw))
        if dirty:
            Ms = rng.integers(20, 81, 2048)
            first = rng.integers(0, V - 80, 2048)
            for g0 in range(0, 2048, 64):
                eng.submit_genes_bed_dev(list(range(g0, g0 + 64)), [d_bed + int(f) * cb for f in first[g0:g0 + 64]], Ms[g0:g0 + 64])
                eng.collect_ready()
            assert len(eng.collect()) > 0
        outs.append(eng.score_bed_dev(d_bed, V))
        if dirty:
            outs.append(eng.score_bed_dev(d_bed, V))
        eng.bed_free(d_bed)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    assert outs[0][0].sum() > V // 2


def test_binary_score_refusals_leave_the_context_usable(engine_factory):
    """More covariates than the tile holds, and a null model whose weighted column the digit planes cannot carry (one entry
    2^16 times beyond the typical one): RVT_E_STATE, never a weaker result — and a quantitative null model on the same context
    scores the rows afterwards."""
    import rvtests_amd
    N, V = 2003, 40
    rng = np.random.default_rng(9)
    raw = rng.binomial(2, 10 ** rng.uniform(-2.0, -0.4, V), size=(N, V)).astype(np.float64)
    raw[rng.random((N, V)) < 0.01] = -9.0
    G = orc.impute_mean(np.asfortranarray(raw))
    Xq = np.asfortranarray(np.column_stack([np.ones(N), rng.normal(size=N)]))
    yq = 0.3 * Xq[:, 1] + rng.normal(size=N)
    rc, o = orc.metascore(G, Xq, yq, 0)
    assert rc == 0

    def quantitative_still_works(eng):
        eng.fit_null(0, Xq, yq)
        d_bed, rows = resident(eng, raw)
        check(o, as_dict(eng.score_bed_dev(rows, V)))
        eng.bed_free(d_bed)

    X14 = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(13)]))
    yb = (rng.random(N) < 0.4).astype(np.float64)
    eng = engine_factory()
    eng.fit_null(1, X14, yb)
    d_bed, rows = resident(eng, raw)
    with pytest.raises(rvtests_amd.RvtError, match="13 covariates"):
        eng.score_bed_dev(rows, V)
    eng.bed_free(d_bed)
    quantitative_still_works(eng)

    X, y, res, v, s2 = synth.make_null(N, 2, 1, 12)
    X = np.asfortranarray(X).copy(order="F")
    X[:, 1] = 1.0
    X[17, 1] = 1e7
    eng = engine_factory()
    eng.set_null(1, X, res, v)
    d_bed, rows = resident(eng, raw)
    with pytest.raises(rvtests_amd.RvtError, match="digit planes"):
        eng.score_bed_dev(rows, V)
    eng.bed_free(d_bed)
    quantitative_still_works(eng)
