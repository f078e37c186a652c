"""GPU: FamSKAT, FamCMC and FamZeggini from rows of a resident .bed matrix (rvt_run_fam_tests_bed_dev) under the three installed
forms of U, against the fp64 block route (rvt_run_fam_tests) on the uploaded imputed columns of the same calls and against the
oracle.  Every test lays the genes out the same way: packed with set padding bits, behind an odd number of other rows (odd row
addresses when the pitch is odd, N = 515: 129 bytes), handed over in descending address order, one row shared by two genes."""
import ctypes as C

import numpy as np
import pytest

import fam_bed_cases
import fam_genes_bed_cases as cases
import orc
from test_fam_cpu import make_family_case
from test_gpu_fam import device_null_for_oracle
from test_gpu_fam_bed import install_family, resident
from test_gpu_kinship_bed import calls as kinship_calls, with_null
from test_gpu_kinship_families import null_for_layout, p_close, rel, spd_cohort
from test_gpu_single_fam import grm_case

pytestmark = pytest.mark.gpu

FAM_ALL = 16 | 32 | 64   # RVT_TEST_FAMSKAT | FAMCMC | FAMZEGGINI
LEAD = 3


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


def bed_call(eng, base, N, order, tests):
    cb = (N + 3) // 4
    return eng.run_fam_tests_bed_dev([base + g[1] * cb for g in order], [g[2] for g in order],
                                     ids=100 + np.arange(len(order)), tests=tests)


def both_routes(eng, raw, genes, tests=FAM_ALL):
    """(records from the resident rows, records of the block route on the uploaded imputed columns, the genes in call order)"""
    order = genes[::-1]
    d_bed, base = resident(eng, raw, lead=LEAD)
    bed = bed_call(eng, base, raw.shape[0], order, tests)
    eng.bed_free(d_bed)
    ptrs = [eng.upload_block(cases.gene_columns(raw, g)) for g in order]
    blk = eng.run_fam_blocks(ptrs, [g[2] for g in order], ids=100 + np.arange(len(order)), tests=tests)
    for p in ptrs:
        eng.free_block(p)
    return bed, blk, order


def bits(r):
    return bytes(r)   # the whole record: every field as the bits it holds


BURDEN = (("famcmc_ok", "famcmc_af", "famcmc_U", "famcmc_V", "famcmc_p"), ("famzeg_ok", "famzeg_af", "famzeg_U", "famzeg_V", "famzeg_p"))


def p_same(a, b):
    """p_close, or the very same value (the reference hands out -1 where Davies' method fails: the hand-made gene)"""
    return a == b or p_close(a, b)


def check_close(bed, blk):
    """The between-routes figures of test_gpu_fam_bed.py::check_routes (U, V 1e-8, af 1e-9, p_close), and Q 1e-7."""
    for b, k in zip(bed, blk):
        for f in ("gene_id", "n_variants", "n_poly", "famskat_ok", "famcmc_ok", "famzeg_ok", "skat_nlambda"):
            assert getattr(b, f) == getattr(k, f), f
        if k.famskat_ok:
            print("gene %d: Q relative difference between the routes %.3g" % (k.gene_id, abs(b.famskat_Q - k.famskat_Q) / k.famskat_Q))
            assert rel(b.famskat_Q, k.famskat_Q, 1e-7) and p_same(b.famskat_p, k.famskat_p)
        for ok, af, u, v, p in BURDEN:
            if getattr(k, ok):
                assert rel(getattr(b, u), getattr(k, u), 1e-8) and rel(getattr(b, v), getattr(k, v), 1e-8)
                assert rel(getattr(b, af), getattr(k, af), 1e-9) and p_same(getattr(b, p), getattr(k, p))


def check_oracle(records, order, raw, X, y, U, S, onul, tests=FAM_ALL):
    """The tolerances of test_fam_burden_matches_oracle / test_famskat_matches_oracle; the counts keep the comparison from
    passing empty: at least four FamSKAT records, four (gene, burden test) pairs and one NA record."""
    n_skat = n_burden = n_na = 0
    for r, gene in zip(records, order):
        G = cases.gene_columns(raw, gene)
        rc, o = orc.famskat(G, X, y, U, S, onul)
        assert r.n_variants == gene[2] and r.n_poly == o.n_poly, gene[0]
        assert r.famskat_ok == (1 if rc == 0 and tests & 16 else 0), gene[0]
        if r.famskat_ok:
            n_skat += 1
            assert abs(r.famskat_Q - o.Q) <= 1e-7 * o.Q, gene[0]
            assert r.skat_nlambda == o.n_lambda
            assert abs(r.famskat_p - o.pvalue) <= 2e-6 * abs(o.pvalue) + 1e-12, gene[0]
        any_ok = r.famskat_ok
        for which, (ok, af, u, v, p) in enumerate(BURDEN):
            rc, o = orc.fam_burden(G, X, y, U, S, onul, which)
            assert getattr(r, ok) == (1 if rc == 0 and tests & (32 << which) else 0), (gene[0], which)
            if not getattr(r, ok):
                continue
            n_burden += 1
            any_ok = 1
            assert r.n_poly == o.num_site
            assert abs(getattr(r, u) - o.U) <= 1e-8 * abs(o.U) + 1e-12, gene[0]
            assert abs(getattr(r, v) - o.V) <= 1e-8 * o.V, gene[0]
            assert abs(getattr(r, af) - o.af) <= 1e-9 * abs(o.af) + 1e-15, gene[0]
            assert abs(getattr(r, p) - o.pvalue) <= 1e-6 * o.pvalue, gene[0]
        n_na += 0 if any_ok else 1
    assert n_skat >= (4 if tests & 16 else 0) and n_burden >= (4 if tests & 96 else 0) and n_na >= 1, (n_skat, n_burden, n_na)


# ---- 1. the family form: bit for bit ------------------------------------------------------------------------------------------
def test_family_form_records_bit_equal_the_block_route_and_match_the_oracle(eng):
    c, X, y, _, Ub, S, nul = install_family(eng, 0)
    raw, genes = cases.gene_set(c.N, 500)
    bed, blk, order = both_routes(eng, raw, genes)
    for b, k, gene in zip(bed, blk, order):
        assert bits(b) == bits(k), gene[0]
    check_oracle(bed, order, raw, X, y, c.dense(Ub).astype(np.float64), S.astype(np.float64), device_null_for_oracle(nul, X.shape[1]))
    # FamSKAT alone: the same famskat_* fields (here also the kept rows without a missing call alone: M17 no missing)
    alone, blk_alone, _ = both_routes(eng, raw, genes, tests=16)
    for a, b, k in zip(alone, bed, blk_alone):
        assert bits(a) == bits(k)
        assert (a.famskat_ok, a.famskat_Q, a.famskat_p, a.skat_nlambda, a.status) == (b.famskat_ok, b.famskat_Q, b.famskat_p, b.skat_nlambda, b.status)
        assert a.famcmc_ok == 0 and a.famzeg_ok == 0
    only = [g for g in genes if g[0] == "M17 no missing"]
    bed1, blk1, _ = both_routes(eng, raw, only)
    assert bits(bed1[0]) == bits(blk1[0]) and bed1[0].famskat_ok == 1


# ---- 2. dense U on digit planes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(300, 2), (515, 3)])
def test_dense_form_against_the_block_route_and_the_oracle(eng, N, d):
    N, K, U, S, X, y = grm_case(N, d, 41 + N)
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    assert eng.kinship_structure() == 1.0
    nul = eng.fit_fam_null(X, y)
    raw, genes = cases.gene_set(N, 500)
    bed, blk, order = both_routes(eng, raw, genes)
    check_close(bed, blk)
    names = [g[0] for g in order]
    i = names.index("M17 no missing")
    assert bits(bed[i]) == bits(blk[i])                       # one exact plane on both routes, in a batch with missing calls
    check_oracle(bed, order, raw, X, y, U, S, device_null_for_oracle(nul, d))
    # a batch without a missing call in any kept row skips the m half; with FamSKAT alone it is the block route's direct path
    only = [g for g in genes if g[0] in ("M17 no missing", "monomorphic")]
    for tests in (FAM_ALL, 16):
        bed1, blk1, _ = both_routes(eng, raw, only, tests=tests)
        assert [bits(r) for r in bed1] == [bits(r) for r in blk1] and bed1[0].famskat_ok == 1
    # FamSKAT alone on the whole set: a different split of the same integer product
    alone, _, _ = both_routes(eng, raw, genes, tests=16)
    for a, b in zip(alone, bed):
        assert a.famskat_ok == b.famskat_ok and a.skat_nlambda == b.skat_nlambda and a.famcmc_ok == 0 and a.famzeg_ok == 0
        if b.famskat_ok:
            assert rel(a.famskat_Q, b.famskat_Q, 1e-7)
    check_oracle(alone, order, raw, X, y, U, S, device_null_for_oracle(nul, d), tests=16)


# ---- 2b. one gene whose kept rows are not consecutive, rows at every byte alignment ------------------------------------------------
def scattered_families(N, seed):
    """Nuclear families of 4 (make_family_case's block) whose members are scattered over the sample order, singletons for the
    rest: (U, S, X, y) with four non-zeros per eigenvector at rows far apart — the column-compressed form of rvt_set_kinship."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N)
    s4, u4 = np.linalg.eigh(np.array([[1, 0, .5, .5], [0, 1, .5, .5], [.5, .5, 1, .5], [.5, .5, .5, 1]]))
    U, S = np.zeros((N, N)), np.ones(N)
    for f in range(N // 4):
        U[np.ix_(perm[4 * f:4 * f + 4], np.arange(4 * f, 4 * f + 4))] = u4
        S[4 * f:4 * f + 4] = s4
    for k in range(4 * (N // 4), N):
        U[perm[k], k] = 1.0
    U = U.astype(np.float32).astype(np.float64)
    S = S.astype(np.float32).astype(np.float64)
    X = np.column_stack([np.ones(N), rng.standard_normal(N)])
    y = 0.3 * X[:, 1] + (U * np.sqrt(0.4 * S)) @ rng.standard_normal(N) + np.sqrt(0.6) * rng.standard_normal(N)
    return U, S, X, y


@pytest.mark.parametrize("form", ["family", "dense", "gather"])
def test_kept_rows_around_a_dropped_row_at_every_row_alignment(eng, form):
    """N = 515 (pitch 129) and the gene of the four hand-made rows alone: rows 0, 1 and 3 are kept around the monomorphic row 2,
    rows 1 and 3 are flipped, and every kept row has missing calls (row 3 in its last byte only).  The list of kept rows is
    what the rotation, the expansion (gather form: N mod 4 = 3, so its last thread stores sample by sample) and the collapse
    read; the block route on the uploaded imputed columns is the reference."""
    N = 515
    raw = np.asfortranarray(cases.hand_rows(N, 5150))
    gene = ("hand", 0, raw.shape[1])
    flip, keep, mu = cases.decisions(raw)
    assert keep.tolist() == [True, True, False, True] and flip[keep].tolist() == [False, True, True]
    assert ((raw < 0).sum(0) > 0).all() and (raw[:4 * (N // 4), 3] >= 0).all()
    if form == "family":
        c = spd_cohort([64, 1, 33, 5, 64, 3, 64, 1, 64, 64, 64, 33, 55], 61)
        assert c.N == N
        rng = np.random.default_rng(62)
        X = np.column_stack([np.ones(N), rng.standard_normal(N)])
        y = 0.3 * X[:, 1] + rng.standard_normal(N)
        null_for_layout(eng, N)
        eng.kinship_decompose_families(c.fam_ptr, c.members, c.flat(c.K), install=True)
    elif form == "dense":
        N, K, U, S, X, y = grm_case(N, 3, 41 + N)
        null_for_layout(eng, N)
        eng.set_kinship(U, S)
        assert eng.kinship_structure() == 1.0
    else:
        U, S, X, y = scattered_families(N, 63)
        null_for_layout(eng, N)
        eng.set_kinship(U, S)
        assert eng.kinship_structure() != 1.0                 # column-compressed U: the kept rows are expanded on the device
    eng.fit_fam_null(X, y)
    bed, blk, order = both_routes(eng, raw, [gene])
    assert bed[0].n_variants == 4 and bed[0].n_poly == 3
    assert blk[0].famskat_ok == 1 and blk[0].famcmc_ok + blk[0].famzeg_ok >= 1   # (the comparison below is not empty)
    if form == "family":
        assert bits(bed[0]) == bits(blk[0])                   # the tile holds the doubles the block route reads
    check_close(bed, blk)


# ---- 3. column-compressed U with scattered supports ------------------------------------------------------------------------------
def test_gather_form_against_the_block_route(eng):
    """Nuclear families as rvt_set_kinship takes them at N = 160 (test_gpu_fam_bed.py::test_pieces_beyond_one_block): the kept
    rows are expanded, flipped, to fp64 on the device and take the gather of rotate_columns."""
    N, K, U, S, X, y = make_family_case(40, 2, 77)
    null_for_layout(eng, N)
    eng.set_kinship(U, S)
    assert eng.kinship_structure() != 1.0
    nul = eng.fit_fam_null(X, y)
    raw, genes = cases.gene_set(N, 500)
    bed, blk, order = both_routes(eng, raw, genes)
    check_close(bed, blk)
    check_oracle(bed, order, raw, X, y, U, S, device_null_for_oracle(nul, X.shape[1]))


# ---- 4. the chain, independence of earlier work, the refusals --------------------------------------------------------------------
def test_chain_from_resident_rows_to_the_gene_tests(eng):
    """bed upload -> kinship_from_bed(install=True) -> fit_fam_null -> run_fam_tests_bed_dev on genes of the same rows."""
    N, V = 300, 2000
    X, y = with_null(eng, N)
    G = kinship_calls(N, V, 0.05, special=False)
    d_bed = eng.bed_alloc(V)
    eng.bed_upload(d_bed, 0, eng.pack_bed(G))
    eng.kinship_from_bed(d_bed, V, method="bn", install=True)
    nul = eng.fit_fam_null(X, y)
    assert np.isfinite(nul.delta)
    raw = np.asfortranarray(G.astype(np.float64))
    order = [("d", 1500, 64), ("c", 40, 17), ("b", 30, 20), ("a", 7, 1)]       # b and c share rows 40 .. 49
    bed = bed_call(eng, d_bed, N, order, FAM_ALL)
    ptrs = [eng.upload_block(cases.gene_columns(raw, g)) for g in order]
    blk = eng.run_fam_blocks(ptrs, [g[2] for g in order], ids=100 + np.arange(len(order)), tests=FAM_ALL)
    check_close(bed, blk)
    assert sum(r.famskat_ok for r in bed) >= 3 and sum(r.famcmc_ok + r.famzeg_ok for r in bed) >= 6
    eng.bed_free(d_bed)


def test_records_do_not_depend_on_earlier_work_on_the_context(eng):
    c, X, y, other, Ub, S, nul = install_family(eng, 0)
    raw, genes = cases.gene_set(c.N, 500)
    order = genes[::-1]
    d_bed, base = resident(eng, raw, lead=LEAD)
    first = bed_call(eng, base, c.N, order, FAM_ALL)
    d_other, other_rows = resident(eng, other)
    eng.score_bed_dev_fam(other_rows, other.shape[1])
    ptr = eng.upload_block(fam_bed_cases.imputed(other))
    eng.run_fam_blocks([ptr], [other.shape[1]], tests=FAM_ALL)
    again = bed_call(eng, base, c.N, order, FAM_ALL)
    assert [bits(r) for r in again] == [bits(r) for r in first]
    assert sum(r.famskat_ok for r in first) >= 4
    eng.free_block(ptr)
    eng.bed_free(d_other)
    eng.bed_free(d_bed)


@pytest.mark.parametrize("form", ["family", "dense"])
def test_no_work_space_is_read_before_it_is_written(eng, monkeypatch, form):
    """The same call again with every work space that is large enough refilled with 0xff bytes in front of the call
    (RVT_SCRIBBLE, DevBuf::grow): bit-equal records."""
    if form == "family":
        N = install_family(eng, 0)[0].N
    else:
        N, K, U, S, X, y = grm_case(300, 2, 341)
        null_for_layout(eng, N)
        eng.set_kinship(U, S)
        eng.fit_fam_null(X, y)
    raw, genes = cases.gene_set(N, 500)
    order = genes[::-1]
    d_bed, base = resident(eng, raw, lead=LEAD)
    small_first = bed_call(eng, base, N, order[:2], FAM_ALL)
    first = bed_call(eng, base, N, order, FAM_ALL)
    monkeypatch.setenv("RVT_SCRIBBLE", "255")
    again = bed_call(eng, base, N, order, FAM_ALL)
    smaller = bed_call(eng, base, N, order[:2], FAM_ALL)          # fewer rows under the same, larger blocks
    monkeypatch.delenv("RVT_SCRIBBLE")
    assert [bits(r) for r in again] == [bits(r) for r in first]
    assert [bits(r) for r in smaller] == [bits(r) for r in small_first]
    assert sum(r.famskat_ok for r in first) >= 4
    eng.bed_free(d_bed)


def test_refusals_write_nothing():
    import rvtests_amd
    from rvtests_amd.engine import GeneResult
    N = 50
    raw = fam_bed_cases.calls(N, 9, seed=3)
    e = rvtests_amd.Engine(0)
    try:
        L = e.L
        L.rvt_run_fam_tests_bed_dev.restype = C.c_int
        L.rvt_run_fam_tests_bed_dev.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                                C.c_uint32, C.POINTER(GeneResult)]
        null_for_layout(e, N)
        d_bed, d_rows = resident(e, raw)
        cb = (N + 3) // 4

        def call(rows, Ms, tests, ctx=e.ctx):
            """(return code, whether the pre-filled records are as they were)"""
            n = len(Ms)
            out = (GeneResult * n)()
            C.memset(out, 0x5A, C.sizeof(out))
            before = bytes(out)
            rc = L.rvt_run_fam_tests_bed_dev(ctx, n, (C.c_void_p * n)(*rows), (C.c_int * n)(*Ms), None, tests, out)
            return rc, bytes(out) == before

        good = [d_rows + 5 * cb, d_rows]
        assert call(good, [4, 5], FAM_ALL) == (-4, True)                       # no family null model
        members = np.arange(N, dtype=np.int32)
        e.set_kinship_families(np.arange(N + 1, dtype=np.int64), members, np.ones(N, dtype=np.float32), np.ones(N, dtype=np.float32))
        rng = np.random.default_rng(5)
        e.fit_fam_null(np.column_stack([np.ones(N), rng.standard_normal(N)]), rng.standard_normal(N))
        assert call(good, [4, 5], 0) == (-1, True)
        assert call(good, [4, 5], FAM_ALL | 1) == (-1, True)
        assert call(good, [4, 0], FAM_ALL) == (-5, True)
        assert call(good, [4, 1024 + 1], FAM_ALL) == (-5, True)
        assert call([d_rows, None], [4, 5], FAM_ALL) == (-1, True)
        assert L.rvt_run_fam_tests_bed_dev(e.ctx, 2, None, (C.c_int * 2)(4, 5), None, FAM_ALL, (GeneResult * 2)()) == -1
        assert L.rvt_run_fam_tests_bed_dev(e.ctx, 0, None, None, None, FAM_ALL, None) == 0
        null_for_layout(e, N + 10)                                             # an ordinary null model of another N
        assert call(good, [4, 5], FAM_ALL) == (-4, True)
        null_for_layout(e, N)
        rc, untouched = call(good, [4, 5], FAM_ALL)
        assert rc == 0 and not untouched
        e.bed_free(d_bed)
    finally:
        e.close()
