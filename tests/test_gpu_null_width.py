"""GPU: every integer kernel at the null-model widths d where its route changes (null_width_cases.py has the models, the route
table, the long-double reference and the bounds; test_null_width_cases_cpu.py checks all of those without a GPU).

What each route is run at, which bound holds its T = G'[tile] and u entry by entry, and what the bound would catch:

* binary blocks, d = 5, 6 (gene_suffstat_hcx; d = 6: the LDS stage of 8 columns is full, and one gene has a fifth of its calls
  mean-imputed in every column, so the masked-entry rounds walk E x 8 items).  T from six digit planes: c_j max|z_k| 2^-40 +
  8 u a_jk.  A digit plane of weight 128^-p that is lost or mis-weighted moves an entry by about 2^(42 - 7 p) units of the first
  term (the lowest one: 2^6, the last PAIR 2^13); scale[k] of a neighbour column is a factor 2^+-1 .. 2^11 on every entry of
  column k (the columns' shifts differ: intercept, age-like, PC-like, just under and exactly at a power of two); a stride
  of 4 * 16 * 7 instead of 4 * 16 * 8 bytes per plane reads column k + 1's digits: an error of the order of the entry itself.
* binary blocks, d = 7, 13 (gene_suffstat_hcw: the tile product is fp64), d = 14, 16 (fp64 kernels): N u a_jk.  S of every
  binary route: sum g g 2^-43 + N u sum v g g — the weights' 42 fractional bits; a lost weight digit of 128^-6 is 2^-42 per
  sample, twice the first term.
* quantitative blocks, d = 13 (gene_suffstat_hc, tile of 14 of 16 columns), d = 14 (fp64): N u a_jk; S of hard calls is exact.
* host 2-bit rows, d = 1, 7, 13 (gene_suffstat_hcp with its fp64 product), d = 14 (expanded: bit-identical to the int8
  hand-off): records only — the rows' statistics are not observable one by one.
* resident rows, d = 1, 4, 8, 12, 13 (gene_tnull_hcp: eight digit planes of ncx = d + 1 columns; rvt_debug_suffstat_bed_dev says
  the planes formed T), d = 14 (expanded).  c_j max|z_k| 2^-54 + 8 u a_jk: the quantisation sits 2^-54 below a column's
  largest entry, the lowest plane PAIR weighs 2^-42 of it — lost or mis-weighted, it misses the bound by a factor ~2^12 x
  the pair's typical digit (test_null_width_cases_cpu.py shows > 100 for that case).  plane_stride = 64 ncx with the wrong
  ncx, or the lane gate v < ncx off by one at ncx = 14, drops or swaps a whole column: errors of the order of T itself.
* rvt_score_bed_dev, quantitative, d = 1, 6, 13 (planes), d = 14 (refused); decimal dosages d = 13 (gene_suffstat_lat) / 14
  (fp64); float dosages d = 6 (gene_suffstat_fdx, 15 of its 16 stage columns) / 7 (fp64).

The debug runs (rvt_debug_suffstat, rvt_debug_suffstat_bed_dev) are batches of one gene under the same plan as the records'
batches: the same kernel (the timing counters are read around them: hard-call, nothing handed back), another split of the
samples into wave-parts at most.  Records are held to the suite's own bars against the oracle; under a binary trait the
burden tests (undefined in the reference with covariates) against the engine's own fp64 route."""
import numpy as np
import pytest

import null_width_cases as nw
import orc

pytestmark = pytest.mark.gpu

FIELDS = ("skat_Q", "skat_p", "skato_Q", "skato_p", "skato_rho", "cmc_U", "cmc_V", "cmc_stat", "cmc_p", "zeg_U", "zeg_V",
          "zeg_stat", "zeg_p", "cmc_nonref", "n_poly", "status")
N0 = 2003


def _install(engine, N, d, binary):
    X, y, res, v, s2 = nw.case_model(N, d, binary)
    engine.set_null(binary, X, res, v, s2)
    return X, y, res, v, s2


def _run_blocks(engine, genes, hard=True):
    """records and timing counters of one batch of fp64 blocks; hard=False confines the engine to the fp64 kernels"""
    ptrs = [engine.upload_block(G) for G, af in genes]
    engine.set_hardcall(hard)
    engine.set_profiling(True)
    engine.timing(reset=True)
    try:
        out = engine.run_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes])
        tm = engine.timing(reset=True)
    finally:
        engine.set_profiling(False)
        engine.set_hardcall(True)
        for p in ptrs:
            engine.free_block(p)
    return out, tm


def _debug_block(engine, G):
    """(S, T, u, counters) of rvt_debug_suffstat on one block"""
    ptr = engine.upload_block(G)
    engine.set_profiling(True)
    engine.timing(reset=True)
    try:
        S, T, u, cs, mn, mx = engine.debug_suffstat(ptr, G.shape[1])
        tm = engine.timing(reset=True)
    finally:
        engine.set_profiling(False)
        engine.free_block(ptr)
    return S, T, u, tm


def _same(a, b):
    for f in FIELDS:
        x, y_ = getattr(a, f), getattr(b, f)
        assert x == y_ or (x != x and y_ != y_), (f, x, y_)


def _check_entries(tag, S, T, u, G, w, tile, d, route, binary, imputed):
    """S, T and u entry by entry against the long-double reference under the route's bounds; zero bounds: exactly zero."""
    S0, T0 = nw.ref_suffstat(G, w, tile[:, :d + 1])
    TU = np.column_stack([T, u])
    bt = nw.t_bound(G, tile[:, :d + 1], route)
    bs = nw.s_bound(G, w, binary, imputed)
    et = np.abs((TU.astype(np.longdouble) - T0).astype(np.float64))
    es = np.abs((S.astype(np.longdouble) - S0).astype(np.float64))
    worst_t = float(np.max(et[bt > 0] / bt[bt > 0])) if np.any(bt > 0) else 0.0
    worst_s = float(np.max(es[bs > 0] / bs[bs > 0])) if np.any(bs > 0) else 0.0
    k_worst = int(np.argmax(np.max(np.where(bt > 0, et / np.where(bt > 0, bt, 1.0), 0.0), axis=0)))
    print("%s %s: worst |T - ref| / bound = %.3g (tile column %d), |S - ref| / bound = %.3g" % (tag, route, worst_t, k_worst, worst_s))
    assert np.all(et[bt == 0] == 0) and np.all(es[bs == 0] == 0), tag
    assert np.all(et <= bt), (tag, route, worst_t, k_worst)
    assert np.all(es <= bs), (tag, route, worst_s)


def _check_records(tag, r, G, af, X, y, res, v, binary):
    """One record against orc.skat / orc.skato / orc.burden at the suite's bars; counts exactly."""
    rc, a = orc.skat(G, af, X, res, v, binary)
    assert r.n_poly == a.n_poly, tag
    if a.n_poly:
        assert abs(r.skat_Q - a.Q) <= 1e-10 * a.Q, (tag, r.skat_Q, a.Q)
        assert abs(r.skat_p - a.pvalue) <= 1e-6 * a.pvalue + 1e-14, (tag, r.skat_p, a.pvalue)
        rc2, o = orc.skato(G, af, X, res, v, binary)
        if rc2 == 0:
            assert abs(r.skato_p - o.pvalue) <= 1e-6 * o.pvalue + 5e-13, (tag, r.skato_p, o.pvalue)
    if binary:
        return                                               # (burden tests: against the engine's fp64 route, by the caller)
    Gf = orc.flip_poly(G)[0]
    for which, ok, stat, nonref in ((0, r.cmc_ok, r.cmc_stat, r.cmc_nonref), (1, r.zeg_ok, r.zeg_stat, None)):
        rc3, b = orc.burden(G, X, y, 0, which)
        if rc3 != 0:
            continue
        if nonref is not None:
            assert nonref == b.nonref_site, tag
        c = orc.collapse(Gf, which)
        if c.min() == c.max():
            continue                                         # every sample carries: U is the sum of the residuals, rounding on both sides
        assert ok and abs(stat - b.stat) <= 1e-9 * b.stat + 1e-13, (tag, which, stat, b.stat)


def _burden_same_as_fp64(tag, a, b, G):
    """binary trait: the integer route's record against the fp64 route's, as test_binary_trait_weighted_hardcall_path holds
    them.  A collapsed genotype that is the same for every sample (wide genes, N = 61: every sample carries) has the variance
    0 up to rounding on either route — its sign decides RVT_ST_CMC_FAIL, its size the statistic: that test's fields and its
    failure bit are not compared (the oracle's own collapse says when)."""
    Gf = orc.flip_poly(G)[0]
    skip = tuple(p for p, which in (("cmc_", 0), ("zeg_", 1)) if np.ptp(orc.collapse(Gf, which)) == 0.0)
    bits = ~np.uint32((4 if "cmc_" in skip else 0) | (8 if "zeg_" in skip else 0))
    assert a.n_poly == b.n_poly and a.cmc_nonref == b.cmc_nonref, tag
    assert np.uint32(a.status) & bits == np.uint32(b.status) & bits, (tag, a.status, b.status)
    for f in FIELDS[:13]:
        if f.startswith(skip) if skip else False:
            continue
        x, y_ = getattr(a, f), getattr(b, f)
        floor = 1e-11 if f in ("cmc_stat", "zeg_stat", "cmc_U", "zeg_U") else 1e-300
        assert abs(x - y_) <= 1e-9 * abs(y_) + floor, (tag, f, x, y_)


# ---- fp64 blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(N0, 5), (N0, 6), (61, 6), (N0, 7), (61, 7), (N0, 13), (N0, 14), (N0, 16)])
def test_binary_blocks_by_width(engine, N, d):
    """hcx at d = 5, 6; hcw at d = 7, 13; the fp64 kernels at d = 14, 16.  gene_suffstat_hcw hands a gene with mean-imputed
    entries to the fp64 kernel (gene_suffstat_hcx keeps it): its genes here have no missing call, and one that has is counted
    as handed back.  The two densely masked genes are what found hcx_masked_slice dropping a slice's masked entries when more
    than kHcxListCap = 48 lanes held one at the same time (the round ended empty): S and T lost their imputed part — every
    T column 1e10 .. 2e11 bounds off, Q wrong by 4 .. 18 % at d = 3, 5 and 6 alike — with no flag raised."""
    route = nw.expected_route(d, 1, "block")
    X, y, res, v, s2 = _install(engine, N, d, 1)
    assert engine.hardcall_kernel() == (None if route == "fp64" else route)
    hcw = route == "gene_suffstat_hcw"
    genes = [nw.gene(N, M, missing=not hcw) for M in (5, 33, 80)]
    if route == "gene_suffstat_hcx" and d == 6:
        genes.append(nw.masked_gene(N, 33))                  # every lane of a slice holds masked entries, many rounds of 48
    if route == "gene_suffstat_hcx" and d == 5:
        genes.append(nw.masked_gene(N, 80, rate=0.02))       # few entries over five tiles: still more than 48 lanes at once
    if hcw:
        genes.append(nw.gene(N, 33, missing=True))
    blocks = [(G, af) for raw, G, af in genes]
    got, tm = _run_blocks(engine, blocks, True)
    ref, tm_ref = _run_blocks(engine, blocks, False)
    assert tm.genes == len(genes) and tm_ref.genes_hard_call == 0
    assert tm.genes_hard_call == (0 if route == "fp64" else len(genes))
    assert tm.genes_handed_back == (1 if hcw else 0)
    tile = nw.null_tile(X, res, v, 1)
    for k, ((raw, G, af), a, b) in enumerate(zip(genes, got, ref)):
        tag = "binary N=%d d=%d M=%d #%d" % (N, d, G.shape[1], k)
        _check_records(tag, a, G, af, X, y, res, v, 1)
        _burden_same_as_fp64(tag, a, b, G)
        S, T, u, tmd = _debug_block(engine, G)
        back = hcw and k == 3
        assert tmd.genes_hard_call == (0 if route == "fp64" else 1) and tmd.genes_handed_back == (1 if back else 0), tag
        _check_entries(tag, S, T, u, G, v, tile, d, "fp64" if back else route, 1, bool((raw < 0).any()))


@pytest.mark.parametrize("N,d", [(N0, 13), (N0, 14), (61, 7)])
def test_quantitative_blocks_by_width(engine, N, d):
    """gene_suffstat_hc up to d = 13 (imputed entries stay on it: the masked-entry tiles), the fp64 kernels from d = 14."""
    route = nw.expected_route(d, 0, "block")
    X, y, res, v, s2 = _install(engine, N, d, 0)
    genes = [nw.gene(N, M, missing=M not in (17, 80)) for M in (1, 17, 33, 80, 96)]
    got, tm = _run_blocks(engine, [(G, af) for raw, G, af in genes], True)
    assert tm.genes == len(genes) and tm.genes_handed_back == 0
    assert tm.genes_hard_call == (0 if route == "fp64" else len(genes))
    tile = nw.null_tile(X, res, v, 0)
    for (raw, G, af), a in zip(genes, got):
        tag = "quantitative N=%d d=%d M=%d" % (N, d, G.shape[1])
        _check_records(tag, a, G, af, X, y, res, v, 0)
        S, T, u, tmd = _debug_block(engine, G)
        assert tmd.genes_hard_call == (0 if route == "fp64" else 1) and tmd.genes_handed_back == 0, tag
        imputed = bool((raw < 0).any())
        _check_entries(tag, S, T, u, G, np.ones(N), tile, d, route, 0, imputed or route == "fp64")


# ---- 2-bit rows -------------------------------------------------------------------------------------------------------------------
def _resident(engine, raws, N):
    """the genes' rows in one resident matrix, three rows of something else in front: (d_bed, [device address of a gene's rows])"""
    cb = (N + 3) // 4
    Ms = [r.shape[1] for r in raws]
    first = np.concatenate([[0], np.cumsum(Ms)[:-1]]) + 3
    d_bed = engine.bed_alloc(int(first[-1] + Ms[-1] + 2))
    engine.bed_upload(d_bed, 0, np.full((3, cb), 0x55, dtype=np.uint8))
    for f, r in zip(first, raws):
        engine.bed_upload(d_bed, int(f), engine.pack_bed(r))
    return d_bed, [d_bed + int(f) * cb for f in first]


def _host_rows(engine, raws):
    engine.set_profiling(True)
    engine.timing(reset=True)
    try:
        afs = [engine.submit_gene_bed(g, engine.pack_bed(r), r.shape[1]) for g, r in enumerate(raws)]
        out = engine.collect()
        tm = engine.timing(reset=True)
    finally:
        engine.set_profiling(False)
    return out, afs, tm


@pytest.mark.parametrize("N,d", [(N0, 1), (N0, 7), (N0, 13), (N0, 14), (61, 7)])
def test_host_rows_by_width(engine, N, d):
    """rvt_submit_gene_bed: gene_suffstat_hcp (fp64 product with the tile) up to d = 13; at d = 14 the rows are expanded and the
    records are those of the int8 hand-off of the same matrix, bit for bit."""
    X, y, res, v, s2 = _install(engine, N, d, 0)
    genes = [nw.gene(N, M, missing=M not in (17, 80)) for M in (1, 17, 33, 80, 96)]
    got, afs, tm = _host_rows(engine, [raw for raw, G, af in genes])
    assert tm.genes == len(genes) and tm.genes_handed_back == 0
    if nw.expected_route(d, 0, "bed") == "expanded":
        assert tm.genes_hard_call == 0
        for g, (raw, G, af) in enumerate(genes):
            engine.submit_gene_raw(g, raw.astype(np.int8), want_af=False)
        for a, b in zip(got, engine.collect()):
            _same(a, b)
    else:
        assert tm.genes_hard_call == len(genes)
    for (raw, G, af), a, f in zip(genes, got, afs):
        assert np.array_equal(f, af)
        _check_records("host rows N=%d d=%d M=%d" % (N, d, G.shape[1]), a, G, af, X, y, res, v, 0)


@pytest.mark.parametrize("N,d", [(N0, 1), (N0, 4), (N0, 8), (N0, 12), (N0, 13), (N0, 14), (61, 7), (20011, 13)])
def test_resident_rows_by_width(engine, N, d):
    """rvt_submit_genes (resident rows) and rvt_debug_suffstat_bed_dev: up to d = 13 the planes form T (planes_used == 1) and
    every entry of T and u is inside c_j max|z_k| 2^-54 + 8 u a_jk; at d = 14 the genes are expanded — the records of the host
    rows bit for bit, and the debug entry refuses.  N = 20 011: twenty wave-parts per gene."""
    import rvtests_amd
    X, y, res, v, s2 = _install(engine, N, d, 0)
    Ms = (1, 17, 33, 80, 96) if N <= N0 else (17, 96)         # (the large cohort: the narrowest and the widest multi-tile class)
    genes = [nw.gene(N, M, missing=M not in (17, 80)) for M in Ms]
    raws = [raw for raw, G, af in genes]
    d_bed, addr = _resident(engine, raws, N)
    try:
        engine.set_profiling(True)
        engine.timing(reset=True)
        try:
            engine.submit_genes_bed_dev(list(range(len(genes))), addr, [r.shape[1] for r in raws])
            got = engine.collect()
            tm = engine.timing(reset=True)
        finally:
            engine.set_profiling(False)
        assert tm.genes == len(genes) and tm.genes_handed_back == 0
        tile = nw.null_tile(X, res, v, 0)
        if nw.expected_route(d, 0, "bed_dev") == "expanded":
            assert tm.genes_hard_call == 0
            want, afs, _ = _host_rows(engine, raws)
            for a, b in zip(got, want):
                _same(a, b)
            with pytest.raises(rvtests_amd.RvtError):
                engine.debug_suffstat_bed_dev(addr[2], raws[2].shape[1])
        else:
            assert tm.genes_hard_call == len(genes)
            for (raw, G, af), a_dev in zip(genes, addr):
                tag = "resident N=%d d=%d M=%d" % (N, d, G.shape[1])
                S, T, u, cs, used = engine.debug_suffstat_bed_dev(a_dev, G.shape[1])
                assert used == 1, tag
                assert np.max(np.abs(cs - G.sum(0))) <= 1e-12 * N, tag
                _check_entries(tag, S, T, u, G, np.ones(N), tile, d, "gene_tnull_hcp", 0, bool((raw < 0).any()))
        for (raw, G, af), a in zip(genes, got):
            _check_records("resident N=%d d=%d M=%d" % (N, d, G.shape[1]), a, G, af, X, y, res, v, 0)
    finally:
        engine.bed_free(d_bed)


@pytest.mark.parametrize("d", [1, 6, 13, 14])
def test_score_of_resident_rows_by_width(engine, d):
    """rvt_score_bed_dev under a quantitative trait, V = 70 (two slices of 32 and one of 6): the planes up to d = 13 — against the
    oracle's MetaScore and against rvt_score_block on the same matrix as doubles; d = 14 is refused, and the next call, under
    a model of d = 2, works."""
    import rvtests_amd
    N, V = N0, 70
    raw = np.asfortranarray(np.column_stack([nw.gene(N, 33)[0], nw.gene(N, 17, missing=False)[0], nw.gene(N, 33)[0][:, :20]]))
    G = orc.impute_mean(raw)
    want_cnt = np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1)

    def score(dd):
        X, y, res, v, s2 = _install(engine, N, dd, 0)
        d_bed, addr = _resident(engine, [raw], N)
        try:
            ok, U, Vs, eff, se, p, cnt = engine.score_bed_dev(addr[0], V)
        finally:
            engine.bed_free(d_bed)
        rc, o = orc.metascore(G, X, y, 0)
        assert rc == 0 and np.array_equal(ok, o["ok"]) and np.array_equal(cnt, want_cnt)
        k = ok.astype(bool)
        assert k.sum() > V // 2
        ptr = engine.upload_block(G)
        r = engine.score_block(ptr, V)
        engine.free_block(ptr)
        assert np.array_equal(r["ok"], ok)
        for f, a in (("U", U), ("V", Vs), ("effect", eff), ("se", se), ("p", p)):
            assert np.allclose(a[k], o[f][k], rtol=1e-6, atol=1e-9 * np.abs(o[f][k]).max()), (dd, f)
            assert np.allclose(a[k], r[f][k], rtol=1e-9, atol=1e-12 * np.abs(r[f][k]).max()), (dd, f)

    if nw.expected_route(d, 0, "score_bed_dev") == "refused":
        _install(engine, N, d, 0)
        d_bed, addr = _resident(engine, [raw], N)
        try:
            with pytest.raises(rvtests_amd.RvtError, match="13 covariates"):
                engine.score_bed_dev(addr[0], V)
        finally:
            engine.bed_free(d_bed)
        score(2)
    else:
        score(d)


# ---- dosages ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(N0, 13), (N0, 14), (61, 7)])
def test_lattice_dosages_by_width(engine, N, d):
    """decimal dosages (den = 1000): gene_suffstat_lat up to d = 13 — its G'G is the exact integer K'K divided once —, the fp64
    kernel at d = 14; read as test_gpu_lattice.py reads the path (content hint 0, the counters)."""
    den, M = 1000, 33
    route = nw.expected_route(d, 0, "lattice")
    X, y, res, v, s2 = _install(engine, N, d, 0)
    K, G, af = nw.lattice_gene(N, M, den)
    engine.set_content_hint(0)
    engine.set_dosage_lattice(den)
    try:
        (a,), tm = _run_blocks(engine, [(G, af)], True)
        S, T, u, tmd = _debug_block(engine, G)
    finally:
        engine.set_dosage_lattice(0)
        engine.set_content_hint(-1)
    lat = route == "gene_suffstat_lat"
    assert tm.genes == 1 and tm.genes_hard_call == (1 if lat else 0) and tm.genes_handed_back == 0
    assert tmd.genes_hard_call == (1 if lat else 0) and tmd.genes_handed_back == 0
    tag = "lattice N=%d d=%d" % (N, d)
    _check_records(tag, a, G, af, X, y, res, v, 0)
    if lat:
        assert np.array_equal(np.triu(S), np.triu((K.T @ K).astype(np.float64) / float(den * den)))
    _check_entries(tag, S, T, u, G, np.ones(N), nw.null_tile(X, res, v, 0), d, route, 0, True)


@pytest.mark.parametrize("N,d", [(N0, 6), (N0, 7), (61, 4)])
def test_float_dosages_by_width(engine, N, d):
    """float-precision dosages after rvt_set_dosage_float: gene_suffstat_fdx while 2 d + 3 <= 16 stage columns, the fp64 kernel
    from d = 7; the records against the oracle either way."""
    M = 33
    route = nw.expected_route(d, 0, "float")
    X, y, res, v, s2 = _install(engine, N, d, 0)
    G, af = nw.float_gene(N, M)
    engine.set_content_hint(0)
    engine.set_dosage_float(True)
    try:
        (a,), tm = _run_blocks(engine, [(G, af)], True)
    finally:
        engine.set_dosage_float(False)
        engine.set_content_hint(-1)
    assert tm.genes == 1 and tm.genes_handed_back == 0
    assert tm.genes_hard_call == (1 if route == "gene_suffstat_fdx" else 0)
    _check_records("float N=%d d=%d" % (N, d), a, G, af, X, y, res, v, 0)


# ---- one context, widths going down and up ------------------------------------------------------------------------------------------
# d = 13, 2, 14, 6, 13 with the traits in turn, either trait first: (model, installed by rvt_fit_null) per step
WALKS = {
    "quantitative_first": (((N0, 13, 0), False), ((61, 2, 1), True), ((N0, 14, 0), False), ((N0, 6, 1), False), ((N0, 13, 0), False)),
    "binary_first": (((N0, 13, 1), True), ((61, 2, 0), False), ((N0, 14, 1), False), ((N0, 6, 0), False), ((N0, 13, 1), True)),
}


def _bits(rec):
    return tuple(np.float64(getattr(rec, f)).tobytes() for f in FIELDS)


def _walk_step(e, key, fitted):
    """Everything one model is asked for, as bytes: resident genes, their T (the planes' or the expanded block's), a block on
    the model's integer kernel, float dosages, rvt_score_bed_dev, the Wald fit that needs y on the device."""
    import rvtests_amd
    N, d, binary = key
    X, y, res, v, s2 = nw.case_model(N, d, binary)
    if fitted:
        e.fit_null(binary, X, y)
    else:
        e.set_null(binary, X, res, v, s2)
    out = {"kernel": e.hardcall_kernel()}
    genes = [nw.gene(N, M) for M in (17, 33)]
    raws = [raw for raw, G, af in genes]
    d_bed, addr = _resident(e, raws, N)
    try:
        e.submit_genes_bed_dev([0, 1], addr, [17, 33])
        out["resident"] = [_bits(r) for r in e.collect()]
        if nw.expected_route(d, binary, "bed_dev") == "gene_tnull_hcp":
            S, T, u, cs, used = e.debug_suffstat_bed_dev(addr[1], 33)
            assert used == 1
        else:
            ptr = e.upload_block(genes[1][1])
            S, T, u = e.debug_suffstat(ptr, 33)[:3]
            e.free_block(ptr)
        out["S"], out["T"], out["u"] = S.tobytes(), T.tobytes(), u.tobytes()
        try:
            out["score"] = [np.asarray(a).tobytes() for a in e.score_bed_dev(addr[1], 33)]
        except rvtests_amd.RvtError:
            out["score"] = "refused"
    finally:
        e.bed_free(d_bed)
    assert (out["score"] == "refused") == (d > nw.HC_MAX_D)
    ptrs = [e.upload_block(G) for raw, G, af in genes]
    out["blocks"] = [_bits(r) for r in e.run_blocks(ptrs, [17, 33], [af for raw, G, af in genes])]
    if binary:
        try:
            w = e.wald_block(ptrs[0], 17)
            out["wald"] = [w[f].tobytes() for f in ("ok", "beta", "se", "p")]
        except rvtests_amd.RvtError:
            out["wald"] = "refused"
        assert (out["wald"] == "refused") == (not fitted)      # (y reaches the device with rvt_fit_null only)
    else:
        Gf, aff = nw.float_gene(N, 33)
        pf = e.upload_block(Gf)
        e.set_content_hint(0)
        e.set_dosage_float(True)
        try:
            out["float"] = [_bits(r) for r in e.run_blocks([pf], [33], [aff])]
        finally:
            e.set_dosage_float(False)
            e.set_content_hint(-1)
            e.free_block(pf)
    for p in ptrs:
        e.free_block(p)
    return out


@pytest.mark.parametrize("poison", [None, "255"])
@pytest.mark.parametrize("walk", sorted(WALKS))
def test_one_context_through_widths_going_down_and_up(monkeypatch, walk, poison):
    """d = 13, 2, 14, 6, 13 on ONE context, quantitative and binary in turn (either first), N = 2003, 61, 2003: every record,
    every T and every score statistic equals, bit for bit, what a fresh context gives under that model alone — the digit planes
    (quantitative first: 14 columns, 4 of a weighted tile, none, 8 of a weighted tile, 14 again), the cooperative kernel's
    tile (binary, d <= 6), the float-digit tile (quantitative, d <= 6: the wider model after it must not find it) and the y of
    the fitted binary model (dropped by the next rvt_set_null: the Wald fit is refused under the next binary model, installed
    without y) do not survive their model.  Once more with RVT_POISON=255: fresh work spaces hold 0xff bytes, nothing may be
    read unwritten."""
    import rvtests_amd
    if poison:
        monkeypatch.setenv("RVT_POISON", poison)
    steps = WALKS[walk]
    walked = rvtests_amd.Engine(0)
    try:
        got = [_walk_step(walked, key, f) for key, f in steps]
    finally:
        walked.close()
    for (key, f), g in zip(steps, got):
        if key[2]:
            assert g["kernel"] == (None if key[1] > nw.HC_MAX_D else nw.expected_route(key[1], 1, "block")), key
    assert steps[0] == steps[4] and got[0] == got[4]
    for (key, f), g in zip(steps[:4], got):
        fresh = rvtests_amd.Engine(0)
        try:
            want = _walk_step(fresh, key, f)
        finally:
            fresh.close()
        assert sorted(want) == sorted(g)
        for name in want:
            assert want[name] == g[name], (key, name)
