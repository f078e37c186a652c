"""GPU: rvt_burden_blocks (--burden cmcWald, zegginiWald, fp, exactCMC) against the numpy statements of
tests/test_burden_wald_cpu.py: the collapsed columns and counts of burden_columns_kernel, the Wald / score fits on them, Fisher's
exact test of fisher_2x2_kernel, the state rules, and the host driver's rows."""
import functools
import math

import numpy as np
import pytest

import orc
import synth
import rvtests_amd
from rvtests_amd import engine as E
from test_gpu_metacov import engine_factory  # noqa: F401  (fixture)
from test_burden_wald_cpu import (burden_statement, fisher_2x2, fisher_near_tie, fp_collapse, table_2x2, wald_rows, fp_row,
                                  exact_row, SITE_HEADER, WALD_HEADER, FP_HEADER, EXACT_HEADER)

pytestmark = pytest.mark.gpu

REL = 1e-6        # BASELINE.json north_star tolerance (tests/test_gpu_single.py)
REL_SCORE = 1e-9  # score statistics (tests/test_gpu_parity.py)
MS = (1, 3, 33, 70)


def make_genes(N, y, seed, n=44):
    """n genes of M in {1, 3, 33, 70}: hard calls with mean-imputed entries (fractions below 1), a flipped column (af > 0.5),
    entries that are >= 1 after the flip without being hard calls, an all-zero gene between two good ones, a gene whose kept
    columns hold imputed fractions only, and a planted causal gene."""
    rng = np.random.default_rng(seed)
    genes = []
    for g in range(n):
        M = MS[g % 4]
        Graw, G, af = synth.make_gene(N, M, seed=seed * 1000 + g, missing=0.02, common=True, mono=True, maf_lo=-2.3, maf_hi=-1.0)
        G = np.asfortranarray(G)
        if g == 2:        # M = 33: column 2 is flipped (make_gene, common); 0.6 there is 1.4 after the flip; 1.4 in column 0 as stored
            G[rng.choice(N, 7, replace=False), 2] = 0.6
            G[rng.choice(N, 7, replace=False), 0] = 1.4
        if g == 5:        # all zero, between two good genes
            G[:] = 0.0
        if g == 6:        # every kept column: 0 and an imputed fraction — CMC and Zeggini are constant, Fp is not
            G[:] = 0.0
            for j in range(M):
                G[rng.choice(N, 9, replace=False), j] = 0.37
        if g == 9 and y is not None:    # carriers among the cases
            cases = np.flatnonzero(y == 1)
            G[cases[: max(8, len(cases) // 6)], 0] = 1.0
        genes.append((G, af))
    return genes


@functools.lru_cache(maxsize=None)
def case(N, binary, d, seed):
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=seed)
    genes = make_genes(N, y if binary else None, seed)
    st = [burden_statement(G, af, X, y, binary) for G, af in genes]
    return X, y, genes, st


def run(eng, X, y, genes, binary, which=E.BURDEN_ALL, fit=True):
    if fit:
        eng.fit_null(binary, X, y)
    ptrs = [eng.upload_block(G) for G, af in genes]
    out = eng.burden_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes], y, which)
    return ptrs, out


def record_tuple(r, d):
    w = []
    for f in (r.cmc_wald, r.zeggini_wald):
        w += [f.ok, f.rounds] + list(f.beta[:d]) + list(f.se[:d]) + list(f.pvalue[:d])
    return tuple([r.n_poly, r.nonref_site] + w + [r.fp_ok, r.exact_ok, r.fp_u, r.fp_v, r.fp_pvalue, r.n00, r.n01, r.n10, r.n11,
                                                  r.exact_p_two, r.exact_p_less, r.exact_p_greater])


def check_records(out, st, d, binary, y):
    for g, (r, s) in enumerate(zip(out, st)):
        assert r.n_poly == s["n_poly"], g
        assert r.nonref_site == s["nonref"], g
        for f, (ok, rounds, beta, se, p) in zip((r.cmc_wald, r.zeggini_wald), s["wald"]):
            assert f.ok == ok, g
            if s["n_poly"]:
                assert f.rounds == rounds, g
            if not ok:
                continue
            got_b, got_s, got_p = (np.array(a[:d]) for a in (f.beta, f.se, f.pvalue))
            assert np.allclose(got_b, beta, rtol=REL, atol=1e-9 * np.abs(beta).max()), (g, got_b, beta)
            for got, want in ((got_s, se), (got_p, p)):
                assert (np.abs(got - want) <= REL * np.abs(want)).all(), (g, got, want)
        assert r.fp_ok == s["fp_ok"], g
        if s["fp_ok"]:
            for got, want in ((r.fp_u, s["fp_u"]), (r.fp_v, s["fp_v"]), (r.fp_pvalue, s["fp_p"])):
                assert abs(got - want) <= REL_SCORE * abs(want), (g, got, want)
        assert r.exact_ok == s["exact_ok"], g
        if s["exact_ok"]:
            assert [r.n00, r.n01, r.n10, r.n11] == s["table"], g
            assert not fisher_near_tie(*s["table"]), "near-tie: choose another seed"
            for got, want in zip((r.exact_p_two, r.exact_p_less, r.exact_p_greater), s["exact_p"]):
                assert abs(got - want) <= REL * abs(want), (g, s["table"], got, want)


CASES = [(700, 1, 1, 11), (1500, 0, 3, 12), (9001, 1, 3, 13), (1500, 0, 1, 14)]


@pytest.mark.parametrize("N,binary,d,seed", CASES)
def test_collapsed_columns_and_counts(engine_factory, N, binary, d, seed):
    X, y, genes, st = case(N, binary, d, seed)
    eng = engine_factory()
    ptrs, out = run(eng, X, y, genes, binary)
    n = len(genes)
    cmc, zeg, fp = (eng.burden_last_columns(t, n) for t in (E.BURDEN_CMCWALD, E.BURDEN_ZEGGINIWALD, E.BURDEN_FP))
    for g, ((G, af), s) in enumerate(zip(genes, st)):
        assert np.array_equal(cmc[:, g], s["cmc"]), g
        assert np.array_equal(zeg[:, g], s["zeg"]), g
        bound = 2.1 * (G.shape[1] + 1) * 2.0 ** -53       # non-negative terms: any summation order, with or without fma
        assert (np.abs(fp[:, g] - s["fp"]) <= bound * np.abs(s["fp"])).all(), g
        assert out[g].nonref_site == s["nonref"], g
        if s["exact_ok"]:
            assert [out[g].n00, out[g].n01, out[g].n10, out[g].n11] == s["table"], g
    assert st[5]["n_poly"] == 0 and st[4]["n_poly"] > 0 and st[6]["n_poly"] > 0
    assert st[6]["nonref"] == 0 and st[6]["fp"].max() > 0 and st[6]["wald"][0][0] == 0 and st[6]["fp_ok"] == 1
    assert st[2]["zeg"].max() >= 1 and orc.flip_poly(genes[2][0])[1].any()          # a flipped column is present


@pytest.mark.parametrize("N,binary,d,seed", CASES)
def test_records_match_the_statements(engine_factory, N, binary, d, seed):
    X, y, genes, st = case(N, binary, d, seed)
    eng = engine_factory()
    ptrs, out = run(eng, X, y, genes, binary)
    check_records(out, st, d, binary, y)
    if binary and d == 1:
        assert y.sum() != len(y) - y.sum()                                          # cases != controls
        assert out[9].exact_p_two < 1e-4                                            # the planted gene
    out2 = eng.burden_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes], y)
    assert [record_tuple(r, d) for r in out] == [record_tuple(r, d) for r in out2]  # the same bits again


def test_only_the_tests_asked_for(engine_factory):
    N, binary, d, seed = CASES[0]
    X, y, genes, st = case(N, binary, d, seed)
    eng = engine_factory()
    ptrs, full = run(eng, X, y, genes[:8], binary)
    for which in (E.BURDEN_CMCWALD, E.BURDEN_ZEGGINIWALD, E.BURDEN_FP, E.BURDEN_EXACTCMC, E.BURDEN_FP | E.BURDEN_CMCWALD):
        out = eng.burden_blocks(ptrs, [G.shape[1] for G, af in genes[:8]], [af for G, af in genes[:8]], y, which)
        for a, b in zip(out, full):
            assert a.n_poly == b.n_poly and a.nonref_site == b.nonref_site
            assert a.cmc_wald.ok == (b.cmc_wald.ok if which & E.BURDEN_CMCWALD else 0)
            assert a.zeggini_wald.ok == (b.zeggini_wald.ok if which & E.BURDEN_ZEGGINIWALD else 0)
            assert a.fp_ok == (b.fp_ok if which & E.BURDEN_FP else 0) and a.exact_ok == (b.exact_ok if which & E.BURDEN_EXACTCMC else 0)
            if which & E.BURDEN_FP:
                assert a.fp_pvalue == b.fp_pvalue
            if which & E.BURDEN_EXACTCMC:
                assert (a.exact_p_two, a.n11) == (b.exact_p_two, b.n11)
            if which & E.BURDEN_CMCWALD:
                assert list(a.cmc_wald.pvalue[:d]) == list(b.cmc_wald.pvalue[:d])
        if not which & E.BURDEN_ZEGGINIWALD:
            with pytest.raises(rvtests_amd.RvtError):
                eng.burden_last_columns(E.BURDEN_ZEGGINIWALD, 8)


def test_a_batch_cut_into_several_chunks(monkeypatch, engine_factory):
    """RVT_BURDEN_CHUNK = 7: the 44 genes run as six chunks of 7 and one of 2 — counters, records and kept-column lists are indexed
    by the gene of the batch, the collapsed blocks by the gene of the chunk"""
    N, binary, d, seed = CASES[0]
    X, y, genes, st = case(N, binary, d, seed)
    n = len(genes)
    assert n % 7 == 2
    monkeypatch.setenv("RVT_BURDEN_CHUNK", "7")
    eng = engine_factory()
    ptrs, out = run(eng, X, y, genes, binary)
    check_records(out, st, d, binary, y)
    cmc, zeg, fp = (eng.burden_last_columns(t, 2) for t in (E.BURDEN_CMCWALD, E.BURDEN_ZEGGINIWALD, E.BURDEN_FP))   # the last chunk
    for k, g in enumerate((n - 2, n - 1)):
        assert np.array_equal(cmc[:, k], st[g]["cmc"]) and np.array_equal(zeg[:, k], st[g]["zeg"]), g
        assert (np.abs(fp[:, k] - st[g]["fp"]) <= 2.1 * (genes[g][0].shape[1] + 1) * 2.0 ** -53 * np.abs(st[g]["fp"])).all(), g
    with pytest.raises(rvtests_amd.RvtError):
        eng.burden_last_columns(E.BURDEN_CMCWALD, n)                    # the blocks hold one chunk, not the batch
    monkeypatch.delenv("RVT_BURDEN_CHUNK")
    out1 = eng.burden_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes], y)
    ints = lambda r: (r.n_poly, r.nonref_site, r.n00, r.n01, r.n10, r.n11, r.cmc_wald.ok, r.zeggini_wald.ok, r.fp_ok, r.exact_ok,
                      r.exact_p_two, r.exact_p_less, r.exact_p_greater)      # what no fit's slice width touches: the same bits
    assert [ints(r) for r in out] == [ints(r) for r in out1]


def test_fisher_table_at_half_a_million_samples(engine_factory):
    N, M = 500000, 20
    rng = np.random.default_rng(5)
    y = (rng.random(N) < 0.3).astype(np.float64)
    maf = 10 ** rng.uniform(-3.3, -2.3, M)
    G = np.asfortranarray(rng.binomial(2, maf, size=(N, M)).astype(np.float64))
    G[:, 0] += (y == 1) * (rng.random(N) < 0.002)
    af = G.sum(0) / (2.0 * N)
    Gf, fl, kp = orc.flip_poly(G)
    tab = table_2x2(orc.collapse(Gf, 0), y)
    want = fisher_2x2(*tab)
    assert not fisher_near_tie(*tab), "near-tie: choose another seed"
    eng = engine_factory()
    eng.fit_null(1, np.ones((N, 1)), y)
    ptr = eng.upload_block(G)
    r = eng.burden_blocks([ptr], [M], [af], y, E.BURDEN_EXACTCMC)[0]
    assert r.exact_ok == 1 and [r.n00, r.n01, r.n10, r.n11] == tab and sum(tab) == N
    print("table", tab, "got", r.exact_p_two, r.exact_p_less, r.exact_p_greater, "want", want)
    for got, w in zip((r.exact_p_two, r.exact_p_less, r.exact_p_greater), want):
        assert abs(got - w) <= REL * abs(w), (tab, got, w)


def test_poisoned_work_spaces_give_the_same_records(monkeypatch, engine_factory):
    N, binary, d, seed = CASES[0]
    X, y, genes, st = case(N, binary, d, seed)
    outs = []
    for poison in ("255", None):
        if poison:
            monkeypatch.setenv("RVT_POISON", poison)
        else:
            monkeypatch.delenv("RVT_POISON", raising=False)
        eng = engine_factory()
        ptrs, out = run(eng, X, y, genes, binary)
        outs.append([record_tuple(r, d) for r in out])
    assert outs[0] == outs[1]
    check_records(out, st, d, binary, y)


def test_two_analyses_of_different_n_on_one_context(engine_factory):
    eng = engine_factory()
    for N, binary, d, seed in (CASES[1], CASES[0], CASES[1]):
        X, y, genes, st = case(N, binary, d, seed)
        ptrs, out = run(eng, X, y, genes, binary)
        check_records(out, st, d, binary, y)
        for p in ptrs:
            eng.free_block(p)


def test_state_rules(engine_factory):
    N, binary, d, seed = CASES[0]
    X, y, genes, st = case(N, binary, d, seed)
    eng = engine_factory()
    with pytest.raises(rvtests_amd.RvtError, match="no null model"):
        eng.burden_blocks([1], [4], [np.full(4, 0.1)], y)
    rc, beta, p, v = orc.fit_logistic(X, y)
    eng.set_null(1, X, y - p, v)                            # a caller's null model: no estimates, no y
    ptrs = [eng.upload_block(G) for G, af in genes[:3]]
    Ms, afs = [G.shape[1] for G, af in genes[:3]], [af for G, af in genes[:3]]
    for which in (E.BURDEN_CMCWALD, E.BURDEN_ZEGGINIWALD, E.BURDEN_ALL):
        with pytest.raises(rvtests_amd.RvtError, match="rvt_fit_null"):
            eng.burden_blocks(ptrs, Ms, afs, y, which)
    out = eng.burden_blocks(ptrs, Ms, afs, y, E.BURDEN_FP | E.BURDEN_EXACTCMC)   # any installed null model will do
    for r, s in zip(out, st):
        assert r.fp_ok == s["fp_ok"] and abs(r.fp_pvalue - s["fp_p"]) <= REL_SCORE * s["fp_p"]
        assert r.exact_ok == 1 and [r.n00, r.n01, r.n10, r.n11] == s["table"]
    with pytest.raises(rvtests_amd.RvtError):
        eng.burden_blocks(ptrs, Ms, afs, None, E.BURDEN_EXACTCMC)                 # exactCMC needs y
    with pytest.raises(rvtests_amd.RvtError):
        eng.burden_blocks(ptrs, Ms, afs, y, 16)
    # exactCMC: a quantitative null model, or covariates -> ok = 0, the other tests unaffected
    for N2, b2, d2, seed2 in (CASES[3], CASES[2]):
        X2, y2, genes2, st2 = case(N2, b2, d2, seed2)
        eng2 = engine_factory()
        eng2.fit_null(b2, X2, y2)
        ptrs2, out2 = run(eng2, X2, y2 if b2 else (y2 > np.median(y2)).astype(float), genes2[:3], b2, fit=False)
        assert all(r.exact_ok == 0 and r.exact_p_two == 1.0 and r.n00 == 0 for r in out2)
        assert [r.fp_ok for r in out2] == [s["fp_ok"] for s in st2[:3]]
    # a phenotype that is not 0 / 1
    y3 = y.copy()
    y3[0] = 2.0
    assert all(r.exact_ok == 0 for r in eng.burden_blocks(ptrs, Ms, afs, y3, E.BURDEN_EXACTCMC))


# ---- the host driver's rows --------------------------------------------------------------------------------------------------------
def _same_row(got, want):
    """site columns, integers and NA are the statement's text; a number printed with six digits may differ from the statement's in
    its last digit (the engine's value is within REL of the statement's): 2e-6 relative, as tests/test_gpu_single.py"""
    g, w = got.split("\t"), want.split("\t")
    assert len(g) == len(w), (got, want)
    for a, b in zip(g, w):
        if a == b:
            continue
        assert "NA" not in (a, b) and abs(float(a) - float(b)) <= 2e-6 * abs(float(b)), (got, want)


def driver_statement_rows(genes, X, y, binary):
    """{output name: rows} as the four classes print them, gene after gene"""
    d = X.shape[1]
    rows = {"CMCWald": [], "ZegginiWald": [], "Fp": [], "CMCFisherExact": []}
    prev_cols = 0
    for g, G in enumerate(genes):
        af = G.sum(0) / (2.0 * len(y))
        s = burden_statement(G, af, X, y, binary)
        site = "gene%d\t%d\t%d\t\t" % (g, len(y), G.shape[1])
        for k, name in enumerate(("CMCWald", "ZegginiWald")):
            rows[name] += wald_rows(site, name, s["wald"][k] if s["n_poly"] else None, s["nonref"], d, prev_cols)
        if s["n_poly"]:
            prev_cols = d + 1
        rows["Fp"].append(fp_row(site, s["fp_ok"], s.get("fp_p")))
        rows["CMCFisherExact"].append(exact_row(site, s["exact_ok"], s.get("table"), s.get("exact_p")))
    return rows


def _driver_case(tmp_path, binary, d, zero_first, spec="cmcwald,zegginiwald,fp,exactcmc"):
    import test_vtprice_cpu as vt
    from test_burdenperm_cpu import write_input, run_burden_driver, split_outputs
    vt._ensure_driver()
    N = 700
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=60 + binary + d)
    pool = [G for G, af in make_genes(N, y if binary else None, 77, n=10)]
    good1, good2, zero, frac = pool[1], pool[2], pool[5], pool[6]
    genes = [zero, good1, good2, zero, frac] if zero_first else [good1, zero, good2, frac]
    path = str(tmp_path / "in.bin")
    write_input(path, y, binary, genes, cov=X[:, 1:] if d > 1 else None)
    rc, out, err = run_burden_driver(path, spec)
    assert rc == 0, err
    f = split_outputs(out)
    want = driver_statement_rows(genes, X, y, binary)
    headers = dict(WALD_HEADER, Fp=FP_HEADER, CMCFisherExact=EXACT_HEADER)
    for name, rows in want.items():
        got = f["out.%s.assoc" % name]
        assert got[0] == SITE_HEADER + headers[name], name
        assert len(got) - 1 == len(rows), (name, got, rows)
        for a, b in zip(got[1:], rows):
            _same_row(a, b)
    return f, want, err


@pytest.mark.parametrize("binary,d,zero_first", [(1, 1, True), (1, 3, False), (0, 2, True), (0, 1, False)])
def test_driver_rows_equal_the_statements(tmp_path, binary, d, zero_first):
    f, want, err = _driver_case(tmp_path, binary, d, zero_first)
    assert len(want["CMCWald"]) == 4 * d       # the zero gene FIRST prints nothing, AFTER a good gene d NA rows; every other gene d rows
    if zero_first:
        assert not any(r.startswith("gene0\t") for r in want["CMCWald"])                          # ... first: none
    if binary and d > 1:
        assert all(r.endswith("NA\tNA\tNA\tNA\tNA\tNA\tNA") for r in want["CMCFisherExact"])
        assert "does not support covariates" in err
    if not binary:
        assert "does not support continuous outcomes" in err


@pytest.mark.parametrize("window", ["1", "2"])
def test_driver_rows_do_not_depend_on_the_batch_window(tmp_path, monkeypatch, window):
    """the adapters defer their genes: the default window takes the five genes in one rvt_burden_blocks call; a window of two cuts
    them into three calls (the Wald tests' NA rows follow the previous gene's X across a call's end), a window of one runs gene by
    gene; CMC beside them goes through the gene tests' own queue"""
    monkeypatch.setenv("RVT_ADAPTER_BATCH", window)
    f, want, err = _driver_case(tmp_path, 1, 1, True, spec="cmc,cmcwald,zegginiwald,fp,exactcmc")
    assert len(f["out.CMC.assoc"]) == 1 + 5
