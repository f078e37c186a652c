"""RareCover and Madsen-Browning (--burden rarecover[...],mb[...]) through the C ABI and the host driver, against the numpy
statements of tests/test_burdenperm_cpu.py.  Exact mode: the reference's own shuffles, so the counters are the statement's gene
after gene; counter mode: other shuffles, the same estimator, independent of gene order and context."""
import numpy as np
import pytest

import orc
import test_burdenperm_cpu as bp
import test_vtprice_cpu as vt

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


def _null(e, y, X=None):
    """the logistic null model: it defines N, and Madsen-Browning's observed statistic is its score test"""
    N = len(y)
    if X is None:
        X = np.ones((N, 1))
    e.fit_null(1, np.asfortranarray(X), np.asarray(y, dtype=np.float64).copy())


def _run(e, which, genes, y, nperm, alpha):
    ptrs = [e.upload_block(G) for G in genes]
    fn = e.rarecover_blocks if which == "rc" else e.mb_blocks
    out = fn(ptrs, [G.shape[1] for G in genes], y, nperm, alpha)
    for p in ptrs:
        e.free_block(p)
    return out


def _rc_tuple(r):
    return (r.fit_ok, r.n_poly, r.n_carrier, r.n_selected, r.stat, r.num_perm, r.actual_perm, r.num_greater, r.num_equal, r.perm_pvalue)


def _mb_tuple(r):
    return (r.fit_ok, r.n_poly, r.n_entries, r.stat, r.num_perm, r.actual_perm, r.num_greater, r.num_equal, r.perm_pvalue)


def _pheno(rng, N, G=None, effect=0.0, base=-0.6):
    eta = base + (effect * (G > 0).sum(1) if G is not None else 0.0)
    return (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)


# ---- RareCover ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [700, 1500, 9001])
def test_rarecover_exact_mode_equals_the_statement_gene_after_gene(eng, N):
    rng = np.random.default_rng(40 + N)
    nperm, alpha = 200, 0.05
    genes = [bp.gene(rng, N, 12, ties=True), bp.gene(rng, N, 9, lo=-1.6, hi=-1.2, flip=True, imputed=True), np.zeros((N, 3)),
             bp.gene(rng, N, 30, ties=True)]
    y = _pheno(rng, N, genes[1], effect=1.2)                      # gene 1 is causal: it uses all nPerm
    _null(eng, y)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    out = _run(eng, "rc", genes, y, nperm, alpha)
    probe = _run(eng, "rc", genes[:1], y, 40, 0.4)                # its counts depend on where the stream stands now
    orc.rand_seed(1)
    for k, (r, G) in enumerate(zip(list(out) + list(probe), genes + genes[:1])):
        s = bp.rarecover_statement(G, y, *((nperm, alpha) if k < len(genes) else (40, 0.4)))
        print("N", N, "gene", k, _rc_tuple(r), s.get("stat"), s.get("selected"))
        if not s["fit_ok"]:
            assert (r.fit_ok, r.n_poly, r.actual_perm, r.perm_pvalue, r.stat) == (0, 0, 0, 1.0, -1.0)
            continue
        assert (r.fit_ok, r.n_poly, r.n_carrier, r.n_selected) == (1, s["n_poly"], s["n_carrier"], s["n_selected"])
        assert r.stat == s["stat"]                                # bit for bit
        assert (r.actual_perm, r.num_greater, r.num_equal, r.perm_pvalue) == (s["actual"], s["num_x"], s["num_eq"], s["pvalue"]), k
    assert out[1].actual_perm == nperm and out[1].num_greater == 0
    assert any(r.actual_perm < nperm for r in out if r.fit_ok)


def test_rarecover_phenotype_that_is_not_0_1_fails_and_draws_nothing(eng):
    N = 700
    rng = np.random.default_rng(3)
    G = bp.gene(rng, N, 8)
    y = _pheno(rng, N)
    _null(eng, y)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    bad = _run(eng, "rc", [G], rng.normal(size=N), 50, 0.4)[0]
    bad2 = _run(eng, "mb", [G], np.ones(N), 50, 0.4)[0]
    assert (bad.fit_ok, bad.actual_perm, bad.perm_pvalue) == (0, 0, 1.0) and (bad2.fit_ok, bad2.actual_perm) == (0, 0)
    r = _run(eng, "rc", [G], y, 50, 0.4)[0]
    orc.rand_seed(1)
    s = bp.rarecover_statement(G, y, 50, 0.4)
    assert (r.actual_perm, r.num_greater, r.num_equal) == (s["actual"], s["num_x"], s["num_eq"])


# ---- Madsen-Browning ------------------------------------------------------------------------------------------------------------
def _k_quantisation(Gf):
    """relative error of a Gram entry that the integer-plane product adds for a column with non-integer values: every entry is
    rounded to a multiple of 2^-(39 - ilogb(max)) = 2^-38 for a column maximum in [2, 4), so a product of two entries is off by at
    most (2 d / g_min + (d / g_min)^2) of itself, d = 2^-39, g_min the smallest non-zero entry; 0 for hard calls (one exact plane)"""
    if (Gf == np.round(Gf)).all():
        return 0.0
    d = 2.0 ** -39
    gmin = float(Gf[Gf > 0].min())
    return 2 * d / gmin + (d / gmin) ** 2


@pytest.mark.parametrize("N,ncov", [(700, 0), (1500, 2)])
def test_madsen_browning_exact_mode_counters_equal_the_statement_s(eng, N, ncov):
    rng = np.random.default_rng(140 + N)
    nperm, alpha = 150, 0.1
    genes = [bp.gene(rng, N, 12), bp.gene(rng, N, 9, lo=-1.6, hi=-1.2, flip=True, imputed=True), np.zeros((N, 3)), bp.gene(rng, N, 30)]
    X = np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(ncov)])
    eta = -0.5 + (0.4 * X[:, 1] if ncov else 0.0) + 0.9 * (genes[1] > 0).sum(1)
    y = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    _null(eng, y, X)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    out = _run(eng, "mb", genes, y, nperm, alpha)
    orc.rand_seed(1)
    for k, (r, G) in enumerate(zip(out, genes)):
        Gf = orc.flip_poly(G)[0]
        if Gf.shape[1] == 0:
            assert (r.fit_ok, r.n_poly, r.actual_perm, r.perm_pvalue) == (0, 0, 0, 1.0)
            continue
        obs = bp.mb_observed(Gf, X, y)
        print("N", N, "gene", k, _mb_tuple(r), "statement", obs)
        # 1e-9 relative: the tolerance of the score statistics after the device IRLS (tests/test_gpu_parity.py, _check_gene:
        # close(stat, b.stat, 1e-9, ...))
        assert r.fit_ok == 1 and r.n_poly == Gf.shape[1] and r.n_entries == np.count_nonzero(Gf)
        assert abs(r.stat - obs) <= 1e-9 * obs
        s = bp.mb_statement(G, X, y, nperm, alpha, obs=r.stat, keep=True)
        # the device's permuted statistic is the Gram form in another summation order (+ the quantised Gram entries of an imputed
        # column): within mb_bound + stat x the quantisation of the statement's.  No shuffle of the statement lies that close to
        # the observed value, so the counters are comparable.
        eq = _k_quantisation(Gf)
        margin = [b + p * eq for p, b in zip(s["perms"], s["bounds"])]
        assert all(abs(p - r.stat) > mg for p, mg in zip(s["perms"], margin)), "near-tie: choose another seed"
        assert (r.num_perm, r.actual_perm, r.num_greater, r.num_equal) == (nperm, s["actual"], s["num_x"], s["num_eq"]), k
        assert r.perm_pvalue == s["pvalue"]
    assert out[1].actual_perm == nperm and any(r.actual_perm < nperm for r in out if r.fit_ok)


def test_madsen_browning_needs_a_binary_null_model(eng):
    N = 700
    rng = np.random.default_rng(8)
    G = bp.gene(rng, N, 8)
    y = _pheno(rng, N)
    eng.fit_null(0, np.asfortranarray(np.ones((N, 1))), rng.normal(size=N))
    r = _run(eng, "mb", [G], y, 50, 0.4)[0]
    assert (r.fit_ok, r.actual_perm, r.perm_pvalue) == (0, 0, 1.0) and r.n_poly > 0


# ---- counter mode, both tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rc", "mb"])
def test_counter_mode_is_independent_of_gene_order_and_context_and_agrees_with_the_exact_mode(eng, which):
    import rvtests_amd
    N, nperm = 1500, 2000
    rng = np.random.default_rng(99)
    genes = [bp.gene(rng, N, int(rng.integers(3, 30)), lo=-2.3, hi=-0.9) for _ in range(6)]
    y = _pheno(rng, N, genes[2], effect=0.25)
    tup = _rc_tuple if which == "rc" else _mb_tuple
    _null(eng, y)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    exact = _run(eng, which, genes, y, nperm, 1.0)
    eng.set_perm_exact(False)
    eng.rand_seed(1)
    cb = _run(eng, which, genes, y, nperm, 1.0)
    other = rvtests_amd.Engine(0)
    _null(other, y)
    other.set_perm_exact(False)
    other.rand_seed(1)
    cb2 = _run(other, which, genes[::-1], y, nperm, 1.0)[::-1]
    other.close()
    assert [tup(r) for r in cb] == [tup(r) for r in cb2]          # bit-equal
    for a, b in zip(exact, cb):
        assert a.fit_ok and b.fit_ok and a.stat == b.stat and a.actual_perm == b.actual_perm == nperm
        pa, pb = a.perm_pvalue, b.perm_pvalue
        print(which, "exact", pa, "counter", pb, "5 se", 5 * np.sqrt(pa * (1 - pa) / nperm))
        assert abs(pb - pa) <= 5 * np.sqrt(pa * (1 - pa) / nperm)


@pytest.mark.parametrize("which", ["rc", "mb"])
def test_a_causal_gene_reaches_the_floor_in_both_modes(eng, which):
    N, nperm = 3000, 1000
    rng = np.random.default_rng(5)
    G = bp.gene(rng, N, 15, lo=-1.8, hi=-1.2)
    y = _pheno(rng, N, G, effect=1.5, base=-1.0)
    _null(eng, y)
    for exact in (True, False):
        eng.set_perm_exact(exact)
        eng.rand_seed(1)
        r = _run(eng, which, [G], y, nperm, 0.05)[0]
        assert (r.fit_ok, r.actual_perm, r.num_greater) == (1, nperm, 0)


@pytest.mark.parametrize("exact", [True, False])
def test_two_analyses_of_different_n_on_one_context_and_poisoned_work_spaces(eng, exact, monkeypatch):
    """N = 700 with 300 shuffles, then N = 9 001 with 30, on one context = what a fresh context with poisoned allocations gives"""
    import rvtests_amd
    outs = []
    for fresh in (False, True):
        if fresh:
            monkeypatch.setenv("RVT_POISON", "255")
        e = rvtests_amd.Engine(0) if fresh else eng
        for N, nperm in ((700, 300), (9001, 30)) if not fresh else ((9001, 30),):
            rng = np.random.default_rng(N)
            genes = [bp.gene(rng, N, M) for M in (24, 7, 40)]
            y = _pheno(rng, N)
            _null(e, y)
            e.set_perm_exact(exact)
            e.rand_seed(1)
            out = [_rc_tuple(r) for r in _run(e, "rc", genes, y, nperm, 0.4)] + [_mb_tuple(r) for r in _run(e, "mb", genes, y, nperm, 0.4)]
        outs.append(out)
        if fresh:
            e.close()
    assert outs[0] == outs[1] and all(t[0] == 1 for t in outs[0]) and all(t[-4] > 0 for t in outs[0])


def test_rarecover_one_gene_at_half_a_million_samples_in_counter_mode(eng):
    """c and Y of a shuffle are kept in LDS up to 4 096 words each (K <= 262 144 carriers), beyond that in the global work space: one
    gene of each kind"""
    N = 500000
    rng = np.random.default_rng(12)
    words = []
    for lo, hi in ((-3.3, -2.0), (-1.6, -1.3)):
        maf = 10 ** rng.uniform(lo, hi, 50)
        G = np.asfortranarray(rng.binomial(2, maf, size=(N, 50)).astype(np.float64))
        y = _pheno(rng, N)
        _null(eng, y)
        eng.set_perm_exact(False)
        eng.rand_seed(1)
        r = _run(eng, "rc", [G], y, 200, 0.05)[0]
        Gf = orc.flip_poly(G)[0]
        samp, bits = bp.rc_bitsets(Gf)
        stat, selected = bp.rc_stat_bitset(bits, bp.y_bits(samp, y), int(y.sum()), N)
        print("K", len(samp), "words", (len(samp) + 63) // 64, "stat", r.stat, stat, "selected", selected, "perms", r.actual_perm)
        assert (r.fit_ok, r.n_poly, r.n_carrier, r.n_selected) == (1, Gf.shape[1], len(samp), len(selected)) and r.stat == stat
        assert 0 < r.actual_perm <= 200 and 0.0 < r.perm_pvalue <= 1.0
        words.append((len(samp) + 63) // 64)
    assert words[0] <= 4096 < words[1]


# ---- the host driver ----------------------------------------------------------------------------------------------------------------
def test_driver_rows_equal_the_statement_s_text(tmp_path):
    vt._ensure_driver()
    N, nperm, alpha = 900, 120, 0.1
    rng = np.random.default_rng(31)
    genes = [bp.gene(rng, N, 8), np.zeros((N, 2)), bp.gene(rng, N, 20, ties=True), bp.gene(rng, N, 4)]
    y = _pheno(rng, N, genes[2][:, :6], effect=0.8)
    path = str(tmp_path / "in.bin")
    spec = "rarecover[nPerm=%d,alpha=%g],mb[nPerm=%d,alpha=%g]" % (nperm, alpha, nperm, alpha)
    X1 = np.ones((N, 1))

    def site(g):
        return "gene%d\t%d\t%d\t\t" % (g, N, genes[g].shape[1])

    # (a) binary trait, no covariates: RareCover rows, then (a second run: the models of one run share the stream) Madsen-Browning's
    bp.write_input(path, y, 1, genes)
    rc, out, err = bp.run_burden_driver(path, spec.split(",mb")[0], perm_exact=True)
    assert rc == 0, err
    f = bp.split_outputs(out)["out.RareCover.assoc"]
    assert f[0] == bp.SITE_HEADER + "NumIncludeMarker\t" + bp.PERM_HEADER
    orc.rand_seed(1)
    for g, G in enumerate(genes):
        want = site(g) + bp.rarecover_row(nperm, bp.rarecover_statement(G, y, nperm, alpha))
        assert f[1 + g] == want, (g, f[1 + g], want)
    assert f[2].split("\t")[4] == "NA"                              # the failed gene between two good ones
    rc, out, err = bp.run_burden_driver(path, "mb" + spec.split(",mb")[1], perm_exact=True)
    assert rc == 0, err
    f = bp.split_outputs(out)["out.MadsonBrowning.assoc"]
    assert f[0] == bp.SITE_HEADER + bp.PERM_HEADER and len(f) == 1 + len(genes)
    orc.rand_seed(1)
    for g, G in enumerate(genes):
        s = bp.mb_statement(G, X1, y, nperm, alpha, keep=True)
        row = f[1 + g].split("\t")
        if not s["fit_ok"]:
            assert f[1 + g] == site(g) + bp.perm_fields(nperm, s)
            continue
        # the printed Stat is the device's observed value (6 significant digits of a value good to 1e-9); the counters are the
        # statement's when no shuffle lies within the bound of the observed value
        assert all(abs(p - s["stat"]) > b + 2e-9 * s["stat"] for p, b in zip(s["perms"], s["bounds"])), "near-tie: choose another seed"
        assert f[1 + g] == site(g) + bp.perm_fields(nperm, s), (g, row)
    # (b) covariates: RareCover warns and prints an NA row, Madsen-Browning fits its null model with them
    cov = rng.normal(size=(N, 2))
    bp.write_input(path, y, 1, genes[:1], cov=cov)
    rc, out, err = bp.run_burden_driver(path, spec, perm_exact=True)
    assert rc == 0, err
    fo = bp.split_outputs(out)
    assert fo["out.RareCover.assoc"][1] == site(0) + "NA\t" + bp.perm_fields(nperm, {"fit_ok": False})
    orc.rand_seed(1)
    s = bp.mb_statement(genes[0], np.column_stack([X1, cov]), y, nperm, alpha, keep=True)
    assert all(abs(p - s["stat"]) > b + 2e-9 * s["stat"] for p, b in zip(s["perms"], s["bounds"])), "near-tie: choose another seed"
    assert fo["out.MadsonBrowning.assoc"][1] == site(0) + bp.perm_fields(nperm, s)
    # (c) a quantitative trait: both fail; Madsen-Browning's header is "Pvalue" and an empty line, its rows NA
    bp.write_input(path, rng.normal(size=N), 0, genes[:2])
    rc, out, err = bp.run_burden_driver(path, spec, perm_exact=True)
    assert rc == 0, err
    fo = bp.split_outputs(out)
    assert fo["out.RareCover.assoc"][1:] == [site(g) + "NA\t" + bp.perm_fields(nperm, {"fit_ok": False}) for g in (0, 1)]
    assert fo["out.MadsonBrowning.assoc"] == [bp.SITE_HEADER + "Pvalue", ""] + [site(g) + "NA" for g in (0, 1)]
