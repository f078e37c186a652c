"""Price's variable-threshold permutation test (--vt price) through the C ABI and the host driver, against the numpy statement
of tests/test_vtprice_cpu.py.  Exact mode: the reference's own shuffles, so ActualPerm / NumGreater / NumEqual are the
statement's gene after gene; counter mode: other shuffles, the same estimator, independent of gene order and context."""
import numpy as np
import pytest

import orc
import test_vtprice_cpu as vt

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


def _set_n(e, N, seed=0):
    """a null model only defines N for this test (covariates are ignored)"""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(np.ones((N, 1)))
    y = rng.normal(size=N)
    e.fit_null(0, X, y.copy())


def _gene(rng, N, M, lo=-2.2, hi=-1.0, ties=False):
    maf = 10 ** rng.uniform(lo, hi, M)
    G = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    if ties:
        for j in range(1, M, 3):
            G[:, j] = G[rng.permutation(N), j - 1]               # the same allele count: one frequency group
    G = np.asfortranarray(G)
    return G, G.sum(0) / (2.0 * N)


def _run(e, genes, y, nperm, alpha):
    ptrs = [e.upload_block(G) for G, af in genes]
    out = e.vtprice_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes], y, nperm, alpha)
    for p in ptrs:
        e.free_block(p)
    return out


def _tuple(r):
    return (r.fit_ok, r.n_poly, r.n_threshold, r.n_carrier_entries, r.opt_freq, r.zmax, r.num_perm, r.actual_perm, r.num_greater,
            r.num_equal, r.perm_pvalue)


@pytest.mark.parametrize("N", [700, 9001])
def test_exact_mode_counts_follow_the_statement_gene_after_gene(eng, N):
    rng = np.random.default_rng(40 + N)
    nperm, alpha = 200, 0.05
    genes = [_gene(rng, N, 12), _gene(rng, N, 9, lo=-1.6, hi=-1.2), (np.zeros((N, 3)), np.zeros(3)), _gene(rng, N, 70, ties=True),
             _gene(rng, N, 5)]
    y = rng.normal(size=N) + 1.2 * (genes[1][0] > 0).sum(1)       # gene 1 is causal: it uses all nPerm
    _set_n(eng, N)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    out = _run(eng, genes, y, nperm, alpha)
    out2 = _run(eng, genes[:1], y, 100, 0.001)                    # (int)(100 x 0.001 x 2) = 0: no shuffle, p = 1
    probe = _run(eng, genes[4:], y, 60, 0.4)                      # its counts depend on where the stream stands now
    probe += _run(eng, genes[:1], y, 40, 0.4)                     # ... and this one's on where the first probe left it
    orc.rand_seed(1)
    early = 0
    for k, (r, (G, af)) in enumerate(zip(list(out) + list(out2) + list(probe), genes + genes[:1] + genes[4:] + genes[:1])):
        np_, al = (nperm, alpha) if k < len(genes) else [(100, 0.001), (60, 0.4), (40, 0.4)][k - len(genes)]
        ref = vt.statement(G, af, y, 0, al)                       # observed statistic only: draws nothing
        if not ref["fit_ok"]:
            assert r.fit_ok == 0 and r.n_poly == 0 and r.actual_perm == 0 and r.perm_pvalue == 1.0
            continue
        bound = vt.zmax_bound(ref)
        print("N", N, "gene", k, "zmax", r.zmax, "statement", ref["zmax"], "bound", bound, "nnz", ref["nnz"])
        assert r.fit_ok == 1 and r.n_poly == ref["n_poly"] and r.n_threshold == ref["n_threshold"]
        assert r.n_carrier_entries == ref["nnz"] and r.opt_freq == ref["opt_freq"]
        assert abs(r.zmax - ref["zmax"]) <= bound
        s = vt.statement(G, af, y, np_, al, obs=r.zmax, keep=True)
        # no permuted statistic of the statement within twice the bound of the observed one (the device's permuted statistic
        # carries a reordering error of the same size as the observed one's): the counts are then comparable
        assert all(abs(p - r.zmax) > 2 * bound for p in s["perms"]), "near-tie: choose another seed"
        assert (r.num_perm, r.actual_perm, r.num_greater, r.num_equal) == (np_, s["actual"], s["num_x"], s["num_eq"]), k
        assert r.perm_pvalue == s["pvalue"]
        early += k < len(genes) and s["actual"] < np_
    assert out[1].actual_perm == nperm and out[1].num_greater == 0 and early >= 1
    assert out[3].n_poly > 64 and out[3].n_threshold < out[3].n_poly
    assert out2[0].actual_perm == 0 and out2[0].perm_pvalue == 1.0 and out2[0].fit_ok == 1


def _binary_case():
    N = 700
    rng = np.random.default_rng(77)
    genes = [_gene(rng, N, 6, lo=-2.0, hi=-1.5), _gene(rng, N, 14)]
    return N, genes, (rng.random(N) < 0.35).astype(np.float64)


def test_binary_trait_counts_equal_the_integer_exact_statement(eng):
    """With the stop rule active (alpha = 0.2) the counts are those of the integer-exact statement.  The sample-order fp64
    statement is no yardstick here: one tie that it splits differently moves the stopping point, after which ActualPerm and
    every later count differ (gene 1: 160 shuffles, p = 0.746875 here; 162 shuffles, p = 0.740741 there)."""
    N, genes, y = _binary_case()
    nperm, alpha = 300, 0.2
    _set_n(eng, N)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    out = _run(eng, genes, y, nperm, alpha)
    orc.rand_seed(1)
    exact = [vt.statement(G, af, y, nperm, alpha, binary_exact=True) for G, af in genes]
    for r, s in zip(out, exact):
        assert r.zmax == s["zmax"] and r.opt_freq == s["opt_freq"]
        assert (r.actual_perm, r.num_greater, r.num_equal) == (s["actual"], s["num_x"], s["num_eq"]) and r.perm_pvalue == s["pvalue"]
    assert any(r.actual_perm < nperm for r in out) and sum(r.num_equal for r in out) > 0


def test_binary_trait_p_value_is_within_half_numequal_of_the_sample_order_statement(eng):
    """alpha = 1: the stop rule cannot fire, both forms run the same nPerm shuffles, and the shuffles that tie here may fall on
    either side there: |p - p'| <= 0.5 NumEqual / ActualPerm.  Asserted on the integers 2 ActualPerm p = 2 NumGreater + NumEqual,
    where the bound has no rounding of its own."""
    N, genes, y = _binary_case()
    nperm, alpha = 300, 1.0
    _set_n(eng, N)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    out = _run(eng, genes, y, nperm, alpha)
    orc.rand_seed(1)
    exact = [vt.statement(G, af, y, nperm, alpha, binary_exact=True) for G, af in genes]
    orc.rand_seed(1)
    plain = [vt.statement(G, af, y, nperm, alpha) for G, af in genes]
    for r, s, q in zip(out, exact, plain):
        assert (r.actual_perm, r.num_greater, r.num_equal) == (s["actual"], s["num_x"], s["num_eq"]) and r.perm_pvalue == s["pvalue"]
        assert r.actual_perm == q["actual"] == nperm
        print("engine", r.num_greater, r.num_equal, r.perm_pvalue, "sample-order statement", q["num_x"], q["num_eq"], q["pvalue"])
        assert abs((2 * r.num_greater + r.num_equal) - (2 * q["num_x"] + q["num_eq"])) <= r.num_equal
        assert r.perm_pvalue == (2 * r.num_greater + r.num_equal) / (2.0 * r.actual_perm)
        assert q["pvalue"] == (2 * q["num_x"] + q["num_eq"]) / (2.0 * q["actual"])
    assert sum(r.num_equal for r in out) > 0                      # ties with the observed value did occur


def test_binary_trait_in_counter_mode_ties_exactly_and_agrees_with_the_exact_mode(eng):
    """the uncentred 0 / 1 phenotype through vtp_segsum_kernel<kVtpCounter>: ties with the observed value, the same record on
    another context in the other gene order, p-values within binomial error of the exact mode's"""
    import rvtests_amd
    N, genes, y = _binary_case()
    nperm = 4000
    _set_n(eng, N)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    ex = _run(eng, genes, y, nperm, 1.0)
    eng.set_perm_exact(False)
    eng.rand_seed(1)
    cb = _run(eng, genes, y, nperm, 1.0)
    other = rvtests_amd.Engine(0)
    _set_n(other, N)
    other.set_perm_exact(False)
    other.rand_seed(1)
    cb2 = _run(other, genes[::-1], y, nperm, 1.0)[::-1]
    other.close()
    assert [_tuple(r) for r in cb] == [_tuple(r) for r in cb2]
    for a, b in zip(ex, cb):
        assert a.zmax == b.zmax and a.opt_freq == b.opt_freq and a.actual_perm == b.actual_perm == nperm
        pa, pb = a.perm_pvalue, b.perm_pvalue
        se = np.sqrt(pa * (1 - pa) / nperm + pb * (1 - pb) / nperm) + 1e-9
        print("exact", a.num_greater, a.num_equal, pa, "counter", b.num_greater, b.num_equal, pb, "z", (pb - pa) / se)
        assert abs(pb - pa) <= 5 * se
    assert sum(r.num_equal for r in cb) > 0


def test_counter_mode_is_independent_of_gene_order_and_context_and_agrees_with_the_exact_mode(eng):
    import rvtests_amd
    N, n_genes, nperm, alpha = 2000, 200, 2000, 0.05
    rng = np.random.default_rng(99)
    genes = [_gene(rng, N, int(rng.integers(3, 40)), lo=-2.3, hi=-0.8) for _ in range(n_genes)]
    y = rng.normal(size=N)
    _set_n(eng, N)
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    exact = _run(eng, genes, y, nperm, alpha)
    eng.set_perm_exact(False)
    eng.rand_seed(1)
    cb = _run(eng, genes, y, nperm, alpha)
    other = rvtests_amd.Engine(0)
    _set_n(other, N)
    other.set_perm_exact(False)
    other.rand_seed(1)
    cb2 = _run(other, genes[::-1], y, nperm, alpha)[::-1]
    other.close()
    assert [_tuple(r) for r in cb] == [_tuple(r) for r in cb2]     # bit-equal
    z = []
    for a, b in zip(exact, cb):
        assert a.fit_ok and b.fit_ok and a.zmax == b.zmax
        pa, pb = a.perm_pvalue, b.perm_pvalue
        se = np.sqrt(pa * (1 - pa) / a.actual_perm + pb * (1 - pb) / b.actual_perm) + 1e-9
        z.append((pb - pa) / se)
    z = np.array(z)
    print("z mean", z.mean(), "sd", z.std(), "max", np.abs(z).max())
    assert abs(z.mean()) < 0.25 and 0.7 < z.std() < 1.35 and (np.abs(z) > 4).sum() == 0, (z.mean(), z.std(), np.abs(z).max())


def test_a_causal_gene_reaches_the_floor_in_both_modes(eng):
    N, nperm = 3000, 1000
    rng = np.random.default_rng(5)
    G, af = _gene(rng, N, 15, lo=-1.8, hi=-1.2)
    y = rng.normal(size=N) + 1.0 * (G > 0).sum(1)
    _set_n(eng, N)
    for exact in (True, False):
        eng.set_perm_exact(exact)
        eng.rand_seed(1)
        r = _run(eng, [(G, af)], y, nperm, 0.05)[0]
        assert (r.actual_perm, r.num_greater, r.num_equal, r.perm_pvalue) == (nperm, 0, 0, 0.0)


@pytest.mark.parametrize("exact", [True, False])
def test_two_analyses_of_different_n_on_one_context_and_poisoned_work_spaces(eng, exact, monkeypatch):
    """N = 700 with 400 shuffles, then N = 9 001 with 30, on one context = what a fresh context with poisoned allocations gives"""
    import rvtests_amd
    outs = []
    for fresh in (False, True):
        if fresh:
            monkeypatch.setenv("RVT_POISON", "255")
        e = rvtests_amd.Engine(0) if fresh else eng
        for N, nperm in ((700, 400), (9001, 30)) if not fresh else ((9001, 30),):
            rng = np.random.default_rng(N)
            genes = [_gene(rng, N, M) for M in (24, 7, 40)]
            y = rng.normal(size=N)
            _set_n(e, N)
            e.set_perm_exact(exact)
            e.rand_seed(1)
            out = _run(e, genes, y, nperm, 0.4)
        outs.append([_tuple(r) for r in out])
        if fresh:
            e.close()
    assert outs[0] == outs[1] and all(t[7] > 0 for t in outs[0])


def test_one_gene_at_half_a_million_samples_in_counter_mode(eng):
    N = 500000
    rng = np.random.default_rng(12)
    G, af = _gene(rng, N, 30, lo=-3.3, hi=-1.3)
    y = rng.normal(size=N)
    _set_n(eng, N)
    eng.set_perm_exact(False)
    eng.rand_seed(1)
    r = _run(eng, [(G, af)], y, 2000, 0.05)[0]
    ref = vt.statement(G, af, y, 0, 0.05)
    bound = vt.zmax_bound(ref)
    print("zmax", r.zmax, "statement", ref["zmax"], "bound", bound, "nnz", ref["nnz"], "perms", r.actual_perm, "p", r.perm_pvalue)
    assert r.fit_ok == 1 and r.n_threshold == ref["n_threshold"] and r.n_carrier_entries == ref["nnz"]
    assert r.opt_freq == ref["opt_freq"] and abs(r.zmax - ref["zmax"]) <= bound
    assert 0 < r.actual_perm <= 2000 and 0.0 < r.perm_pvalue <= 1.0


def test_driver_rows_equal_the_statement_s_including_a_failed_gene(tmp_path):
    vt._ensure_driver()
    N, nperm, alpha = 900, 150, 0.1
    rng = np.random.default_rng(31)
    genes = [_gene(rng, N, 8), (np.zeros((N, 2)), np.zeros(2)), _gene(rng, N, 20, ties=True), _gene(rng, N, 4)]
    y = rng.normal(size=N) + 0.8 * (genes[2][0][:, :6] > 0).sum(1)
    path = str(tmp_path / "in.bin")
    vt._write_input(path, y, 0, genes)
    rc, out, err = vt.run_vt_driver(path, "price[nPerm=%d,alpha=%g]" % (nperm, alpha), perm_exact=True)
    assert rc == 0, err
    lines = out.split("\n")
    assert lines[0] == "== out.VariableThresholdPrice.assoc"
    assert lines[1] == "Range\tN_INFORMATIVE\tNumVar\tNumPolyVar\t" + "\tOptFreq\tZmax\t" + vt.PERM_HEADER
    orc.rand_seed(1)
    last = (-1.0, -1.0)
    for g, (G, af) in enumerate(genes):
        s = vt.statement(G, af, y, nperm, alpha)
        want = "gene%d\t%d\t%d\t\t" % (g, N, G.shape[1]) + vt.format_row(s, nperm, last)
        assert lines[2 + g] == want, (g, lines[2 + g], want)
        if s["fit_ok"]:
            last = (s["opt_freq"], s["zmax"])
    assert lines[3].split("\t")[5:7] == lines[2].split("\t")[5:7]      # the failed gene repeats the previous OptFreq / Zmax
