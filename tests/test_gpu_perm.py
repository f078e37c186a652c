"""SKAT permutation p-values through the C ABI.  Exact mode (rvt_set_perm_exact): the same emulated glibc rand() stream as
the oracle, so the permutations — and with them ActualPerm / NumGreater / NumEqual — are identical, gene after gene.
Counter-based mode (the default): other random numbers, the same estimator — compared with the exact mode within binomial
error.

The second half holds both modes against tests/permref.py shuffle by shuffle (Engine.debug_perm_trace hands out the statistics
the stop rule consumed), on the cases of tests/perm_cases.py: the routes a large cohort takes — the integer-plane product beyond
2048 samples, several 2048-shuffle chunks on one stream, the counter-based kernel at sizes around its groups, slices and
passes.  tests/test_perm_ref_cpu.py proves the premises (the tie condition) from the reference alone."""
import numpy as np
import pytest

import orc
import perm_cases as pc
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


def test_glibc_stream_matches_libc():
    """the oracle's generator is glibc's: compare with the C library itself"""
    import ctypes
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(1)
    orc.rand_seed(1)
    assert [libc.rand() for _ in range(2000)] == [orc.lib().orc_rand() for _ in range(2000)]


# (300 x 0.0333 x 2 = 19.98: the reference's threshold is an INT member, src/Permutation.h:153 -> 19, not 19.98 -> a stop one
#  hit earlier; 100 x 0.001 x 2 = 0.2 -> 0: no permutation at all, p = 1 — both pinned on the reference's compiled class in
#  tests/test_oracle_ref.py)
@pytest.mark.parametrize("N,n_perm,alpha,explicit", [(331, 300, 0.05, True), (1000, 120, 0.2, True), (331, 300, 0.05, False),
                                                     (331, 300, 0.0333, True), (331, 100, 0.001, True)])
def test_permutation_counts_match_oracle(eng, N, n_perm, alpha, explicit):
    """explicit = False: NO mode is selected — a fresh single context must reproduce the reference's counters by DEFAULT
    (the counter-based mode is for genes dealt over several devices, or on request)."""
    import rvtests_amd
    if not explicit:
        eng = rvtests_amd.Engine(0)     # a context nobody has configured
    d = 2
    genes = [synth.make_gene(N, M, seed=500 + M, missing=0.01, common=True, mono=True)[1:] for M in (8, 1, 21, 5)]
    genes.insert(2, (np.zeros((N, 3)), np.zeros(3)))       # no polymorphic column: no permutations, no draws
    X, y, res, v, s2 = synth.make_null(N, d, 0, seed=8, G_effect=0.8 * genes[0][0][:, :2].sum(1))
    eng.set_null(0, X, res, v, s2)
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, n_perm, alpha)
    ptrs = [eng.upload_block(G) for G, af in genes]
    if explicit:
        eng.set_perm_exact(True)
        eng.rand_seed(1)
    out = eng.run_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes],
                         tests=rvtests_amd.TEST_SKAT, params=prm)
    orc.rand_seed(1)
    stopped_early = 0
    for r, (G, af) in zip(out, genes):
        rc, a = orc.skat(G, af, X, res, v, 0)
        if a.n_poly == 0:
            assert r.skat_ok == 0 and r.perm_ok == 0
            continue
        assert abs(r.skat_Q - a.Q) <= 1e-10 * a.Q
        # the oracle permutes in fp64 with the device's observed statistic as threshold reference
        rc, p = orc.skat_permute(G, af, res, r.skat_Q, n_perm, alpha)
        assert rc == 0
        assert r.perm_ok == 1 and r.perm_num_perm == n_perm
        assert (r.perm_actual_perm, r.perm_num_greater, r.perm_num_equal) == (p.actual_perm, p.num_x, p.num_equal)
        assert r.perm_pvalue == p.pvalue
        stopped_early += p.actual_perm < n_perm
    assert stopped_early >= 1          # the adaptive stop was exercised
    if n_perm == 100:                  # threshold truncated to 0: Permutation::next() is false before the first shuffle
        assert all(r.perm_actual_perm == 0 and r.perm_pvalue == 1.0 for r in out if r.perm_ok)


def test_counter_based_mode_agrees_with_the_exact_mode_within_binomial_error(eng):
    """200 null genes, N = 2000: permutation p-values of the counter-based mode against the replay of the reference's
    stream — two Monte-Carlo estimates of the same tail probability, so their difference scales with the binomial
    standard errors; and against the analytic SKAT p-value (both modes estimate it)."""
    import rvtests_amd
    N, d, n_genes, n_perm, alpha = 2000, 2, 200, 2000, 0.05
    rng = np.random.default_rng(99)
    X, y, res, v, s2 = synth.make_null(N, d, 0, seed=21)
    eng.set_null(0, X, res, v, s2)
    genes = []
    for g in range(n_genes):
        M = int(rng.integers(3, 40))
        G = np.asfortranarray(rng.binomial(2, 10 ** rng.uniform(-2.3, -0.8, M), size=(N, M)).astype(np.float64))
        genes.append((G, G.sum(0) / (2.0 * N)))
    ptrs = [eng.upload_block(G) for G, af in genes]
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, n_perm, alpha)
    Ms, afs = [G.shape[1] for G, af in genes], [af for G, af in genes]
    eng.set_perm_exact(True)
    eng.rand_seed(1)
    exact = eng.run_blocks(ptrs, Ms, afs, tests=rvtests_amd.TEST_SKAT, params=prm)
    eng.set_perm_exact(False)
    eng.rand_seed(1)
    cb = eng.run_blocks(ptrs, Ms, afs, tests=rvtests_amd.TEST_SKAT, params=prm, ids=list(range(100, 100 + n_genes)))
    cb2 = eng.run_blocks(ptrs[::-1], Ms[::-1], afs[::-1], tests=rvtests_amd.TEST_SKAT, params=prm,
                         ids=list(range(100, 100 + n_genes))[::-1])[::-1]
    z = []
    for a, b, b2 in zip(exact, cb, cb2):
        assert a.perm_ok and b.perm_ok
        # keyed by gene id: the order of the genes does not matter
        assert (b.perm_actual_perm, b.perm_num_greater, b.perm_pvalue) == (b2.perm_actual_perm, b2.perm_num_greater, b2.perm_pvalue)
        pa, pb = a.perm_pvalue, b.perm_pvalue
        se = np.sqrt(pa * (1 - pa) / a.perm_actual_perm + pb * (1 - pb) / b.perm_actual_perm) + 1e-9
        z.append((pb - pa) / se)
    z = np.array(z)
    assert abs(z.mean()) < 0.25 and 0.7 < z.std() < 1.35 and (np.abs(z) > 4).sum() == 0, (z.mean(), z.std(), np.abs(z).max())
    # both estimate the analytic p-value (Davies): no systematic offset of the counter-based estimates
    dev = np.array([(b.perm_pvalue - b.skat_p) for b in cb])
    assert abs(dev.mean()) < 0.02
    for p in ptrs:
        eng.free_block(p)


@pytest.mark.parametrize("exact", [True, False])
def test_a_context_whose_null_model_grows_keeps_no_buffer_of_the_old_size(eng, exact):
    """One context, two analyses: N = 700 with 400 permutations, then N = 9 001 with 30 (fewer shuffles of more samples: the
    chunk of shuffles N x B shrinks while every per-sample buffer grows).  The second analysis gives what a fresh context gives
    (round 6: the flipped-genotype buffer of the permutation stage was kept by its column count alone and overran)."""
    import rvtests_amd
    outs = []
    for fresh in (False, True):
        e = rvtests_amd.Engine(0) if fresh else eng
        for N, n_perm in ((700, 400), (9001, 30)) if not fresh else ((9001, 30),):
            genes = [synth.make_gene(N, M, seed=900 + M, missing=0.01, common=True, mono=True)[1:] for M in (24, 7, 40)]
            X, y, res, v, s2 = synth.make_null(N, 2, 0, seed=18, G_effect=0.5 * genes[0][0][:, :2].sum(1))
            e.set_null(0, X, res, v, s2)
            prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, n_perm, 0.4)
            e.set_perm_exact(exact)
            if exact:
                e.rand_seed(1)
            ptrs = [e.upload_block(G) for G, af in genes]
            out = e.run_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes], tests=rvtests_amd.TEST_SKAT,
                               params=prm, ids=[0, 1, 2])   # (the counter-based shuffles are a function of the gene id)
            for p in ptrs:
                e.free_block(p)
        outs.append([(r.skat_Q, r.skat_p, r.perm_actual_perm, r.perm_num_greater, r.perm_num_equal, r.perm_pvalue) for r in out])
        if fresh:
            e.close()
    assert outs[0] == outs[1] and all(t[2] > 0 for t in outs[0])


# ---- shuffle by shuffle against tests/permref.py ------------------------------------------------------------------------------
LD = np.longdouble


def _within_bound(Qdev, ref, what):
    """Every traced statistic lies inside the reference's a-priori bound; returns (and prints) the largest |dQ| / bound."""
    n = Qdev.size
    assert n <= ref.st.Q.size, what
    ratio = np.abs(Qdev.astype(LD) - ref.st.Q[:n]) / ref.dQ[:n]
    worst = float(ratio.max()) if n else 0.0
    print("%s: %d shuffles, largest |Q_dev - Q_ref| / bound = %.3g (at shuffle %d)" % (what, n, worst, int(ratio.argmax()) if n else -1))
    assert worst <= 1.0, (what, worst, int(ratio.argmax()))
    return worst


def _fields(r):
    vals = [(f[0], getattr(r, f[0])) for f in r._fields_]
    return [(k, v if v == v else "nan") for k, v in vals]      # (a NaN field equals itself here)


def _upload(eng, genes):
    return [eng.upload_block(G) for G, af in genes], [G.shape[1] for G, af in genes], [af for G, af in genes]


def _check_exact_gene(r, ref, n_perm):
    p = ref.perm
    assert abs(r.skat_Q - ref.obs) <= pc.OBS_TOL * ref.obs
    assert r.perm_ok == 1 and r.perm_num_perm == n_perm
    assert (r.perm_actual_perm, r.perm_num_greater, r.perm_num_equal) == (p.actual_perm, p.num_x, p.num_equal)
    assert r.perm_pvalue == p.pvalue


@pytest.mark.parametrize("N", pc.SWITCH_N)
def test_exact_mode_matches_the_oracle_on_both_sides_of_the_2048_sample_switch(eng, N):
    """Five genes on one stream at N = 2048 (sample-order sums), 2049 (the integer planes, the last K chunk 127 rows of
    padding) and 4100: counters and p-value equal the oracle's gene after gene, and every statistic of the M = 21 gene (six
    digit planes) lies inside the bound of its route."""
    import rvtests_amd
    genes, (X, y, res, v, s2), refs = pc.switch_case(N)
    eng.set_null(0, X, res, v, s2)
    eng.set_perm_exact(True)
    eng.rand_seed(pc.SWITCH_SEED)
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, pc.SWITCH_NPERM, pc.SWITCH_ALPHA)
    ptrs, Ms, afs = _upload(eng, genes)
    t = pc.SWITCH_TRACED
    out = eng.run_blocks(ptrs[:t], Ms[:t], afs[:t], tests=rvtests_amd.TEST_SKAT, params=prm)
    trace = eng.debug_perm_trace(pc.SWITCH_NPERM)          # (one arming = one gene: the stream goes on over the two calls)
    out += eng.run_blocks(ptrs[t:], Ms[t:], afs[t:], tests=rvtests_amd.TEST_SKAT, params=prm)
    for r, ref in zip(out, refs):
        if ref.obs is None:
            assert r.skat_ok == 0 and r.perm_ok == 0
        else:
            _check_exact_gene(r, ref, pc.SWITCH_NPERM)
    Qdev = trace()
    assert Qdev.size == refs[t].perm.actual_perm
    _within_bound(Qdev, refs[t], "switch N=%d, route %s" % (N, refs[t].route))


@pytest.mark.parametrize("N", pc.CHUNKS_N)
def test_exact_mode_carries_vector_and_stream_across_chunks(eng, N):
    """Three genes on one stream: 5000 shuffles that never stop (chunks of 2048 + 2048 + 904, all traced), 5000 that stop inside
    the second chunk, and 200 more that only match the oracle if the stream stood behind the shuffles PERFORMED."""
    import rvtests_amd
    genes, (X, y, res, v, s2), refs = pc.chunks_case(N)
    assert 2048 < refs[1].perm.actual_perm < 4096
    eng.set_null(0, X, res, v, s2)
    eng.set_perm_exact(True)
    eng.rand_seed(pc.CHUNKS_SEED)
    ptrs, Ms, afs = _upload(eng, genes)
    trace = eng.debug_perm_trace(pc.CHUNKS_RUNS[0][0])
    for k, (n_perm, alpha) in enumerate(pc.CHUNKS_RUNS):
        prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, n_perm, alpha)
        r = eng.run_blocks(ptrs[k:k + 1], Ms[k:k + 1], afs[k:k + 1], tests=rvtests_amd.TEST_SKAT, params=prm, ids=[k])[0]
        _check_exact_gene(r, refs[k], n_perm)
    Qdev = trace()
    assert Qdev.size == 5000
    _within_bound(Qdev, refs[0], "chunks N=%d, route %s" % (N, refs[0].route))
    for s in (2047, 2048, 4095, 4096):                      # (named: both sides of either chunk boundary)
        assert abs(LD(Qdev[s]) - refs[0].st.Q[s]) <= refs[0].dQ[s]


def _run_counter(eng, ptr, M, af, ref):
    import rvtests_amd
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, ref.n_perm, ref.alpha)
    trace = eng.debug_perm_trace(ref.n_perm)
    r = eng.run_blocks([ptr], [M], [af], tests=rvtests_amd.TEST_SKAT, params=prm, ids=[ref.gene_id])[0]
    assert abs(r.skat_Q - ref.obs) <= pc.OBS_TOL * ref.obs
    assert r.perm_ok == 1 and r.perm_num_perm == ref.n_perm and r.gene_id == ref.gene_id
    return r, trace()


@pytest.mark.parametrize("N,m", pc.COUNTER_SIZES)
def test_counter_based_mode_shuffle_by_shuffle(eng, N, m):
    """perm_counter_partial_kernel / perm_counter_q_kernel against the long-double product of the same keyed shuffles: a run of
    100 shuffles (36 live rows in the last 64-shuffle block) and one of 2300 (the second chunk starts at shuffle 2048), every
    statistic inside gamma_N, the counters those of the stop rule on the reference's statistics."""
    (G, af), (X, y, res, v, s2), refs = pc.counter_case(N, m)
    eng.set_null(0, X, res, v, s2)
    eng.set_perm_exact(False)
    eng.rand_seed(pc.COUNTER_SEED)
    ptr = eng.upload_block(G)
    for ref in refs:
        r, Qdev = _run_counter(eng, ptr, G.shape[1], af, ref)
        assert Qdev.size == ref.n_perm
        _within_bound(Qdev, ref, "counter N=%d m=%d nPerm=%d" % (N, m, ref.n_perm))
        assert (r.perm_actual_perm, r.perm_num_greater, r.perm_num_equal, r.perm_pvalue) == ref.counters


def test_counter_based_mode_short_first_chunk_and_early_stop(eng):
    """alpha = 0.05 of 1000: the first chunk is 250 shuffles, the gene stops in the second one (which starts at shuffle 250)."""
    (G, af), (X, y, res, v, s2), ref = pc.counter_stop_case()
    assert 250 < ref.counters[0] < ref.n_perm
    eng.set_null(0, X, res, v, s2)
    eng.set_perm_exact(False)
    eng.rand_seed(pc.COUNTER_SEED)
    r, Qdev = _run_counter(eng, eng.upload_block(G), G.shape[1], af, ref)
    assert Qdev.size == ref.counters[0]                     # what the chunk generated past the stop is not recorded
    _within_bound(Qdev, ref, "counter stop")
    assert (r.perm_actual_perm, r.perm_num_greater, r.perm_num_equal, r.perm_pvalue) == ref.counters


@pytest.mark.parametrize("exact", [True, False])
def test_the_armed_trace_changes_no_record(eng, exact):
    """The same genes unarmed, armed, and armed-then-disarmed: records equal field for field, a short buffer is not overrun,
    a disarmed one is not written."""
    import rvtests_amd
    if exact:
        genes, (X, y, res, v, s2), refs = pc.switch_case(2049)
        genes, n_perm, alpha, seed = genes[:3], pc.SWITCH_NPERM, pc.SWITCH_ALPHA, pc.SWITCH_SEED
    else:
        (G, af), (X, y, res, v, s2), ref = pc.counter_stop_case()
        genes, n_perm, alpha, seed = [(G, af)], ref.n_perm, ref.alpha, pc.COUNTER_SEED
    eng.set_null(0, X, res, v, s2)
    eng.set_perm_exact(exact)
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, n_perm, alpha)
    ptrs, Ms, afs = _upload(eng, genes)
    ids = [77 + 5 * k for k in range(len(genes))]
    runs = []
    for mode in ("unarmed", "armed", "short", "disarmed"):
        eng.rand_seed(seed)
        trace = eng.debug_perm_trace({"armed": n_perm, "short": 7, "disarmed": n_perm}[mode]) if mode != "unarmed" else None
        if mode == "disarmed":
            assert eng.debug_perm_trace(None) is None
        out = eng.run_blocks(ptrs, Ms, afs, tests=rvtests_amd.TEST_SKAT, params=prm, ids=ids)
        runs.append([_fields(r) for r in out])
        if mode == "armed":                                 # the first gene of the call was traced, and only that one
            full = trace()
            assert full.size == out[0].perm_actual_perm > 7
        elif mode == "short":
            assert np.array_equal(trace(), full[:7])
        elif mode == "disarmed":
            assert trace().size == 0
    assert runs[0] == runs[1] == runs[2] == runs[3]
