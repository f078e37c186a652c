"""GPU: the launch shapes of the hard-call sufficient-statistics kernel (rvtests_amd/csrc/k2_hardcall.hip: ring depth x
waves per SIMD per tile class, RVT_HC_CFG) and the one launch for the one-wave classes (gene_suffstat_hc_any,
RVT_HC_FUSE).  A launch shape decides where a wave-part runs and what it keeps in flight, never what it computes: every
record must come out with the same bits whatever the shapes, and the default context must agree with the oracle.

The reference context of the bit comparison (one launch per class, the parent's shapes) runs the same kernel body as the
others, pad lanes of the null tile included (lanes v > d read nothing): an error there shows in the oracle comparison of
the default context, not in the bit comparison.  At N = 100 (six full steps) the depth-3 shapes take the remainder path
alone; the shapes whose ring iteration is four steps run one iteration first."""

import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu

D = 3
MS = (20, 32, 33, 48, 49, 64, 65, 80, 96, 48, 64, 80)          # nine widths (classes 2 .. 6) plus three repeats
PARENT = "3:2x2,4:2x2,2:2x3"                                    # the launch shapes before RVT_HC_CFG existed
# the engine's default shapes (rvt_engine_int.h: hc_shape) and the one-wave depth of gene_suffstat_hc_any per class
# (suffstat_hc.hip.h: hc_any_depth)
DEFAULT_SHAPES = {1: (2, 4), 2: (4, 1), 3: (3, 1), 4: (2, 2), 5: (1, 1), 6: (1, 1)}
ANY_DEPTH = {2: 4, 3: 3, 4: 2, 5: 1}


def _genes(N, maf_hi):
    """Hard-call genes of the widths MS; gene 2 has a flipped column (af > 0.5), gene 4 a mean-imputed column (0.5 % of
    its entries, at least one), gene 6 a monomorphic column."""
    genes = []
    for i, M in enumerate(MS):
        rng = np.random.default_rng(1000 * N + 31 * i + M)
        maf = 10 ** rng.uniform(-3.3, maf_hi, M)
        G = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
        if i == 2:
            G[:, 7] = rng.binomial(2, 0.85, size=N)
        if i == 4:
            col = rng.binomial(2, 0.2, size=N).astype(np.float64)
            miss = rng.random(N) < 0.005
            miss[N // 3] = True
            col[miss] = col[~miss].mean()
            G[:, 11] = col
        if i == 6:
            G[:, 5] = 0.0
        genes.append((np.asfortranarray(G), G.sum(0) / (2.0 * N)))
    return genes


def _planned_launches(Ms, fuse, shapes):
    """launch_hardcall_classes (rvt_engine.hip): the classes whose shape is the one-wave shape of gene_suffstat_hc_any
    share one launch when there are at least two of them; every other class has its own."""
    classes = {(M + 15) // 16 for M in Ms}
    fused = {c for c in classes if fuse and c in ANY_DEPTH and shapes[c] == (ANY_DEPTH[c], 1)}
    if len(fused) < 2:
        fused = set()
    return (1 if fused else 0) + len(classes - fused)


def _shapes(cfg):
    s = dict(DEFAULT_SHAPES)
    for item in (cfg or "").split(","):
        if item:
            mt, shape = item.split(":")
            s[int(mt)] = tuple(int(x) for x in shape.split("x"))
    return s


def _field_bytes(r):
    raw = bytes(r)
    return {name: raw[getattr(type(r), name).offset:getattr(type(r), name).offset + getattr(type(r), name).size]
            for name, _ in type(r)._fields_}


@pytest.fixture
def contexts(monkeypatch):
    """make(fuse, cfg) -> an engine whose context was created under RVT_HC_FUSE / RVT_HC_CFG (None: unset)"""
    import rvtests_amd
    made = []

    def make(fuse=None, cfg=None):
        for name, val in (("RVT_HC_FUSE", fuse), ("RVT_HC_CFG", cfg)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, val)
        e = rvtests_amd.Engine(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


def _run(eng, genes, null):
    X, y, res, v, s2 = null
    eng.set_null(0, X, res, v, s2)
    ptrs = [eng.upload_block(G) for G, af in genes]
    eng.set_profiling(True)
    eng.timing(reset=True)
    try:
        out = eng.run_blocks(ptrs, [G.shape[1] for G, af in genes], [af for G, af in genes])
        tm = eng.timing(reset=True)
    finally:
        eng.set_profiling(False)
    recs = [_field_bytes(r) for r in out]
    vals = [{name: getattr(r, name) for name, _ in type(r)._fields_} for r in out]
    for p in ptrs:
        eng.free_block(p)
    return recs, vals, tm


# (fuse, cfg) of every context compared with the parent's launch shapes: the default, then each one-wave shape forced —
# alone in a launch of its own, and with the other one-wave classes in gene_suffstat_hc_any — and the deeper two-wave ring
FORCED = [(None, None),
          ("0", "3:3x1"), ("0", "4:3x1"), ("0", "4:2x1"), ("0", "2:4x1"), ("0", "2:4x2"),
          ("0", "2:4x1,3:3x1,4:2x1"), ("1", "2:4x1,3:3x1,4:2x1"), ("1", "2:2x3,4:2x2"), ("1", "2:2x3,3:2x2")]


@pytest.mark.parametrize("N,maf_hi", [(5003, -1.0), (100, -0.5)])
def test_records_do_not_depend_on_the_launch_shapes(contexts, monkeypatch, N, maf_hi):
    """N = 5 003 in three wave-parts: ring iterations, and a last part whose remainder is a multiple of neither 16 nor
    64 (masked tail).  N = 100: at most one ring iteration, then the remainder path."""
    monkeypatch.setenv("RVT_WPARTS", "3")
    genes = _genes(N, maf_hi)
    null = synth.make_null(N, D, 0, seed=5, G_effect=0.4 * genes[4][0][:, :3].sum(1))
    X, y, res, v, s2 = null
    ref, _, tm = _run(contexts("0", PARENT), genes, null)
    n_classes = len({(M + 15) // 16 for M in MS})
    assert tm.genes_hard_call == len(genes) and tm.genes_handed_back == 0
    # one launch per class present.  (MS holds FIVE classes, M = 96 being class 6; the four launches of the flagship
    # workload are its four classes, M = 20 .. 80: the batch without the M = 96 gene, below)
    assert tm.n_suffstat_hc_launches == n_classes == 5
    for fuse, cfg in FORCED:
        got, vals, tm = _run(contexts(fuse, cfg), genes, null)
        assert tm.genes_hard_call == len(genes) and tm.genes_handed_back == 0
        assert tm.n_suffstat_hc_launches == _planned_launches(MS, fuse != "0", _shapes(cfg)), (fuse, cfg)
        for g, (a, b) in enumerate(zip(got, ref)):
            for name in a:
                assert a[name] == b[name], (fuse, cfg, MS[g], name)
        if (fuse, cfg) != (None, None):
            continue
        # the default context against the oracle, at the tolerances of tests/test_gpu_hardcall.py
        # (test_mean_imputed_columns_stay_on_the_hardcall_kernel)
        for r, (G, af) in zip(vals, genes):
            rc, o = orc.skat(G, af, X, res, v, 0)
            assert r["n_poly"] == o.n_poly
            if o.n_poly:
                assert abs(r["skat_Q"] - o.Q) <= 1e-10 * o.Q and abs(r["skat_p"] - o.pvalue) <= 1e-6 * o.pvalue + 1e-14
            rc2, so = orc.skato(G, af, X, res, v, 0)
            if rc2 == 0 and o.n_poly:
                assert abs(r["skato_p"] - so.pvalue) <= 1e-6 * so.pvalue + 5e-13
            for which, ok, p in ((0, r["cmc_ok"], r["cmc_p"]), (1, r["zeg_ok"], r["zeg_p"])):
                rc3, c = orc.burden(G, X, y, 0, which)
                if rc3 == 0:
                    assert ok and abs(p - c.pvalue) <= 1e-6 * c.pvalue + 1e-14
                    if which == 0:
                        assert r["cmc_nonref"] == c.nonref_site


def test_launch_counts_of_the_four_flagship_classes(contexts, monkeypatch):
    """M = 20 .. 80 is four classes: four launches with RVT_HC_FUSE=0, and what the plan says otherwise."""
    monkeypatch.setenv("RVT_WPARTS", "3")
    N = 5003
    keep = [i for i, M in enumerate(MS) if M <= 80]
    genes = [g for i, g in enumerate(_genes(N, -1.0)) if i in keep]
    Ms = [MS[i] for i in keep]
    null = synth.make_null(N, D, 0, seed=5)
    ref, _, tm = _run(contexts("0", PARENT), genes, null)
    assert tm.n_suffstat_hc_launches == 4
    assert _run(contexts("0", None), genes, null)[2].n_suffstat_hc_launches == 4
    assert _planned_launches(Ms, True, DEFAULT_SHAPES) == 2                     # the default: MT 2, 3, 5 in one launch, then MT 4
    for fuse, cfg, want in ((None, None, _planned_launches(Ms, True, DEFAULT_SHAPES)), ("1", "2:4x1,3:3x1,4:2x1", 1),
                            ("1", "4:2x1,2:2x3", 2), ("1", "2:2x3,4:2x2", 3), ("1", PARENT, 4)):
        got, _, tm = _run(contexts(fuse, cfg), genes, null)
        assert tm.n_suffstat_hc_launches == want, (fuse, cfg)
        assert got == ref, (fuse, cfg)


def test_a_shape_that_is_not_compiled_in_is_an_error(contexts):
    import rvtests_amd
    for cfg in ("2:7x7", "9:2x2", "3:3x1;4:2x1", "nonsense", "1:1x14", "2:3x11", "3:4x-9"):
        with pytest.raises(rvtests_amd.RvtError):
            contexts("0", cfg)
