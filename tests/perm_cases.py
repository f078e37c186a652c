"""The cases of the shuffle-by-shuffle tests of the SKAT permutation stage (tests/test_perm_ref_cpu.py proves their premises from
the reference alone, tests/test_gpu_perm.py runs them on the device): for every case N, the genes, the seed, nPerm, alpha and
the gene ids, and — computed once per process and shared — the reference's statistics, counters and bounds (tests/permref.py).

Three families
  SWITCH   exact mode on both sides of the 2048 | 2049 switch between the sample-order sums and the integer-plane product, and
           N = 4100: five genes on one stream, 300 shuffles, alpha = 0.05; one gene is causal.
  CHUNKS   exact mode across the 2048-shuffle chunks: three runs on one stream, (5000, 0.5) never stops, (5000, 0.125) stops
           inside the second chunk, (200, 0.05) proves where the stream stood afterwards.
  COUNTER  counter-based mode, sizes N x m around the kernel's 16-sample groups, sample slices and 64-variant passes; two runs
           per gene, 100 shuffles and 2300 (chunks of 2048 + 252), and one gene at alpha = 0.05 whose short first chunk (250
           shuffles) is followed by a second one in which it stops.

The tie condition: counters are compared exactly, so no reference statistic of any case may lie within TIE * obs of the observed
statistic, and TIE * obs must exceed the case's a-priori bound on |Q_device - Q_reference| plus the 1e-10 * obs the tests allow
between the device's observed statistic and the oracle's.
"""
import numpy as np

import orc
import permref
import synth

TIE = 1e-8          # relative distance every reference statistic keeps from the observed one
OBS_TOL = 1e-10     # |device skat_Q - oracle Q| / Q the GPU tests allow
COUNTER_SEED = 7


def _gene(N, M, seed, **kw):
    """synth.make_gene's gene with the LAST sample made a heterozygous carrier of every polymorphic column: a product that
    drops the last sample, its group of 16 or its K chunk (N = 2049: one row and 127 of padding) is then wrong in every
    column — rare variants alone leave the last few samples without a single carrier."""
    Graw = synth.make_gene(N, M, seed=seed, **kw)[0]
    kept = orc.flip_poly(orc.impute_mean(Graw))[2]
    Graw[N - 1, kept == 1] = 1.0
    return np.asfortranarray(orc.impute_mean(Graw)), orc.counter_af(Graw)


# ---- SWITCH ---------------------------------------------------------------------------------------------------------------
SWITCH_N = (2048, 2049, 4100)
SWITCH_NPERM, SWITCH_ALPHA, SWITCH_SEED = 300, 0.05, 1
SWITCH_TRACED = 2          # the M = 21 gene
SWITCH_CAUSAL = 1          # the hard-call gene carries the effect


def switch_genes(N):
    """M = 1 | M = 8 hard calls (one digit plane) | M = 21 with imputed means (six planes) | no polymorphic column (no draws) |
    M = 70 hard calls with a flipped column, a monomorphic one and one monomorphic after the flip."""
    return [_gene(N, 1, 3100, maf_lo=-1.5, maf_hi=-1.0),
            _gene(N, 8, 3108, maf_lo=-2.0, maf_hi=-1.0),
            _gene(N, 21, 3121, missing=0.01),
            (np.zeros((N, 3), order="F"), np.zeros(3)),
            _gene(N, 70, 3170, common=True, mono=True)]


def switch_null(N, genes):
    return synth.make_null(N, 2, 0, seed=41, G_effect=0.6 * genes[SWITCH_CAUSAL][0].sum(1))


# ---- CHUNKS ---------------------------------------------------------------------------------------------------------------
CHUNKS_N = (331, 2049)
CHUNKS_RUNS = ((5000, 0.5), (5000, 0.125), (200, 0.05))      # (nPerm, alpha) of the three genes, in stream order
CHUNKS_SEED = 1
CHUNKS_GENE_SEED = {331: (5201, 5212, 5203), 2049: (5301, 5306, 5303)}


def chunks_genes(N):
    s = CHUNKS_GENE_SEED[N]
    return [_gene(N, 8, s[0], missing=0.01, maf_lo=-2.0), _gene(N, 6, s[1], maf_lo=-2.0), _gene(N, 12, s[2], missing=0.01, maf_lo=-2.0)]


def chunks_null(N):
    return synth.make_null(N, 2, 0, seed=43)


# ---- COUNTER --------------------------------------------------------------------------------------------------------------
# every N meets m = 65 (the pass switch), every m meets N = 2003 (N % 16 = 3); N = 4099: more than one sample slice
COUNTER_SIZES = ((2003, 5), (2003, 16), (2003, 40), (2003, 64), (2003, 65), (2003, 130), (2000, 65), (4099, 65), (4099, 130))
COUNTER_RUNS = ((100, 0.5), (2300, 0.5))        # nothing stops: 100 = one chunk, 36 live rows in its last 64-shuffle block;
                                                # 2300 = 2048 + 252, the second chunk starts at shuffle 2048
COUNTER_STOP = dict(N=2003, m=16, gene_seed=6408, n_perm=1000, alpha=0.05, gene_id=90210)


def counter_gene(N, m, gene_seed=None):
    """m polymorphic hard-call columns (frequencies from 10^-2.5: dozens of carriers at these N); N = 2003, m = 40 with imputed means."""
    return _gene(N, m, 6000 + N + m if gene_seed is None else gene_seed, maf_lo=-2.5, missing=0.01 if (N, m) == (2003, 40) else 0.0)


def counter_gene_id(N, m, run):
    return 100000 * (run + 1) + 31 * N + m          # nothing like a position in a batch


def counter_null(N):
    return synth.make_null(N, 2, 0, seed=47)


# ---- the reference, once per process -------------------------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class GeneRef:
    """One gene's reference: obs (the oracle's observed Q; None without a polymorphic column), the oracle's counters `perm`,
    the statistics `st` (permref.Stats of the shuffles added, or of all nPerm in the counter-based mode), their bound dQ, and
    the smallest |Q_s - obs| / obs."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _finish(route, G, af, res, obs, st, **kw):
    Gfp = orc.flip_poly(G)[0]
    w = permref.weights(af)[:Gfp.shape[1]]
    dQ = permref.bound_dQ(route, Gfp, w, res, st)
    tie = float(np.min(np.abs(st.Q - obs)) / obs) if st.Q.size else np.inf
    return GeneRef(obs=obs, st=st, dQ=dQ, tie=tie, route=route, m=Gfp.shape[1], **kw)


def _exact_stream(N, genes, null, runs, seed):
    """The genes in order on the oracle's stream from srand(seed); runs: (nPerm, alpha) per gene."""
    X, y, res, v, s2 = null
    orc.rand_seed(seed)
    out = []
    for (G, af), (n_perm, alpha) in zip(genes, runs):
        rc, a = orc.skat(G, af, X, res, v, 0)
        if a.n_poly == 0:
            out.append(GeneRef(obs=None))
            continue
        perm, st = permref.exact_Q(G, af, res, a.Q, n_perm, alpha, n_perm)
        out.append(_finish(permref.exact_route(N), G, af, res, a.Q, st, perm=perm, n_perm=n_perm, alpha=alpha))
    return out


def switch_case(N):
    def make():
        genes = switch_genes(N)
        null = switch_null(N, genes)
        return genes, null, _exact_stream(N, genes, null, [(SWITCH_NPERM, SWITCH_ALPHA)] * len(genes), SWITCH_SEED)
    return _once(("switch", N), make)


def chunks_case(N):
    def make():
        genes = chunks_genes(N)
        null = chunks_null(N)
        return genes, null, _exact_stream(N, genes, null, CHUNKS_RUNS, CHUNKS_SEED)
    return _once(("chunks", N), make)


def _counter_ref(G, af, null, n_perm, alpha, gene_id):
    X, y, res, v, s2 = null
    rc, a = orc.skat(G, af, X, res, v, 0)
    Gfp = orc.flip_poly(G)[0]
    st = permref.counter_Q(Gfp, permref.weights(af)[:Gfp.shape[1]], res, COUNTER_SEED, gene_id, 0, n_perm)
    return _finish("sum", G, af, res, a.Q, st, n_perm=n_perm, alpha=alpha, gene_id=gene_id,
                   counters=permref.expected_counters(n_perm, alpha, a.Q, st.Q))


def counter_case(N, m):
    def make():
        G, af = counter_gene(N, m)
        null = counter_null(N)
        return (G, af), null, [_counter_ref(G, af, null, n_perm, alpha, counter_gene_id(N, m, k))
                               for k, (n_perm, alpha) in enumerate(COUNTER_RUNS)]
    return _once(("counter", N, m), make)


def counter_stop_case():
    def make():
        c = COUNTER_STOP
        G, af = counter_gene(c["N"], c["m"], c["gene_seed"])
        null = counter_null(c["N"])
        return (G, af), null, _counter_ref(G, af, null, c["n_perm"], c["alpha"], c["gene_id"])
    return _once(("counter_stop",), make)


def margin_ok(ref):
    """The tie condition of one gene: every statistic keeps TIE * obs from obs, and that exceeds bound + OBS_TOL * obs."""
    return ref.tie >= TIE and float(np.max(ref.dQ)) + OBS_TOL * ref.obs < TIE * ref.obs
