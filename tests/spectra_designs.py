"""Seeded genes whose spectra are the hard ones for the per-gene tail (tridiagonalisation, bisection, eigenvalue filter,
Davies), and a plain numpy statement of the SKAT matrix whose eigenvalues the tail computes.

Every generator returns (G, af): G is N x M, imputed and UNFLIPPED as the engine takes it, af the M allele frequencies handed
to the tests.  G is integer-valued (no missing calls) except in `near`, so G'G is exact in any summation order and a
difference between two builds is a difference of the tail, not of the Gram.

  dup         a synth.make_gene gene in which every third column copies its left neighbour: exactly repeated columns, so
              exactly zero eigenvalues (variants in perfect LD)
  singletons  M variants on M disjoint carriers: a tight cluster of nearly equal eigenvalues
  rng         singletons plus one MAF-0.4 column: a spectrum over eight decades (the `range` design)
  near        the eps-collinear family of test_models_cpu.py: the last column is the first plus eps * noise on its carriers
  fewpoly     M = 300 columns of which a handful are polymorphic; af is random and non-zero everywhere (see below)
  crowded     more columns than samples (N = 40): at most N - d non-zero eigenvalues whatever M
  wide        plain genes of independent binomial columns, every column polymorphic

fewpoly and the weights: a kept column takes its weight from the frequency at its COMPACTED index, and
a frequency <= 1e-30 gives weight 0.  With frequencies counted from a mostly monomorphic G the kept columns would read the
zeros of the monomorphic ones in front and drop out (Q = 0); the caller-supplied af avoids that."""
import math

import numpy as np

import synth


def _all_polymorphic(G):
    """A column that came out all-zero gets one carrier (row = its index), so that every column is kept."""
    N, M = G.shape
    for j in np.flatnonzero(G.min(0) == G.max(0)):
        G[:, j] = 0.0
        G[j % N, j] = 1.0
    return G


def wide(N, M, seed, maf_lo=-2.3, maf_hi=-1.0):
    Graw, G, af = synth.make_gene(N, M, seed, maf_lo=maf_lo, maf_hi=maf_hi)
    G = _all_polymorphic(np.array(G, order="F"))
    return G, G.sum(0) / (2.0 * N)


def crowded(N, M, seed, free=5):
    """More columns than samples: common variants (MAF 0.05 .. 0.3) on N - free samples; the first `free` samples carry
    nothing, so the collapsed burden vectors are not constant."""
    r = np.random.default_rng(seed)
    G = np.asfortranarray(r.binomial(2, 10 ** r.uniform(-1.3, -0.5, M), size=(N, M)).astype(np.float64))
    G[:free] = 0.0
    for j in np.flatnonzero(G.min(0) == G.max(0)):
        G[:, j] = 0.0
        G[free + j % (N - free), j] = 1.0
    return G, G.sum(0) / (2.0 * N)


def dup(N, M, seed):
    G, af = wide(N, M, seed)
    for j in range(2, M, 3):
        G[:, j] = G[:, j - 1]
        af[j] = af[j - 1]
    return G, af


def singletons(N, M, seed):
    assert M <= N
    rng = np.random.default_rng(seed)
    G = np.zeros((N, M), order="F")
    G[rng.permutation(N)[:M], np.arange(M)] = 1.0
    return G, G.sum(0) / (2.0 * N)


def rng(N, M, seed):
    """singletons, with column M // 2 replaced by a MAF-0.4 variant"""
    G, af = singletons(N, M, seed)
    g = np.random.default_rng(seed + 1).binomial(2, 0.4, size=N).astype(np.float64)
    G[:, M // 2] = g
    af[M // 2] = g.sum() / (2.0 * N)
    return G, af


NEAR_EPS = (0.0, 1e-9, 3e-5, 2e-3, 0.3)


def near(eps, N=400, M=7):
    """Exactly the gene of test_skato_rho_moments_with_nearly_collinear_columns."""
    r = np.random.default_rng(77)
    Graw, G, af = synth.make_gene(N, M, 5, missing=0.0, common=True, mono=False, maf_hi=-0.8)
    G = np.array(G, order="F")
    G[:, M - 1] = G[:, 0] + eps * r.normal(size=N) * (G[:, 0] > 0)
    af = af.copy()
    af[M - 1] = af[0]
    return G, af


FEWPOLY_COLS = ((0, 150, 299), (15, 16, 17, 160, 161, 298))


def fewpoly(cols, N, seed, M=300):
    r = np.random.default_rng(seed)
    G = np.zeros((N, M), order="F")
    for j in cols:
        g = r.binomial(2, 0.03, size=N).astype(np.float64)
        g[j % N] = 1.0
        G[:, j] = g
    return G, r.uniform(1e-3, 0.05, M)


def _beta_pdf(x, a, b):
    return math.exp((a - 1.0) * math.log(x) + (b - 1.0) * math.log1p(-x) + math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b))


def skat_matrix(G, af, X, v, binary, sigma2, b1=1.0, b2=25.0):
    """K = W G'P0 G W of Skat.cpp on the flipped, polymorphic columns, W = diag(beta_pdf(maf; b1, b2)) with the weight of kept
    column a read at af[a], P0 = V - V X (X'VX)^-1 X'V.  Quantitative trait: V = sigma2 I, so K = sigma2 W G'(I - H) G W;
    binary trait: V = diag(v).  Formed as B'B from the projected, scaled columns B, so it is symmetric positive
    semi-definite by construction."""
    G = np.asarray(G, dtype=np.float64)
    N = G.shape[0]
    flip = G.sum(0) > N
    Gf = np.where(flip[None, :], 2.0 - G, G)
    Gf = Gf[:, Gf.min(0) != Gf.max(0)]
    m = Gf.shape[1]
    w = np.zeros(m)
    for a in range(m):
        f = af[a] if af[a] <= 0.5 else 1.0 - af[a]
        w[a] = _beta_pdf(f, b1, b2) if f > 1e-30 else 0.0
    sv = np.sqrt(np.asarray(v, dtype=np.float64)) if binary else np.full(N, math.sqrt(sigma2))
    Qx, _ = np.linalg.qr(X * (sv[:, None] if binary else 1.0))
    A = Gf * sv[:, None]
    A = A - Qx @ (Qx.T @ A)
    A = A - Qx @ (Qx.T @ A)          # (a second pass: the projection to rounding)
    B = A * w[None, :]
    return B.T @ B


def lapack_spectrum(K):
    """eigvalsh(K) descending, and the numerical rank: how many lie above 1e-12 of the largest."""
    ev = np.linalg.eigvalsh(K)[::-1]
    return ev, int((ev > 1e-12 * ev[0]).sum())


# ---- the genes the CPU and the GPU file share, and their null models ----------------------------------------------------------
# (design, M, binary); N = 600 up to M = 48 and 1500 above, d = 2.  The sizes sit on the launch switches of the device tail:
# the dense reduction works in LDS up to M = 125 and in global scratch from 126, the all-in-one spectrum kernel takes genes
# up to Mp = 192 (M = 192) and the per-problem kernel those from M = 193.
EIGEN_CASES = [(design, M, 0) for design in ("dup", "singletons", "rng") for M in (12, 48, 125, 126, 193)] + \
              [("dup", 48, 1), ("singletons", 48, 1)]
RANK_DEFICIENT = ("dup",)


def case_id(c):
    return "%s-M%d-%s" % (c[0], c[1], "binary" if c[2] else "quant")


def make_case(design, M, binary, N=None, d=2, effect=0.3, **kw):
    """The gene of a case and its null model: dict(G, af, X, y, res, v, s2, binary, d, N, M)."""
    import synth
    if N is None:
        N = 600 if M <= 48 else 1500
    seed = 10 + M
    G, af = globals()[design](N, M, seed, **kw)
    # (singletons / rng: a null model of its own seed — with the gene's seed SKAT-O's p-value comes out as exactly 1 at M = 48)
    nseed = seed + (1000 if design in ("singletons", "rng") else 0)
    X, y, res, v, s2 = synth.make_null(N, d, binary, nseed, G_effect=effect * G[:, :3].sum(1))
    return dict(G=G, af=af, X=X, y=y, res=res, v=v, s2=s2, binary=binary, d=d, N=N, M=M)


def make_near_case(eps):
    import synth
    G, af = near(eps)
    X, y, res, v, s2 = synth.make_null(400, 2, 0, 5, G_effect=0.4 * G[:, :3].sum(1))
    return dict(G=G, af=af, X=X, y=y, res=res, v=v, s2=s2, binary=0, d=2, N=400, M=G.shape[1])


def make_fewpoly_case(cols):
    import synth
    N = 800
    G, af = fewpoly(cols, N, 7)
    X, y, res, v, s2 = synth.make_null(N, 2, 0, 7, G_effect=0.3 * G[:, :3].sum(1))
    return dict(G=G, af=af, X=X, y=y, res=res, v=v, s2=s2, binary=0, d=2, N=N, M=G.shape[1])


def make_more_columns_than_samples_case(M, binary):
    return make_case("crowded", M, binary, N=40)


def make_plain_case(M, N=1500):
    """A plain gene under a quantitative trait, rare enough (MAF 5e-4 .. 5e-3) that some samples carry no variant even at
    M = 1024: a collapsed CMC vector of all ones is collinear with the intercept and its score test is decided by rounding."""
    return make_case("wide", M, 0, N=N, maf_lo=-3.3, maf_hi=-2.3)


def wide512_oracle(c):
    """(Q, p) of the oracle's SKAT on c = make_plain_case(512, N=1200), recorded by tests/golden/make_spectra_golden.py (the
    oracle's dense eigensolver needs ten seconds there)."""
    import hashlib
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectra_wide512.json")))
    assert hashlib.sha256(np.ascontiguousarray(c["G"].T, dtype=np.float64).tobytes()).hexdigest() == g["G_sha256"], \
        "the seeded generator no longer gives the gene the fixture was recorded for"
    assert abs(float(c["res"] @ c["res"]) - float(g["rss"])) <= 1e-12 * float(g["rss"])
    return float(g["skat_Q"]), float(g["skat_p"])


# ---- the assertions the host build and the device share ------------------------------------------------------------------------
def host_gene(c, stats=None):
    """The device algorithms on the host (hc.gene), fed with numpy's statistics — or with `stats`, hc.gene's (R, colstat) —
    and the collapsers' burden sums."""
    import hc
    G = c["G"]
    cnt = ((np.where(G.sum(0) > c["N"], 2.0 - G, G)).astype(np.int64) > 0).sum(1).astype(np.float64)
    bs = hc.burden_sums((cnt > 0).astype(np.float64), cnt, c["X"], c["res"], c["v"], c["binary"])
    out, flip, kept, lam = hc.gene(G, c["af"], c["X"], c["res"], c["v"], c["binary"], c["s2"], bstats=bs, stats=stats)
    return out, lam[:out.skat_nlambda].copy()


def check_eigenvalues(lam, c):
    """lam: the kept SKAT eigenvalues.  Against LAPACK on the numpy statement of K: descending; those above 1e-12 lmax are as
    many as LAPACK's numerical rank and each within 1e-11 lmax of LAPACK's (the project's bar for the Gram, as
    test_suffstat_matches_numpy); every other kept value is rounding, below 1e-12 lmax in magnitude.  Returns the worst
    difference in units of lmax."""
    ev, rank = lapack_spectrum(skat_matrix(c["G"], c["af"], c["X"], c["v"], c["binary"], c["s2"]))
    lmax = ev[0]
    lam = np.asarray(lam, dtype=np.float64)
    assert lam.size >= rank, (lam.size, rank)
    assert np.all(np.diff(lam) <= 0.0), "kept eigenvalues are not descending"
    n_big = int((lam > 1e-12 * lmax).sum())
    assert n_big == rank, (n_big, rank)
    worst = float(np.max(np.abs(lam[:rank] - ev[:rank])) / lmax)
    assert worst <= 1e-11, worst
    assert np.all(np.abs(lam[rank:]) < 1e-12 * lmax), lam[rank:] / lmax
    return worst


def own_inputs_skat_p(lam, Q):
    """The SKAT p-value the host build gives for THESE eigenvalues and THIS Q: Davies in product form, Liu's where Davies
    faults or returns 0 or 1 (rvt_pvalue.h; a fault comes back as -1)."""
    import hc
    p, fault, nt = hc.davies(lam, Q, fast=True)
    if p <= 0.0 or p == 1.0:
        p = hc.liu(lam, Q)
    return p


# the GeneStats slots of hc.gene's dbg / rvt_debug_spectrum's stats, and the bound on |device - host| / |host| for each:
# ten times the worst disagreement of the HOST build with the oracle's own Qs / taus / muQ / varQ / varZeta / df over
# EIGEN_CASES (tests/test_spectra_cpu.py prints them; measured, rounded up: 2.7e-14, 2.3e-15, 9.8e-14, 2.0e-13, 3.3e-10,
# 4.2e-15 — varZeta is a sum that cancels to 1e-6 of its terms on the singleton designs).  The oracle reports no moments of
# the rho problems: mom_mu / mom_var / mom_df are sums over eigenvalues like muQ / varQ / df and take their bounds.
RHO_FIELDS = (("Qs", slice(0, 11), 2.7e-13), ("mom_mu", slice(11, 22), 9.8e-13), ("mom_var", slice(22, 33), 2.0e-12),
              ("mom_df", slice(33, 44), 4.2e-14), ("tau", slice(44, 55), 2.3e-14), ("muQ", slice(55, 56), 9.8e-13),
              ("varQ", slice(56, 57), 2.0e-12), ("varZeta", slice(57, 58), 3.3e-9), ("df", slice(58, 59), 4.2e-14))
ORACLE_NAMES = {"Qs": "Qs", "tau": "taus", "muQ": "muQ", "varQ": "varQ", "varZeta": "varZeta", "df": "df"}


def rel_diff(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def check_rho_fields(stats, host_stats):
    """Returns {field: worst relative difference}; asserts each within its bound of RHO_FIELDS."""
    seen = {}
    for name, sl, bound in RHO_FIELDS:
        seen[name] = rel_diff(stats[sl], host_stats[sl])
        assert seen[name] <= bound, (name, seen[name], bound)
    return seen


def check_rank_deficient_record(r, c, a, rc2, o):
    """A record of a rank-deficient gene against the oracle's orc.skat (a) and orc.skato (rc2, o).  The survivors of the
    reference's 1e-30 filter sit at 1e-17 lmax and their number depends on rounding, so two correct evaluations of Davies at
    acc = 1e-6 may differ by 2e-6 absolute in the SKAT p-value (Q puts p into [0.01, 0.9]); everything else as _check_gene of
    test_gpu_parity.py."""
    assert r.n_poly == a.n_poly and r.skat_ok == 1
    assert abs(r.skat_Q - a.Q) <= 1e-10 * abs(a.Q)
    assert 0.01 <= a.pvalue <= 0.9, a.pvalue
    assert abs(r.skat_p - a.pvalue) <= 2e-6, (r.skat_p, a.pvalue)
    assert rc2 == 0 and r.skato_ok == 1
    assert abs(r.skato_Q - o.Q) <= 1e-10 * abs(o.Q)
    assert r.skato_rho == o.rho
    assert abs(r.skato_p - o.pvalue) <= 1e-6 * abs(o.pvalue) + 5e-13, (r.skato_p, o.pvalue)
