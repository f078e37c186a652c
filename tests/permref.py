"""Reference for the statistics of the SKAT permutation stage (perm_stage in rvtests_amd/csrc/rvt_perm.hip), shuffle by shuffle:
Q_s = sum_j w_j (g_j . r_s)^2 in np.longdouble for the shuffles of either mode, the counters the stop rule makes of them, and
how far the device's Q_s may lie from them.  Plain numpy, the oracle (the stream, the stop rule) and the host harness (the keyed
bijection of the counter-based mode, checked in test_perm_counter_cpu.py); nothing here calls into the engine.

The bounds (u = 2^-53; derived from the inputs, not from anything the device returned)
  * C_sj = sum_i g_ij r_s,i as N products added in fp64 in ANY order, fused or not:  |dC_sj| <= gamma_N sum_i |g_ij| |r_s,i|,
    gamma_N = N u / (1 - N u).  This covers perm_dot_sequential_kernel (N <= 2048 of the exact mode) and the counter-based
    kernels: the slices' partial sums and their addition are one such summation.
  * the integer-plane product (N > 2048 of the exact mode; the contract stated in rotref.py): every operand entry is off by at
    most 2^-40 of its column's largest magnitude, and a batch of columns that are all integers <= 127 is exact.  The permuted
    residuals are never such a batch, the flipped genotypes are one when no column holds an imputed mean:
        |dC_sj| <= 2^-40 (max|r| ||g_j||_1 + [six planes] max|g_j| ||r||_1) + 2^-80 N max|r| max|g_j| + u |C_sj|.
  * either way  |dQ_s| <= sum_j w_j (2 |C_sj| dC_sj + dC_sj^2) + (2 m + 4) u Q_s  (m products, squares and additions, and the
    square root of the weight squared again).
"""
import ctypes as C

import numpy as np

import hc
import orc
import rotref

LD = np.longdouble
U = 2.0 ** -53
BLOCK = 256          # shuffles per block of the long-double products


def weights(af):
    """SKAT's weights as beta_weights (oracle/orc_models.cpp) defines them for Beta(1, 25): the squared density at the minor
    frequency, (25 (1 - f)^24)^2, and 0 at f <= 1e-30.  np.longdouble."""
    f = np.asarray(af, dtype=np.float64)
    f = np.where(f > 0.5, 1.0 - f, f).astype(LD)
    return np.where(f > 1e-30, LD(625) * (LD(1) - f) ** 48, LD(0))


def counter_indices(seed, gene_id, s, N):
    """pi_{gene, s} of the counter-based mode (perm_counter.h through the host harness): sample i takes res[pi[i]]."""
    L = hc.lib()
    L.hc_perm_indices.restype = None
    L.hc_perm_indices.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    out = np.empty(N, dtype=np.uint32)
    L.hc_perm_indices(int(seed), int(gene_id), int(s), int(N), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out.astype(np.int64)


class Stats:
    """What one gene's shuffles give: Q (n, longdouble), C (n x m, longdouble) and absC = sum_i |g_ij| |r_s,i| (n x m)."""

    def __init__(self, Q, Cm, absC):
        self.Q, self.C, self.absC = Q, Cm, absC


def _products(Gfp, w, res, order):
    """Stats of the shuffles order (n x N: sample i of shuffle s takes res[order[s, i]]).  A zero genotype adds exactly zero to
    the sum and to its bound, so every column is summed over its non-zero samples only — rare variants make that cheap."""
    N, m = Gfp.shape
    n = order.shape[0]
    res_ld = np.asarray(res, dtype=np.float64).astype(LD)
    nz = [np.flatnonzero(Gfp[:, j]) for j in range(m)]
    g = [Gfp[nz[j], j].astype(LD) for j in range(m)]
    Cm = np.zeros((n, m), dtype=LD)
    absC = np.zeros((n, m), dtype=LD)
    for b0 in range(0, n, BLOCK):
        R = res_ld[order[b0:b0 + BLOCK]]                   # (block x N) permuted residuals
        for j in range(m):
            Rj = R[:, nz[j]]
            Cm[b0:b0 + BLOCK, j] = Rj @ g[j]
            absC[b0:b0 + BLOCK, j] = np.abs(Rj) @ np.abs(g[j])
    Q = (Cm * Cm) @ np.asarray(w, dtype=LD)
    return Stats(Q, Cm, absC)


def counter_Q(Gfp, w, res, seed, gene_id, s0, n):
    """Stats of the shuffles s0 .. s0 + n - 1 of the counter-based mode for the gene keyed gene_id.  Gfp: the flipped,
    polymorphic block (orc.flip_poly), w: its m weights."""
    N = Gfp.shape[0]
    order = np.empty((n, N), dtype=np.int64)
    for k in range(n):
        order[k] = counter_indices(seed, gene_id, s0 + k, N)
    return _products(Gfp, w, res, order)


def exact_Q(G, af, res, obs, n_perm, alpha, cap):
    """The cumulative Fisher-Yates shuffles of the reference's stream (it continues the oracle's, as orc.skat_permute does, and
    leaves it where that would): (PermResult of the oracle's own loop, Stats of the first min(actual_perm, cap) shuffles it
    added).  G, af: the gene as the engine gets it."""
    rc, p, stats, order = orc.skat_permute_trace(G, af, res, obs, n_perm, alpha, cap)
    assert rc == 0
    Gfp = orc.flip_poly(G)[0]
    w = weights(af)[:Gfp.shape[1]]
    st = _products(Gfp, w, res, order.astype(np.int64))
    # the oracle's own statistics of the same shuffles are fp64 sums in sample order: they lie inside the "sum" bound (twice
    # the last term: its weights are the oracle's own density, rounded)
    assert np.all(np.abs(st.Q - stats.astype(LD)) <= bound_dQ("sum", Gfp, w, res, st) + LD((2 * Gfp.shape[1] + 4) * U) * st.Q)
    return p, st


def expected_counters(n_perm, alpha, obs, Q):
    """(actual_perm, num_greater, num_equal, pvalue) of Permutation's stop rule (orc_perm_stop_run) fed with Q in order."""
    return orc.perm_stop_run(n_perm, alpha, obs, np.asarray(Q, dtype=np.float64))


def planes_of(Gfp):
    """Digit planes of the genotype operand of the exact mode's integer-plane product (rotref.quantize_g's decision)."""
    return rotref.quantize_g(Gfp)[2]


def bound_dC(route, Gfp, res, st):
    """|dC_sj| (n x m, longdouble) on `route`: "sum" (any fp64 summation of the N products) or "planes"."""
    N = Gfp.shape[0]
    if route == "sum":
        return LD(N * U / (1.0 - N * U)) * st.absC
    assert route == "planes"
    six = planes_of(Gfp) != 1
    max_r, sum_r = np.abs(res).max(), np.abs(res).sum()
    max_g, sum_g = np.abs(Gfp).max(axis=0), np.abs(Gfp).sum(axis=0)
    per_col = 2.0 ** -40 * (max_r * sum_g + (max_g * sum_r if six else 0.0)) + 2.0 ** -80 * N * max_r * max_g
    return per_col.astype(LD)[None, :] + LD(U) * np.abs(st.C)


def bound_dQ(route, Gfp, w, res, st):
    """|dQ_s| (n, longdouble) that follows from bound_dC."""
    dC = bound_dC(route, Gfp, res, st)
    m = Gfp.shape[1]
    return (2 * np.abs(st.C) * dC + dC * dC) @ np.asarray(w, dtype=LD) + LD((2 * m + 4) * U) * st.Q


def exact_route(N):
    """Which product the exact mode takes (perm_stage: sample-order sums up to 2048 samples, the integer planes beyond)."""
    return "sum" if N <= 2048 else "planes"
