"""Inputs of the tests of MetaCov's band from rows of a resident .bed matrix (rvt_cov_band_bed_dev): raw calls with hand-made
rows, their packed rows with garbage in the padding pairs, the columns a caller would have uploaded, and the numpy
restatements of the per-row numbers and of the byte -> nibble mapping (csrc/rvt_bed_nibbles.h)."""
import numpy as np

import fam_bed_cases
import orc
import synth

# the hand-made rows behind the drawn ones, in this order
SPECIAL = ("all_missing", "all_het", "one_value_and_missing", "single_carrier", "no_missing")


def calls(N, V, seed, missing=0.02):
    """(N, V) raw calls, -9 = missing: V - 5 drawn rows (a flipped and two monomorphic ones among them, synth.make_gene) with
    `missing` of their calls missing, then the SPECIAL rows."""
    n = V - len(SPECIAL)
    raw = synth.make_gene(N, n, seed=seed, missing=missing, common=True, mono=True, maf_lo=-2.0, maf_hi=-0.7)[0]
    rng = np.random.default_rng(seed + 1)
    S = np.zeros((N, len(SPECIAL)))
    S[:, 0] = -9.0
    S[:, 1] = 1.0
    S[:, 2] = 2.0
    S[rng.random(N) < 0.1, 2] = -9.0
    S[-1, 2] = -9.0                                     # (a missing call in the row's last byte)
    S[int(rng.integers(0, N)), 3] = 1.0
    S[:, 4] = rng.binomial(2, 0.25, N)
    S[:2, 4] = (0.0, 1.0)
    return np.asfortranarray(np.column_stack([raw, S]))


def without_missing(raw):
    """the same rows with every missing call a call of 0"""
    return np.asfortranarray(np.where(raw < 0, 0.0, raw))


def pack(raw):
    """the rows as the file holds them, the padding pairs of every row's last byte set (0b11: garbage that reads as a call of 2)"""
    return fam_bed_cases.pack(raw)


def counts(raw):
    """(V, 4): calls of 0 / 1 / 2 / missing per row"""
    return np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1).astype(np.int64)


def imputed(raw):
    """The fp64 columns: missing calls at mu = (n1 + 2 n2) / (n0 + n1 + n2), one division of integers; a row without a called
    sample is the zero column."""
    cnt = counts(raw)
    called, ac = cnt[:, 0] + cnt[:, 1] + cnt[:, 2], cnt[:, 1] + 2 * cnt[:, 2]
    mu = np.where(called > 0, ac.astype(np.float64) / np.maximum(called, 1).astype(np.float64), 0.0)
    G = np.array(raw, dtype=np.float64, order="F")
    for j in range(G.shape[1]):
        G[G[:, j] < 0, j] = mu[j]
    return G


def polymorphic(G):
    """1 where the imputed column has two distinct values"""
    return np.array([1 if G[:, j].min() != G[:, j].max() else 0 for j in range(G.shape[1])], dtype=np.int32)


def null_model(N, d, binary, seed):
    """(X, y, res, v, sigma2) as Engine.set_null takes them, fitted by the oracle"""
    X, y = synth.make_null(N, d, binary, seed=seed)[:2]
    if binary:
        rc, beta, p, v = orc.fit_logistic(X, y)
        assert rc == 0
        return X, y, y - p, v, 1.0
    rc, beta, pred, res, s2 = orc.fit_linear(X, y)
    assert rc == 0
    return X, y, res, np.full(N, s2), s2


def nibble_table(live):
    """All 256 .bed bytes of which the first `live` samples exist -> (h nibbles (256,), m nibbles (256,), counts (256, 4) =
    calls of 0 / 1 / 2 / missing): sample e in bits 4 e; h = value << 1 (missing -> 0), m = 0x2 where the call is missing."""
    e = np.arange(4)
    q = (np.arange(256)[:, None] >> (2 * e)) & 3                  # 00 -> 0, 10 -> 1, 11 -> 2, 01 -> missing
    alive = (e < live)[None, :]
    value = np.array([0, 0, 1, 2])[q]
    miss = (q == 1) & alive
    called = (q != 1) & alive
    h = (((value << 1) * called) << (4 * e)).sum(1)
    m = ((2 * miss) << (4 * e)).sum(1)
    cnt = np.stack([(called & (value == 0)).sum(1), (called & (value == 1)).sum(1), (called & (value == 2)).sum(1), miss.sum(1)], axis=1)
    return h.astype(np.uint32), m.astype(np.uint32), cnt.astype(np.uint32)
