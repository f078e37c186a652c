"""Inputs and identities of the tests of rvt_mt_score_bed_dev (tests/test_mtscore_bed_cpu.py, tests/test_gpu_mtscore_bed.py): the
traits and tests of mtscore_ref.base_input, the 37 rows of fam_bed_cases.calls(N, 30, seed=77), the split g = c + mu m and the
column moments from a row's four counts."""
import numpy as np

import fam_bed_cases
import mtscore_ref as mt

SEED = 77
ROWS = 30 + len(fam_bed_cases.HAND_ROWS)
MARGIN = 0.015                     # no cell's nm lies closer to the float sqrt(2 N) threshold of the rare-variant branch


def split(raw):
    """c (calls, missing -> 0), m (missing indicator), counts (V, 4) and mu of raw calls (N, V; negative = missing)."""
    cnt, mu, _, _ = fam_bed_cases.site_pass(raw)
    return np.where(raw < 0, 0.0, raw), (raw < 0).astype(np.float64), cnt, mu


def moments(cnt):
    """mu and sum (g - mu)^2 of the imputed column as the device forms them from the counts: exact integers, one rounding each."""
    n0, n1, n2 = (cnt[:, k].astype(np.int64) for k in range(3))
    called, a, s2 = n0 + n1 + n2, n1 + 2 * n2, n1 + 4 * n2
    den = np.maximum(called, 1).astype(np.float64)
    mu = np.where(called > 0, a.astype(np.float64) / den, 0.0)
    gg = np.where(called > 0, s2.astype(np.float64) - a.astype(np.float64) * a.astype(np.float64) / den, 0.0)
    return mu, gg


def case(N):
    """The traits of base_input(N), the 37 raw rows, their packing with every padding bit set, the imputed columns and the
    statement's U, V, p, terms and flags for them."""
    Y, Z, tests, _ = mt.base_input(N)
    raw = fam_bed_cases.calls(N, 30, seed=SEED)
    G = fam_bed_cases.imputed(raw)
    nul = mt.fit_null(Y, Z, tests)
    return dict(N=N, Y=Y, Z=Z, tests=tests, raw=raw, rows=fam_bed_cases.pack(raw), G=G, nul=nul,
                ref=mt.score(Y, Z, tests, G, want_terms=True, null=nul))


def branch_margin(c):
    """What makes the branch pattern of a case independent of rounding: (smallest relative distance of a cell's nm from the
    float sqrt(2 N) threshold, whether every exact-zero V belongs to a monomorphic row, number of ok tests)."""
    N, G = c["N"], c["G"]
    thr = float(np.float32(np.sqrt(2.0 * N)))
    dist = np.inf
    for rec in c["nul"]["tests"]:
        if rec["ok"]:
            nm = G.T @ rec["ind_model"]
            dist = min(dist, float(np.min(np.abs(nm - thr) / thr)))
    mono = G.min(0) == G.max(0)
    V = c["ref"][1]
    zero_rows = np.any(V == 0, axis=1)
    return dist, bool(np.all(mono[zero_rows])), int(c["nul"]["ok"].sum())
