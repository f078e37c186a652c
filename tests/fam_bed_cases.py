"""Inputs of the tests of the family single-variant calls over resident .bed rows (rvt_score_bed_dev_fam, rvt_lrt_bed_dev_fam;
tests/test_fam_bed_cpu.py and tests/test_gpu_fam_bed.py): the matrix of calls with every row kind the front stage has to get
right, its packing with hostile padding bits, and the identities the device code is built on, in numpy."""
import numpy as np

import orc
import synth

HAND_ROWS = ("all 0", "all 2", "all heterozygous", "all missing", "one called sample only",
             "missing calls in the last byte only", "no missing call")


def hand_rows(N, seed):
    """(N, 7) hard calls, -9 = missing: the row kinds of HAND_ROWS, in that order."""
    rng = np.random.default_rng(seed)
    R = np.zeros((N, len(HAND_ROWS)))
    R[:, 1] = 2.0
    R[:, 2] = 1.0
    R[:, 3] = -9.0
    R[:, 4] = -9.0
    R[int(rng.integers(0, N)), 4] = 1.0
    R[:, 5] = rng.binomial(2, 0.3, N)
    R[4 * ((N + 3) // 4 - 1):, 5] = -9.0               # the samples of the last byte, and nobody else
    R[:, 6] = rng.binomial(2, 0.2, N)
    R[:2, 6] = (0.0, 1.0)                              # (polymorphic whatever the draw)
    return R


def calls(N, V, seed, maf_hi=-0.8):
    """(N, V + 7) raw calls: synth.make_gene's with 2 % missing, a flipped, a monomorphic and a monomorphic-after-the-flip column,
    and the hand-made rows behind them."""
    raw = synth.make_gene(N, V, seed=seed, missing=0.02, common=True, mono=True, maf_hi=maf_hi)[0]
    return np.asfortranarray(np.column_stack([raw, hand_rows(N, seed + 1)]))


def pack(raw):
    """Engine.pack_bed's rows with every padding bit of a row's last byte set."""
    from rvtests_amd import Engine
    rows = Engine.pack_bed(raw).copy()
    pad = (-raw.shape[0]) % 4
    if pad:
        rows[:, -1] |= np.uint8((0xFF << (2 * (4 - pad))) & 0xFF)
    return rows


def imputed(raw):
    """The fp64 columns a caller uploads: missing calls at the mean of the called ones (DataConsolidator)."""
    return orc.impute_mean(np.asfortranarray(raw, dtype=np.float64))


def site_pass(raw):
    """The front stage's site pass restated: (counts (V, 4) = n0 n1 n2 missing, mu, column sum, polymorphic flag)."""
    cnt = np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1).astype(np.int64)
    n0, n1, n2, nm = (cnt[:, k] for k in range(4))
    called, ac = n0 + n1 + n2, n1 + 2 * n2
    mu = np.where(called > 0, ac / np.maximum(called, 1), 0.0)
    poly = ((n0 > 0).astype(int) + (n1 > 0) + (n2 > 0)) >= 2
    return cnt, mu, ac + nm * mu, poly


def fill_fixed_point(cnt, mu):
    """mu as the six digit planes of its imputed column hold it (rotref.quantize_g: 2^-s, s = 39 - ilogb(the column's largest
    entry), and that entry is the row's largest call): what the dense rotation multiplies U'm with."""
    s = np.where(cnt[:, 2] > 0, 38, 39)
    return np.ldexp(np.rint(np.ldexp(mu, s)), -s)
