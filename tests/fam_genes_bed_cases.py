"""Inputs of the tests of the gene-based family tests over resident .bed rows (rvt_run_fam_tests_bed_dev;
tests/test_fam_genes_bed_cpu.py and tests/test_gpu_fam_genes_bed.py): one matrix of calls holding every gene of the set, the
hand-made rows the flip / keep / collapse rules have to get right, and those rules restated in numpy."""
import functools

import numpy as np

import fam_bed_cases
import synth

HAND_ROWS = ("a == called with missing calls: mu == 1.0 exactly", "a == called + 1 with missing calls: flipped",
             "monomorphic only after dropping the missing calls", "flipped, missing calls in the last byte only")


def hand_rows(N, seed):
    """(N, 4) hard calls, -9 = missing: the row kinds of HAND_ROWS, in that order (N >= 40)."""
    rng = np.random.default_rng(seed)
    R = np.ones((N, len(HAND_ROWS)))
    p = rng.permutation(N)
    k = (N - 12) // 2                                                      # (most samples 0 or 2: the collapsed columns vary)
    R[p[:k], 0], R[p[k:2 * k], 0], R[p[2 * k:2 * k + 5], 0] = 0.0, 2.0, -9.0      # n0 = n2: a = n1 + 2 n2 = called
    p = rng.permutation(N)
    R[p[:k - 1], 1], R[p[k - 1:2 * k - 1], 1], R[p[2 * k - 1:2 * k + 5], 1] = 0.0, 2.0, -9.0   # n2 = n0 + 1: a = called + 1
    R[:, 2] = 2.0
    R[p[:9], 2] = -9.0                                                     # two codes in the row, one value in the column
    R[:, 3] = 2.0 - rng.binomial(2, 0.2, N)
    R[:3, 3] = (2.0, 1.0, 0.0)
    R[4 * ((N + 3) // 4 - 1):, 3] = -9.0                                   # the samples of the last byte, and nobody else
    return R


@functools.lru_cache(maxsize=None)
def gene_set(N, seed):
    """(raw, genes): raw (N, V) calls of one matrix, genes = [(name, first row, M)] in ascending row order.  The genes of
    test_gpu_fam.py::dense_genes from raw calls (M = 1, 17, 64 with 2 % missing, a flipped column; M = 64 with monomorphic rows
    inside), an all-monomorphic gene, the hand-made rows — whose gene also takes the first row of the gene behind it, so one row
    is shared by two genes — and the M = 17 gene again with its missing calls set to 0."""
    parts, genes, at = [], [], 0
    for M in (1, 17, 64):
        parts.append(synth.make_gene(N, M, seed=seed + M, missing=0.02, common=True, mono=(M > 5), maf_hi=-0.8)[0])
        genes.append(("M%d" % M, at, M))
        at += M
    parts.append(np.ones((N, 3)))
    genes.append(("monomorphic", at, 3))
    at += 3
    parts.append(hand_rows(N, seed + 1))
    genes.append(("hand", at, len(HAND_ROWS) + 1))
    at += len(HAND_ROWS)
    parts.append(np.where(parts[1] < 0, 0.0, parts[1]))
    genes.append(("M17 no missing", at, 17))
    raw = np.asfortranarray(np.column_stack(parts))
    raw.setflags(write=False)
    return raw, genes


def gene_raw(raw, gene):
    return np.asfortranarray(raw[:, gene[1]:gene[1] + gene[2]])


def gene_columns(raw, gene):
    """the fp64 columns a caller would have uploaded for the gene"""
    return fam_bed_cases.imputed(gene_raw(raw, gene))


def decisions(raw):
    """The site pass of the gene side in integers: (flip, keep, fill value mu = a / called) per row."""
    cnt = fam_bed_cases.site_pass(raw)[0]
    n0, n1, n2 = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    called, a = n0 + n1 + n2, n1 + 2 * n2
    keep = ((n0 > 0).astype(int) + (n1 > 0) + (n2 > 0)) >= 2
    return a > called, keep, np.where(called > 0, a / np.maximum(called, 1), 0.0)


def flipped_kept(raw):
    """The flipped, filtered fp64 block of the block route from the imputed columns: (columns, flip and fill value of each)."""
    flip, keep, mu = decisions(raw)
    G = fam_bed_cases.imputed(raw)
    return np.asfortranarray(np.where(flip[None, :], 2.0 - G, G)[:, keep]), flip[keep], mu[keep]


def collapse_from_codes(raw):
    """(CMC column, Zeggini column) of the gene as fam_bed_collapse_kernel counts them, from the calls and the decisions."""
    flip, keep, mu = decisions(raw)
    n = np.zeros(raw.shape[0], dtype=np.int64)
    for j in np.flatnonzero(keep):
        call = raw[:, j]
        fill = 2.0 - mu[j] if flip[j] else mu[j]
        n += np.where(call < 0, fill >= 1.0, (call < 2) if flip[j] else (call > 0))
    return (n > 0).astype(np.float64), n.astype(np.float64)


def fill_fixed_point_flipped(raw):
    """The fill value after the flip in the fixed point the six digit planes give the flipped kept column: 2^-s, s = 39 -
    ilogb(its largest entry), which is 2 when the row has a call of 0 (2 - 0), else 1.  (kept, flipped rows only)"""
    cnt = fam_bed_cases.site_pass(raw)[0]
    flip, keep, mu = decisions(raw)
    s = np.where(cnt[:, 0] > 0, 38, 39)
    return np.ldexp(np.rint(np.ldexp(2.0 - mu, s)), -s)
