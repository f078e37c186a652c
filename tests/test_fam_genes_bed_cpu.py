"""The gene-based family tests over resident .bed rows (rvt_run_fam_tests_bed_dev), without a GPU: the C ABI, and the rules of its
front stage (rvtests_amd/csrc/fam_bed_kernels.hip.h) in numpy — the flip and keep decisions follow from the four counts of a row
in integers, the burden collapse from the codes, and the dense rotation of a flipped column is the integer statement split in two."""
import os
import re

import numpy as np

import fam_bed_cases
import fam_genes_bed_cases as cases
import rvtests_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_documents_and_the_library_exports():
    src = open(os.path.join(ROOT, "include", "rvtests_amd.h")).read()
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\nint rvt_run_fam_tests_bed_dev\(rvt_ctx\* ctx, int n_genes, const unsigned char\* const\* "
                    r"d_rows, const int\* M, const int64_t\* gene_ids,\s+uint32_t tests, rvt_gene_result\* out\);", src, flags=re.S)
    assert doc
    # a comment of its own, citing what rvt_run_fam_tests cites
    for cited in ("src/Model.h:3048-3145", "src/Model.h:2261-2376", "src/Model.h:2378-2492", "regression/FastLMM.cpp:215-247",
                  "rvt_submit_gene_bed_dev", "RVT_E_INVALID", "RVT_E_TOO_LARGE", "RVT_E_STATE", "Synchronous"):
        assert cited in doc.group(1), cited
    for name in ("README.md", "DESIGN.md", os.path.join("include", "rvtests_amd.h")):
        text = open(os.path.join(ROOT, name)).read()
        for m in re.finditer(r"Not covered from resident rows[^.]*\.", text):
            assert "FamSKAT" not in m.group(0), (name, m.group(0))
    rvtests_amd.build_library()
    lib = rvtests_amd.load_library()
    assert hasattr(lib, "rvt_run_fam_tests_bed_dev")
    assert callable(rvtests_amd.Engine.run_fam_tests_bed_dev)


def all_rows(N):
    return np.column_stack([fam_bed_cases.calls(N, 37, seed=1234), cases.hand_rows(N, 77)])


def test_flip_and_keep_from_the_counts_equal_the_sums_of_the_imputed_column():
    """flip = a > called is sum(imputed column) > N, summed in sequence as the reference does and pairwise as numpy does; keep =
    two of n0, n1, n2 non-zero is min != max of the imputed column.  The hand-made rows sit on the edge: a == called (mu == 1.0
    exactly, the sum is exactly N) and a == called + 1 (the sum is N + N / called)."""
    for N in (237, 515, 160):
        raw = all_rows(N)
        G = fam_bed_cases.imputed(raw)
        flip, keep, mu = cases.decisions(raw)
        seq = np.zeros(G.shape[1])
        for i in range(N):
            seq = seq + G[i]
        assert np.array_equal(flip, seq > N)
        assert np.array_equal(flip, G.sum(0) > N)
        assert np.array_equal(keep, G.min(0) != G.max(0))
        h = raw.shape[1] - len(cases.HAND_ROWS)
        cnt = fam_bed_cases.site_pass(raw)[0]
        called, a = cnt[:, :3].sum(1), cnt[:, 1] + 2 * cnt[:, 2]
        assert a[h] == called[h] and cnt[h, 3] > 0 and mu[h] == 1.0 and keep[h] and not flip[h] and seq[h] == N
        assert a[h + 1] == called[h + 1] + 1 and cnt[h + 1, 3] > 0 and keep[h + 1] and flip[h + 1]
        assert len(np.unique(raw[:, h + 2])) == 2 and not keep[h + 2] and G[:, h + 2].min() == G[:, h + 2].max()
        last = 4 * ((N + 3) // 4 - 1)
        assert flip[h + 3] and keep[h + 3] and (raw[last:, h + 3] < 0).all() and (raw[:last, h + 3] >= 0).all()
        assert flip.sum() >= 4 and (~keep).sum() >= 5 and (keep & ~flip).sum() >= 10


def test_collapse_from_the_codes_equals_the_count_on_the_flipped_imputed_columns():
    for N in (237, 515, 160):
        raw, genes = cases.gene_set(N, 500)
        for gene in genes + [("all rows", 0, raw.shape[1])]:
            g = cases.gene_raw(raw, gene)
            Gf, flip, mu = cases.flipped_kept(g)
            n = (Gf.astype(np.int64) > 0).sum(1)                 # (int)g > 0, src/Model.cpp:73-89,115-130
            cmc, zeg = cases.collapse_from_codes(g)
            assert np.array_equal(cmc, (n > 0).astype(np.float64)), gene[0]
            assert np.array_equal(zeg, n.astype(np.float64)), gene[0]
        # the gene with the mu == 1.0 row: its missing samples are counted, those of the other rows are not
        hand = cases.gene_raw(raw, genes[4])
        one = np.asfortranarray(hand[:, :1])
        assert cases.decisions(one)[2][0] == 1.0
        miss = one[:, 0] < 0
        assert miss.sum() == 5 and (cases.collapse_from_codes(one)[1][miss] == 1.0).all()
        flipped = np.asfortranarray(hand[:, 1:2])
        assert (cases.collapse_from_codes(flipped)[1][flipped[:, 0] < 0] == 0.0).all()
        assert (cases.collapse_from_codes(hand)[1][miss] >= 1.0).all()


def test_the_dense_route_of_a_flipped_column_is_the_integer_statement_split_in_two():
    """U'c' + muq' U'm from exact integer products against tests/rotref.py's statement of the six-plane product of the flipped
    imputed columns, within its accumulation bound (cf. test_the_dense_route_is_the_integer_statement_split_in_two)."""
    import rotref
    N = 130
    U, S = rotref.householder_u(N, 7)
    raw = all_rows(N)
    raw = np.column_stack([raw, np.where(raw[:, :12] < 0, -9.0, 2.0 - raw[:, :12])])   # (more rows whose alt allele is the common one)
    flip, keep, mu = cases.decisions(raw)
    sel = flip & keep
    assert sel.sum() >= 8
    raw = np.asfortranarray(raw[:, sel])
    G = 2.0 - fam_bed_cases.imputed(raw)
    assert np.array_equal(G, cases.flipped_kept(raw)[0])
    qu = rotref.quantize_u(U)
    ref, planes = rotref.exact_rotation(U, G, qu)
    assert planes == rotref.PLANES_G
    muq = cases.fill_fixed_point_flipped(raw)
    assert (np.abs(muq - (2.0 - mu[sel])) <= 2.0 ** -39).all() and (muq != 2.0 - mu[sel]).any()
    c = np.where(raw < 0, 0, 2 - raw).astype(np.int64).astype(object)
    m = (raw < 0).astype(np.int64).astype(object)
    assert (m.sum(0) > 0).any()
    den = float(1 << rotref.U_SEXP)
    Uc = (qu.T.astype(object) @ c).astype(np.float64) / den
    Um = (qu.T.astype(object) @ m).astype(np.float64) / den
    acc, _, _ = rotref.rotation_bounds(N, planes, 1, np.abs(G).sum(0), float(np.abs(U).max()), np.abs(G).max(0))
    assert (np.abs(Uc + muq[None, :] * Um - ref) <= acc[None, :]).all()
