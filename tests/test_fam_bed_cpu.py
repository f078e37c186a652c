"""The family single-variant calls over resident .bed rows, without a GPU: their C ABI, and the identities of the front stage
(rvtests_amd/csrc/fam_bed_kernels.hip.h) in numpy — the imputed column is exactly c + mu m, and its sum and polymorphic flag
follow from the four counts of a row."""
import os
import re

import numpy as np

import fam_bed_cases
import rvtests_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rvt_score_bed_dev_fam", "rvt_lrt_bed_dev_fam", "rvt_debug_rotate_bed")


def test_header_declares_documents_and_the_library_exports():
    src = open(os.path.join(ROOT, "include", "rvtests_amd.h")).read()
    assert ("int rvt_score_bed_dev_fam(rvt_ctx* ctx, const unsigned char* d_rows, int64_t V, int binary, int* ok, double* ustat, "
            "double* vstat,") in src
    assert "int rvt_lrt_bed_dev_fam(rvt_ctx* ctx, const unsigned char* d_rows, int64_t V, int* ok, double* af, double* null_loglik," in src
    assert "int rvt_debug_rotate_bed(rvt_ctx* ctx, const unsigned char* d_rows, int ncols, double* out);" in src
    # documented: one comment in front of the two calls (the second declaration follows the first), one in front of the hook
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\nint rvt_score_bed_dev_fam\([^;]*;\nint rvt_lrt_bed_dev_fam\(", src, flags=re.S)
    assert doc and re.search(r"\*/\nint rvt_debug_rotate_bed\(", src)
    for cited in ("src/Model.h:3398-3499", "src/Model.h:620-712", "src/DataConsolidator.cpp:217-245", "RVT_E_STATE", "counts"):
        assert cited in doc.group(1), cited
    rvtests_amd.build_library()
    lib = rvtests_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("score_bed_dev_fam", "lrt_bed_dev_fam", "debug_rotate_bed"):
        assert callable(getattr(rvtests_amd.Engine, name))


def test_the_imputed_column_is_c_plus_mu_m_and_the_counts_give_its_sum_and_flag():
    for N in (237, 515, 160):                              # N mod 4 = 1, 3, 0
        raw = fam_bed_cases.calls(N, 37, seed=1234)
        kinds = raw[:, -len(fam_bed_cases.HAND_ROWS):]
        assert (kinds[:, 0] == 0).all() and (kinds[:, 1] == 2).all() and (kinds[:, 2] == 1).all() and (kinds[:, 3] < 0).all()
        assert (kinds[:, 4] >= 0).sum() == 1
        last = 4 * ((N + 3) // 4 - 1)
        assert (kinds[last:, 5] < 0).all() and (kinds[:last, 5] >= 0).all()
        assert (kinds[:, 6] >= 0).all()
        G = fam_bed_cases.imputed(raw)
        cnt, mu, colsum, poly = fam_bed_cases.site_pass(raw)
        c = np.where(raw < 0, 0.0, raw)
        m = (raw < 0).astype(np.float64)
        assert np.array_equal(c + mu[None, :] * m, G)      # exactly: one product, and it is added to 0
        assert (np.abs(colsum - G.sum(0)) <= N * np.spacing(np.abs(G.sum(0)))).all()
        assert np.array_equal(poly, G.min(0) != G.max(0))
        assert mu[-4] == 0.0 and not poly[-4] and (G[:, -4] == 0).all()     # the row with no called sample
        assert cnt.sum(1).tolist() == [N] * raw.shape[1]


def test_the_dense_route_is_the_integer_statement_split_in_two():
    """U'c + muq U'm from exact integer products, in numpy, against tests/rotref.py's statement of the six-plane product of the
    imputed columns: within its accumulation bound — only the double roundings of the two quotients and the fma separate them."""
    import rotref
    N = 130
    U, S = rotref.householder_u(N, 7)
    raw = fam_bed_cases.calls(N, 37, seed=1234)
    G = fam_bed_cases.imputed(raw)
    qu = rotref.quantize_u(U)
    ref, planes = rotref.exact_rotation(U, G, qu)
    assert planes == rotref.PLANES_G
    cnt, mu, _, _ = fam_bed_cases.site_pass(raw)
    muq = fam_bed_cases.fill_fixed_point(cnt, mu)
    assert (np.abs(muq - mu) <= 2.0 ** -39).all() and (muq != mu).any()
    c = np.where(raw < 0, 0, raw).astype(np.int64).astype(object)
    m = (raw < 0).astype(np.int64).astype(object)
    den = float(1 << rotref.U_SEXP)
    Uc = (qu.T.astype(object) @ c).astype(np.float64) / den
    Um = (qu.T.astype(object) @ m).astype(np.float64) / den
    acc, _, _ = rotref.rotation_bounds(N, planes, 1, np.abs(G).sum(0), float(np.abs(U).max()), np.abs(G).max(0))
    assert (np.abs(Uc + muq[None, :] * Um - ref) <= acc[None, :]).all()


def test_hostile_padding_bits_decode_to_the_same_calls():
    for N in (237, 515, 160):
        raw = fam_bed_cases.calls(N, 9, seed=5)
        rows = fam_bed_cases.pack(raw)
        clean = rvtests_amd.Engine.pack_bed(raw)
        pad = (-N) % 4
        assert rows.shape == (raw.shape[1], (N + 3) // 4)
        assert np.array_equal(rows[:, :-1], clean[:, :-1])
        if pad:
            assert (rows[:, -1] >> (2 * (4 - pad)) == (0xFF >> (2 * (4 - pad)))).all() and (rows[:, -1] != clean[:, -1]).all()
        code = (rows[:, :, None] >> (2 * np.arange(4))[None, None, :]) & 3
        val = np.array([0.0, -9.0, 1.0, 2.0])[code.reshape(rows.shape[0], -1)[:, :N]].T
        assert np.array_equal(val, np.where(raw < 0, -9.0, raw))
