"""MetaCov's band from rows of a resident .bed matrix, without a GPU: the C ABI of rvt_cov_band_bed_dev, the byte -> nibble
mapping the front stage and the harness share (rvtests_amd/csrc/rvt_bed_nibbles.h) over every byte value, and the identities
the front stage rests on, in numpy."""
import ctypes as C
import os
import re

import numpy as np

import hc
import metacov_bed_cases as cases
import rvtests_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_documents_and_the_library_exports():
    src = open(os.path.join(ROOT, "include", "rvtests_amd.h")).read()
    assert ("int rvt_cov_band_bed_dev(rvt_ctx* ctx, const unsigned char* d_rows, int H, int W, int halo, float scale, "
            "float* band,") in src
    assert "int rvt_cov_band_bed_last_timing(rvt_ctx* ctx, double* ms3);" in src
    for name in ("rvt_cov_band_bed_dev", "rvt_cov_band_bed_last_timing"):
        doc = re.search(r"/\*((?:(?!\*/).)*)\*/\nint %s\(" % name, src, flags=re.S)
        assert doc, name
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\nint rvt_cov_band_bed_dev\(", src, flags=re.S).group(1)
    for cited in ("src/DataConsolidator.cpp:217-245", "RVT_E_INVALID", "RVT_E_STATE", "counts", "RVT_METACOV_FP64"):
        assert cited in doc, cited
    rvtests_amd.build_library()
    lib = rvtests_amd.load_library()
    for name in ("rvt_cov_band_bed_dev", "rvt_cov_band_bed_last_timing"):
        assert hasattr(lib, name), name
    for name in ("cov_band_bed", "cov_band_bed_last_timing"):
        assert callable(getattr(rvtests_amd.Engine, name))


def test_every_byte_under_every_live_mask_gives_the_restated_nibbles_and_counts():
    L = hc.lib()
    L.hc_bed_byte_nibbles.restype = None
    L.hc_bed_byte_nibbles.argtypes = [C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    out = (C.c_uint * 6)()
    for live in (1, 2, 3, 4):
        h, m, cnt = cases.nibble_table(live)
        assert (cnt.sum(1) == live).all()
        got = np.zeros((256, 6), dtype=np.uint32)
        for byte in range(256):
            L.hc_bed_byte_nibbles(byte, live, out)
            got[byte] = list(out)
        assert np.array_equal(got[:, 0], h), live
        assert np.array_equal(got[:, 1], m), live
        assert np.array_equal(got[:, 2:], cnt), live
        # nothing of a sample that does not exist: the nibbles behind the live ones are zero whatever the byte holds
        assert ((got[:, 0] | got[:, 1]) >> (4 * live) == 0).all()
        # E2M1: 0x2 = 1.0, 0x4 = 2.0; a sample is a call or missing, never both
        nib = (got[:, :2, None] >> (4 * np.arange(4))) & 0xF
        assert set(np.unique(nib[:, 0])) <= {0, 2, 4} and set(np.unique(nib[:, 1])) <= {0, 2}
        assert ((nib[:, 0] != 0) & (nib[:, 1] != 0)).sum() == 0


def test_the_rows_numbers_follow_from_their_counts():
    """g = h + mu m exactly, the column sum and the polymorphic flag from the four counts — on the hand-made rows too."""
    for N in (237, 515, 160):
        raw = cases.calls(N, 30, seed=77)
        G = cases.imputed(raw)
        cnt = cases.counts(raw)
        assert cnt.sum(1).tolist() == [N] * raw.shape[1]
        called, ac = cnt[:, :3].sum(1), cnt[:, 1] + 2 * cnt[:, 2]
        mu = np.where(called > 0, ac / np.maximum(called, 1), 0.0)
        h = np.where(raw < 0, 0.0, raw)
        m = (raw < 0).astype(np.float64)
        assert np.array_equal(h + mu[None, :] * m, G)
        colsum = ac + mu * cnt[:, 3]
        assert (np.abs(colsum - G.sum(0)) <= N * np.spacing(np.abs(G.sum(0)))).all()
        poly = ((cnt[:, 0] > 0).astype(int) + (cnt[:, 1] > 0) + (cnt[:, 2] > 0)) >= 2
        assert np.array_equal(poly.astype(np.int32), cases.polymorphic(G))
        k = raw.shape[1] - len(cases.SPECIAL)
        assert cnt[k, 3] == N and not poly[k] and (G[:, k] == 0).all()               # all missing: the zero column
        assert cnt[k + 1, 1] == N and not poly[k + 1]                                  # all het
        assert cnt[k + 2, 3] > 0 and cnt[k + 2, 2] == N - cnt[k + 2, 3] and not poly[k + 2] and (G[:, k + 2] == 2).all()
        assert cnt[k + 3, 1] == 1 and cnt[k + 3, 0] == N - 1 and poly[k + 3]           # a single carrier
        assert cnt[k + 4, 3] == 0 and poly[k + 4]                                      # no missing call
