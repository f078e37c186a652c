"""The column blocks' bookkeeping (rvt_block_alloc and the operations on columns of such a block): one scripted sequence of
every operation against its numpy statement, the range check of every operation, and a null model replaced under a queued column.
N = 4099: the upload queue and the 2-bit packing engage from 4096 on, and 4099 is no multiple of 4, 16 or 128."""
import ctypes as C

import numpy as np
import pytest

import orc
from rvtests_amd import CODING_DOMINANT
from test_gpu_metacov import engine_factory  # noqa: F401  (fixture)
from test_gpu_meta_coded import recode
from test_metacov_cpu import make_case

pytestmark = pytest.mark.gpu

N = 4099
RVT_E_INVALID = -1


def _case(V, d, seed):
    G, chrom, pos, X, y = make_case(N, V, d, 0, seed)
    rc, beta, pred, res, s2 = orc.fit_linear(X, y)
    return np.asfortranarray(np.rint(G)), X, y, res, s2


def _impute(col, rng, rate=0.03):
    miss = rng.random(N) < rate
    col = col.copy()
    col[miss] = col[~miss].mean()
    return col


def test_scripted_sequence_against_numpy(engine_factory):
    """A ring of 80 columns filled with 70 columns one call each (column 5 mean-imputed: queued with its other value; column 40 a
    dosage: it crosses as doubles, behind the 32 + 8 columns queued before it and in front of the later ones), then columns
    7..9 overwritten by one upload of three (9 mean-imputed), columns 10..29 copied into a second block, the ring moved forward
    by 8, and 33 of its columns — the dosage among them — recoded dominant into the second block.  After every step both
    blocks download as the numpy statement of the step, bit for bit.  At the end the bands of the ring are those of a block that
    received the same columns in a few uploads of many (the dosage on its own, so that its neighbours are packed as in the
    ring; the column with the missing code -9 too: an upload of several columns packs other values inside [0, 2] only):
    windows left and right of the dosage on the integer band, the whole ring on the fp64 one."""
    G, X, y, res, s2 = _case(70, 2, 4099)
    rng = np.random.default_rng(11)
    G[:, 5] = _impute(G[:, 5], rng)
    G[:, 40] = G[:, 40] * 0.5 + 0.25 * rng.integers(0, 3, N)          # several values that are no hard calls
    G[rng.random(N) < 0.02, 20] = -9.0                                # (missing calls: the recoding writes their average)
    eng = engine_factory()
    eng.set_null(0, X, res, np.full(N, s2), s2)
    ring, other = eng.alloc_block(80), eng.alloc_block(40)
    m_ring, m_other = np.zeros((N, 80), order="F"), np.zeros((N, 40), order="F")

    def check(step):
        assert np.array_equal(eng.download_columns(ring, 0, 80), m_ring), step
        assert np.array_equal(eng.download_columns(other, 0, 40), m_other), step

    for j in range(70):
        eng.upload_columns(ring, j, G[:, j])
    m_ring[:, :70] = G
    check("70 columns, one call each")
    three = np.asfortranarray(np.rint(rng.random((N, 3)) * 2.2).clip(0, 2))
    three[:, 2] = _impute(three[:, 2], rng)
    eng.upload_columns(ring, 7, three)
    m_ring[:, 7:10] = three
    check("three columns over 7..9")
    eng._check(eng.L.rvt_block_copy_columns(eng.ctx, C.c_void_p(other), 3, C.c_void_p(ring), 10, 20))
    m_other[:, 3:23] = m_ring[:, 10:30]
    check("20 columns copied")
    eng.move_columns(ring, 0, 8, 72)
    m_ring[:, :72] = m_ring[:, 8:80].copy()
    check("ring moved forward by 8")
    eng.block_recode(other, 5, ring, 2, 33, CODING_DOMINANT)
    m_other[:, 5:38] = recode(m_ring[:, 2:35], CODING_DOMINANT)[0]
    check("33 columns recoded")

    assert not np.array_equal(m_ring[:, 32], np.rint(m_ring[:, 32]))  # (the dosage: column 40 before the move)
    ref = eng.alloc_block(80)
    assert (m_ring[:, 12] < 0).any()                                  # (the column with missing calls: 20 before the move)
    for a, b in ((0, 12), (12, 13), (13, 32), (32, 33), (33, 72)):
        eng.upload_columns(ref, a, m_ring[:, a:b])
    for col0, W, integer in ((0, 32, True), (33, 29, True), (0, 72, False)):   # (columns 62..71 were never uploaded: no cache entry)
        got = eng.cov_band(ring, 0, col0, W, W, 20)
        path = eng.cov_band_last_path()
        want = eng.cov_band(ref, 0, col0, W, W, 20)
        assert path == eng.cov_band_last_path() and (path != 0) == integer, (col0, W, path)
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[3], want[3])


@pytest.mark.parametrize("queued", [False, True])
def test_column_ranges_are_checked(engine_factory, queued):
    """Every column operation refuses a range that leaves a block of rvt_block_alloc with RVT_E_INVALID, on the host and before
    any device work — with a column waiting in the upload queue or without —, and the blocks stay what they were."""
    G, X, y, res, s2 = _case(34, 2, 16)
    eng = engine_factory()
    eng.set_null(0, X, res, np.full(N, s2), s2)
    blk, other = eng.alloc_block(16), eng.alloc_block(16)
    eng.upload_columns(blk, 0, G[:, :16])
    eng.upload_columns(other, 0, G[:, 16:32])
    want = G[:, :16].copy()
    L, ctx, p = eng.L, eng.ctx, C.c_void_p
    two = np.asfortranarray(G[:, 32:34])
    calls = [
        lambda: L.rvt_block_upload_columns(ctx, p(blk), 15, 2, two.ctypes.data_as(C.POINTER(C.c_double))),
        lambda: L.rvt_block_copy_columns(ctx, p(blk), 10, p(other), 0, 7),      # the target leaves its block
        lambda: L.rvt_block_copy_columns(ctx, p(other), 0, p(blk), 10, 7),      # the source
        lambda: L.rvt_block_move_columns(ctx, p(blk), 0, 10, 7),
    ]
    for k, call in enumerate(calls):
        if queued:
            want[:, 3] = G[:, 32 + k % 2]
            eng.upload_columns(blk, 3, want[:, 3])
        assert call() == RVT_E_INVALID, k
        assert b"leave the block (16 columns)" in L.rvt_last_error(ctx), k
        assert np.array_equal(eng.download_columns(blk, 0, 16), want), k
        assert np.array_equal(eng.download_columns(other, 0, 16), G[:, 16:32]), k


def test_null_model_replaced_under_a_queued_column(engine_factory):
    """A column waiting in the upload queue was packed for the installed model: rvt_set_null sends it to its block before
    the model goes.  It downloads as uploaded, and the block scores under the new model as the same block uploaded at once."""
    G, X, y, res, s2 = _case(3, 3, 77)
    eng = engine_factory()
    eng.set_null(0, X, res, np.full(N, s2), s2)
    blk = eng.alloc_block(3)
    eng.upload_columns(blk, 1, G[:, 1])
    X2 = X.copy()
    X2[:, 1] = X[:, 1] ** 2
    rc, beta2, pred2, res2, s22 = orc.fit_linear(X2, y)
    eng.set_null(0, X2, res2, np.full(N, s22), s22)
    assert np.array_equal(eng.download_columns(blk, 1, 1)[:, 0], G[:, 1])
    M = np.zeros((N, 3), order="F")
    M[:, 1] = G[:, 1]
    got, want = eng.score_block(blk, 3), eng.score_block(eng.upload_block(M), 3)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
