"""GPU: the kinship rotation G~ = U'G itself (rotate_columns through rvt_debug_rotate), entry by entry against the exact
integer statement of tests/rotref.py, within the bound derived there (rotref.rotation_bounds: the fp64 additions of the
plane-pair / slice partials and nothing else).  U is dense — the product of two Householder reflectors, or the eigenvectors
of a random GRM — so rot_gemm_i8_kernel runs (kinship_structure() == 1.0), at the smallest sizes that reach each of its
mechanisms: pad rows and columns of a tile, a second row panel with one live row, the second column tile, forced and default
K slices with the slice reduction, and the second panel set of the XCD mapping (N > 8192)."""
import functools

import numpy as np
import pytest

import rotref
from test_fam_cpu import make_family_case

pytestmark = pytest.mark.gpu


@pytest.fixture
def engine_factory():
    import rvtests_amd
    made = []

    def make():
        e = rvtests_amd.Engine(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


@functools.lru_cache(maxsize=2)
def dense_u(maker, N):
    U, S = getattr(rotref, maker)(N, 1000 + N)
    U.setflags(write=False)
    return U, S, rotref.quantize_u(U)


def structure_of(U32):
    """rvt_set_kinship's choice restated: ("short", visited share, installed order of the eigenpairs), ("gather", share, None)
    or ("dense", 1.0, None)."""
    N = U32.shape[0]
    nz = U32 != 0
    lo = np.where(nz.any(0), nz.argmax(0), N)
    hi = np.where(nz.any(0), N - 1 - nz[::-1].argmax(0), -1)
    order = np.argsort(lo, kind="stable")
    nrp, nchunk, visited = -(-N // rotref.BM), -(-N // rotref.KC), 0
    for rp in range(nrp):
        k = order[rp * rotref.BM:(rp + 1) * rotref.BM]
        l, h = lo[k].min(), hi[k].max()
        visited += 0 if h < l else h // rotref.KC + 1 - l // rotref.KC
    frac = visited / (nrp * nchunk)
    if frac < 0.5:
        return "short", frac, order
    if nz.sum() <= 64 * N:
        return "gather", nz.sum() / (N * N), None
    return "dense", 1.0, None


def install(eng, U, S):
    """A null model (it defines N and the block layout) and the kinship."""
    N = U.shape[0]
    rng = np.random.default_rng(N)
    X = np.column_stack([np.ones(N), rng.standard_normal(N)])
    eng.set_null(0, X, rng.standard_normal(N), np.ones(N), 1.0)
    eng.set_kinship(U, S)


def rotate(eng, G):
    ptr = eng.upload_block(G)
    out = eng.debug_rotate(ptr, G.shape[1])
    eng.free_block(ptr)
    return out


def check(out, U, G, rot_slices=None, rot_kmax=None, rows=None, contract_only=False, label="", qu=None):
    """out against the statement within `acc` (the kernel adds nothing but fp64 roundings to it), and — for the first columns,
    where N allows a long-double product — against the real product of the float U and the double G within acc + uq + gq,
    the contract of rot_gemm.hip.h.  contract_only: the paths that never quantise (the fp64 gather) are held to the contract
    against the same statement."""
    N, ncols = G.shape
    ref, planes = rotref.exact_rotation(U, G, qu)
    if rows is not None:
        ref = ref[rows]
    slices = rotref.k_slices(N, ncols, planes, rot_slices, rot_kmax)
    sum_g, max_g, max_u = np.abs(G).sum(0), np.abs(G).max(0), float(np.abs(U).max())
    acc, uq, gq = rotref.rotation_bounds(N, planes, slices, sum_g, max_u, max_g)
    tol = acc + uq + gq if contract_only else acc
    err = np.abs(out - ref)
    worst = (err / np.maximum(tol[None, :], 1e-300)).max()
    print("%s N=%d ncols=%d planes=%d slices=%d: max |err| %.3g, max err/bound %.3g (bound %.3g .. %.3g)"
          % (label, N, ncols, planes, slices, err.max(), worst, tol.min(), tol.max()))
    assert out.shape == ref.shape and np.isfinite(out).all()
    assert (err <= tol[None, :]).all(), (label, worst, np.argwhere(err > tol[None, :])[:8].tolist())
    if N <= 1000:
        c = min(ncols, 40)
        real = U.astype(np.longdouble).T @ G[:, :c].astype(np.longdouble)
        if rows is not None:
            real = real[rows]
        full = (acc + uq + gq)[:c] + N * 2.0 ** -63 * max_u * sum_g[:c]
        err = np.abs((out[:, :c].astype(np.longdouble) - real).astype(np.float64))
        assert (err <= full[None, :]).all(), (label, (err / np.maximum(full[None, :], 1e-300)).max())
    return planes, slices


def batches(N, sizes):
    """(label, G): a mixed batch per size — hard calls rare and common, all 0, all 2, one carrier, a mean-imputed column (its
    one non-integer value puts the whole batch on six planes), three-decimal dosages, and one entry of 1e6 among entries of
    1e-3, whose bound is relative to that maximum (the contract: rotref.rotation_bounds, gq) — and a hard-call-only batch,
    which is one exact plane and must meet the accumulation bound alone."""
    out = []
    for n in sizes:
        out.append(("mixed", rotref.columns(N, n, 10 * N + n, rotref.KINDS)))
        out.append(("hard", rotref.columns(N, n, 20 * N + n, rotref.HARD)))
    return out


def run_dense(engine_factory, maker, N, sizes, rot_slices=None, rot_kmax=None, extra=()):
    U, S, qu = dense_u(maker, N)
    eng = engine_factory()
    install(eng, U, S)
    assert eng.kinship_structure() == 1.0                  # the dense kernel
    seen = set()
    for label, G in list(batches(N, sizes)) + list(extra):
        seen.add(check(rotate(eng, G), U, G, rot_slices, rot_kmax, label=label, qu=qu))
    return seen


@pytest.mark.parametrize("maker", ["householder_u", "grm_u"])
def test_one_row_panel_and_padded_k(engine_factory, maker):
    """N = 130: one row panel, K padded to 256 bytes; 1 and 7 columns: the pad rows and columns of a 256 x 256 tile."""
    single = [("imputed-1", rotref.columns(130, 1, 5, ("imputed",))), ("outlier-1", rotref.columns(130, 1, 6, ("outlier",)))]
    seen = run_dense(engine_factory, maker, 130, (1, 7), extra=single)
    assert seen == {(1, 1), (6, 1)}


@pytest.mark.parametrize("maker", ["householder_u", "grm_u"])
def test_second_row_panel_with_one_live_row(engine_factory, maker):
    """N = 257: the second row panel holds one live row; K = 384 bytes, three chunks through the two-stage ring."""
    run_dense(engine_factory, maker, 257, (33,))


@pytest.mark.parametrize("maker", ["householder_u", "grm_u"])
@pytest.mark.parametrize("env,value,slices", [("RVT_ROT_SLICES", "3", 3), ("RVT_ROT_KMAX", "128", 6), (None, None, 1)])
def test_second_column_tile_and_forced_slices(engine_factory, monkeypatch, maker, env, value, slices):
    """N = 700 with 255 / 256 / 257 columns (the second column tile has one live column), K cut into 3 slices of two chunks
    and into 6 of one, each with the slice reduction, and uncut."""
    if env:
        monkeypatch.setenv(env, value)
    seen = run_dense(engine_factory, maker, 700, (255, 256, 257), rot_slices=3 if env == "RVT_ROT_SLICES" else None,
                     rot_kmax=128 if env == "RVT_ROT_KMAX" else None)
    assert seen == {(1, slices), (6, slices)}


def test_default_split_k(engine_factory):
    """N = 4100, 8 columns: 17 output tiles, so planes_gemm splits K by itself — 4224 bytes as slices of 17 and 16 chunks."""
    seen = run_dense(engine_factory, "householder_u", 4100, (8,))
    assert seen == {(1, 2), (6, 2)}


def test_second_panel_set(engine_factory):
    """N = 8200: 33 row panels, the last one in the second panel set of the workgroup mapping (rpg = 1), 8 live rows."""
    seen = run_dense(engine_factory, "householder_u", 8200, (8,))
    assert seen == {(1, 4), (6, 4)}


@pytest.mark.parametrize("n_fam", [60, 150])
def test_three_rotations_one_answer(engine_factory, monkeypatch, n_fam):
    """A nuclear-family U installed three ways — as it is, with the samples shuffled (supports scattered: the fp64 gather,
    reached as in test_gpu_decompose.py::test_shuffled_families_through_famskat) and with RVT_KINSHIP_DENSE=1 — meets the
    same statement within the same bound.  That bound is the full contract acc + uq + gq, because the gather multiplies the
    unquantised values; four non-zeros per eigenvector are fewer additions than acc allows for.
    Which kernel `as it is` selects depends on N: at 60 families (N = 240) the single row panel spans both K chunks, the
    visited share is 1 and rvt_set_kinship falls through to the gather; at 150 families (N = 600) the three panels visit 5
    of 15 chunks and rot_gemm_i8_short runs, on eigenpairs re-ordered by first non-zero row (restated here)."""
    N, K, U, S, X, y = make_family_case(n_fam, 2, 21)
    U32 = np.asfortranarray(U.astype(np.float32))
    G_all = batches(N, (7, 130))
    # as it is
    kernel, share, rows = structure_of(U32)
    assert kernel == ("short" if n_fam == 150 else "gather") and share < 0.5
    eng = engine_factory()
    install(eng, U32, S)
    assert abs(eng.kinship_structure() - share) < 1e-12
    for label, G in G_all:
        check(rotate(eng, G), U32, G, rows=rows, contract_only=True, label="default-" + label)
        if kernel == "short":                                          # an integer kernel: the accumulation bound alone
            check(rotate(eng, G), U32, G, rows=rows, label="short-" + label)
    # shuffled samples
    perm = np.random.default_rng(4).permutation(N)
    Up = np.asfortranarray(U32[perm])
    kernel, share, _ = structure_of(Up)
    assert kernel == "gather"
    eng = engine_factory()
    install(eng, Up, S)
    assert abs(eng.kinship_structure() - share) < 1e-12
    for label, G in G_all:
        check(rotate(eng, G), Up, G, contract_only=True, label="shuffled-" + label)
    # the dense kernel
    monkeypatch.setenv("RVT_KINSHIP_DENSE", "1")
    eng = engine_factory()
    install(eng, U32, S)
    assert eng.kinship_structure() == 1.0
    for label, G in G_all:
        check(rotate(eng, G), U32, G, contract_only=True, label="dense-" + label)
        check(rotate(eng, G), U32, G, label="dense-" + label)          # and to the accumulation bound, as any dense U


@pytest.mark.parametrize("env", [None, "RVT_ROT_SLICES"])
def test_same_inputs_same_bits(engine_factory, monkeypatch, env):
    if env:
        monkeypatch.setenv(env, "3")
    U, S, _ = dense_u("householder_u", 700)
    G = rotref.columns(700, 257, 3, rotref.KINDS)
    eng = engine_factory()
    install(eng, U, S)
    a = rotate(eng, G)
    b = rotate(eng, G)
    assert a.tobytes() == b.tobytes()
    other = engine_factory()
    install(other, U, S)
    assert rotate(other, G).tobytes() == a.tobytes()


def test_kinship_grows_in_one_context(engine_factory):
    """N = 130 and then N = 700 in the same context: the N = 700 answers, with no buffer left at the old size (U's planes,
    the column planes, the rotated columns), then back to 130."""
    eng = engine_factory()
    for N in (130, 700, 130):
        U, S = rotref.householder_u(N, 50 + N)
        install(eng, U, S)
        assert eng.kinship_structure() == 1.0
        for label, G in batches(N, (7 if N == 130 else 257,)):
            check(rotate(eng, G), U, G, label="grow-%d-%s" % (N, label))


def test_no_kinship_is_an_error(engine_factory):
    import rvtests_amd
    eng = engine_factory()
    rng = np.random.default_rng(1)
    eng.set_null(0, np.ones((130, 1)), rng.standard_normal(130), np.ones(130), 1.0)
    ptr = eng.upload_block(np.ones((130, 2)))
    with pytest.raises(rvtests_amd.RvtError, match="rvt_set_kinship"):
        eng.debug_rotate(ptr, 2)
