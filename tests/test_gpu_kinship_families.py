"""GPU: the family form of the kinship (rvt_set_kinship_families, rvt_kinship_decompose_families) — the family-blocked
rotation against numpy's fp64 block products, every family consumer against a dense installation of the equivalent U on the
same engine, the blockwise decomposition, a cohort whose N x N would not fit the card, the refusals, and the host driver's
--kin-families."""
import functools
import struct
import subprocess

import numpy as np
import pytest
import torch  # before the engine's library is loaded: both then share one HIP runtime (case 4 asks torch for the free memory)

import orc
import synth
from test_host_driver import DRIVER, _ensure_driver, write_input
from test_single_fam_cpu import run_single_fam, write_kinship

pytestmark = pytest.mark.gpu

COL_TILE = 16        # kRotFamCols (rvtests_amd/csrc/rot_gemm.hip.h)
EPS = 2.0 ** -53


@pytest.fixture
def eng():
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    yield e
    e.close()


class Cohort:
    """Families of the given sizes: a random positive-definite "kinship" block per family (that of
    test_family_structure_is_detected_and_changes_nothing), its float eigenpairs block by block, members in order or shuffled."""

    def __init__(self, sizes, seed, shuffle):
        rng = np.random.default_rng(seed)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.fam_ptr = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.N = int(self.fam_ptr[-1])
        self.members = (rng.permutation(self.N) if shuffle else np.arange(self.N)).astype(np.int32)
        self.K, self.U, S = [], [], []
        for sz in self.sizes:
            A = rng.uniform(0.1, 0.5, (sz, sz))
            Kf = ((A + A.T) / 2 + np.eye(sz)).astype(np.float32)
            s, u = np.linalg.eigh(Kf.astype(np.float64))
            self.K.append(Kf)
            self.U.append(u.astype(np.float32))
            S.append(s.astype(np.float32))
        self.S = np.concatenate(S)

    def flat(self, blocks):
        return np.concatenate([b.ravel(order="F") for b in blocks]).astype(np.float32)

    def rows(self, f):
        return self.members[self.fam_ptr[f]:self.fam_ptr[f + 1]]

    def dense(self, blocks, square=False):
        """The equivalent N x N float matrix: eigenvectors (rows = samples, columns = eigenpairs) or, square, the kinship."""
        D = np.zeros((self.N, self.N), dtype=np.float32, order="F")
        for f, b in enumerate(blocks):
            lo, hi = self.fam_ptr[f], self.fam_ptr[f + 1]
            D[np.ix_(self.rows(f), self.rows(f) if square else np.arange(lo, hi))] = b
        return D

    def rotate(self, blocks, G):
        """U'G in fp64 from the float blocks, and the dot-product bound 2 k 2^-53 sum |u_r g_r| of every output."""
        want, bound = np.zeros((self.N, G.shape[1])), np.zeros((self.N, G.shape[1]))
        for f, b in enumerate(blocks):
            u, g = b.astype(np.float64), G[self.rows(f)]
            lo, hi = self.fam_ptr[f], self.fam_ptr[f + 1]
            want[lo:hi] = u.T @ g
            bound[lo:hi] = 2 * len(u) * EPS * (np.abs(u).T @ np.abs(g))
        return want, bound

    def install(self, eng):
        eng.set_kinship_families(self.fam_ptr, self.members, self.flat(self.U), self.S)


def null_for_layout(eng, N):
    rng = np.random.default_rng(N)
    X = np.column_stack([np.ones(N), rng.standard_normal(N)])
    eng.set_null(0, X, rng.standard_normal(N), np.ones(N), 1.0)


# ---- 1. the rotation against numpy ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rotation_cohort(shuffle):
    rng = np.random.default_rng(21)
    mid = rng.choice([1, 2, 3, 4, 7], size=150)
    sizes = np.concatenate([[64, 1], mid, [1, 64, 3, 64]])       # a 64 beside singletons; the last family ends at N - 1
    c = Cohort(sizes, 22, shuffle)
    assert 600 < c.N < 800 and c.fam_ptr[-1] == c.N
    return c


@functools.lru_cache(maxsize=None)
def rotation_columns(N, hard):
    rng = np.random.default_rng(23)
    if hard:
        G = rng.choice([0.0, 1.0, 2.0], size=(N, 70), p=[0.8, 0.15, 0.05])
    else:
        G = rng.standard_normal((N, 70)) * 10.0 ** rng.integers(-3, 4, size=(1, 70))
    G.setflags(write=False)
    return G


@pytest.mark.parametrize("hard", [True, False], ids=["hardcalls", "doubles"])
@pytest.mark.parametrize("shuffle", [False, True], ids=["contiguous", "permuted"])
def test_rotation_matches_numpy_block_products(eng, shuffle, hard):
    c = rotation_cohort(shuffle)
    G = rotation_columns(c.N, hard)
    null_for_layout(eng, c.N)
    c.install(eng)
    assert abs(eng.kinship_structure() - float((c.sizes ** 2).sum()) / c.N ** 2) < 1e-15
    ptr = eng.upload_block(G)
    want, bound = c.rotate(c.U, G)
    for ncols in (1, COL_TILE + 1, 70):
        got = eng.debug_rotate(ptr, ncols)
        err = np.abs(got - want[:, :ncols])
        print("ncols %d: worst error / bound %.3g" % (ncols, (err / np.maximum(bound[:, :ncols], 1e-300)).max()))
        assert (err <= bound[:, :ncols]).all()
        again = eng.debug_rotate(ptr, ncols)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


# ---- 2. every family consumer: family form against the dense installation of the same U --------------------------------
def rel(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= tol * np.abs(b)).all())


def p_close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= 1e-8 * b + 1e-14).all())


FAM_ALL = 16 | 32 | 64   # RVT_TEST_FAMSKAT | FAMCMC | FAMZEGGINI


def consumers(eng, X, y, genes, G_single):
    """Everything a family call returns, on the installed kinship."""
    d = X.shape[1]
    out = {"null": eng.fit_fam_null(X, y)}
    ptrs = [eng.upload_block(G) for G in genes]
    Ms = [G.shape[1] for G in genes]
    out["fam"] = eng.run_fam_blocks(ptrs, Ms, tests=FAM_ALL)
    out["vt"] = eng.fam_analytic_vt(ptrs, Ms)
    ps = eng.upload_block(G_single)
    V = G_single.shape[1]
    out["score"] = eng.score_block_fam(ps, V)
    out["lrt"] = eng.lrt_block_fam(ps, V)
    out["cov"] = eng.cov_block_fam(ps, V, d)
    eng.fit_grammar_null(X, y)
    out["grammar"] = [eng.grammar_block(ps, V, af) for af in (0, 1)]
    for p in ptrs + [ps]:
        eng.free_block(p)
    return out


def famskat_against_oracle(fam_records, nul, genes, X, y, U32, S32):
    """FamSKAT's Q against the oracle's literal N x N restatement with the dense U, at 1e-6.  The oracle's own FastLMM fit is held
    to the device's as tests/test_gpu_fam.py::test_fam_null_matches_oracle holds it — the likelihood is flat at its optimum, so
    rounding decides Brent's trajectory and delta is pinned to ~1e-3 only — and FamSKAT is then given the device's (delta,
    sigma2, beta), as test_famskat_matches_oracle does: with the oracle's own delta Q follows that 1e-3 (measured on the
    interleaved cohort of case 2: 4.5e-5 relative, the family form and the dense installation agreeing to 1e-11)."""
    U64, S64 = U32.astype(np.float64), S32.astype(np.float64)
    d = X.shape[1]
    rc, own = orc.fastlmm_null(X, y, U64, S64)
    assert rc == 0 and abs(nul.delta - own.delta) <= 2e-3 + 1e-3 * own.delta
    assert abs(nul.sigma2_g - own.sigma2) <= 5e-3 * own.sigma2
    onul = orc.FamNull()
    onul.ok = 1
    onul.delta, onul.sigma2 = nul.delta, nul.sigma2_g
    for k in range(d):
        onul.beta[k] = nul.beta[k]
    for r, G in zip(fam_records, genes):
        rc, s = orc.famskat(G, X, y, U64, S64, onul)
        print("FamSKAT Q: device %.15g oracle %.15g" % (r.famskat_Q, s.Q))
        assert rc == 0 and r.famskat_ok == 1 and abs(r.famskat_Q - s.Q) <= 1e-6 * s.Q


def structure_cohort(shuffle):
    sizes = np.random.default_rng(5).choice([1, 2, 3, 4, 6], size=700)
    return Cohort(sizes, 6, shuffle)


def phenotype_and_genes(N, seed=7, d=3):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N)] + [rng.standard_normal(N) for _ in range(d - 1)])
    y = 0.3 * X[:, 1] + rng.standard_normal(N)
    genes = [synth.make_gene(N, M, seed=800 + M, missing=0.01, common=True)[1] for M in (5, 24, 40)]
    G_single = synth.make_gene(N, 30, seed=77, missing=0.01, common=True, mono=True)[1]
    return X, y, genes, G_single


@pytest.mark.parametrize("shuffle", [False, True], ids=["contiguous", "interleaved"])
def test_every_family_consumer_agrees_with_the_dense_install(eng, shuffle):
    c = structure_cohort(shuffle)
    X, y, genes, G_single = phenotype_and_genes(c.N)
    U = c.dense(c.U)
    eng.set_kinship(U, c.S)
    dense = consumers(eng, X, y, genes, G_single)
    c.install(eng)
    assert eng.kinship_structure() < 0.01
    fam = consumers(eng, X, y, genes, G_single)

    a, b = fam["null"], dense["null"]
    assert a.brent_evals == b.brent_evals and abs(a.delta - b.delta) <= 1e-9 * b.delta
    for r, s in zip(fam["fam"], dense["fam"]):
        assert (r.famskat_ok, r.famcmc_ok, r.famzeg_ok, r.n_poly) == (s.famskat_ok, s.famcmc_ok, s.famzeg_ok, s.n_poly)
        assert r.famskat_ok == 1 and rel(r.famskat_Q, s.famskat_Q, 1e-11)
        assert p_close([r.famskat_p, r.famcmc_p, r.famzeg_p], [s.famskat_p, s.famcmc_p, s.famzeg_p])
    for name, cols in (("score", ("U", "V")), ("lrt", ("null_ll", "alt_ll"))):
        r, s = fam[name], dense[name]
        assert (r["ok"] == s["ok"]).all() and (s["ok"] == 1).sum() > 20
        k = s["ok"] == 1
        for col in cols:
            assert rel(r[col][k], s[col][k], 1e-9), (name, col)
        assert p_close(r["p"][k], s["p"][k]), name
    for r, s in zip(fam["grammar"], dense["grammar"]):
        assert (r["ok"] == s["ok"]).all()
        k = s["ok"] == 1
        assert rel(r["beta"][k], s["beta"][k], 1e-9) and rel(r["af"][k], s["af"][k], 1e-9) and p_close(r["p"][k], s["p"][k])
    (cov, xz, zz, poly), (cov0, xz0, zz0, poly0) = fam["cov"], dense["cov"]
    assert (poly == poly0).all()
    V = len(poly0)
    m = np.triu(np.ones((V, V), dtype=bool)) & ~np.isnan(cov0)      # cov[h, j] is defined for j >= h only
    assert (np.isnan(cov) == np.isnan(cov0))[np.triu_indices(V)].all() and m.sum() > V
    assert np.allclose(cov[m], cov0[m], rtol=1e-8, atol=1e-9 * np.abs(cov0[m]).max())
    assert np.allclose(xz, xz0, rtol=1e-8, atol=1e-9 * max(np.abs(xz0).max(), 1.0))
    assert np.allclose(zz, zz0, rtol=1e-8, atol=1e-9 * np.abs(zz0).max())
    for r, s in zip(fam["vt"], dense["vt"]):
        assert r.vt_ok == s.vt_ok == 1
        assert (r.vt_optnum, r.vt_ncutoff) == (s.vt_optnum, s.vt_ncutoff)
        assert rel([r.vt_minmaf, r.vt_maxmaf, r.vt_optmaf, r.vt_U, r.vt_V, r.vt_stat],
                   [s.vt_minmaf, s.vt_maxmaf, s.vt_optmaf, s.vt_U, s.vt_V, s.vt_stat], 1e-9)
        assert abs(r.vt_p - s.vt_p) <= r.vt_p_error + s.vt_p_error
    famskat_against_oracle(fam["fam"], fam["null"], genes, X, y, U, c.S)


# ---- 3. the decomposition ----------------------------------------------------------------------------------------------------
def spd_cohort(sizes, seed, shuffle=True):
    c = Cohort(sizes, seed, shuffle)
    rng = np.random.default_rng(seed + 1)
    c.K = []
    for sz in c.sizes:
        A = rng.standard_normal((sz, sz))
        Kf = (A @ A.T / sz + np.eye(sz)).astype(np.float32)
        c.K.append(np.maximum(Kf, Kf.T))                      # exactly symmetric after the cast
    return c


def blocks_of(c, flat):
    off = np.concatenate([[0], np.cumsum(c.sizes ** 2)])
    return [flat[off[f]:off[f + 1]].reshape(c.sizes[f], c.sizes[f], order="F") for f in range(len(c.sizes))]


def test_decomposition_block_by_block(eng):
    c = spd_cohort([1, 2, 5, 33, 64, 2, 1, 64, 5, 33, 1, 5, 2], 31)
    U_flat, S, info = eng.kinship_decompose_families(c.fam_ptr, c.members, c.flat(c.K))
    assert info.sweeps == 0
    Ub = blocks_of(c, U_flat)
    for f, (Kf, u) in enumerate(zip(c.K, Ub)):
        s = S[c.fam_ptr[f]:c.fam_ptr[f + 1]].astype(np.float64)
        u = u.astype(np.float64)
        tol = 64 * 2.0 ** -23
        assert np.abs((u * s) @ u.T - Kf).max() <= tol * np.abs(Kf).max(), f
        assert np.abs(u.T @ u - np.eye(len(s))).max() <= tol * min(1.0, np.abs(Kf).max()), f
        assert (np.diff(s) >= 0).all(), f
    U_dense, S_dense, _ = eng.kinship_decompose(c.dense(c.K, square=True), want_vectors=False)
    assert rel(np.sort(S), np.sort(S_dense), 1e-6)


def test_decomposition_installs_through_the_family_form(eng):
    c = spd_cohort(np.random.default_rng(8).choice([1, 2, 3, 4, 6], size=260), 41)
    X, y, genes, _ = phenotype_and_genes(c.N, seed=9)
    U_flat, S, info = eng.kinship_decompose_families(c.fam_ptr, c.members, c.flat(c.K), install=True)
    assert eng.kinship_structure() < 0.02
    nul = eng.fit_fam_null(X, y)
    ptrs = [eng.upload_block(G) for G in genes]
    recs = eng.run_fam_blocks(ptrs, [G.shape[1] for G in genes])
    famskat_against_oracle(recs, nul, genes, X, y, c.dense(blocks_of(c, U_flat)), S)


# ---- 4. no N x N anywhere --------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_samples_install_and_rotate_in_under_a_gigabyte(eng):
    n_fam, k = 50000, 4
    N = n_fam * k
    rng = np.random.default_rng(51)
    fam_ptr = np.arange(0, N + 1, k, dtype=np.int64)
    members = (np.arange(n_fam)[:, None] + n_fam * np.arange(k)[None, :]).astype(np.int32)   # interleaved: family i holds i + r n_fam
    A = rng.uniform(0.1, 0.5, (n_fam, k, k))
    K = ((A + A.transpose(0, 2, 1)) / 2 + np.eye(k)).astype(np.float32)
    s, u = np.linalg.eigh(K.astype(np.float64))
    U32 = u.astype(np.float32)                                    # U32[f, r, j]
    flat = lambda B: np.ascontiguousarray(B.transpose(0, 2, 1)).ravel()   # column-major inside every block
    X = np.column_stack([np.ones(N), rng.standard_normal(N)])
    y = rng.standard_normal(N)
    G = rng.choice([0.0, 1.0, 2.0], size=(N, 8), p=[0.8, 0.15, 0.05])
    gm = G[members.ravel()].reshape(n_fam, k, 8)
    want = np.einsum("frj,frc->fjc", U32.astype(np.float64), gm).reshape(N, 8)
    bound = 2 * k * EPS * np.einsum("frj,frc->fjc", np.abs(U32).astype(np.float64), np.abs(gm)).reshape(N, 8)

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    eng.set_kinship_families(fam_ptr, members.ravel(), flat(U32), s.astype(np.float32).ravel())
    taken = free0 - torch.cuda.mem_get_info()[0]
    print("install of N = %d took %.1f MB of device memory" % (N, taken / 2 ** 20))
    assert taken <= 2 ** 30
    assert abs(eng.kinship_structure() - 4.0 / N) < 1e-15
    nul = eng.fit_fam_null(X, y)
    assert nul.brent_evals >= 4 and np.isfinite(nul.delta)
    ptr = eng.upload_block(G)
    got = eng.debug_rotate(ptr, 8)
    assert (np.abs(got - want) <= bound).all()
    eng.free_block(ptr)

    U_flat, S, info = eng.kinship_decompose_families(fam_ptr, members.ravel(), flat(K), install=True)
    assert free0 - torch.cuda.mem_get_info()[0] <= 2 ** 30
    assert rel(np.sort(S.reshape(n_fam, k), axis=1), s, 1e-5)     # float eigenvalues of well separated 4 x 4 blocks
    assert np.isfinite(eng.fit_fam_null(X, y).delta)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(eng):
    import rvtests_amd
    c = structure_cohort(False)
    c = Cohort(c.sizes[:60], 61, True)
    X, y, genes, _ = phenotype_and_genes(c.N, seed=62)
    c.install(eng)
    eng.fit_fam_null(X, y)
    ptr = eng.upload_block(genes[0])
    before = eng.run_fam_blocks([ptr], [genes[0].shape[1]])[0]

    def refused(fam_ptr, members, blocks, S, word):
        with pytest.raises(rvtests_amd.RvtError, match=word):
            eng.set_kinship_families(fam_ptr, members, blocks, S)

    big = np.array([0, 65, 70], dtype=np.int64)                   # a family of 65
    refused(big, np.arange(70), np.zeros(65 * 65 + 25, dtype=np.float32), np.ones(70, dtype=np.float32), "family 0 has 65")
    empty = c.fam_ptr.copy()
    empty[3] = empty[2]                                           # an empty family (its neighbour grows)
    sz = np.diff(empty)
    refused(empty, c.members, np.zeros(int((sz ** 2).sum()), dtype=np.float32), c.S, "family 2 is empty")
    dup = c.members.copy()
    dup[5] = dup[4]
    refused(c.fam_ptr, dup, c.flat(c.U), c.S, "listed twice")
    short = c.fam_ptr.copy()
    short[-1] -= 1                                                # fam_ptr[n_fam] != N
    refused(short, c.members, c.flat(c.U), c.S, "fam_ptr")
    nan = c.flat(c.U)
    nan[7] = np.nan
    refused(c.fam_ptr, c.members, nan, c.S, "non-finite")
    with pytest.raises(rvtests_amd.RvtError, match="non-finite"):
        eng.kinship_decompose_families(c.fam_ptr, c.members, nan)

    after = eng.run_fam_blocks([ptr], [genes[0].shape[1]])[0]     # the installed decomposition and null model are untouched
    assert (after.famskat_ok, after.famskat_Q, after.famskat_p) == (before.famskat_ok, before.famskat_Q, before.famskat_p)


def test_kinship_and_null_model_must_agree_in_N(eng):
    import rvtests_amd
    c = Cohort([2, 3, 4, 1] * 10, 63, True)
    X, y, _, _ = phenotype_and_genes(c.N + 5, seed=64)
    messages = []
    for install in (lambda: eng.set_kinship(c.dense(c.U), c.S), lambda: c.install(eng)):
        install()
        with pytest.raises(rvtests_amd.RvtError) as ei:
            eng.fit_fam_null(X, y)
        messages.append(str(ei.value))
    assert messages[0] == messages[1]


def write_kin_families(path, c, cut=0):
    blob = struct.pack("<qq", c.N, len(c.sizes)) + c.fam_ptr.astype("<i8").tobytes() + c.members.astype("<i4").tobytes() + \
        c.flat(c.U).astype("<f4").tobytes() + c.S.astype("<f4").tobytes()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) - cut])


def driver_case(tmp_path):
    sizes = np.random.default_rng(71).choice([1, 2, 3, 4, 6], size=600)
    n = int(np.searchsorted(np.cumsum(sizes), 600))               # families until 600 samples are reached; the last one is cut
    sizes = sizes[:n + 1]
    sizes[-1] -= sizes.sum() - 600
    c = Cohort(sizes, 72, True)
    X, y, _, _ = phenotype_and_genes(c.N, seed=73)
    _, G, af = synth.make_gene(c.N, 10, seed=74, missing=0.0, common=True, mono=True)
    path, sites = str(tmp_path / "in.bin"), str(tmp_path / "sites.txt")
    write_input(path, y, X[:, 1:], 0, [(G[:, :6], af[:6]), (G[:, 6:], af[6:])])
    with open(sites, "w") as f:
        for j in range(G.shape[1]):
            f.write("1 %d\n" % (500 + j))
    return c, path, sites


def run_kin_families(path, sites, single, kin):
    p = subprocess.run([DRIVER, path, "-", "-", "-", sites, "--single", single, "--kin-families", kin],
                       capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_driver_kin_families_prints_the_rows_of_the_dense_file(tmp_path):
    _ensure_driver()
    c, path, sites = driver_case(tmp_path)
    assert c.N == 600
    dense, fam = str(tmp_path / "kin.bin"), str(tmp_path / "kinfam.bin")
    write_kinship(dense, c.dense(c.U), c.S)
    write_kin_families(fam, c)
    rc0, sec0, err0 = run_single_fam(path, sites, "famscore", dense)
    assert rc0 == 0, err0
    rc1, out1, err1 = run_kin_families(path, sites, "famscore", fam)
    assert rc1 == 0, err1
    rows0 = sec0["out.FamScore.assoc"]
    rows1 = out1.split("== out.FamScore.assoc\n")[1].splitlines()[:len(rows0)]
    assert len(rows0) == 11 and rows1 == rows0
    assert sum(r.split("\t")[-1] != "NA" for r in rows0[1:]) >= 8


def test_driver_refuses_a_truncated_kin_families_file(tmp_path):
    _ensure_driver()
    c, path, sites = driver_case(tmp_path)
    fam = str(tmp_path / "kinfam.bin")
    write_kin_families(fam, c, cut=10)
    rc, out, err = run_kin_families(path, sites, "famscore", fam)
    assert rc == 1 and "bad kinship file" in err
