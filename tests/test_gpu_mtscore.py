"""GPU: the multiple-trait score test (rvt_mt_fit_null / rvt_mt_score_block, `--single fastmtscore`) against the fp64 numpy
statement of tests/mtscore_ref.py.

Tolerance (all tests): REL = 1e-6 — the project's north-star tolerance — element by element for V and p; for U rtol = 1e-6 with an
absolute floor of 1e-9 times the largest |term| of the cell (|GYZ[:, y] scale_xy| or |xz zz_inv zy|: the two may cancel); NaN
exactly where the statement has NaN."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mtscore_ref as mt
from test_host_driver import DRIVER, write_input

pytestmark = pytest.mark.gpu

REL = 1e-6
FLOOR = 1e-9
SIZES = (1500, 20000)


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


@pytest.fixture(scope="module")
def base():
    out = {}
    for N in SIZES:
        Y, Z, tests, G = mt.base_input(N)
        nul = mt.fit_null(Y, Z, tests)
        out[N] = dict(Y=Y, Z=Z, tests=tests, G=G, nul=nul, ref=mt.score(Y, Z, tests, G, want_terms=True, null=nul))
    return out


def check(dev, ref, what=""):
    U, V, P, terms = ref[:4]
    worst = {}
    for name, got, want, floor in (("U", dev["U"], U, FLOOR * terms), ("V", dev["V"], V, None), ("p", dev["p"], P, None)):
        ok, w = mt.close_cells(got, want, REL, floor)
        worst[name] = w
        print("%s %s: worst error / tolerance %.3g" % (what, name, w))
    assert all(w <= 1.0 for w in worst.values()), (what, worst)


def run(eng, case, G=None):
    nul = eng.mt_fit_null(case["Y"], case["Z"], case["tests"])
    G = case["G"] if G is None else G
    ptr = eng.upload_block(G)
    out = eng.mt_score_block(ptr, G.shape[1])
    eng.free_block(ptr)
    return nul, out


@pytest.mark.parametrize("N", SIZES)
def test_device_matches_statement(engine_factory, base, N):
    case = base[N]
    nul, out = run(engine_factory(), case)
    ref = case["nul"]
    assert nul["ok"].tolist() == ref["ok"].tolist()
    assert nul["obs"].tolist() == ref["obs"].tolist()                       # exact
    ok, w = mt.close_cells(nul["sigma2"], ref["sigma2"], REL)
    assert ok, (nul["sigma2"], ref["sigma2"])
    check(out, case["ref"], "N=%d" % N)
    # a piece of hard calls alone: the one-plane path of the same columns
    hard = list(range(10)) + [12, 13]
    eng = engine_factory()
    _, out_h = run(eng, case, np.ascontiguousarray(case["G"][:, hard]))
    check(out_h, tuple(a[hard] for a in case["ref"][:4]), "N=%d hard calls" % N)


def test_tile_edges(engine_factory):
    """304 resident value rows and 300 patterns (ragged 256-row panels), 260 hard-call columns (one column tile and four)."""
    N, P, Q, V = 1500, 300, 4, 260
    rng = np.random.default_rng(5)
    Zs = rng.standard_normal((N, Q))
    Z = Zs * [1.0, 3.0, 0.2, 10.0] + [0.0, 100.0, -5.0, 40.0]
    Y = (rng.standard_normal((N, P)) + 0.4 * Zs[:, [1]]) * rng.uniform(0.1, 100.0, P) + rng.uniform(-1e3, 1e3, P)
    for j in range(P):
        Y[rng.random(N) < rng.uniform(0.0, 0.5), j] = np.nan
    Z[rng.random(N) < 0.05, 2] = np.nan
    sets = ([], [0], [1, 2], [0, 1, 2, 3], [3, 0])
    tests = [(j, sets[j % len(sets)]) for j in range(P)]
    G = rng.binomial(2, rng.uniform(0.002, 0.5, V), (N, V)).astype(float)
    case = dict(Y=Y, Z=Z, tests=tests, G=G)
    nul, out = run(engine_factory(), case)
    rn = mt.fit_null(Y, Z, tests)
    assert nul["ok"].tolist() == rn["ok"].tolist() and nul["obs"].tolist() == rn["obs"].tolist()
    check(out, mt.score(Y, Z, tests, G, want_terms=True, null=rn), "tile edges")


@pytest.mark.parametrize("env,value", [("RVT_ROT_KMAX", "256"), ("RVT_ROT_SLICES", "3")])
def test_range_cut_and_slices(engine_factory, monkeypatch, base, env, value):
    monkeypatch.setenv(env, value)
    case = base[1500]
    nul, out = run(engine_factory(), case)
    assert nul["obs"].tolist() == case["nul"]["obs"].tolist()
    check(out, case["ref"], "%s=%s" % (env, value))


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("U", "V", "p"))


def test_determinism_and_placement(engine_factory, base):
    case = base[1500]
    G = case["G"]
    eng = engine_factory()
    eng.mt_fit_null(case["Y"], case["Z"], case["tests"])
    # one piece plus 70 columns of the 14 base columns, tiled: a copy gives the same bits wherever it lies
    V = 1024 + 70
    cols = np.arange(V) % 14
    ptr = eng.upload_block(np.ascontiguousarray(G[:, cols]))
    a = eng.mt_score_block(ptr, V)
    b = eng.mt_score_block(ptr, V)
    assert same_bits(a, b)
    for k in ("U", "V", "p"):
        for j in range(14):
            rows = a[k][cols == j].view(np.uint64)
            assert np.all(rows == rows[0]), (k, j)
    check({k: a[k][:14] for k in a}, case["ref"], "tiled")
    eng.free_block(ptr)
    # a piece of hard calls only next to a piece that holds the dosage column: different planes, the same numbers within the tolerance
    hard = np.array(list(range(10)) + [12, 13])
    cols2 = np.concatenate([hard[np.arange(1024) % len(hard)], np.arange(70) % 14])
    ptr = eng.upload_block(np.ascontiguousarray(G[:, cols2]))
    c = eng.mt_score_block(ptr, V)
    eng.free_block(ptr)
    ref = tuple(r[cols2] for r in case["ref"][:4])
    check(c, ref, "hard-call piece + dosage piece")
    for j in hard:
        first, second = np.flatnonzero(cols2[:1024] == j)[0], 1024 + np.flatnonzero(cols2[1024:] == j)[0]
        pair = tuple(r[[j]] for r in case["ref"][:4])
        for i in (first, second):
            check({k: c[k][[i]] for k in c}, pair, "column %d at %d" % (j, i))


def test_state_and_isolation(engine_factory, base):
    import rvtests_amd
    import synth
    case = base[1500]
    N = 1500
    G = case["G"]
    eng = engine_factory()
    # a context with only the multiple-trait null: not before it, then blocks work
    with pytest.raises(rvtests_amd.RvtError, match="error -4"):
        eng.alloc_block(2)
    eng.N = N
    with pytest.raises(rvtests_amd.RvtError, match="error -4"):
        eng.mt_score_block(1 << 20, 1)
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.mt_fit_null(case["Y"], case["Z"], [(0, [4])])
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.mt_fit_null(case["Y"], case["Z"], [(6, [])])
    nul, out = run(eng, case)
    check(out, case["ref"], "mt-only context")
    # fit_null + score_block on this context (it holds a multiple-trait null and has just run it) and on a fresh one: same bits
    X, y, res, v, s2 = synth.make_null(N, 3, 0, seed=9)
    Gh = np.ascontiguousarray(G[:, :10])
    outs = []
    for e in (eng, engine_factory()):
        if e is eng:
            ptr = e.upload_block(G)
            e.mt_score_block(ptr, 14)
            e.free_block(ptr)
        e.fit_null(0, X, y)
        ptr = e.upload_block(Gh)
        outs.append(e.score_block(ptr, 10))
        e.free_block(ptr)
    for k in ("U", "V", "effect", "se", "p"):
        assert np.array_equal(outs[0][k].view(np.uint64), outs[1][k].view(np.uint64)), k
    assert np.array_equal(outs[0]["ok"], outs[1]["ok"])
    # ... and the multiple-trait null is still there beside the other one
    ptr = eng.upload_block(G)
    check(eng.mt_score_block(ptr, 14), case["ref"], "beside a fitted null")
    eng.mt_clear()
    with pytest.raises(rvtests_amd.RvtError, match="error -4"):
        eng.mt_score_block(ptr, 14)
    eng.free_block(ptr)


def fmt(x):
    return "nan" if np.isnan(x) else "%g" % x


def test_driver(engine_factory, base, tmp_path):
    """host_driver --single fastmtscore over 30 sites in blocks of 8 (three full blocks and a tail) and in one block: the header,
    one row per site in file order, every field formatG of the ABI's number."""
    case = base[1500]
    N = 1500
    G = np.ascontiguousarray(case["G"][:, np.arange(30) % 14])
    Y, Z, tests = case["Y"], case["Z"], case["tests"]
    path = str(tmp_path / "in.bin")
    write_input(path, np.zeros(N), np.zeros((N, 0)), 0, [(G[:, :11], np.full(11, 0.1)), (G[:, 11:], np.full(19, 0.1))])
    mp = str(tmp_path / "mp.bin")
    with open(mp, "wb") as f:
        f.write(struct.pack("<qiii", N, Y.shape[1], Z.shape[1], len(tests)))
        f.write(np.asfortranarray(Y, dtype="<f8").tobytes(order="F"))
        f.write(np.asfortranarray(Z, dtype="<f8").tobytes(order="F"))
        for y, zs in tests:
            f.write(struct.pack("<ii%di" % len(zs), y, len(zs), *zs))
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        for i in range(30):
            f.write("%d %d\n" % (1 + i // 20, 1000 + 7 * i))
    eng = engine_factory()
    _, out = run(eng, case, G)
    texts = []
    for block in ("8", "1024"):
        env = dict(os.environ, RVT_SINGLE_BLOCK=block)
        p = subprocess.run([DRIVER, path, "-", "-", "-", sites, "--single", "fastmtscore", "--multi-pheno", mp], capture_output=True,
                           text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr
        texts.append(p.stdout)
    assert texts[0] == texts[1]
    lines = texts[0].splitlines()
    assert lines[0] == "== out.FastMultipleTraitScore.assoc"
    assert lines[1].split("\t") == ["CHROM", "POS", "U_STAT", "V_STAT", "PVALUE"]
    rows = [ln.split("\t") for ln in lines[2:]]
    assert len(rows) == 30
    for i, r in enumerate(rows):
        assert r[:2] == [str(1 + i // 20), str(1000 + 7 * i)]
        for field, M in zip(r[2:], (out["U"], out["V"], out["p"])):
            assert field == ",".join(fmt(x) for x in M[i]), (i, field)
