"""GPU: the multiple-trait score test over rows of a resident .bed matrix (rvt_mt_score_bed_dev) against the fp64 numpy statement
of tests/mtscore_ref.py on the mean-imputed columns of the same calls, and against rvt_mt_score_block bit for bit where the two
routes run the same products.

Traits and tests: mtscore_ref.base_input(N); rows: fam_bed_cases.calls(N, 30, seed=77) — 30 drawn rows (2 % missing, a flipped
frequency, monomorphic ones) and the seven hand rows — packed with every padding bit set and uploaded one row into the matrix,
so that rows start at odd addresses where the pitch is odd.

Tolerance: that of tests/test_gpu_mtscore.py — REL = 1e-6 for V and p, for U 1e-6 plus a floor of 1e-9 times the largest term
of the cell, NaN exactly where the statement has NaN.  The branch pattern of the inputs is not decided by rounding (asserted)."""
import ctypes as C

import numpy as np
import pytest

import fam_bed_cases
import mtscore_bed_cases as cases
import mtscore_ref as mt

pytestmark = pytest.mark.gpu

REL = 1e-6
FLOOR = 1e-9
SIZES = (1497, 1502, 20000)      # odd pitch and three padding pairs; two padding pairs; several pass row blocks and K chunks
KEYS = ("U", "V", "p")


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
    return {N: cases.case(N) for N in SIZES}


def check(dev, ref, what=""):
    U, V, P, terms = ref[:4]
    worst = {}
    for name, got, want, floor in (("U", dev["U"], U, FLOOR * terms), ("V", dev["V"], V, None), ("p", dev["p"], P, None)):
        ok, w = mt.close_cells(got, want, REL, floor)
        worst[name] = w
        print("%s %s: worst error / tolerance %.3g" % (what, name, w))
    assert all(w <= 1.0 for w in worst.values()), (what, worst)


def pick(ref, sel):
    return tuple(a[sel] for a in ref[:4])


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(a[k][rows_a].view(np.uint64), b[k][rows_b].view(np.uint64)) for k in KEYS)


def run_bed(eng, rows, lead=1):
    """rows (V, pitch) uploaded `lead` rows into a fresh resident matrix and scored there"""
    V, pitch = rows.shape
    d_bed = eng.bed_alloc(lead + V + 1)
    eng.bed_upload(d_bed, lead, rows)
    out = eng.mt_score_bed_dev(d_bed + lead * pitch, V)
    eng.bed_free(d_bed)
    return out


def fitted(eng, case):
    eng.mt_fit_null(case["Y"], case["Z"], case["tests"])
    return eng


@pytest.mark.parametrize("N", SIZES)
def test_statement_parity(engine_factory, base, N):
    case = base[N]
    dist, zero_v_is_mono, n_ok = cases.branch_margin(case)
    print("N=%d: nm at least %.3g of the threshold away from it, %d tests ok" % (N, dist, n_ok))
    assert dist >= cases.MARGIN and zero_v_is_mono and n_ok == 7
    assert case["rows"].shape == (cases.ROWS, (N + 3) // 4)
    out = run_bed(fitted(engine_factory(), case), case["rows"])
    check(out, case["ref"], "N=%d" % N)
    assert np.array_equal(out["counts"], fam_bed_cases.site_pass(case["raw"])[0])
    assert np.isnan(out["p"]).any() and np.isfinite(out["p"]).any()


def test_no_missing_call_is_the_block_call_bit_for_bit(engine_factory, base):
    for N in (1497, 20000):
        case = base[N]
        keep = np.flatnonzero(~(case["raw"] < 0).any(0))
        assert len(keep) >= 2 and (case["G"][:, keep].min(0) != case["G"][:, keep].max(0)).any()
        eng = fitted(engine_factory(), case)
        bed = run_bed(eng, case["rows"][keep])
        assert (bed["counts"][:, 3] == 0).all()
        G = np.ascontiguousarray(case["G"][:, keep])
        ptr = eng.upload_block(G)
        blk = eng.mt_score_block(ptr, len(keep))
        eng.free_block(ptr)
        assert same_bits(bed, blk), N
        check(bed, pick(case["ref"], keep), "N=%d rows without a missing call" % N)


def test_the_c_half_does_not_see_the_m_half(engine_factory, base):
    case = base[1497]
    rows = case["rows"]
    miss = (case["raw"] < 0).any(0)
    keep = np.flatnonzero(~miss)
    eng = fitted(engine_factory(), case)
    a = run_bed(eng, rows)
    b = run_bed(eng, rows)
    assert same_bits(a, b)
    swapped = rows.copy()
    swapped[miss] = rows[keep[-1]]                     # every row with a missing call becomes a copy of one without
    s = run_bed(eng, swapped)
    assert (s["counts"][:, 3] == 0).all()
    assert same_bits(a, s, keep, keep)
    assert same_bits(s, s, np.flatnonzero(miss), np.full(int(miss.sum()), keep[-1]))


def test_edges_of_the_piece_and_of_the_compaction(engine_factory, base):
    case = base[1497]
    rows, ref = case["rows"], case["ref"]
    miss = (case["raw"] < 0).any(0)
    keep, lost = np.flatnonzero(~miss), np.flatnonzero(miss)
    eng = fitted(engine_factory(), case)
    for j in (int(lost[0]), int(keep[-1])):                                   # V = 1: a row with a missing call, one without
        for lead in (0, 1):
            check(run_bed(eng, rows[[j]], lead), pick(ref, [j]), "V=1, row %d, lead %d" % (j, lead))
    # a full piece followed by a ragged one, the 37 rows tiled: a copy gives the same bits wherever it lies
    V = 1024 + 70
    sel = np.arange(V) % cases.ROWS
    a = run_bed(eng, rows[sel])
    check(a, pick(ref, sel), "tiled")
    for k in KEYS:
        for j in range(cases.ROWS):
            copies = a[k][sel == j].view(np.uint64)
            assert np.all(copies == copies[0]), (k, j)
    assert np.array_equal(a["counts"], fam_bed_cases.site_pass(case["raw"])[0][sel])
    # the first piece without a missing call (no m product), the second with
    sel2 = np.concatenate([keep[np.arange(1024) % len(keep)], np.arange(70) % cases.ROWS])
    b = run_bed(eng, rows[sel2])
    assert (b["counts"][:1024, 3] == 0).all() and (b["counts"][1024:, 3] != 0).any()
    check(b, pick(ref, sel2), "no m product, then one")
    assert same_bits(b, a, slice(1024, V), slice(0, 70))                      # (the rows the tiled call began with)
    # exactly one row of the piece has a missing call
    sel3 = keep[np.arange(21) % len(keep)].copy()
    sel3[7] = lost[3]
    c = run_bed(eng, rows[sel3])
    assert int((c["counts"][:, 3] != 0).sum()) == 1
    check(c, pick(ref, sel3), "one row with a missing call")
    assert same_bits(c, a, [7], [int(lost[3])])


@pytest.mark.parametrize("env,value", [("RVT_ROT_KMAX", "256"), ("RVT_ROT_SLICES", "3")])
def test_range_cut_and_slices(engine_factory, monkeypatch, base, env, value):
    monkeypatch.setenv(env, value)
    case = base[1497]
    out = run_bed(fitted(engine_factory(), case), case["rows"])
    check(out, case["ref"], "%s=%s" % (env, value))


def test_nothing_depends_on_what_a_work_space_held(engine_factory, monkeypatch, base):
    """Fresh allocations filled with 0xFF and every reused work space refilled with 0xAA in front of the call: the same bits."""
    case = base[1497]
    rows = case["rows"]
    keep = np.flatnonzero(~(case["raw"] < 0).any(0))
    plain = run_bed(fitted(engine_factory(), case), rows)
    monkeypatch.setenv("RVT_POISON", "255")
    monkeypatch.setenv("RVT_SCRIBBLE", "170")
    eng = fitted(engine_factory(), case)
    first = run_bed(eng, rows)
    run_bed(eng, rows[keep])                           # (a narrower piece without an m product in between)
    second = run_bed(eng, rows)
    assert same_bits(first, plain) and same_bits(second, plain)
    assert np.array_equal(second["counts"], plain["counts"])


def test_tile_edges(engine_factory):
    """The 304 resident value rows and 300 patterns of tests/test_gpu_mtscore.py::test_tile_edges (ragged 256-row panels) against
    260 rows of which the last 5 carry missing calls: two column tiles for c, a 5-column m."""
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
    raw = rng.binomial(2, rng.uniform(0.002, 0.5, V), (N, V)).astype(float)
    raw[:, V - 5:][rng.random((N, 5)) < 0.03] = -9.0
    eng = engine_factory()
    nul = eng.mt_fit_null(Y, Z, tests)
    rn = mt.fit_null(Y, Z, tests)
    assert nul["ok"].tolist() == rn["ok"].tolist()
    out = run_bed(eng, fam_bed_cases.pack(raw))
    assert (out["counts"][:V - 5, 3] == 0).all() and (out["counts"][V - 5:, 3] > 0).all()
    check(out, mt.score(Y, Z, tests, fam_bed_cases.imputed(raw), want_terms=True, null=rn), "tile edges")


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_state_and_isolation(engine_factory, base):
    import rvtests_amd
    import synth
    case = base[1497]
    N, rows = 1497, case["rows"]
    V, pitch, T = rows.shape[0], rows.shape[1], len(case["tests"])
    eng = engine_factory()

    def refused(e, d_rows, nv, code, null_p=False):
        """the raw call with sentinel-filled outputs: the code, and nothing written"""
        outs = [np.full((V, T), 7.25) for _ in range(3)]
        cnt = np.full((V, 4), -3, dtype=np.int64)
        rc = e.L.rvt_mt_score_bed_dev(e.ctx, C.c_void_p(int(d_rows)), nv, dp(outs[0]), dp(outs[1]), None if null_p else dp(outs[2]),
                                      cnt.ctypes.data_as(C.c_void_p))
        assert rc == code, rc
        assert all((o == 7.25).all() for o in outs) and (cnt == -3).all()

    with pytest.raises(rvtests_amd.RvtError, match="error -4"):               # no model at all: the pitch is unknown
        eng.bed_alloc(4)
    refused(eng, 1 << 20, 1, -4)                                              # before mt_fit_null
    fitted(eng, case)
    d_bed = eng.bed_alloc(V + 2)                                              # a context whose only model is the multiple-trait null
    eng.bed_upload(d_bed, 1, rows)
    d_rows = d_bed + pitch
    refused(eng, d_rows, 0, -1)
    refused(eng, 0, V, -1)
    refused(eng, d_rows, V, -1, null_p=True)
    first = eng.mt_score_bed_dev(d_rows, V)
    check(first, case["ref"], "mt-only context")
    # beside a fitted null of the same N: score_bed_dev before and after the new call, and on a fresh context — the same bits
    X, y, res, v, s2 = synth.make_null(N, 3, 0, seed=9)
    eng.fit_null(0, X, y)
    before = eng.score_bed_dev(d_rows, V)
    again = eng.mt_score_bed_dev(d_rows, V)
    assert same_bits(first, again) and np.array_equal(first["counts"], again["counts"])
    after = eng.score_bed_dev(d_rows, V)
    fresh = engine_factory()
    fresh.fit_null(0, X, y)
    d2 = fresh.bed_alloc(V + 2)
    fresh.bed_upload(d2, 1, rows)
    alone = fresh.score_bed_dev(d2 + pitch, V)
    fresh.bed_free(d2)
    for got in (before, after):
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[6], alone[6])
        for k in range(1, 6):
            assert np.array_equal(got[k].view(np.uint64), alone[k].view(np.uint64)), k
    # a null model of another N beside it: the rows would have another pitch
    X2, y2 = synth.make_null(N + 4, 3, 0, seed=10)[:2]
    eng.fit_null(0, X2, y2)
    refused(eng, d_rows, V, -4)
    eng.fit_null(0, X, y)
    assert same_bits(first, eng.mt_score_bed_dev(d_rows, V))
    eng.mt_clear()
    refused(eng, d_rows, V, -4)                                               # after mt_clear
    eng.bed_free(d_bed)
