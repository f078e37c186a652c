"""rvt_grammar_bed_dev without a GPU: the arithmetic it shares with the host harness (rvtests_amd/csrc/rvt_grammar_bed.h through
hc_grammar_ty_planes, hc_grammar_bed_finish, hc_grammar_bed_plan) against numpy — the digit planes of ty, a row's statistics from
its counts and integer plane sums against GrammarGamma's statement on the imputed column, and the launch plan's cover."""
import itertools

import numpy as np
import pytest

import fam_bed_cases
import grammar_bed_cases as gb
from test_single_fam_cpu import grammar_test


def ty_cases(N=1000):
    rng = np.random.default_rng(20240611)
    normal = rng.standard_normal(N) * 0.37
    spike = rng.standard_normal(N) * 1e-3
    spike[N // 3] = -2.0 ** 20 * 1e-3 * 1.2345
    pow2 = rng.uniform(-1, 1, N) * 0.25
    pow2[7] = -0.5                                        # max |ty| an exact power of two
    return dict(normal=normal, spike=spike, zero=np.zeros(N), pow2=pow2)


@pytest.mark.parametrize("name", ["normal", "spike", "zero", "pow2"])
def test_planes_of_ty(name):
    ty = ty_cases()[name]
    planes, e, totals = gb.ty_planes(ty)
    assert planes.dtype == np.int8
    tmax = float(np.abs(ty).max())
    if tmax == 0.0:
        assert not planes.any() and not totals.any()
        return
    assert tmax < 2.0 ** e and tmax >= 2.0 ** (e - 1)     # e is the smallest exponent with max |ty| < 2^e
    assert (planes[1:] >= 0).all() and planes[0].min() >= -64 and planes[0].max() <= 63
    q = gb.planes_q(planes)
    for i, qi in enumerate(q):                            # the top digit carries the sign
        assert (planes[0, i] < 0) == (qi < 0)
    from fractions import Fraction
    ulp = Fraction(2) ** (e - 55)
    worst = Fraction(0)
    for i, qi in enumerate(q):
        err = abs(Fraction(float(ty[i])) - qi * ulp)
        worst = max(worst, err)
        assert err <= ulp / 2, (i, ty[i])                 # 2^(e - 56) per entry
    big = int(np.argmax(np.abs(ty)))
    assert Fraction(float(ty[big])) == q[big] * ulp       # exact for the largest entry
    assert np.array_equal(totals, planes.astype(np.int64).sum(1))
    print("%s: e = %d, worst digit error %.3g of 2^(e - 56)" % (name, e, float(worst / (ulp / 2))))


def test_planes_refuse_a_vector_that_is_not_finite():
    ty = ty_cases()["normal"].copy()
    ty[5] = np.inf
    assert gb.ty_planes(ty) is None
    ty[5] = np.nan
    assert gb.ty_planes(ty) is None


@pytest.mark.parametrize("N", [237, 515])
def test_row_arithmetic_against_the_statement_on_the_imputed_column(N):
    raw = fam_bed_cases.calls(N, 37, seed=1234)
    rows = fam_bed_cases.pack(raw)                        # (every padding bit set)
    rng = np.random.default_rng(77 + N)
    ty = rng.standard_normal(N) * 0.41
    gamma, ysy = 1.37, 55.5
    planes, e, totals = gb.ty_planes(ty)
    sums = gb.integer_sums(rows, N, planes)
    cnt = fam_bed_cases.site_pass(raw)[0]
    n1, n2, nm = gb.counts_of(sums)
    assert np.array_equal(n1, cnt[:, 1]) and np.array_equal(n2, cnt[:, 2]) and np.array_equal(nm, cnt[:, 3])
    got = gb.finish(cnt, sums, totals, e, gamma, ysy)
    tested, refused = gb.check_against_statement(got, raw, ty, gamma, ysy, grammar_test, what="N = %d" % N)
    assert tested >= 10 and refused >= 4
    hand = got["ok"][-len(fam_bed_cases.HAND_ROWS):]
    assert list(hand) == [0, 0, 0, 0, 0, 1, 1]            # the five monomorphic kinds refused, the other two tested
    poly = fam_bed_cases.site_pass(raw)[3]
    assert np.array_equal(got["ok"] == 1, poly)


OVERRIDES = [(0, 0), (64, 0), (100, 0), (10 ** 7, 0), (0, 1), (0, 3), (192, 5), (0, 1000)]


@pytest.mark.parametrize("cus", [1, 256])
def test_plan_covers_every_row_and_sample_once(cus):
    for N, V, (sl, tl) in itertools.product((1, 3, 64, 237, 515, 20000, 500000), (1, 31, 32, 33, 1024, 4096), OVERRIDES):
        P = gb.plan(N, V, cus, sl, tl)
        assert P["kstep"] == gb.KSTEP
        npad = (N + 63) // 64 * 64
        assert P["npad"] == npad and P["row_tiles"] == (V + 15) // 16
        # the slices tile [0, npad): each a multiple of the K-step, the last one shorter at most, none empty
        assert P["slice"] % gb.KSTEP == 0 and P["slice"] >= gb.KSTEP
        starts = np.arange(P["slices"], dtype=np.int64) * P["slice"]
        ends = np.minimum(starts + P["slice"], npad)
        assert starts[0] == 0 and ends[-1] == npad and (ends > starts).all() and np.array_equal(starts[1:], ends[:-1])
        # the row tiles: groups of `tiles` consecutive tiles, every tile in exactly one group
        assert 1 <= P["tiles"] and P["groups"] >= 1
        assert P["groups"] * P["tiles"] >= P["row_tiles"] > (P["groups"] - 1) * P["tiles"]
        assert 127 * P["slice"] < 2 ** 31                  # int32 accumulators
        assert 9 * P["slice"] <= 64 * 1024                 # the staged B slice
        if sl and sl <= 7168:
            assert P["slice"] == min((sl + 63) // 64 * 64, npad)
        if tl:
            assert P["tiles"] == min(tl, 64, P["row_tiles"])
    assert gb.plan(515, 71, cus, 64)["slices"] == 9 and gb.plan(515, 71, cus, 128)["slices"] == 5
