"""What the tests of rvt_grammar_bed_dev share (tests/test_grammar_bed_cpu.py, tests/test_gpu_grammar_bed.py): the bit planes of
packed rows in numpy, the integer sums the device's product has to return, the loader of the three hc_grammar_* exports of the
host harness, and the comparison of a result with the numpy statement at the tolerances the block route is held to."""
import ctypes as C

import numpy as np

import fam_bed_cases
import hc

KSTEP = 64
PLANES = 8
WEIGHTS = [1 << (7 * (PLANES - 1 - p)) for p in range(PLANES)]    # 128^(7 - p)


def lib():
    L = hc.lib()
    ll, i, d, vp = C.c_longlong, C.c_int, C.c_double, C.c_void_p
    L.hc_grammar_ty_planes.restype = i
    L.hc_grammar_ty_planes.argtypes = [vp, ll, vp, C.POINTER(i), vp]
    L.hc_grammar_bed_finish.restype = i
    L.hc_grammar_bed_finish.argtypes = [ll, ll, ll, ll, vp, vp, i, d, d, vp]
    L.hc_grammar_bed_plan.restype = i
    L.hc_grammar_bed_plan.argtypes = [ll, ll, i, ll, i, vp]
    return L


def ty_planes(ty):
    """(planes (8, N) int8, e, totals (8) int64) of hc_grammar_ty_planes, or None when it refuses ty."""
    ty = np.ascontiguousarray(ty, dtype=np.float64)
    N = len(ty)
    planes = np.zeros((PLANES, N), dtype=np.int8)
    totals = np.zeros(PLANES, dtype=np.int64)
    e = C.c_int(0)
    ok = lib().hc_grammar_ty_planes(ty.ctypes.data, N, planes.ctypes.data, C.byref(e), totals.ctypes.data)
    return (planes, e.value, totals) if ok else None


def planes_q(planes):
    """The 56-bit integers the digits stand for, exactly (python ints)."""
    return [sum(int(planes[p, i]) * WEIGHTS[p] for p in range(PLANES)) for i in range(planes.shape[1])]


def planes_value(planes, e):
    """q 2^(e - 55) as doubles (|q| < 2^55: the conversion rounds at 2^-53 relative, far below what the callers ask)."""
    q = np.zeros(planes.shape[1], dtype=np.int64)
    for p in range(PLANES):
        q += planes[p].astype(np.int64) * WEIGHTS[p]
    return np.ldexp(q.astype(np.float64), e - 55)


def bit_planes(rows, N):
    """H = hi bits, L = lo bits, HL = hi & lo of packed rows (V, ceil(N / 4)) as (3, V, N) int64; samples >= N dropped, so
    whatever the padding pairs hold is gone."""
    V = rows.shape[0]
    pairs = np.stack([(rows >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(V, -1)[:, :N].astype(np.int64)
    lo, hi = pairs & 1, pairs >> 1
    return np.stack([hi, lo, hi & lo])


def integer_sums(rows, N, planes):
    """(V, 3, 9) int64: H, L, HL of every row against the eight planes and a column of ones."""
    X = bit_planes(rows, N)
    B = np.column_stack([planes.astype(np.int64).T, np.ones(N, dtype=np.int64)])
    return np.ascontiguousarray(np.einsum("ovn,nc->voc", X, B))


def counts_of(sums):
    """n0 n1 n2 missing from the ones column: sum H = n1 + n2, sum L = missing + n2, sum HL = n2 (N is not needed for three)."""
    sH, sL, sHL = sums[:, 0, 8], sums[:, 1, 8], sums[:, 2, 8]
    return sH - sHL, sHL, sL - sHL


def finish(cnt, sums, totals, e, gamma, ysy):
    """hc_grammar_bed_finish per row: dict of ok, af, beta, beta_var, p."""
    V = cnt.shape[0]
    out = dict(ok=np.zeros(V, dtype=np.int32), af=np.zeros(V), beta=np.zeros(V), beta_var=np.zeros(V), p=np.zeros(V))
    L = lib()
    totals = np.ascontiguousarray(totals, dtype=np.int64)
    for v in range(V):
        S = np.ascontiguousarray(sums[v, :, :PLANES], dtype=np.int64)
        o = np.zeros(4)
        out["ok"][v] = L.hc_grammar_bed_finish(int(cnt[v, 0]), int(cnt[v, 1]), int(cnt[v, 2]), int(cnt[v, 3]), S.ctypes.data,
                                               totals.ctypes.data, int(e), float(gamma), float(ysy), o.ctypes.data)
        out["af"][v], out["beta"][v], out["beta_var"][v], out["p"][v] = o
    return out


def plan(N, V, cus, slice_req=0, tiles_req=0):
    o = np.zeros(6, dtype=np.int64)
    k = lib().hc_grammar_bed_plan(int(N), int(V), int(cus), int(slice_req), int(tiles_req), o.ctypes.data)
    return dict(kstep=k, npad=int(o[0]), slice=int(o[1]), slices=int(o[2]), row_tiles=int(o[3]), tiles=int(o[4]), groups=int(o[5]))


def check_against_statement(got, raw, ty, gamma, ysy, grammar_test, kin=(), what=""):
    """got (dict of ok, af, beta, beta_var, p) against grammar_test on the imputed columns of raw.  ok equal everywhere; where ok
    the tolerances of test_gpu_single_fam.check_grammar — af 1e-8, beta and beta_var 1e-7, p 1e-6, relative — and for beta also
    the floor B / (gg gamma), B = (n1 + 2 n2 + mu nm) max|ty| 2^-50: the rounding of either route's sum of n products of that
    size (8 ulp of the sum of the magnitudes), which is all that is left of beta for a variant whose g'ty cancels.  Returns
    (tested, refused) and prints the worst ratio of a difference to what it is allowed."""
    G = fam_bed_cases.imputed(raw)
    cnt, mu, _, _ = fam_bed_cases.site_pass(raw)
    tmax = float(np.abs(ty).max())
    tested = refused = 0
    worst = dict(af=0.0, beta=0.0, beta_var=0.0, p=0.0)
    for h in range(G.shape[1]):
        ok, af, b, bv, p = grammar_test(G[:, h], gamma, ty, ysy, *kin)
        assert got["ok"][h] == ok, (what, h, got["ok"][h], ok)
        allowed = 1e-8 * abs(af) + 1e-300
        worst["af"] = max(worst["af"], abs(got["af"][h] - af) / allowed)
        assert abs(got["af"][h] - af) <= allowed, (what, h, got["af"][h], af)
        if not ok:
            refused += 1
            assert np.isnan(got["beta"][h]) and np.isnan(got["beta_var"][h]) and np.isnan(got["p"][h])
            continue
        tested += 1
        gc = G[:, h] - G[:, h].mean()
        gg = float(gc @ gc)
        n1, n2, nm = (int(cnt[h, k]) for k in (1, 2, 3))
        floor = (n1 + 2 * n2 + mu[h] * nm) * tmax * 2.0 ** -50 / (gg * gamma)
        for f, ref, allowed in (("beta", b, 1e-7 * abs(b) + floor), ("beta_var", bv, 1e-7 * abs(bv)), ("p", p, 1e-6 * abs(p) + 1e-300)):
            worst[f] = max(worst[f], abs(got[f][h] - ref) / allowed)
            assert abs(got[f][h] - ref) <= allowed, (what, f, h, got[f][h], ref)
    print("%s: %d tested, %d refused; worst difference / allowed: %s" %
          (what, tested, refused, ", ".join("%s %.3g" % kv for kv in worst.items())))
    return tested, refused
