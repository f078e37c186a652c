"""Reference for the kinship rotation G~ = U'G (rvtests_amd/csrc/rot_gemm.hip.h, rotate_columns in rvt_fam.hip): the exact
statement of what the integer GEMM promises, in integer arithmetic, and the tolerance that follows from it.  Plain numpy and
Python integers; nothing here calls into the library.

The statement
  * U arrives as float.  rvt_set_kinship stores q_u = rint(u * 2^40) (uq_sexp = 7 kRotPlanesU - 2, round half to even) as
    six signed base-128 digits in [-64, 63]: 40 fractional bits, |u - q_u 2^-40| <= 2^-41.
  * A batch of columns whose entries are all integers of magnitude <= 127 is ONE plane holding the entries themselves.  Any
    other batch is six planes for every column: q_g = rint(g * 2^s_j), s_j = 7 kRotPlanesG - 3 - ilogb(max_i |g_ij|)
    (0 for an all-zero column), so |g - q_g 2^-s_j| <= 2^-40 max_i |g_ij|.
  * G~[k, j] = 2^-(40 + s_j) * sum_i q_u[i, k] q_g[i, j], the sum in integers, converted to double once.

The tolerance (rotation_bounds) is derived below from how the kernel adds its pieces, not from anything it returned.
"""
import math

import numpy as np

PLANES_U = 6                    # kRotPlanesU
PLANES_G = 6                    # kRotPlanesG
U_SEXP = 7 * PLANES_U - 2       # rvt_set_kinship: uq_sexp
KC, BM, BN = 128, 256, 256      # kRotKC, kRotBM, kRotBN
# sum_p 128^p |d_p| <= DIGIT_SUM * |q| for the digits d_p in [-64, 63] of an integer q: with t the top non-zero digit,
# sum_{p<t} 128^p |d_p| < (64/127) 128^t, hence |q| > (|d_t| - 64/127) 128^t and the sum < (|d_t| + 64/127) 128^t; the ratio
# is largest for |d_t| = 1: (1 + 64/127) / (1 - 64/127) = 3.0318
DIGIT_SUM = 3.04


def quantize_u(U):
    """q_u (int64) of a float matrix."""
    U32 = np.asarray(U, dtype=np.float32)
    return np.rint(U32.astype(np.float64) * 2.0 ** U_SEXP).astype(np.int64)


def quantize_g(G):
    """(q_g int64, s_j per column, planes) as quantize_columns decides them for the whole batch."""
    G = np.asarray(G, dtype=np.float64)
    mx = np.abs(G).max(axis=0)
    integer = (G == np.rint(G)).all(axis=0)
    if bool((integer & (mx <= 127.0)).all()):
        return G.astype(np.int64), np.zeros(G.shape[1], dtype=np.int64), 1
    # (the column scan hands a non-integer column's maximum over as -(max) - 1 and the host undoes that: restated, because the
    #  round trip can move the last bit of the maximum)
    mx = np.where(integer, mx, -(-mx - 1.0) - 1.0)
    sexp = np.array([0 if m == 0.0 else 7 * PLANES_G - 3 - (math.frexp(m)[1] - 1) for m in mx], dtype=np.int64)
    q = np.rint(np.ldexp(G, sexp[None, :].astype(np.int32))).astype(np.int64)
    return q, sexp, PLANES_G


def _limbs(q, n):
    """q = sum_a limb_a 2^(14 a): n limbs as float64, the low ones in [0, 2^14), the top one signed."""
    out = []
    for a in range(n):
        if a == n - 1:
            out.append(q.astype(np.float64))
        else:
            out.append((q & 0x3FFF).astype(np.float64))
            q = q >> 14
    return out


def _int_product(qu, qg):
    """qu' qg exactly, as an object array of Python integers.  |q_u| < 2^42 and |q_g| < 2^41 are cut into three 14-bit limbs;
    a product of two limb matrices is a sum of N integers below 2^28, exact in float64 for any N < 2^25 in whatever order the
    BLAS adds them, and the nine products are recombined in Python integers."""
    N, ncols = qg.shape
    assert N < (1 << 25) and np.abs(qu).max(initial=0) < (1 << 42) and np.abs(qg).max(initial=0) < (1 << 42)
    small_g = np.abs(qg).max(initial=0) < (1 << 14)
    gl = [qg.astype(np.float64)] if small_g else _limbs(qg, 3)
    R = np.zeros((qu.shape[1], ncols), dtype=object)
    for k0 in range(0, qu.shape[1], 1024):               # eigenvectors in chunks: bounded temporaries at N = 8200
        ul = _limbs(qu[:, k0:k0 + 1024], 3)
        for a, ua in enumerate(ul):
            for b, gb in enumerate(gl):
                M = ua.T @ gb
                assert np.abs(M).max(initial=0) < 2.0 ** 53
                R[k0:k0 + 1024] += M.astype(np.int64).astype(object) * (1 << (14 * (a + b)))
    return R


def exact_rotation(U, G, qu=None):
    """The statement: U'G from the quantised operands in integers, converted to double once.  Returns (N x ncols float64,
    planes of the batch).  qu: quantize_u(U), when the caller keeps it for several batches."""
    if qu is None:
        qu = quantize_u(U)
    qg, sexp, planes = quantize_g(G)
    R = _int_product(qu, qg)
    out = np.empty(R.shape, dtype=np.float64)
    for j in range(R.shape[1]):
        den = 1 << int(U_SEXP + sexp[j])                  # (int / int: correctly rounded)
        out[:, j] = [int(r) / den for r in R[:, j]]
    return out, planes


def exact_rotation_python(U, G):
    """The same statement in Python integers only (slow: small cases, to check _int_product)."""
    qu = quantize_u(U).astype(object)
    qg, sexp, planes = quantize_g(G)
    R = qu.T.dot(qg.astype(object))
    out = np.empty(R.shape, dtype=np.float64)
    for j in range(R.shape[1]):
        den = 1 << int(U_SEXP + sexp[j])
        out[:, j] = [int(r) / den for r in R[:, j]]
    return out, planes


def k_slices(N, ncols, planes_g, rot_slices=None, rot_kmax=None):
    """How many K slices planes_gemm cuts the rotation of ncols columns into (its rule restated; the two arguments are the
    RVT_ROT_SLICES / RVT_ROT_KMAX overrides)."""
    def cdiv(a, b):
        return -(-a // b)
    nrp, nct = cdiv(N, BM), cdiv(ncols, BN)
    kbytes = cdiv(N, KC) * KC
    bound = 64 * (127 if planes_g == 1 else 64)
    kmax = max(KC, ((1 << 31) - 1) // bound // KC * KC)
    if rot_kmax is not None:
        kmax = max(KC, min(kmax, rot_kmax // KC * KC))
    tiles = nrp * nct
    slices = 1
    if tiles < 256:
        slices = min(cdiv(512, tiles), max(1, kbytes // (16 * KC)))
    slices = max(slices, cdiv(kbytes, kmax))
    if rot_slices is not None:
        slices = max(1, rot_slices)
    kslice = min(cdiv(cdiv(kbytes, slices), KC) * KC, kmax)
    return cdiv(kbytes, kslice)


def rotation_bounds(N, planes_g, slices, sum_abs_g, max_u, max_g):
    """Per column (sum_abs_g, max_g: arrays over the columns): (acc, uq, gq).

    acc — the kernel against the statement.  Every int32 tile sum is exact, and so is its product with the power of two
    128^(p+q) 2^-(40+s_j); what rounds is the fp64 addition of those pieces: PLANES_U * planes_g plane pairs, each arriving
    as `slices` slice partials (rot_reduce_slices_kernel adds them one after the other into C), i.e. at most
    PLANES_U * planes_g * slices additions.  The structured kernel instead folds the six planes of U in registers and adds
    once per plane of G: PLANES_U * planes_g + planes_g additions.  One more rounding is the statement's own conversion to
    double.  An addition errs by at most 2^-53 of its result, and every partial result is bounded by the sum of the
    magnitudes of all pieces,
        T = 2^-(40+s_j) sum_i (sum_p 128^p |d_p(u_i)|) (sum_q 128^q |e_q(g_i)|)
          <= DIGIT_SUM (max|u| + 2^-41) * c_g * (sum_i |g_i| + N 2^-40 max|g|),
    with c_g = 1 for one plane (the plane IS g, and the 2^-40 term is absent) and DIGIT_SUM for six.  So
        acc = (PLANES_U planes_g slices + planes_g + 1) 2^-53 T            (second-order terms 2^-106 are left out).
    uq  — the statement against the real product, from U's fixed point: 2^-41 per entry of U, times sum_i |q_g 2^-s|.
    gq  — the same from a six-plane column's fixed point: 2^-40 max|g| per entry, times sum_i |u_i| <= N max|u|.  The bound
          is relative to the column's LARGEST entry: that is the contract, an outlier costs the small entries their digits.
    """
    sum_abs_g = np.asarray(sum_abs_g, dtype=np.float64)
    max_g = np.asarray(max_g, dtype=np.float64)
    six = planes_g != 1
    sum_q = sum_abs_g + (N * 2.0 ** -40 * max_g if six else 0.0)
    T = DIGIT_SUM * (max_u + 2.0 ** -41) * (DIGIT_SUM if six else 1.0) * sum_q
    acc = (PLANES_U * planes_g * slices + planes_g + 1) * 2.0 ** -53 * T
    uq = 2.0 ** -41 * sum_q
    gq = 2.0 ** -40 * max_g * N * max_u if six else np.zeros_like(max_g)
    return acc, uq, gq


# ---- inputs -----------------------------------------------------------------------------------------------------------
def householder_u(N, seed):
    """A dense orthogonal matrix as the product of two Householder reflectors (I - 2aa')(I - 2bb'), |a| = |b| = 1, in
    O(N^2): diagonal near 1, off-diagonals of size about 1/N — the dynamic range the fixed point has to hold.  float32."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(N)
    b = rng.standard_normal(N)
    a /= np.linalg.norm(a)
    b /= np.linalg.norm(b)
    U = np.outer(-2.0 * a, a)
    U += np.outer(4.0 * (a @ b) * a - 2.0 * b, b)
    U[np.diag_indices(N)] += 1.0
    return np.asfortranarray(U.astype(np.float32)), rng.uniform(0.05, 2.0, N).astype(np.float32)


def grm_u(N, seed):
    """Eigenvectors / eigenvalues of the GRM of random genotypes (dense U, small eigenvalues), float32."""
    rng = np.random.default_rng(seed)
    m = 3 * N
    Z = rng.binomial(2, rng.uniform(0.05, 0.5, m), (N, m)).astype(float)
    Z = (Z - Z.mean(0)) / np.maximum(Z.std(0), 1e-9)
    S, U = np.linalg.eigh(Z @ Z.T / m)
    return np.asfortranarray(U.astype(np.float32)), S.astype(np.float32)


KINDS = ("rare", "common", "zero", "twos", "single", "imputed", "dosage", "outlier")


def column(N, kind, rng):
    if kind == "rare":
        g = rng.binomial(2, 0.01, N).astype(np.float64)
        g[rng.integers(0, N)] = 1.0                        # (at least one carrier)
        return g
    if kind == "common":
        return rng.binomial(2, 0.3, N).astype(np.float64)
    if kind == "zero":
        return np.zeros(N)
    if kind == "twos":
        return np.full(N, 2.0)
    if kind == "single":                                   # one carrier: the rotated column is one row of U, entry by entry
        g = np.zeros(N)
        g[rng.integers(0, N)] = 1.0
        return g
    if kind == "imputed":                                  # hard calls, the missing ones at the mean of the others
        g = rng.binomial(2, 0.2, N).astype(np.float64)
        miss = rng.random(N) < 0.03
        miss[0] = True
        g[miss] = g[~miss].mean()
        return g
    if kind == "dosage":
        return np.round(np.clip(rng.binomial(2, 0.3, N) + rng.normal(0, 0.15, N), 0, 2), 3)
    if kind == "outlier":                                  # one entry of 1e6 among entries of about 1e-3
        g = rng.uniform(0.5e-3, 1.5e-3, N)
        g[rng.integers(0, N)] = 1e6
        return g
    raise ValueError(kind)


def columns(N, ncols, seed, kinds=KINDS):
    """ncols columns cycling through `kinds` (all of them: a six-plane batch; HARD: hard calls, one plane)."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.column_stack([column(N, kinds[j % len(kinds)], rng) for j in range(ncols)]))


HARD = ("rare", "common", "zero", "twos", "single")
