"""CPU: the exact statement of the kinship rotation (tests/rotref.py) is right before it judges the kernel — it agrees with
a long-double product of the UNQUANTISED float U and double G within what rot_gemm.hip.h promises for the fixed point
(2^-41 per entry of U times sum |g|; for a six-plane column also 2^-40 of the column's largest entry per entry of g)."""
import numpy as np
import pytest

import rotref

CASES = [(130, 1, ("imputed",)), (130, 1, ("outlier",)), (130, 7, rotref.KINDS), (257, 33, rotref.KINDS), (700, 257, rotref.KINDS),
         (130, 1, rotref.HARD), (257, 33, rotref.HARD), (700, 256, rotref.HARD)]


def real_product(U, G):
    return np.asarray(U, dtype=np.float32).astype(np.longdouble).T @ np.asarray(G, dtype=np.float64).astype(np.longdouble)


@pytest.mark.parametrize("make_u", [rotref.householder_u, rotref.grm_u])
@pytest.mark.parametrize("N,ncols,kinds", CASES)
def test_statement_is_the_real_product_to_the_fixed_point(make_u, N, ncols, kinds):
    U, _ = make_u(N, 7 * N + ncols)
    G = rotref.columns(N, ncols, N + ncols, kinds)
    ref, planes = rotref.exact_rotation(U, G)
    assert planes == (1 if set(kinds) <= set(rotref.HARD) else rotref.PLANES_G)
    real = real_product(U, G)
    sum_g, max_g, max_u = np.abs(G).sum(0), np.abs(G).max(0), float(np.abs(U).max())
    _, uq, gq = rotref.rotation_bounds(N, planes, 1, sum_g, max_u, max_g)
    # + the statement's conversion to double and the long-double sum itself (64-bit significands: N 2^-64 per product)
    tol = uq + gq + (2.0 ** -53 + N * 2.0 ** -63) * max_u * sum_g
    err = np.abs((ref.astype(np.longdouble) - real).astype(np.float64))
    assert (err <= tol[None, :]).all(), (err / np.maximum(tol[None, :], 1e-300)).max()
    if planes == 1:                                       # hard calls: nothing but U's 2^-41 per entry
        assert (gq == 0).all() and np.allclose(uq, 2.0 ** -41 * sum_g, rtol=0, atol=0)
    assert (ref[:, max_g == 0] == 0).all()


def test_limb_product_is_the_python_integer_product():
    for kinds, seed in ((rotref.KINDS, 1), (rotref.HARD, 2)):
        U, _ = rotref.householder_u(130, seed)
        G = rotref.columns(130, 9, seed, kinds)
        a, pa = rotref.exact_rotation(U, G)
        b, pb = rotref.exact_rotation_python(U, G)
        assert pa == pb and (a == b).all()


def test_quantisation_rules():
    U = np.array([[1.0, -1.0], [2.0 ** -40, 3 * 2.0 ** -42]], dtype=np.float32)
    q = rotref.quantize_u(U)
    assert q.tolist() == [[1 << 40, -(1 << 40)], [1, 1]]
    G = np.column_stack([[0.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.5, 1.0, 1.75], [1e6, 1e-3, 0.0]])
    qg, sexp, planes = rotref.quantize_g(G)
    assert planes == 6 and sexp.tolist() == [38, 0, 39, 20]
    assert qg[:, 0].tolist() == [0, 1 << 39, 1 << 38] and (qg[:, 1] == 0).all()
    assert np.abs(qg).max() < 1 << 40
    qg, sexp, planes = rotref.quantize_g(G[:, :2])
    assert planes == 1 and (qg == G[:, :2]).all() and (sexp == 0).all()


def test_slice_rule():
    assert rotref.k_slices(130, 7, 6) == 1 and rotref.k_slices(700, 257, 6) == 1
    assert rotref.k_slices(700, 255, 6, rot_slices=3) == 3 and rotref.k_slices(700, 255, 1, rot_kmax=128) == 6
    assert rotref.k_slices(4100, 8, 6) == 2 and rotref.k_slices(8200, 8, 1) == 4


def test_inputs_are_dense_and_orthogonal():
    U, S = rotref.householder_u(257, 3)
    U = U.astype(np.float64)
    assert np.abs(U.T @ U - np.eye(257)).max() < 1e-6 and (U != 0).all()
    assert np.abs(np.diag(U)).min() > 0.5 and np.abs(U - np.diag(np.diag(U))).max() < 0.3
