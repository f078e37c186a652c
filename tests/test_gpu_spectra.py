"""GPU: the per-gene tail kernels (gene_assemble / gene_tridiag / gene_spectrum, gene_spectrum_all / gene_pvalue) on the genes
of spectra_designs.py — exactly repeated and zero eigenvalues, tight clusters, spectra over eight decades, nearly collinear
columns, a few polymorphic columns among 300, more columns than samples — and on both sides of the two launch switches
(dense reduction in LDS up to M = 125 / in global scratch from 126; all-in-one spectrum kernel up to M = 192 / one workgroup
per eigenproblem from 193), up to RVT_MAX_VARIANTS columns.  The device eigenvalues come from rvt_debug_spectrum.

tests/test_spectra_cpu.py makes the same assertions of the host build of the same code, which is how the designs and the
bounds were checked; spectra_designs.py holds both files' assertions."""
import functools

import numpy as np
import pytest

import orc
import spectra_designs as sd
from test_gpu_parity import ABS_P, ABS_SKATO, _check_gene

pytestmark = pytest.mark.gpu

# check (b): |skat_p(device) - skat_p(host build on the device's eigenvalues and Q)| <= P_OWN_ABS.  Measured on an MI355X
# over the 30 genes of this file that make the check (M = 3 .. 1024, p = 0.008 .. 0.94): 14 identical, the worst
# 4.44e-16 — two units in the last place of a p-value that both sides form as 1 - qf, which is why the bound is absolute
# (1.4e-14 of p at p = 0.008).  Ten times that; a bound looser than 1e-9 p + 1e-14 here would be a finding, not a tolerance.
P_OWN_ABS = 4.5e-15


@functools.lru_cache(maxsize=None)
def _case(case):
    return sd.make_case(*case)


_device_runs = {}


def _run(engine, c, beside=None, suffstat=False):
    """The gene's spectrum stage on the device; suffstat: also the sufficient statistics it started from, as hc.gene's
    (R, colstat) under the key `suffstat`."""
    engine.set_null(c["binary"], c["X"], c["res"], c["v"], c["s2"])
    ptr = engine.upload_block(c["G"])
    bptr = engine.upload_block(beside["G"]) if beside is not None else None
    try:
        dev = engine.debug_spectrum(ptr, c["M"], c["af"], None if beside is None else (bptr, beside["M"], beside["af"]))
        if suffstat:
            S, T, u, cs, mn, mx = engine.debug_suffstat(ptr, c["M"])
            dev["suffstat"] = (np.column_stack([S, T, u]), np.vstack([cs, mn, mx]))
        return dev
    finally:
        engine.free_block(ptr)
        if bptr is not None:
            engine.free_block(bptr)


def _device(engine, case):
    """One device run per case, shared by the checks (a), (b) and (c)."""
    if case not in _device_runs:
        _device_runs[case] = _run(engine, _case(case), suffstat=True)
    return _device_runs[case]


def _check_own_inputs(dev):
    r = dev["rec"]
    p_own = sd.own_inputs_skat_p(dev["lam"], r.skat_Q)
    diff = abs(r.skat_p - p_own)
    print("skat_p %.17g, host build on the device's inputs %.17g, difference %.3g (%.3g of p)" % (r.skat_p, p_own, diff, diff / p_own))
    assert diff <= P_OWN_ABS, (r.skat_p, p_own)
    return diff / p_own


def _check_against_oracle(r, c, rank_deficient):
    if rank_deficient:
        rc, a = orc.skat(c["G"], c["af"], c["X"], c["res"], c["v"], c["binary"])
        rc2, o = orc.skato(c["G"], c["af"], c["X"], c["res"], c["v"], c["binary"])
        sd.check_rank_deficient_record(r, c, a, rc2, o)
        return o
    _check_gene(r, c["G"], c["af"], c["X"], c["y"], c["res"], c["v"], c["binary"], c["d"])
    return None


# ---- (a) eigenvalues ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sd.EIGEN_CASES, ids=sd.case_id)
def test_device_eigenvalues_match_lapack(engine, case):
    """The kept SKAT eigenvalues of the device against numpy.linalg.eigvalsh of the numpy statement of K: as many above
    1e-12 lmax as LAPACK's numerical rank, each within 1e-11 lmax of LAPACK's, the rest rounding, all descending
    (spectra_designs.check_eigenvalues).  skat_nlambda itself is not compared on the rank-deficient designs: how many
    rounding-level values survive the reference's 1e-30 filter depends on the rounding.

    The rho-problem fields Qs, mom_mu / mom_var / mom_df, tau, muQ, varQ, varZeta, df against the host build's, each within
    ten times the host build's own worst disagreement with the oracle over these cases (spectra_designs.RHO_FIELDS):
    2.7e-13, 9.8e-13, 2.0e-12, 4.2e-14, 2.3e-14, 9.8e-13, 2.0e-12, 3.3e-9, 4.2e-14 relative.  The host build starts from the
    DEVICE's sufficient statistics (rvt_debug_suffstat), so that the comparison is of the tail alone: under a binary trait the
    statistics kernels read the null model from 42-bit fixed point, which alone moves Q_rho by 1e-12 of itself (measured on
    dup-M48-binary against numpy's statistics; test_gpu_parity.py's _check_gene allows for the same effect)."""
    dev = _device(engine, case)
    worst = sd.check_eigenvalues(dev["lam"], _case(case))
    h, _ = sd.host_gene(_case(case), stats=dev["suffstat"])
    seen = sd.check_rho_fields(dev["stats"], h.dbg)
    print("eigenvalues within %.3g lmax of LAPACK; rho-problem fields vs the host build:" % worst,
          ", ".join("%s %.2g" % kv for kv in seen.items()))
    assert dev["stats"][61] == 0 and dev["stats"][62] == case[1]


# ---- (b) the p-value kernel on its own inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sd.EIGEN_CASES, ids=sd.case_id)
def test_skat_p_is_davies_of_the_device_eigenvalues(engine, case):
    """gene_pvalue_kernel against the host build of the same algorithm on the DEVICE's eigenvalues and Q: Davies in product
    form (hc.davies(fast=True)), Liu's where Davies faults or gives 0 or 1.  Bound: P_OWN_ABS = 4.5e-15 absolute, ten times
    the worst difference measured (4.44e-16; see P_OWN_ABS)."""
    _check_own_inputs(_device(engine, case))


# ---- (c) against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sd.EIGEN_CASES, ids=sd.case_id)
def test_designed_genes_match_oracle(engine, case):
    """Full-rank designs (singletons, rng): _check_gene of test_gpu_parity.py.  Rank-deficient (dup): SKAT's p-value within
    2e-6 absolute, the rest as _check_gene (spectra_designs.check_rank_deficient_record); the sharp check of their p-value is
    (b)."""
    _check_against_oracle(_device(engine, case)["rec"], _case(case), case[0] in sd.RANK_DEFICIENT)


@pytest.mark.parametrize("eps", sd.NEAR_EPS)
def test_nearly_collinear_columns(engine, eps):
    """The eps-collinear family of test_models_cpu.py on the device: eps >= 2e-3 is full rank, below that the last eigenvalue
    is rounding or inside the reference's filter band; at eps = 0 and 1e-9 the quadrature takes the oracle's steps."""
    c = sd.make_near_case(eps)
    dev = _run(engine, c)
    sd.check_eigenvalues(dev["lam"], c)
    _check_own_inputs(dev)
    o = _check_against_oracle(dev["rec"], c, eps < 2e-3)
    if eps <= 1e-9:
        assert dev["rec"].skato_qags_neval == o.qags_neval


@pytest.mark.parametrize("cols", sd.FEWPOLY_COLS, ids=lambda t: "%dpoly" % len(t))
def test_few_polymorphic_columns_among_300(engine, cols):
    c = sd.make_fewpoly_case(cols)
    dev = _run(engine, c)
    assert dev["rec"].n_poly == len(cols)
    sd.check_eigenvalues(dev["lam"], c)
    _check_own_inputs(dev)
    _check_against_oracle(dev["rec"], c, False)


@pytest.mark.parametrize("M,binary", [(41, 0), (41, 1), (100, 0), (100, 1)])
def test_more_columns_than_samples(engine, M, binary):
    c = sd.make_more_columns_than_samples_case(M, binary)
    dev = _run(engine, c)
    assert dev["lam"].size <= 40                 # Skat.cpp keeps at most min(N, m) eigenvalues
    sd.check_eigenvalues(dev["lam"], c)
    _check_own_inputs(dev)
    _check_against_oracle(dev["rec"], c, False)


# ---- (d) the launch switches ------------------------------------------------------------------------------------------------------
def test_narrow_gene_is_bit_identical_across_the_launch_paths(engine):
    """A gene of M = 20 beside one of M = 125 / 126 / 192 / 193 / 208: the batch's widest gene decides whether the dense
    reduction's matrix lives in LDS and which spectrum kernel runs — the arithmetic is the same, so the narrow gene's record
    and eigenvalues are the same bits in all five batches.  The wide partners against the oracle."""
    narrow = sd.make_plain_case(20)
    runs = []
    for M in (125, 126, 192, 193, 208):
        wide = dict(sd.make_plain_case(M), **{k: narrow[k] for k in ("X", "y", "res", "v", "s2")})   # (one null model)
        dev = _run(engine, narrow, beside=wide)
        _check_against_oracle(dev["beside_rec"], wide, False)
        runs.append(dev)
    _check_against_oracle(runs[0]["rec"], narrow, False)
    sd.check_eigenvalues(runs[0]["lam"], narrow)
    for dev in runs[1:]:
        for name, _ in type(dev["rec"])._fields_:
            x, y = getattr(dev["rec"], name), getattr(runs[0]["rec"], name)
            assert x == y or (x != x and y != y), (name, x, y)
        assert np.array_equal(dev["lam"], runs[0]["lam"]) and np.array_equal(dev["lam_zimz"], runs[0]["lam_zimz"])
        assert np.array_equal(dev["stats"], runs[0]["stats"], equal_nan=True)


def test_record_without_the_vt_test_has_zero_vt_fields(engine):
    """What the bit-identity test above found when it ran behind the suite's AnalyticVT tests: gene_pvalue_kernel cleared every
    field of the record except vt_*, which only gene_vt_kernel writes — a batch without that test handed back whatever an
    earlier batch had left at the record's place in the slot's work space (vt_optmaf = 9.0 in one batch, 0.0 in the next).
    Here: batches WITH the test through every slot, then batches without it through every slot."""
    from rvtests_amd.engine import MAX_INFLIGHT, TEST_ALL, TEST_ANALYTICVT
    c = sd.make_plain_case(20)
    engine.fit_null(0, c["X"], c["y"])           # (as tests/test_gpu_vt.py installs the null model of its batches)
    ptr = engine.upload_block(c["G"])
    try:
        for _ in range(MAX_INFLIGHT + 1):
            r = engine.run_blocks([ptr], [20], [c["af"]], tests=TEST_ALL | TEST_ANALYTICVT)[0]
            assert r.vt_ok == 1 and r.vt_optmaf > 0.0 and r.vt_stat > 0.0
        for _ in range(MAX_INFLIGHT + 1):
            r = engine.run_blocks([ptr], [20], [c["af"]])[0]
            for name, _ in type(r)._fields_:
                if name.startswith("vt_"):
                    assert getattr(r, name) == 0, (name, getattr(r, name))
    finally:
        engine.free_block(ptr)


# ---- (e) width --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(512, 1200), (1024, 2500)])
def test_wide_genes(engine, M, N):
    """Up to RVT_MAX_VARIANTS columns: eigenvalues against LAPACK as in (a), skat_p as in (b), the whole record against the
    host build at test_full_size_properties' bounds (the oracle's SKAT-O needs 18 s at M = 512 and minutes at 1024; its SKAT
    at M = 512 is the recorded result of tests/golden/spectra_wide512.json)."""
    c = sd.make_plain_case(M, N=N)
    dev = _run(engine, c)
    r = dev["rec"]
    sd.check_eigenvalues(dev["lam"], c)
    _check_own_inputs(dev)
    h, _ = sd.host_gene(c)
    assert r.n_poly == h.n_poly == M
    assert abs(r.skat_Q - h.skat_Q) <= 1e-11 * h.skat_Q and abs(r.skat_p - h.skat_p) <= 1e-6 * h.skat_p + ABS_P
    assert r.skato_ok == h.skato_ok == 1
    assert r.skato_rho == h.skato_rho and abs(r.skato_p - h.skato_p) <= 1e-6 * h.skato_p + ABS_SKATO
    assert r.cmc_nonref == h.cmc_nonref and r.cmc_ok == h.cmc_ok == 1 and r.zeg_ok == h.zeg_ok == 1
    assert abs(r.cmc_p - h.cmc_p) <= 1e-8 * h.cmc_p and abs(r.zeg_p - h.zeg_p) <= 1e-8 * h.zeg_p
    if M == 512:
        Q, p = sd.wide512_oracle(c)
        assert abs(r.skat_Q - Q) <= 1e-10 * Q and abs(r.skat_p - p) <= 1e-6 * p + ABS_P


# ---- (f) FamSKAT ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["dup", "singletons"])
def test_famskat_on_designed_genes(design):
    """FamSKAT reaches the same dense reduction, spectrum and p-value kernels behind fam_assemble_kernel: a dup and a singletons
    gene of M = 48 against orc.famskat at test_gpu_fam.py's tolerances (the eigenvalue count only on the full-rank one)."""
    import rvtests_amd
    from test_fam_cpu import make_family_case
    N, K, U, S, X, y = make_family_case(40, 2, 22)
    G, af = getattr(sd, design)(N, 48, 58)
    eng = rvtests_amd.Engine(0)
    try:
        eng.set_kinship(U, S)
        nul = eng.fit_fam_null(X, y)
        onul = orc.FamNull()
        onul.ok = 1
        onul.delta, onul.sigma2 = nul.delta, nul.sigma2_g
        for k in range(2):
            onul.beta[k] = nul.beta[k]
        r = eng.run_fam_blocks([eng.upload_block(G)], [48])[0]
    finally:
        eng.close()
    rc, o = orc.famskat(G, X, y, U, S, onul)
    assert rc == 0 and r.famskat_ok == 1
    assert r.n_variants == 48 and r.n_poly == o.n_poly
    assert abs(r.famskat_Q - o.Q) <= 1e-7 * o.Q
    if design == "singletons":
        assert r.skat_nlambda == o.n_lambda
    print("famskat_p %.17g, oracle %.17g" % (r.famskat_p, o.pvalue))
    assert abs(r.famskat_p - o.pvalue) <= 2e-6 * abs(o.pvalue) + 1e-12
