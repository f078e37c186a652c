"""CPU: the designed genes of spectra_designs.py through the HOST build of the per-gene tail (hc.gene, one lane) against the
oracle and LAPACK, with the assertions tests/test_gpu_spectra.py makes of the device build.  This is where the designs and
the tolerances are checked without a GPU: a design the host build cannot hold to a bound does not belong in the GPU file."""
import numpy as np
import pytest

import hc
import orc
import spectra_designs as sd

REL, ABS_P, ABS_SKATO = 1e-6, 1e-14, 5e-13       # test_gpu_parity.py's bars


def _oracle(c):
    rc, a = orc.skat(c["G"], c["af"], c["X"], c["res"], c["v"], c["binary"])
    rc2, o = orc.skato(c["G"], c["af"], c["X"], c["res"], c["v"], c["binary"])
    return a, rc2, o


def _check_full_rank(r, c, burden=True):
    """_check_gene of test_gpu_parity.py, word for word, on a host-build record."""
    a, rc2, o = _oracle(c)
    assert r.n_poly == a.n_poly and r.skat_ok == 1
    assert abs(r.skat_Q - a.Q) <= 1e-10 * abs(a.Q)
    assert abs(r.skat_p - a.pvalue) <= REL * abs(a.pvalue) + ABS_P, (r.skat_p, a.pvalue)
    assert rc2 == 0 and r.skato_ok == 1
    assert abs(r.skato_Q - o.Q) <= 1e-10 * abs(o.Q)
    assert r.skato_rho == o.rho
    assert abs(r.skato_p - o.pvalue) <= REL * abs(o.pvalue) + ABS_SKATO, (r.skato_p, o.pvalue)
    if burden and not (c["binary"] and c["d"] > 1):
        for which, ok, stat, p, nonref in ((0, r.cmc_ok, r.cmc_stat, r.cmc_p, r.cmc_nonref), (1, r.zeg_ok, r.zeg_stat, r.zeg_p, None)):
            rc3, b = orc.burden(c["G"], c["X"], c["y"], c["binary"], which)
            assert ok == (rc3 == 0)
            if ok:
                assert abs(stat - b.stat) <= 1e-9 * abs(b.stat) + 1e-13
                assert abs(p - b.pvalue) <= REL * abs(b.pvalue) + ABS_P
                if nonref is not None:
                    assert nonref == b.nonref_site
    return o


@pytest.mark.parametrize("case", sd.EIGEN_CASES, ids=sd.case_id)
def test_designed_genes_on_the_host_build(case):
    """Eigenvalues against LAPACK (the host build is within 4e-14 lmax), the SKAT p-value against Davies on the build's own
    eigenvalues (identical: it is the same call), the record against the oracle, and the rho-problem fields against the
    oracle's — the figures RHO_FIELDS' bounds are ten times of."""
    c = sd.make_case(*case)
    r, lam = sd.host_gene(c)
    worst = sd.check_eigenvalues(lam, c)
    p_own = sd.own_inputs_skat_p(lam, r.skat_Q)
    print("eigenvalues %.2g lmax, p on own inputs %.2g" % (worst, abs(r.skat_p - p_own)))
    assert abs(r.skat_p - p_own) <= 1e-9 * p_own + 1e-14
    if case[0] in sd.RANK_DEFICIENT:
        a, rc2, o = _oracle(c)
        sd.check_rank_deficient_record(r, c, a, rc2, o)
    else:
        o = _check_full_rank(r, c)
    for name, sl, bound in sd.RHO_FIELDS:
        if name in sd.ORACLE_NAMES:
            ref = getattr(o, sd.ORACLE_NAMES[name])
            seen = sd.rel_diff(r.dbg[sl], list(ref) if sl.stop - sl.start > 1 else ref)
            print("%s host vs oracle %.2g" % (name, seen))
            assert seen <= bound, (name, seen, bound)    # (the worst over the cases is a tenth of the bound)


@pytest.mark.parametrize("eps", sd.NEAR_EPS)
def test_nearly_collinear_columns(eps):
    c = sd.make_near_case(eps)
    r, lam = sd.host_gene(c)
    sd.check_eigenvalues(lam, c)
    if eps >= 2e-3:
        o = _check_full_rank(r, c)
    else:
        a, rc2, o = _oracle(c)
        sd.check_rank_deficient_record(r, c, a, rc2, o)
    if eps <= 1e-9:
        assert r.skato_qags_neval == o.qags_neval


@pytest.mark.parametrize("cols", sd.FEWPOLY_COLS, ids=lambda t: "%dpoly" % len(t))
def test_few_polymorphic_columns_among_300(cols):
    c = sd.make_fewpoly_case(cols)
    r, lam = sd.host_gene(c)
    assert r.n_poly == len(cols)
    sd.check_eigenvalues(lam, c)
    _check_full_rank(r, c)


def test_frequencies_counted_from_a_mostly_monomorphic_gene_silence_it():
    """Why fewpoly passes frequencies of its own: kept column a reads af[a], and with af counted from
    G those are the zeros of the monomorphic columns in front — weight 0, Q = 0, in the oracle and the host build alike."""
    c = sd.make_fewpoly_case((5, 150, 299))
    af = c["G"].sum(0) / (2.0 * c["N"])
    r, _, _, _ = hc.gene(c["G"], af, c["X"], c["res"], c["v"], 0, c["s2"])
    rc, a = orc.skat(c["G"], af, c["X"], c["res"], c["v"], 0)
    assert r.n_poly == a.n_poly == 3 and r.skat_Q == 0.0 and a.Q == 0.0


@pytest.mark.parametrize("M,binary", [(41, 0), (41, 1), (100, 0), (100, 1)])
def test_more_columns_than_samples(M, binary):
    c = sd.make_more_columns_than_samples_case(M, binary)
    r, lam = sd.host_gene(c)
    assert lam.size <= 40                       # Skat.cpp keeps at most min(N, m) eigenvalues
    sd.check_eigenvalues(lam, c)
    _check_full_rank(r, c)


@pytest.mark.parametrize("M", [125, 126, 192, 193, 208])
def test_plain_genes_at_the_launch_switches(M):
    """The partners of the GPU file's path-switch batches."""
    c = sd.make_plain_case(M)
    r, lam = sd.host_gene(c)
    sd.check_eigenvalues(lam, c)
    _check_full_rank(r, c)


def test_width_512():
    """M = 512 (the GPU file also runs 1024): eigenvalues against LAPACK, SKAT against the oracle's recorded result
    (tests/golden/spectra_wide512.json; the oracle's SKAT needs ten seconds at this width, its SKAT-O far longer)."""
    c = sd.make_plain_case(512, N=1200)
    r, lam = sd.host_gene(c)
    sd.check_eigenvalues(lam, c)
    Q, p = sd.wide512_oracle(c)
    assert abs(r.skat_Q - Q) <= 1e-10 * Q and abs(r.skat_p - p) <= REL * p + ABS_P
