"""GPU: a call's output does not depend on what the context ran before.  A context lives for a whole analysis and owns about a
hundred device buffers; half of them are grow-only work spaces that every call lays out afresh from its own shapes, several
shared between unrelated call families.  A call that reads a word of such a buffer before writing it reads what an earlier
call — of another N, d, M, V or trait — left at an offset that now means something else.

ONE engine runs every step (= one entry-point family at one shape set, STEPS below) at shape set A, then at B, then at A
again — grow, shrink under a larger block, another shape under an equal block — with RVT_POISON=255 (fresh work spaces hold
0xff bytes) and RVT_SCRIBBLE=255 (a work space that is large enough already is refilled with 0xff bytes before the call
gets it: DESIGN.md, "Device buffers: state and work space").  A second engine runs the same list B first and reversed
inside every pass.  Every output equals, bit for bit (NaN = NaN), the output of the same step on a fresh engine that runs
nothing else, with both variables unset.  A step whose two fresh runs differ in a bit would be held to its own test's
statement instead; no step of the list does (test_fresh_engines_agree checks every one), so none is compared by a tolerance.
A family that refuses a shape (a binary trait under the lattice kernel, KBAC with covariates, ..) appears with its refusal —
the error text — as the expected output.

Shape sets: A has N = 4099 (above the 4096 samples from which columns and genes are packed on the way, and no multiple of 4,
16 or 64: tests/test_gpu_block_reuse.py), d = 4, a quantitative trait, genes of 40 and blocks of 70 columns, 75 families, a
dense kinship of order 300; B has N = 130, d = 1, a binary trait where the family takes one, genes of 3 and blocks of 9
columns, 40 families, a dense kinship of order 130 (both orders take the tridiagonal route, from 128 on).

The switch itself is checked by test_scribble_is_live.  No work space can be read back between two calls without new ABI
(burden_last_columns refuses every part of d_burden_cols the last call did not write; download_columns reads blocks, which
are no DevBuf), so that test asserts on the host-side trace of the refills (RVT_SCRIBBLE_TRACE=1: one line per refilled
block on stderr, with the buffer's name where the site gives one) and on DESIGN.md's table."""
import ctypes
import os
import re

import numpy as np
import pytest

import bgengen
import fam_bed_cases
import perm_cases
import synth
import vcfgen
from test_fam_cpu import make_family_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "A": dict(N=4099, d=4, trait=0, M=40, V=70, n_fam=75, K=300),
    "B": dict(N=130, d=1, trait=1, M=3, V=9, n_fam=40, K=130),
}
ENV = ("RVT_POISON", "RVT_SCRIBBLE")


# ---- inputs, made once per shape set and never changed ------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _null(s):
    sh = SHAPES[s]
    return _once(("null", s), lambda: synth.make_null(sh["N"], sh["d"], sh["trait"], seed=11))


def _gene(s, missing=0.02):
    """(raw with -9, imputed, counter frequencies) of the shape set's gene: a flipped and two monomorphic columns at 40"""
    sh = SHAPES[s]
    return _once(("gene", s, missing), lambda: synth.make_gene(sh["N"], sh["M"], seed=21, missing=missing, common=True, mono=True,
                                                               maf_lo=-2.0, maf_hi=-0.7))


def _block(s):
    """the V columns of the block calls (raw, imputed, frequencies)"""
    sh = SHAPES[s]
    return _once(("block", s), lambda: synth.make_gene(sh["N"], sh["V"], seed=31, missing=0.02, common=True, mono=True,
                                                       maf_lo=-2.0, maf_hi=-0.7))


def _dosage(s, den=0):
    """dosages in [0, 2]: float-precision ones (den = 0), or multiples of 1 / den"""
    sh = SHAPES[s]

    def make():
        rng = np.random.default_rng(41 + den)
        maf = 10 ** rng.uniform(-2.0, -0.7, sh["M"])
        G = np.clip(rng.binomial(2, maf, size=(sh["N"], sh["M"])) + rng.normal(0.0, 0.05, size=(sh["N"], sh["M"])), 0.0, 2.0)
        if den:
            G = np.rint(G * den) / den
        else:
            G = G.astype(np.float32).astype(np.float64)
        G = np.asfortranarray(G)
        return G, G.mean(0) / 2.0
    return _once(("dosage", s, den), make)


def _fam(s):
    sh = SHAPES[s]
    return _once(("fam", s), lambda: make_family_case(sh["n_fam"], sh["d"], seed=51))


def _fam_calls(s):
    """raw calls of the family case's samples: V columns + fam_bed_cases' hand-made rows"""
    sh = SHAPES[s]
    return _once(("famcalls", s), lambda: fam_bed_cases.calls(4 * sh["n_fam"], sh["V"], seed=61))


def _dense_kinship(s):
    """a dense float kinship of order K with distinct eigenvalues"""
    K = SHAPES[s]["K"]

    def make():
        rng = np.random.default_rng(71)
        A = rng.standard_normal((K, 2 * K))
        return np.asfortranarray((A @ A.T / (2 * K)).astype(np.float32))
    return _once(("dense", s), make)


def _mt(s):
    sh = SHAPES[s]

    def make():
        rng = np.random.default_rng(81)
        N = sh["N"]
        Y = rng.standard_normal((N, 3))
        Z = rng.standard_normal((N, 2))
        Y[rng.random((N, 3)) < 0.02] = np.nan
        return Y, Z, [(0, [0]), (1, [0, 1]), (2, [])]
    return _once(("mt", s), make)


def _vcf_lines(s):
    sh = SHAPES[s]

    def make():
        rng = np.random.default_rng(91)
        return [vcfgen.make_record(rng, sh["N"], fmt=b"GT:DP", pos=1000 + j) for j in range(sh["M"])]
    return _once(("vcf", s), make)


def _bgen_blocks(s):
    sh = SHAPES[s]

    def make():
        rng = np.random.default_rng(101)
        return [bgengen.layout2_block_fast(rng, sh["N"], bits=16, missing=0.02) for _ in range(sh["M"])]
    return _once(("bgen", s), make)


# ---- one engine and what is installed on it -------------------------------------------------------------------------------------
class _Run:
    """An engine, and the model state its next step needs: installed when it differs from what is there ("the null model and
    the kinship are re-installed whenever the shape set changes")."""

    def __init__(self):
        import rvtests_amd
        self.e = rvtests_amd.Engine(0)
        self.state = None
        self.g, self.g_shape = None, None

    def group(self, s):
        """A device group of one member that lives as long as this engine does (its member is a context of its own, with work
        spaces of its own that the calls of every pass reuse), under the shape set's null model: fitted again when the shape
        set changes."""
        import rvtests_amd
        if self.g is None:
            self.g = rvtests_amd.Group([0])
        if self.g_shape != s:
            X, y = _null(s)[:2]
            self.g.fit_null(SHAPES[s]["trait"], X, y)
            self.g_shape = s
        return self.g

    def need(self, kind, s):
        """kind "null": the shape set's null model, fitted on the device.  "fam": the family case — an ordinary null model of
        ITS samples (the blocks' layout, the pitch of resident rows), the kinship in eigenvector form and the FastLMM null."""
        if self.state == (kind, s):
            return
        e = self.e
        if kind == "null":
            X, y = _null(s)[:2]
            e.fit_null(SHAPES[s]["trait"], X, y)
        else:
            N, K, U, S, X, y = _fam(s)
            e.fit_null(0, X, y)
            e.set_kinship(U, S)
            e.fit_fam_null(X, y)
        e.vcf_set_samples(np.arange(e.N, dtype=np.int32))
        self.state = (kind, s)

    def close(self):
        if self.g is not None:
            self.g.close()
        self.e.close()


def _blocks(e, mats):
    return [e.upload_block(G) for G in mats]


def _free(e, ptrs):
    for p in ptrs:
        e.free_block(p)


def _resident(e, raw):
    """raw calls as a resident .bed matrix, two other rows in front: (handle, address of the first row of `raw`)"""
    cb = (raw.shape[0] + 3) // 4
    d_bed = e.bed_alloc(raw.shape[1] + 2)
    e.bed_upload(d_bed, 0, np.full((2, cb), 0x55, dtype=np.uint8))
    e.bed_upload(d_bed, 2, fam_bed_cases.pack(raw))
    return d_bed, d_bed + 2 * cb


# ---- the steps: run(r, s) -> arrays / records ---------------------------------------------------------------------------------------
STEPS = {}


def step(kind):
    def deco(fn):
        STEPS[fn.__name__[3:]] = (kind, fn)
        return fn
    return deco


@step("null")
def st_fit_null(r, s):
    X, y = _null(s)[:2]
    out = r.e.fit_null(SHAPES[s]["trait"], X, y)
    return out, r.e.null_summary()


def _run_blocks(r, mats, afs, tests=15, params=None):
    ptrs = _blocks(r.e, mats)
    try:
        return r.e.run_blocks(ptrs, [G.shape[1] for G in mats], afs, tests=tests, params=params)
    finally:
        _free(r.e, ptrs)


@step("null")
def st_run_blocks_hardcall(r, s):
    raw, G, af = _gene(s, missing=0.0)
    return _run_blocks(r, [G, G[:, :max(1, G.shape[1] // 2)]], [af, af[:max(1, G.shape[1] // 2)]], tests=15 | 128)


@step("null")
def st_run_blocks_imputed(r, s):
    raw, G, af = _gene(s)
    return _run_blocks(r, [G, G[:, 1:]], [af, af[1:]])


@step("null")
def st_run_blocks_dosage(r, s):
    G, af = _dosage(s)
    r.e.set_content_hint(0)
    r.e.set_dosage_float(True)
    try:
        return _run_blocks(r, [G], [af])
    finally:
        r.e.set_dosage_float(False)
        r.e.set_content_hint(-1)


@step("null")
def st_run_blocks_lattice(r, s):
    G, af = _dosage(s, den=1000)
    r.e.set_content_hint(0)
    try:
        r.e.set_dosage_lattice(1000)
        return _run_blocks(r, [G], [af])
    finally:
        r.e.set_dosage_lattice(0)
        r.e.set_content_hint(-1)


def _collected(r, af):
    (rec,) = r.e.collect()
    return af, rec


@step("null")
def st_submit_bed(r, s):
    raw = _gene(s)[0]
    return _collected(r, r.e.submit_gene_bed(7, fam_bed_cases.pack(raw), raw.shape[1]))


@step("null")
def st_submit_i8(r, s):
    return _collected(r, r.e.submit_gene_raw(8, _gene(s)[0].astype(np.int8)))


@step("null")
def st_submit_raw_f64(r, s):
    return _collected(r, r.e.submit_gene_raw(9, _gene(s)[0]))


@step("null")
def st_submit_f64(r, s):
    raw, G, af = _gene(s)
    r.e.submit_gene(10, G, af)
    return _collected(r, None)


@step("null")
def st_submit_bed_dev(r, s):
    raw = _gene(s)[0]
    d_bed, rows = _resident(r.e, raw)
    try:
        r.e.submit_genes_bed_dev([11], [rows], [raw.shape[1]])
        return _collected(r, None)
    finally:
        r.e.bed_free(d_bed)


@step("null")
def st_submit_vcf(r, s):
    return _collected(r, r.e.submit_gene_vcf(12, _vcf_lines(s)))


@step("null")
def st_submit_bgen(r, s):
    return _collected(r, r.e.submit_gene_bgen(13, _bgen_blocks(s), 2))


def _with_block(r, s, fn, dosage=False):
    G = _dosage(s)[0] if dosage else _block(s)[1]
    (p,) = _blocks(r.e, [G])
    try:
        return fn(p, G.shape[1])
    finally:
        _free(r.e, [p])


def _with_columns(r, s, fn):
    """the block filled column range by column range (rvt_block_upload_columns: packed on the way from 4096 samples on, the
    column cache behind it), as the adapters' ring is"""
    G = _block(s)[1]
    V = G.shape[1]
    p = r.e.alloc_block(V)
    try:
        r.e.upload_columns(p, 0, G[:, :V // 2])
        for j in range(V // 2, V):
            r.e.upload_columns(p, j, G[:, j])
        return fn(p, V)
    finally:
        _free(r.e, [p])


@step("null")
def st_score_block(r, s):
    return _with_block(r, s, r.e.score_block), _with_columns(r, s, r.e.score_block)


@step("null")
def st_score_block_host(r, s):
    """rvt_group_score_block_host runs on the contexts of a device group: the long-lived run keeps ONE group beside its engine
    (_Run.group), so the member's work spaces see every pass under both switches; a fresh run has a fresh group.  Hard calls,
    then dosages: the member picks its kernel by what the columns hold."""
    g = r.group(s)
    return g.score_block_host(_block(s)[1]), g.score_block_host(_dosage(s)[0])


@step("null")
def st_cov_block(r, s):
    return _with_block(r, s, r.e.cov_block), _with_block(r, s, r.e.cov_block, dosage=True)


@step("null")
def st_cov_rect(r, s):
    return _with_block(r, s, lambda p, V: r.e.cov_rect(p, 1, V // 2, V - 1)), \
        _with_columns(r, s, lambda p, V: r.e.cov_rect(p, 0, V - 2, V))


@step("null")
def st_cov_band(r, s):
    """the band ring: a window that wraps"""
    def band(p, V):
        H = V // 2
        return r.e.cov_band(p, V, V - 3, H, H + 4, 4), r.e.cov_band_last_path()
    return _with_columns(r, s, band), _with_block(r, s, band)


@step("null")
def st_wald_block(r, s):
    return _with_block(r, s, r.e.wald_block)


def _y01(s):
    """the 0 / 1 phenotype the permutation burden tests take: the binary trait at B; at A, whose trait is quantitative, a fixed
    draw (y is a free argument of these calls) — so that their work spaces are laid out at both shape sets"""
    if SHAPES[s]["trait"]:
        return _null(s)[1]
    return _once(("y01", s), lambda: (np.random.default_rng(111).random(SHAPES[s]["N"]) < 0.3).astype(np.float64))


def _gene_blocks(r, s, fn):
    raw, G, af = _gene(s)
    h = max(1, G.shape[1] // 2)
    ptrs = _blocks(r.e, [G, G[:, :h]])
    try:
        return fn(ptrs, [G.shape[1], h], [af, af[:h]])
    finally:
        _free(r.e, ptrs)


@step("null")
def st_burden_blocks(r, s):
    y = _null(s)[1]
    return _gene_blocks(r, s, lambda p, M, af: r.e.burden_blocks(p, M, af, y=y))


@step("null")
def st_kbac_blocks(r, s):
    y = _y01(s)
    return _gene_blocks(r, s, lambda p, M, af: r.e.kbac_blocks(p, M, af, y, 300, 0.05))


@step("null")
def st_vtprice_blocks(r, s):
    y = _y01(s)
    return _gene_blocks(r, s, lambda p, M, af: r.e.vtprice_blocks(p, M, af, y, nperm=300, alpha=0.05))


@step("null")
def st_rarecover_blocks(r, s):
    y = _y01(s)
    return _gene_blocks(r, s, lambda p, M, af: r.e.rarecover_blocks(p, M, y, nperm=300, alpha=0.05))


@step("null")
def st_mb_blocks(r, s):
    y = _y01(s)
    return _gene_blocks(r, s, lambda p, M, af: r.e.mb_blocks(p, M, y, nperm=300, alpha=0.05))


@step("null")
def st_mtscore(r, s):
    Y, Z, tests = _mt(s)
    fit = r.e.mt_fit_null(Y, Z, tests)
    try:
        return fit, _with_block(r, s, r.e.mt_score_block), _with_block(r, s, r.e.mt_score_block, dosage=True)
    finally:
        r.e.mt_clear()


@step("null")
def st_block_recode(r, s):
    import rvtests_amd
    raw = _block(s)[0]

    def recode(p, V):
        cnt = r.e.block_recode(p, 0, p, 0, V, rvtests_amd.CODING_DOMINANT)
        return cnt, r.e.download_columns(p, 0, V), r.e.score_block(p, V)
    (p,) = _blocks(r.e, [np.where(raw < 0, np.nan, raw)])
    try:
        return recode(p, raw.shape[1])
    finally:
        _free(r.e, [p])


@step("null")
def st_bed_recode_block(r, s):
    import rvtests_amd
    raw = _block(s)[0]
    V = raw.shape[1]
    d_bed, rows = _resident(r.e, raw)
    p = r.e.alloc_block(V)
    try:
        cnt = r.e.bed_recode_block(rows, V, rvtests_amd.CODING_RECESSIVE, p, 0)
        return cnt, r.e.download_columns(p, 0, V), r.e.score_block(p, V)
    finally:
        _free(r.e, [p])
        r.e.bed_free(d_bed)


def _skat_perm(r, s, exact):
    import rvtests_amd
    G, af = perm_cases.counter_gene(SHAPES[s]["N"], SHAPES[s]["M"])
    prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, 400, 0.05)
    r.e.set_perm_exact(exact)
    try:
        return _run_blocks(r, [G], [af], tests=1, params=prm)
    finally:
        r.e.set_perm_exact(True)


@step("null")
def st_skat_perm_exact(r, s):
    return _skat_perm(r, s, True)


@step("null")
def st_skat_perm_counter(r, s):
    return _skat_perm(r, s, False)


@step("null")
def st_score_bed_dev(r, s):
    """quantitative at A, binary at B"""
    raw = _block(s)[0]
    d_bed, rows = _resident(r.e, raw)
    try:
        return r.e.score_bed_dev(rows, raw.shape[1])
    finally:
        r.e.bed_free(d_bed)


def _with_fam_block(r, s, fn):
    G = fam_bed_cases.imputed(_fam_calls(s))
    (p,) = _blocks(r.e, [G])
    try:
        return fn(p, G.shape[1])
    finally:
        _free(r.e, [p])


@step("fam")
def st_fam_null(r, s):
    """set_kinship + fit_fam_null again on the context that has them: the fit's own work spaces"""
    N, K, U, S, X, y = _fam(s)
    r.e.set_kinship(U, S)
    out = r.e.fit_fam_null(X, y)
    return out, r.e.fam_null_summary(X.shape[1]), r.e.kinship_structure()


@step("fam")
def st_run_fam_blocks(r, s):
    def run(p, V):
        h = max(1, V // 2)
        return r.e.run_fam_blocks([p, p], [V, h], tests=16 | 32 | 64), r.e.run_fam_blocks([p], [h], tests=16)
    return _with_fam_block(r, s, run)


@step("fam")
def st_fam_analytic_vt(r, s):
    return _with_fam_block(r, s, lambda p, V: r.e.fam_analytic_vt([p, p], [V, max(1, V // 3)]))


@step("fam")
def st_fam_score_block(r, s):
    def run(p, V):
        out = [r.e.score_block_fam(p, V)]
        if SHAPES[s]["trait"]:
            # (the scale b^2 is a state of the family null model that every later family call multiplies by, until the next
            #  fit_fam_null: the next step installs the models again)
            out += [r.e.fam_binary_scale(V, 3 * V), r.e.score_block_fam(p, V, binary=1)]
            r.state = None
        return out
    return _with_fam_block(r, s, run)


@step("fam")
def st_fam_lrt_block(r, s):
    return _with_fam_block(r, s, lambda p, V: (r.e.lrt_block_fam(p, V), r.e.lrt_block_fam(p, V // 2)))


@step("fam")
def st_fam_grammar_block(r, s):
    N, K, U, S, X, y = _fam(s)
    fit = r.e.fit_grammar_null(X, y)
    return fit, _with_fam_block(r, s, lambda p, V: (r.e.grammar_block(p, V), r.e.grammar_block(p, V, af_kinship=1)))


@step("fam")
def st_fam_cov_block(r, s):
    d = SHAPES[s]["d"]
    return _with_fam_block(r, s, lambda p, V: (r.e.cov_block_fam(p, V, d), r.e.cov_rect_fam(p, 1, V // 2, V - 1, d)))


def _with_fam_rows(r, s, fn):
    raw = _fam_calls(s)
    d_bed, rows = _resident(r.e, raw)
    try:
        return fn(rows, raw.shape[1])
    finally:
        r.e.bed_free(d_bed)


@step("fam")
def st_score_bed_dev_fam(r, s):
    return _with_fam_rows(r, s, lambda rows, V: r.e.score_bed_dev_fam(rows, V, binary=SHAPES[s]["trait"]))


@step("fam")
def st_lrt_bed_dev_fam(r, s):
    return _with_fam_rows(r, s, r.e.lrt_bed_dev_fam)


@step("fam")
def st_kinship_from_bed(r, s):
    def run(rows, V):
        bn = r.e.kinship_from_bed(rows, V, "bn")
        ibs = r.e.kinship_from_bed(rows, V, "ibs", min_maf=0.01, max_missing=0.5)
        return bn[0], _timeless(bn[1]), ibs[0], _timeless(ibs[1])
    return _with_fam_rows(r, s, run)


def _timeless(info):
    """a KinshipInfo without the device times of its stages"""
    return [getattr(info, n) for n, _ in info._fields_ if not n.startswith("ms_")]


@step("fam")
def st_kinship_decompose_family(r, s):
    """a block-diagonal kinship: family by family"""
    return r.e.kinship_decompose(_fam(s)[1].astype(np.float32))


@step("fam")
def st_kinship_decompose_tridiag(r, s):
    return r.e.kinship_decompose(_dense_kinship(s))


@step("fam")
def st_kinship_decompose_jacobi(r, s):
    os.environ["RVT_KINSHIP_JACOBI"] = "1"
    try:
        return r.e.kinship_decompose(_dense_kinship(s))
    finally:
        del os.environ["RVT_KINSHIP_JACOBI"]


@step("fam")
def st_kinship_decompose_families(r, s):
    n_fam = SHAPES[s]["n_fam"]
    K = _fam(s)[1]
    fam_ptr = 4 * np.arange(n_fam + 1, dtype=np.int64)
    members = np.arange(4 * n_fam, dtype=np.int32)
    blocks = np.concatenate([K[4 * f:4 * f + 4, 4 * f:4 * f + 4].T.ravel() for f in range(n_fam)]).astype(np.float32)
    return r.e.kinship_decompose_families(fam_ptr, members, blocks)


# (the family steps last in a pass: they replace the ordinary null model by one of the family case's samples)
ORDER = list(STEPS)


def _run_step(r, name, s):
    """One step on engine r: its output, or the text of its refusal.  The emulated rand() stream of the permutation tests is a
    state of the context that every call advances: each step starts it again."""
    import rvtests_amd
    kind, fn = STEPS[name]
    r.need(kind, s)
    r.e.rand_seed(1)
    try:
        return fn(r, s)
    except rvtests_amd.RvtError as err:
        if "error -3:" in str(err):     # RVT_E_HIP, a failed HIP call: no refusal, and nothing more may run on this device
            pytest.exit("a HIP call failed in step %s at %s: %s" % (name, s, err), returncode=3)
        # (a refusal may leave the models as they were or half replaced: the next step installs its own again)
        r.state = None
        return "refused: " + re.sub(r"0x[0-9a-f]+", "0x..", str(err))


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _leaves(x, path=""):
    """every number of an output with a name: arrays as they are, structures field by field"""
    if isinstance(x, (ctypes.Structure,)):
        for n, _ in x._fields_:
            yield from _leaves(getattr(x, n), path + "." + n)
    elif isinstance(x, ctypes.Array):
        if len(x) and isinstance(x[0], ctypes.Structure):
            for k, item in enumerate(x):
                yield from _leaves(item, "%s[%d]" % (path, k))
        else:
            yield path, np.array(list(x))
    elif isinstance(x, dict):
        for k in x:
            yield from _leaves(x[k], path + "." + str(k))
    elif isinstance(x, (list, tuple)):
        for k, item in enumerate(x):
            yield from _leaves(item, "%s[%d]" % (path, k))
    else:
        yield path, x


def _same_bits(got, want, where):
    """bit for bit, NaN equal to NaN (tests/test_gpu_block_reuse.py's _same_bits over whole outputs)"""
    a, b = list(_leaves(got)), list(_leaves(want))
    assert [p for p, _ in a] == [p for p, _ in b], (where, "outputs of another shape")
    for (path, x), (_, y) in zip(a, b):
        if isinstance(x, str) or isinstance(y, str):
            assert x == y, (where, path, x, y)
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (where, path, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype.kind == "f":
            same = (x.view("u%d" % x.dtype.itemsize) == y.view("u%d" % y.dtype.itemsize)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x == y
        if not np.all(same):
            bad = np.argwhere(~np.atleast_1d(same))[:4]
            raise AssertionError((where, path, "%d of %d entries differ" % (int((~same).sum()), same.size), bad.tolist(),
                                  np.atleast_1d(x)[~np.atleast_1d(same)][:4], np.atleast_1d(y)[~np.atleast_1d(same)][:4]))


# ---- the two long-lived engines and the fresh ones -----------------------------------------------------------------------------------
def _set_env(values):
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


class _Passes:
    """One engine under both switches and its passes [(shape set, step names), ..], run a step at a time when first asked for, in
    the order of the passes — the tests ask in that order, so that each waits for its own step only: get(k, name) = the output
    of step `name` of pass k.  The variables are set for the length of a step (the engine is created inside the first) and
    restored behind it."""

    def __init__(self, order):
        self.todo = [(k, s, name) for k, (s, names) in enumerate(order) for name in names]
        self.r, self.out, self.done = None, {}, 0

    def get(self, k, name):
        while (k, name) not in self.out:
            kk, s, nn = self.todo[self.done]
            old = _set_env({v: "255" for v in ENV})
            try:
                if self.r is None:
                    self.r = _Run()
                self.out[(kk, nn)] = _run_step(self.r, nn, s)
            finally:
                _set_env(old)
            self.done += 1
        return self.out[(k, name)]

    def close(self):
        if self.r is not None:
            self.r.close()


FORWARD = [("A", ORDER), ("B", ORDER), ("A", ORDER)]
BACKWARD = [("B", ORDER[::-1]), ("A", ORDER[::-1]), ("B", ORDER[::-1])]


def _cases(order):
    return [pytest.param(k, s, name, id="%d-%s-%s" % (k, s, name)) for k, (s, names) in enumerate(order) for name in names]


@pytest.fixture(scope="module")
def forward():
    p = _Passes(FORWARD)
    try:
        yield p
    finally:
        p.close()


@pytest.fixture(scope="module")
def backward():
    p = _Passes(BACKWARD)
    try:
        yield p
    finally:
        p.close()


_fresh_cache = {}


def _fresh(name, s, again=False):
    """the step alone on a fresh engine, both switches unset (computed once; again = a second, independent run)"""
    key = (name, s, again)
    if key not in _fresh_cache:
        old = _set_env({k: None for k in ENV})
        try:
            r = _Run()
            try:
                _fresh_cache[key] = _run_step(r, name, s)
            finally:
                r.close()
        finally:
            _set_env(old)
    return _fresh_cache[key]


@pytest.mark.parametrize("s", ["A", "B"])
@pytest.mark.parametrize("name", ORDER)
def test_fresh_engines_agree(name, s):
    """The rule of comparison rests on this: two fresh engines give the same bits for every step, so every step is compared bit
    for bit and none by a tolerance."""
    _same_bits(_fresh(name, s, again=True), _fresh(name, s), (name, s, "two fresh engines"))


@pytest.mark.parametrize("k, s, name", _cases(FORWARD))
def test_step_after_everything_else(forward, k, s, name):
    _same_bits(forward.get(k, name), _fresh(name, s), (name, "pass %d at %s" % (k, s)))


@pytest.mark.parametrize("k, s, name", _cases(BACKWARD))
def test_step_after_everything_else_reversed(backward, k, s, name):
    _same_bits(backward.get(k, name), _fresh(name, s), (name, "reversed pass %d at %s" % (k, s)))


def test_every_step_computes_somewhere():
    """(a refusal compares equal too: every step returns numbers, not a refusal, at one shape set at least; the refusals are
    printed)"""
    for n in ORDER:
        out = {s: _fresh(n, s) for s in SHAPES}
        for s in SHAPES:
            if isinstance(out[s], str):
                print(s, n, out[s])
        assert not all(isinstance(o, str) for o in out.values()), (n, out)


def test_scribble_is_live(capfd):
    """The same call twice on one engine at one shape: with RVT_SCRIBBLE set the second call's work spaces are refilled — the
    trace has a line per refill, with the buffer's name where the site gives one: the step's packed column uploads must show
    d_colpack (the 2-bit rows) and d_cc_part (the column pass behind them) —, the outputs are the same bits, and without the
    variable nothing is refilled.  The trace, not a read-back: no work space is reachable between two calls without new ABI
    (module docstring).  DESIGN.md's table names the buffers the refill covers."""
    def twice(env):
        old = _set_env(env)
        try:
            r = _Run()
            try:
                first = _run_step(r, "score_block", "A")
                capfd.readouterr()
                second = _run_step(r, "score_block", "A")
                return first, second, capfd.readouterr().err
            finally:
                r.close()
        finally:
            _set_env(old)
    first, second, err = twice({"RVT_SCRIBBLE": "255", "RVT_SCRIBBLE_TRACE": "1", "RVT_POISON": None})
    refills = re.findall(r"rvt: scribble (\S+) (\d+) bytes", err)
    names = {n for n, _ in refills}
    assert {"d_colpack", "d_cc_part"} <= names and all(int(b) > 0 for _, b in refills), (sorted(names), err[:2000])
    _same_bits(second, first, "score_block twice")
    _, _, err = twice({"RVT_SCRIBBLE": None, "RVT_SCRIBBLE_TRACE": "1", "RVT_POISON": None})
    assert "scribble" not in err
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "RVT_SCRIBBLE" in design
    for buf in ("d_rot_part", "d_rotB", "d_cov_work", "d_kind", "d_colpack", "d_cc_part", "d_recode_ws", "d_mt_B", "d_fam_list"):
        assert re.search(r"^\|[^|]*`%s`[^|]*\|\s*work space \|" % buf, design, re.M), buf
