"""GPU: what the engine knows about a resident .bed matrix (rvt_bed_alloc's record, bed_rows_span) at every call that reads its
rows — the last rows of a matrix are in range and give the bits of the same rows at the front of another matrix; one row too
many, an address off a row boundary, an upload past the end and a matrix sized for another N are refused on the host with
nothing written and nothing queued; rvt_bed_free takes the base address of a matrix of its context and nothing else.
N = 515: a pitch of 129 bytes, odd, with a partial last byte; one context carries the quantitative, family (dense U),
multiple-trait (3 traits) and GrammarGamma null models.  No call here reads outside an allocation: every refusal happens before
device work, and no address is used after its matrix is freed."""
import ctypes as C

import numpy as np
import pytest

import fam_bed_cases
import synth
from test_gpu_fam_bed import dense_case

pytestmark = pytest.mark.gpu

N, PITCH, ROWS, V = 515, 129, 40, 7
GENES = (3, 4)                                            # the last V rows as two genes
OK, E_INVALID, E_STATE = 0, -1, -4
FAM_ALL = 16 | 32 | 64
F_SENT, I_SENT = 7.25, -3

vp = C.c_void_p


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _bufs(spec):
    """sentinel-filled outputs: (shape, dtype) each"""
    return [np.full(shape, F_SENT if np.dtype(dt).kind == "f" else I_SENT, dtype=dt) for shape, dt in spec]


def _untouched(bufs):
    return all((b == (F_SENT if b.dtype.kind == "f" else I_SENT)).all() for b in bufs)


# ---- the calls over consecutive rows: name -> (outputs of V rows, the raw call) ----------------------------------------------------
def _stat_spec(n_double):
    return lambda e, v: [((v,), np.int32)] + [((v,), np.float64)] * n_double + [((v, 4), np.int64)]


def _score(e, a, v, b):
    e.L.rvt_score_bed_dev.restype = C.c_int
    e.L.rvt_score_bed_dev.argtypes = [vp, vp, C.c_int64, vp] + [C.POINTER(C.c_double)] * 5 + [vp]
    return e.L.rvt_score_bed_dev(e.ctx, vp(a), v, b[0].ctypes.data_as(vp), *[_dp(x) for x in b[1:6]], b[6].ctypes.data_as(vp))


def _band(e, a, v, b):
    e.L.rvt_cov_band_bed_dev.restype = C.c_int
    e.L.rvt_cov_band_bed_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), vp]
    return e.L.rvt_cov_band_bed_dev(e.ctx, vp(a), v, v, 3, 1.0, b[0].ctypes.data_as(C.POINTER(C.c_float)), _dp(b[1]), _dp(b[2]),
                                    _ip(b[3]), b[4].ctypes.data_as(vp))


def _recode(e, a, v, b):
    """into a block of the call's own; b[1] takes the columns of a successful call"""
    e.L.rvt_bed_recode_block.restype = C.c_int
    e.L.rvt_bed_recode_block.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    blk = e.alloc_block(v)
    rc = e.L.rvt_bed_recode_block(e.ctx, vp(a), v, 1, vp(blk), 0, b[0].ctypes.data_as(vp))
    if rc == OK:
        b[1][...] = e.download_columns(blk, 0, v)
    e.free_block(blk)
    return rc


def _kinship(e, a, v, b):
    from rvtests_amd.engine import KINSHIP_FROM_BED_ARGTYPES, KinshipInfo
    e.L.rvt_kinship_from_bed.restype = C.c_int
    e.L.rvt_kinship_from_bed.argtypes = KINSHIP_FROM_BED_ARGTYPES
    info = KinshipInfo()
    rc = e.L.rvt_kinship_from_bed(e.ctx, vp(a), v, 0, 0.0, 1.0, _dp(b[0]), C.byref(info))
    if rc == OK:
        b[1][...] = (info.sites, info.sites_used, info.filtered_missing, info.filtered_maf, info.monomorphic)
    return rc


def _mt(e, a, v, b):
    return e.L.rvt_mt_score_bed_dev(e.ctx, vp(a), v, _dp(b[0]), _dp(b[1]), _dp(b[2]), b[3].ctypes.data_as(vp))


def _fam_score(e, a, v, b):
    e.L.rvt_score_bed_dev_fam.restype = C.c_int
    e.L.rvt_score_bed_dev_fam.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4 + [vp]
    return e.L.rvt_score_bed_dev_fam(e.ctx, vp(a), v, 0, _ip(b[0]), *[_dp(x) for x in b[1:5]], b[5].ctypes.data_as(vp))


def _fam_lrt(e, a, v, b):
    e.L.rvt_lrt_bed_dev_fam.restype = C.c_int
    e.L.rvt_lrt_bed_dev_fam.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4 + [vp]
    return e.L.rvt_lrt_bed_dev_fam(e.ctx, vp(a), v, _ip(b[0]), *[_dp(x) for x in b[1:5]], b[5].ctypes.data_as(vp))


def _grammar(e, a, v, b):
    e.L.rvt_grammar_bed_dev.restype = C.c_int
    e.L.rvt_grammar_bed_dev.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4 + [vp]
    return e.L.rvt_grammar_bed_dev(e.ctx, vp(a), v, 1, _ip(b[0]), *[_dp(x) for x in b[1:5]], b[5].ctypes.data_as(vp))


ROW_CALLS = {
    "rvt_score_bed_dev": (_stat_spec(5), _score),
    "rvt_cov_band_bed_dev": (lambda e, v: [((v, 4), np.float32), ((v, e.d), np.float64), ((e.d, e.d), np.float64), ((v,), np.int32),
                                           ((v, 4), np.int64)], _band),
    "rvt_bed_recode_block": (lambda e, v: [((v, 4), np.int64), ((N, v), np.float64)], _recode),
    "rvt_kinship_from_bed": (lambda e, v: [((N, N), np.float64), ((5,), np.int64)], _kinship),
    "rvt_mt_score_bed_dev": (lambda e, v: [((v, 3), np.float64)] * 3 + [((v, 4), np.int64)], _mt),
    "rvt_score_bed_dev_fam": (_stat_spec(4), _fam_score),
    "rvt_lrt_bed_dev_fam": (_stat_spec(4), _fam_lrt),
    "rvt_grammar_bed_dev": (_stat_spec(4), _grammar),
}
# (the ordinary null model's d is what Engine.d holds: the context's last fit_null)


def _rec(r):
    """the fields of a record as the bits they hold (not bytes(r): the padding between fields holds anything)"""
    raw = bytes(r)
    return b"".join(raw[f.offset:f.offset + f.size] for f in (getattr(type(r), n) for n, _ in r._fields_))


# ---- the calls over genes: name -> the raw call on [(address, M), ..]; returns (rc, outputs untouched, result of a good call) ------
def _submit_gene(e, genes):
    from rvtests_amd.engine import Params, TEST_ALL
    e.L.rvt_submit_gene_bed_dev.restype = C.c_int
    e.L.rvt_submit_gene_bed_dev.argtypes = [vp, C.c_int64, C.c_int, vp, C.c_uint32, vp, C.POINTER(C.c_double)]
    prm = Params.default()
    afs, rc = [], OK
    for g, (a, m) in enumerate(genes):
        af = np.full(m, F_SENT)
        rc = e.L.rvt_submit_gene_bed_dev(e.ctx, 11 + g, m, vp(a), TEST_ALL, C.byref(prm), _dp(af))
        if rc != OK:
            return rc, _untouched([af]), None
        afs.append(af.tobytes())
    return rc, False, afs + [_rec(r) for r in e.collect()]


def _submit_genes(e, genes):
    from rvtests_amd.engine import Params, TEST_ALL
    n = len(genes)
    e.L.rvt_submit_genes.restype = C.c_int
    e.L.rvt_submit_genes.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_uint32, vp]
    prm = Params.default()
    ids, ms = np.arange(11, 11 + n, dtype=np.int64), np.array([m for a, m in genes], dtype=np.int32)
    rc = e.L.rvt_submit_genes(e.ctx, 7, n, ids.ctypes.data_as(vp), ms.ctypes.data_as(vp), (vp * n)(*[a for a, m in genes]), TEST_ALL,
                              C.byref(prm))
    return rc, True, [_rec(r) for r in e.collect()] if rc == OK else None


def _run_fam(e, genes):
    from rvtests_amd.engine import GeneResult
    n = len(genes)
    e.L.rvt_run_fam_tests_bed_dev.restype = C.c_int
    e.L.rvt_run_fam_tests_bed_dev.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_uint32,
                                              C.POINTER(GeneResult)]
    out = (GeneResult * n)()
    C.memset(out, 0x5A, C.sizeof(out))
    before = bytes(out)
    rc = e.L.rvt_run_fam_tests_bed_dev(e.ctx, n, (vp * n)(*[a for a, m in genes]), (C.c_int * n)(*[m for a, m in genes]), None,
                                       FAM_ALL, out)
    return rc, bytes(out) == before, [_rec(r) for r in out] if rc == OK else None


GENE_CALLS = {"rvt_submit_gene_bed_dev": _submit_gene, "rvt_submit_genes kind 7": _submit_genes, "rvt_run_fam_tests_bed_dev": _run_fam}
READS_ORDINARY_NULL = ("rvt_score_bed_dev", "rvt_cov_band_bed_dev", "rvt_bed_recode_block", "rvt_kinship_from_bed",
                       "rvt_submit_gene_bed_dev", "rvt_submit_genes kind 7")
CALLS = list(ROW_CALLS) + list(GENE_CALLS)


class World:
    """One context with the four null models at N = 515, the matrix of 40 rows (d_bed) and a second matrix whose first V rows
    are the first one's last V (d_front)."""

    def __init__(self):
        import rvtests_amd
        _, U, S, self.X, self.y, _ = dense_case()
        # the hand-made degenerate rows first, ordinary rows last: the last V rows are worth a kinship
        self.rows = fam_bed_cases.pack(np.asfortranarray(fam_bed_cases.calls(N, ROWS - 7, seed=77)[:, ::-1]))
        assert self.rows.shape == (ROWS, PITCH)
        e = self.e = rvtests_amd.Engine(0)
        e.fit_null(0, self.X, self.y)
        e.set_kinship(U, S)
        e.fit_fam_null(self.X, self.y)
        e.fit_grammar_null(self.X, self.y)
        rng = np.random.default_rng(5)
        e.mt_fit_null(rng.standard_normal((N, 3)), rng.standard_normal((N, 2)), [(0, [0]), (1, [0, 1]), (2, [1])])
        self.d_bed = e.bed_alloc(ROWS)
        e.bed_upload(self.d_bed, 0, self.rows)
        self.d_front = e.bed_alloc(V + 2)
        e.bed_upload(self.d_front, 0, self.rows[ROWS - V:])
        e.bed_upload(self.d_front, V, self.rows[:2])
        self.last = self.d_bed + (ROWS - V) * PITCH
        self._want = {}

    def genes_at(self, base):
        return [(base, GENES[0]), (base + GENES[0] * PITCH, GENES[1])]

    def run(self, name, base, v=V):
        """(rc, outputs untouched, result): the call on v rows / the two genes at `base`"""
        if name in GENE_CALLS:
            return GENE_CALLS[name](self.e, self.genes_at(base))
        spec, raw = ROW_CALLS[name]
        b = _bufs(spec(self.e, v))
        rc = raw(self.e, base, v, b)
        return rc, _untouched(b), [x.tobytes() for x in b] if rc == OK else None

    def want(self, name):
        """the bits of the V rows at the front of the second matrix: computed once, never changed"""
        if name not in self._want:
            rc, _, res = self.run(name, self.d_front)
            assert rc == OK and res
            self._want[name] = res
        return self._want[name]

    def good(self, name):
        rc, _, res = self.run(name, self.last)
        want = self.want(name)
        if rc != OK or res != want:                       # say where before the caller's assertion fails
            print("%s on the last rows: rc %d, %s" % (name, rc, self.e.L.rvt_last_error(self.e.ctx).decode() if rc else ""))
            for k, (x, y) in enumerate(zip(res or [], want)):
                if x != y:
                    print("  output %d: bytes %s differ" % (k, [i for i in range(min(len(x), len(y))) if x[i] != y[i]][:32]))
        return rc == OK and res == want

    def refused(self, name, code, rc, untouched):
        assert rc == code, (name, rc, self.e.L.rvt_last_error(self.e.ctx).decode())
        assert untouched, name
        assert self.e.collect_ready() == []
        assert self.good(name), name                      # the next valid call: the bits of the rows in range


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.e.close()


@pytest.mark.parametrize("name", CALLS)
def test_last_rows_in_range(world, name):
    assert world.good(name)


@pytest.mark.parametrize("name", CALLS)
def test_one_row_too_many(world, name):
    w = world
    if name in ROW_CALLS:
        rc, untouched, _ = w.run(name, w.last, V + 1)
        w.refused(name, E_INVALID, rc, untouched)
        return
    call = GENE_CALLS[name]
    first, second = w.genes_at(w.last)
    rc, untouched, _ = call(w.e, [(second[0], second[1] + 1)])          # a gene whose M runs one past the end
    w.refused(name, E_INVALID, rc, untouched)
    if name != "rvt_submit_gene_bed_dev":                               # the second gene of a list: the first is not queued
        rc, untouched, _ = call(w.e, [first, (second[0], second[1] + 1)])
        w.refused(name, E_INVALID, rc, untouched)


def test_one_row_too_many_debug_calls(world):
    """The three *_timed calls and the other debug calls share their front with one of the calls above: one case each."""
    import rvtests_amd
    e, last = world.e, world.last
    for call in (lambda: e.debug_suffstat_bed_dev(last, V + 1),
                 lambda: e.debug_fam_genes_bed_front_timed([last, last + GENES[0] * PITCH], [GENES[0], GENES[1] + 1], FAM_ALL),
                 lambda: e.debug_rotate_bed(last, V + 1),
                 lambda: e.debug_rotate_bed_timed(last, V + 1),
                 lambda: e.debug_grammar_bed(last, V + 1),
                 lambda: e.debug_grammar_bed_timed(last, V + 1)):
        with pytest.raises(rvtests_amd.RvtError, match="error -1:"):
            call()
    assert e.collect_ready() == []


@pytest.mark.parametrize("name", CALLS)
def test_address_off_a_row_boundary(world, name):
    """(V - 1 rows, a gene of 3, from one byte behind a row's start: inside the matrix's bytes, were they read)"""
    if name in GENE_CALLS:
        rc, untouched, _ = GENE_CALLS[name](world.e, [(world.last + 1, GENES[0])])
    else:
        rc, untouched, _ = world.run(name, world.last + 1, V - 1)
    world.refused(name, E_INVALID, rc, untouched)


def test_upload_range(world):
    w, e = world, world.e
    e.L.rvt_bed_upload.restype = C.c_int
    e.L.rvt_bed_upload.argtypes = [vp, vp, C.c_int64, C.c_int64, vp]
    junk = np.full((3, PITCH), 0xE4, dtype=np.uint8)

    def whole():
        return w.run("rvt_score_bed_dev", w.d_bed, ROWS)[2]
    before = whole()
    assert before
    for first, n in ((ROWS - 2, 3), (ROWS, 1), (ROWS + 1, 0)):
        assert e.L.rvt_bed_upload(e.ctx, vp(w.d_bed), first, n, junk.ctypes.data_as(vp)) == E_INVALID, (first, n)
    assert whole() == before                                            # the matrix is unchanged
    assert e.L.rvt_bed_upload(e.ctx, vp(w.d_bed), ROWS - 3, 3, w.rows[ROWS - 3:].ctypes.data_as(vp)) == OK   # first + n == the end
    assert e.L.rvt_bed_upload(e.ctx, vp(w.d_bed), ROWS, 0, junk.ctypes.data_as(vp)) == OK
    assert whole() == before


def test_changed_n(world):
    """A matrix sized for N = 515 under a null model of N = 519 (pitch 130): refused, not re-read at the other pitch."""
    w = world
    for name in CALLS:
        assert w.good(name), name
    X2, y2 = synth.make_null(N + 4, 3, 0, seed=10)[:2]
    w.e.fit_null(0, X2, y2)
    try:
        for name in CALLS:                                              # (the others: an ordinary null of another N beside theirs)
            rc, untouched, _ = w.run(name, w.last)
            assert rc == E_STATE and untouched, (name, rc)
            assert name not in READS_ORDINARY_NULL or "sized for N = 515" in w.e.L.rvt_last_error(w.e.ctx).decode()
        assert w.e.collect_ready() == []
    finally:
        w.e.fit_null(0, w.X, w.y)
    for name in CALLS:
        assert w.good(name), name


def test_free(world):
    """A matrix of its own, which no call reads: an address inside it, its base, its base again, null."""
    e = world.e
    e.L.rvt_bed_free.restype = C.c_int
    e.L.rvt_bed_free.argtypes = [vp, vp]
    d = e.bed_alloc(3)
    assert e.L.rvt_bed_free(e.ctx, vp(d + PITCH)) == E_INVALID
    assert e.L.rvt_bed_free(e.ctx, vp(d)) == OK
    assert e.L.rvt_bed_free(e.ctx, vp(d)) == E_INVALID
    assert e.L.rvt_bed_free(e.ctx, None) == OK
    assert e.L.rvt_bed_free(e.ctx, vp(world.d_bed + PITCH)) == E_INVALID
    assert world.good("rvt_score_bed_dev")                              # the other matrices are as they were
