"""GPU: a gene's record does not depend on which pooled block it got.  The streaming interface keeps the device blocks of
collected genes (rvtests_amd/csrc/block_pool.h) and hands the smallest fitting one out again — a packed block only when it
is at most four times the need.  On one engine: genes of 40 variants, then 3 (40 rows are more than four times 3 rows: a new
block), then 17 (reuses a 40-row block, whose capacity is not its need), then 40 again — through every entry point that
leases blocks, with missing calls in every gene.  Every record equals, bit for bit, the record of the same gene submitted
alone to a fresh engine.  N = 4099: above the 4096 samples from which int8 and fp64 genes are packed on the way, and no
multiple of 4 or 16, so the pad bits of a row's last byte and the pad bytes of a row's pitch are both in play; N = 130: the
unstaged routes."""
import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu

WIDTHS = (40, 3, 17, 40)
ROUTES = ("submit_gene_bed", "submit_gene_i8", "submit_gene", "submit_genes_bed_dev", "score_bed_dev")


def _raw_gene(N, M, seed):
    rng = np.random.default_rng(seed)
    maf = 10 ** rng.uniform(-2.0, -0.5, M)
    raw = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    raw[rng.random((N, M)) < 0.03] = -9.0
    raw[5, :] = -9.0                                           # (a missing call in every column, whatever the draw)
    return np.asfortranarray(raw)


def _same_bits(a, b):
    """Every field of the record, NaN equal to NaN.  The AnalyticVT block too: the test is not requested here (such a gene is
    never kept packed), and the p-value kernel then writes zeros there (pvalue_clear_vt)."""
    for name, _ in type(a)._fields_:
        x, y = getattr(a, name), getattr(b, name)
        assert x == y or (x != x and y != y), (name, x, y)


class _Run:
    """One engine under the null model of the case; the resident matrix holds every gene's rows (three other rows in front:
    the genes' rows start at odd addresses)."""

    def __init__(self, null, genes):
        import rvtests_amd
        self.e = rvtests_amd.Engine(0)
        self.e.set_null(0, *null)
        self.genes = genes
        self.cb = (genes[0].shape[0] + 3) // 4
        self.d_bed = None
        self.first = np.concatenate([[0], np.cumsum([g.shape[1] for g in genes])[:-1]]) + 3

    def resident(self, k):
        if self.d_bed is None:
            self.d_bed = self.e.bed_alloc(int(self.first[-1]) + self.genes[-1].shape[1] + 1)
            self.e.bed_upload(self.d_bed, 0, np.full((3, self.cb), 0x55, dtype=np.uint8))
            for f, g in zip(self.first, self.genes):
                self.e.bed_upload(self.d_bed, int(f), self.e.pack_bed(g))
        return self.d_bed + int(self.first[k]) * self.cb

    def gene(self, route, k):
        """Gene k through `route`, collected: what the entry point returns (frequencies / statistics) and the record."""
        e, raw = self.e, self.genes[k]
        M = raw.shape[1]
        if route == "score_bed_dev":
            return e.score_bed_dev(self.resident(k), M), None
        if route == "submit_gene_bed":
            af = e.submit_gene_bed(k, e.pack_bed(raw), M)
        elif route == "submit_gene_i8":
            af = e.submit_gene_raw(k, raw.astype(np.int8))
        elif route == "submit_gene":
            af = orc.counter_af(raw)
            e.submit_gene(k, orc.impute_mean(raw), af)
        else:
            af = None
            e.submit_genes_bed_dev([k], [self.resident(k)], [M])
        (rec,) = e.collect()
        return (af,), rec

    def close(self):
        if self.d_bed is not None:
            self.e.bed_free(self.d_bed)
        self.e.close()


@pytest.mark.parametrize("N", [4099, 130])
@pytest.mark.parametrize("route", ROUTES)
def test_records_do_not_depend_on_the_block_a_gene_got(route, N):
    genes = [_raw_gene(N, M, seed=100 * k + M) for k, M in enumerate(WIDTHS)]
    X, y, res, v, s2 = synth.make_null(N, 2, 0, seed=8)
    null = (X, res, v, s2)
    one = _Run(null, genes)
    try:
        if route == "score_bed_dev":
            # (its slices take 32-row blocks: a pooled 40-row block serves them, with a capacity that is not their need)
            one.gene("submit_genes_bed_dev", 0)
        got = [one.gene(route, k) for k in range(len(genes))]
    finally:
        one.close()
    for k in range(len(genes)):
        alone = _Run(null, genes)
        try:
            want_out, want_rec = alone.gene(route, k)
        finally:
            alone.close()
        got_out, got_rec = got[k]
        for a, b in zip(got_out, want_out):
            if a is not None:
                assert a.tobytes() == b.tobytes(), (k, a, b)
        if want_rec is not None:
            _same_bits(got_rec, want_rec)
