"""GPU: the dominant / recessive recoding on the device (rvt_block_recode, rvt_bed_recode_block, rvt_block_download_columns)
and `--meta dominant` / `--meta recessive` through the C++ adapters, against the existing oracles (orc.metascore / orc.metacov)
on the numpy-recoded matrix.  The recoding rule is restated here (recode()) from its description:
  missing iff x < 0 (NaN and -0.0 are not); a called value codes to 1 if x > threshold (0.5 dominant, 1.5 recessive) else 0;
  a missing value codes to avg = carriers / nonmissing of the column (0 when nothing is called)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import orc
import synth
import rvtests_amd
from rvtests_amd import CODING_DOMINANT, CODING_RECESSIVE
from test_gpu_metacov import engine_factory  # noqa: F401  (fixture)
from test_gpu_metascore import check
from test_host_driver import DRIVER, _ensure_driver, write_input
from test_meta_coded_cpu import COV_HEADER, sections_of

pytestmark = pytest.mark.gpu

CODINGS = (CODING_DOMINANT, CODING_RECESSIVE)


def recode(raw, coding):
    """(recoded matrix, counts[:, 0] = non-missing calls, counts[:, 1] = carriers) of the raw columns."""
    thr = 0.5 if coding == CODING_DOMINANT else 1.5
    with np.errstate(invalid="ignore"):
        miss = raw < 0
        carrier = ~miss & (raw > thr)
    nonmissing, carriers = (~miss).sum(0), carrier.sum(0)
    avg = np.where(nonmissing > 0, carriers.astype(np.float64) / np.maximum(nonmissing, 1).astype(np.float64), 0.0)
    out = np.where(miss, avg[None, :], carrier.astype(np.float64))
    return np.asfortranarray(out), np.stack([nonmissing, carriers], axis=1).astype(np.int64)


def make_raw(N, V, seed, missing=0.01, special=True):
    """Hard calls with `missing` of -9 and, from V >= 5 on, the special columns:
    0 the values around the thresholds, 1 no missing call, 2 nothing but missing, 3 every called sample a carrier."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.45, V)
    raw = rng.binomial(2, maf, size=(N, V)).astype(np.float64)
    if missing > 0:
        raw[rng.random((N, V)) < missing] = -9.0
    if special and V >= 5:
        vals = [0.5, np.nextafter(0.5, 1), 1.5, np.nextafter(1.5, 2), np.nan, -0.0, -1e-300, 0.3, 1.7]
        raw[3:3 + len(vals), 0] = vals
        raw[:, 1] = np.where(raw[:, 1] < 0, 1.0, raw[:, 1])        # 0 / 1 / 2 only
        raw[:, 2] = -9.0
        raw[:, 3] = np.where(raw[:, 3] < 0, -9.0, 2.0)             # avg 1 under either coding
    return np.asfortranarray(raw)


def same(a, b):
    """bit for bit (NaN nowhere: recoded values are 0, 1 or a quotient of counts)"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.mark.parametrize("ncols", [1, 32, 33, 70])
@pytest.mark.parametrize("N", [1203, 4099, 10007])
def test_recoding_bit_for_bit(engine_factory, monkeypatch, N, ncols):
    """rvt_block_recode -> rvt_block_download_columns equals the restatement, counts included: both codings, in place and into
    another block at another column, the raw columns uploaded one call each and all at once; the neighbours of the written
    range stay as they were.  Uploaded one call each, the columns of hard calls with or without the missing code -9 are still in
    the engine's upload queue when the recoding is asked for (the last matrix: a full queue and more); the column of special
    values crosses as doubles behind whatever was queued.  N = 1203: below the packed-upload switch (4096), odd; 4099: just above it, 3 mod 4; 10007: several
    slices of rows, odd.  ncols around the column queue of 32."""
    monkeypatch.setenv("RVT_POISON", "255")
    total = max(ncols, 5)
    raw_all = make_raw(N, total, seed=N + ncols)
    rng = np.random.default_rng(5)
    eng = engine_factory()
    X = np.column_stack([np.ones(N), rng.normal(size=N)])
    eng.fit_null(0, np.asfortranarray(X), rng.normal(size=N))
    marker = np.asfortranarray(rng.integers(0, 3, size=(N, ncols + 3)).astype(np.float64))
    # (ncols = 1: every special column on its own); then a matrix without any missing call: every column is queued
    windows = [raw_all[:, s:s + ncols] for s in range(0, total - ncols + 1, ncols)]
    windows.append(make_raw(N, ncols, seed=N + ncols + 1, missing=0.0, special=False))
    for raw in windows:
        for coding in CODINGS:
            want, want_cnt = recode(raw, coding)
            for queued in (True, False):
                # in place, columns [1, 1 + ncols) of a block of ncols + 3
                blk = eng.alloc_block(ncols + 3)
                eng.upload_columns(blk, 0, marker[:, :1])         # (the neighbours only: uploads of one column are not
                eng.upload_columns(blk, 1 + ncols, marker[:, 1 + ncols:])   # ordered against each other by the engine)
                if queued:
                    for j in range(ncols):
                        eng.upload_columns(blk, 1 + j, raw[:, j:j + 1])
                else:
                    eng.upload_columns(blk, 1, raw)
                cnt = eng.block_recode(blk, 1, blk, 1, ncols, coding)
                got = eng.download_columns(blk, 0, ncols + 3)
                assert np.array_equal(cnt, want_cnt)
                assert same(got[:, 1:1 + ncols], want)
                assert same(got[:, 0], marker[:, 0]) and same(got[:, 1 + ncols:], marker[:, 1 + ncols:])
                # out of place: the source stays raw, the target's other columns stay
                dst = eng.alloc_block(ncols + 3)
                eng.upload_columns(dst, 0, marker)
                if queued:
                    for j in range(ncols):
                        eng.upload_columns(blk, 1 + j, raw[:, j:j + 1])
                else:
                    eng.upload_columns(blk, 1, raw)
                cnt = eng.block_recode(dst, 2, blk, 1, ncols, coding)
                got = eng.download_columns(dst, 0, ncols + 3)
                src = eng.download_columns(blk, 1, ncols)
                assert np.array_equal(cnt, want_cnt)
                assert same(got[:, 2:2 + ncols], want)
                assert same(got[:, :2], marker[:, :2]) and same(got[:, 2 + ncols:], marker[:, 2 + ncols:])
                assert np.array_equal(src, raw, equal_nan=True)
                eng.free_block(dst)
                eng.free_block(blk)


def _binary_y(X, seed):
    rng = np.random.default_rng(seed)
    lin = -0.5 + (0.3 * X[:, 1] if X.shape[1] > 1 else 0.0)
    return (rng.random(X.shape[0]) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)


def _null_case(N, d, binary, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(d - 1)]))
    y = _binary_y(X, seed + 1) if binary else X @ rng.normal(size=d) + rng.normal(size=N)
    return X, y


@pytest.mark.parametrize("binary", [0, 1])
@pytest.mark.parametrize("N,V,d", [(1203, 33, 1), (4099, 70, 3)])
def test_score_of_recoded_block(engine_factory, monkeypatch, binary, N, V, d):
    """rvt_score_block on a block recoded on the device: the oracle's MetaScore on the numpy-recoded matrix, and the same
    block filled by rvt_block_upload_columns from the host-recoded matrix (same ok; U, V, p to the tolerance between
    kernels of test_score_block_hard_call_slices)."""
    monkeypatch.setenv("RVT_POISON", "255")
    raw = make_raw(N, V, seed=77 + N + binary)
    X, y = _null_case(N, d, binary, 300 + N)
    eng = engine_factory()
    eng.fit_null(binary, X, y)
    for coding in CODINGS:
        want, _ = recode(raw, coding)
        rc, o = orc.metascore(want, X, y, binary)
        assert rc == 0 and 3 < o["ok"].sum() < V
        blk = eng.alloc_block(V)
        eng.upload_columns(blk, 0, raw)
        eng.block_recode(blk, 0, blk, 0, V, coding)
        r = eng.score_block(blk, V)
        check(o, r)
        host = eng.alloc_block(V)
        eng.upload_columns(host, 0, want)
        r2 = eng.score_block(host, V)
        assert np.array_equal(r["ok"], r2["ok"])
        k = o["ok"].astype(bool)
        for f in ("U", "V", "p"):
            assert np.allclose(r[f][k], r2[f][k], rtol=1e-8 if binary else 1e-11, atol=0), f
        eng.free_block(host)
        eng.free_block(blk)


def _fill_ring_raw_and_recode(eng, ring, cap, col0, raw, coding):
    V = raw.shape[1]
    for j in range(V):                                            # one site per call, as the adapters do
        eng.upload_columns(ring, (col0 + j) % cap, raw[:, j:j + 1])
    first = min(V, cap - col0)
    eng.block_recode(ring, col0, ring, col0, first, coding)
    if V > first:
        eng.block_recode(ring, 0, ring, 0, V - first, coding)


def _fill_ring(eng, ring, cap, col0, G):
    V = G.shape[1]
    first = min(V, cap - col0)
    eng.upload_columns(ring, col0, G[:, :first])
    if V > first:
        eng.upload_columns(ring, 0, G[:, first:])


@pytest.mark.parametrize("coding", CODINGS)
@pytest.mark.parametrize("missing,path", [(0.0, 1), (0.01, 4)])
def test_band_of_recoded_ring(engine_factory, monkeypatch, coding, missing, path):
    """rvt_cov_band on a ring of 64 columns filled past its end (the window wraps), recoded on the device, against a second
    ring filled from the host-recoded matrix: the same product (MXFP4 band on the column cache: path 1 without missing calls,
    path 4 — hard calls plus one other value — with them), the same band bit for bit, the same xz and flags."""
    monkeypatch.setenv("RVT_POISON", "255")
    N, V, d, halo, cap, col0 = 4099, 50, 2, 12, 64, 40
    raw = make_raw(N, V, seed=900 + coding, missing=missing, special=False)
    raw[:, 6] = np.where(raw[:, 6] < 0, -9.0, 0.0)                # monomorphic after recoding
    want, _ = recode(raw, coding)
    X, y = _null_case(N, d, 0, 41)
    eng = engine_factory()
    eng.fit_null(0, X, y)
    out = []
    for device in (True, False):
        ring = eng.alloc_block(cap)
        if device:
            _fill_ring_raw_and_recode(eng, ring, cap, col0, raw, coding)
        else:
            _fill_ring(eng, ring, cap, col0, want)
        band = np.full((V, halo + 1), np.nan, dtype=np.float32)
        band, xz, zz, poly = eng.cov_band(ring, cap, col0, V, V, halo, band=band)
        out.append((band.copy(), xz, poly, eng.cov_band_last_path()))
        eng.free_block(ring)
    (b1, xz1, p1, path1), (b2, xz2, p2, path2) = out
    assert path1 == path2 == path
    assert np.array_equal(b1, b2, equal_nan=True)
    assert np.array_equal(xz1, xz2) and np.array_equal(p1, p2) and not p1[6] and p1.sum() > V // 2
    # and it is the oracle's band of the recoded matrix (float32 band: 2e-7 of the largest entry)
    chrom, pos = np.ones(V, dtype=np.int32), np.arange(V, dtype=np.int32)
    rc, kept, ocov, row_end, oxz, ozz = orc.metacov(want, chrom, pos, X, y, 0, halo)
    assert rc == 0 and (p1 == kept).all()
    scale = np.nanmax(np.abs(ocov))
    for h in range(V):
        if kept[h]:
            js = np.arange(h, min(V, h + halo + 1))
            js = js[kept[js].astype(bool)]
            assert np.abs(b1[h, js - h].astype(np.float64) - ocov[h, js]).max() <= 2e-7 * scale


def test_band_of_recoded_ring_binary_trait(engine_factory, monkeypatch):
    """The same two rings under a binary trait (the fp64 band): equal to 1e-11 of the largest entry."""
    monkeypatch.setenv("RVT_POISON", "255")
    N, V, d, halo, cap, col0 = 4099, 50, 2, 12, 64, 40
    raw = make_raw(N, V, seed=950, missing=0.01, special=False)
    X, y = _null_case(N, d, 1, 43)
    eng = engine_factory()
    eng.fit_null(1, X, y)
    for coding in CODINGS:
        want, _ = recode(raw, coding)
        bands = []
        for device in (True, False):
            ring = eng.alloc_block(cap)
            if device:
                _fill_ring_raw_and_recode(eng, ring, cap, col0, raw, coding)
            else:
                _fill_ring(eng, ring, cap, col0, want)
            band = np.full((V, halo + 1), np.nan, dtype=np.float32)
            bands.append(eng.cov_band(ring, cap, col0, V, V, halo, band=band)[0].astype(np.float64).copy())
            assert eng.cov_band_last_path() == 0
            eng.free_block(ring)
        m = ~np.isnan(bands[1])
        assert np.array_equal(np.isnan(bands[0]), np.isnan(bands[1])) and m.sum() > V
        assert np.abs(bands[0][m] - bands[1][m]).max() <= 1e-11 * np.abs(bands[1][m]).max()


@pytest.mark.parametrize("binary", [0, 1])
@pytest.mark.parametrize("N,V", [(4099, 7), (4099, 70), (10007, 7), (10007, 70)])
def test_recoding_of_resident_bed_rows(engine_factory, monkeypatch, binary, N, V):
    """rvt_bed_recode_block: rows of a resident .bed matrix (two other rows in front of them) into the columns of a block —
    the restatement applied to the raw matrix bit for bit, the 0 / 1 / 2 / missing counts, and the score test of the block
    against the oracle.  N = 4099, 10007: the last byte of a row holds three padding samples / one."""
    monkeypatch.setenv("RVT_POISON", "255")
    raw = make_raw(N, V, seed=N + V, special=False)
    raw[:, 1] = np.abs(np.where(raw[:, 1] < 0, 1.0, raw[:, 1]))   # no missing call
    raw[:, 2] = -9.0                                              # nothing but missing
    raw[:, 3] = np.where(raw[:, 3] < 0, -9.0, 2.0)                # every called sample a carrier
    X, y = _null_case(N, 2, binary, 500 + N)
    eng = engine_factory()
    eng.fit_null(binary, X, y)
    cb = (N + 3) // 4
    d_bed = eng.bed_alloc(V + 2)
    eng.bed_upload(d_bed, 0, np.full((2, cb), 0xff, dtype=np.uint8))
    eng.bed_upload(d_bed, 2, eng.pack_bed(raw))
    want_cnt = np.stack([(raw == 0).sum(0), (raw == 1).sum(0), (raw == 2).sum(0), (raw < 0).sum(0)], axis=1)
    for coding in CODINGS:
        want, _ = recode(raw, coding)
        blk = eng.alloc_block(V + 2)
        cnt = eng.bed_recode_block(d_bed + 2 * cb, V, coding, blk, 1)
        got = eng.download_columns(blk, 0, V + 2)
        assert np.array_equal(cnt, want_cnt)
        assert same(got[:, 1:V + 1], want)
        assert not got[:, 0].any() and not got[:, V + 1].any()   # the neighbours keep the zeros of the allocation
        rc, o = orc.metascore(want, X, y, binary)
        assert rc == 0 and o["ok"].sum() >= 3
        r = eng.score_block(blk + 8 * eng.padded_ld(), V)
        check(o, r)
        eng.free_block(blk)
    eng.bed_free(d_bed)


def test_recode_errors(engine_factory):
    N, V = 1203, 6
    raw = make_raw(N, V, seed=3)
    eng = engine_factory()
    with pytest.raises(rvtests_amd.RvtError, match="error -4"):   # RVT_E_STATE: no null model
        eng.block_recode(1 << 20, 0, 1 << 20, 0, 1, CODING_DOMINANT)
    X, y = _null_case(N, 2, 0, 8)
    eng.fit_null(0, X, y)
    blk = eng.alloc_block(V)
    eng.upload_columns(blk, 0, raw)
    for coding in (0, 3):
        with pytest.raises(rvtests_amd.RvtError, match="error -1"):   # RVT_E_INVALID
            eng.block_recode(blk, 0, blk, 0, V, coding)
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.block_recode(blk, 2, blk, 2, V - 1, CODING_DOMINANT)   # one column past the block
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.block_recode(blk, 1, blk, 0, 3, CODING_DOMINANT)       # overlapping ranges that are not the same
    d_bed = eng.bed_alloc(V)
    eng.bed_upload(d_bed, 0, eng.pack_bed(make_raw(N, V, seed=4, special=False)))
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.bed_recode_block(d_bed, V, CODING_RECESSIVE, blk, 1)
    with pytest.raises(rvtests_amd.RvtError, match="error -1"):
        eng.bed_recode_block(d_bed, V, 0, blk, 0)
    assert np.array_equal(eng.download_columns(blk, 0, V), raw, equal_nan=True)   # nothing was written
    eng.bed_free(d_bed)
    eng.free_block(blk)


# ---- the drop-in: host_driver --raw ----------------------------------------------------------------------------------------
def _run(args, env=None):
    p = subprocess.run([DRIVER, "--raw"] + args, capture_output=True, text=True, timeout=300, env=env)
    return p.returncode, p.stdout.splitlines(), p.stderr


def _dropin_case(tmp_path, binary, N=1500, d=3):
    raws = [make_raw(N, M, seed=70 + M, special=False) for M in (30, 25)]
    raws[0][:, 4] = np.where(raws[0][:, 4] < 0, -9.0, 0.0)               # monomorphic, recoded or not
    raws[1][:, 7] = np.where(raws[1][:, 7] < 0, -9.0, np.maximum(raws[1][:, 7], 1.0))   # every call a dominant carrier
    X, y, res, v, s2 = synth.make_null(N, d, binary, seed=9)
    path = str(tmp_path / "in.bin")
    write_input(path, y, X[:, 1:], binary, [(r, np.zeros(r.shape[1])) for r in raws])
    raw = np.asfortranarray(np.concatenate(raws, axis=1))
    V = raw.shape[1]
    pos = np.cumsum(np.random.default_rng(3).integers(1, 300, V)).astype(np.int32)
    chrom = np.where(np.arange(V) < 40, 1, 2).astype(np.int32)
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        for c, p_ in zip(chrom, pos):
            f.write("%d %d\n" % (c, p_))
    return path, sites, raw, chrom, pos, X, y


def _check_score_section(rows_text, raw, want, X, y, binary):
    """rows_text: the section's lines as lists of fields.  Summary header, then one row per site: counters of the RAW calls,
    statistics of the recoded column (NA for a site that is monomorphic after the recoding)."""
    N, V = raw.shape
    rows = [r for r in rows_text if not r[0].startswith("##")]
    assert rows[0][-4:] == ["U_STAT", "SQRT_V_STAT", "ALT_EFFSIZE", "PVALUE"]
    rows = rows[1:]
    assert len(rows) == V
    rc, o = orc.metascore(want, X, y, binary)
    assert rc == 0
    n_na = 0
    for h, row in enumerate(rows):
        g = raw[:, h]
        called = g >= 0
        af = g[called].sum() / (2.0 * called.sum())
        first = lambda t: t.split(":")[0]                         # (binary traits print all:case:control)
        assert float(first(row[2])) == pytest.approx(af, rel=6e-6, abs=1e-12)
        assert float(first(row[4])) == pytest.approx(called.sum() / N, rel=6e-6)
        assert [int(first(row[6])), int(first(row[7])), int(first(row[8]))] == [int((g[called] == 0).sum()), int((g[called] == 1).sum()),
                                                                               int((g[called] == 2).sum())]
        if binary:
            case = called & (y == 1)
            assert float(row[2].split(":")[1]) == pytest.approx(g[case].sum() / (2.0 * case.sum()), rel=6e-6, abs=1e-12)
        stats = row[9:]
        if not o["ok"][h]:
            assert stats == ["NA"] * 4
            n_na += 1
            continue
        for got, w in zip(stats, [o["U"][h], np.sqrt(o["V"][h]), o["effect"][h], o["p"][h]]):
            assert float(got) == pytest.approx(w, rel=6e-6, abs=1e-12)
    assert 0 < n_na < V // 2


def _check_cov_section(rows_text, want, chrom, pos, X, y, binary, window):
    """as test_driver_metacov_rows_match_oracle: the oracle's row structure, numbers after the float / (1/N) / %g formatting"""
    N, V = want.shape
    d = X.shape[1]
    assert rows_text[0] == COV_HEADER
    rows = rows_text[1:]
    rc, kept, cov, row_end, xz, zz = orc.metacov(want, chrom, pos, X, y, binary, window)
    assert rc == 0
    heads = [h for h in range(V) if kept[h]]
    assert len(rows) == len(heads) and len(heads) < V
    scale = np.float32(1.0 / N)
    for row, h in zip(rows, heads):
        js = [j for j in range(h, row_end[h] + 1) if kept[j] and not np.isnan(cov[h, j])]
        assert row[0] == str(chrom[h]) and row[1] == str(pos[h]) and row[2] == str(pos[row_end[h]])
        assert int(row[3]) == len(js)
        assert row[4] == ",".join(str(pos[j]) for j in js)
        parts = row[5].split(":")
        assert len(parts) == (3 if binary else 1)
        got = np.array([float(t) for t in parts[0].split(",")])
        wanted = np.array([float(np.float32(cov[h, j]) * scale) for j in js])
        assert (np.abs(got - wanted) <= 6e-6 * np.abs(wanted) + 1e-30).all()      # %g prints 6 significant digits
        if len(parts) == 3:
            gx = np.array([float(t) for t in parts[1].split(",")])
            wx = np.array([float(np.float32(x) * scale) for x in xz[h]])
            assert np.allclose(gx, wx, rtol=2e-5, atol=1e-5 * max(np.abs(wx).max(), 1e-30))
            gz = np.array([float(t) for t in parts[2].split(",")])
            wz = np.array([zz[a, b] * float(scale) for a in range(d) for b in range(a + 1)])
            assert np.allclose(gz, wz, rtol=2e-5, atol=1e-12)


@pytest.mark.parametrize("binary,name,window,block", [(0, "dominant", 1200, None), (1, "recessive", 450, None),
                                                      (0, "recessive", 450, 16), (1, "dominant", 1200, None)])
def test_driver_coded_rows_match_oracle(tmp_path, binary, name, window, block):
    """--meta dominant / recessive through the C++ adapters on raw calls (host_driver --raw): the score file and the covariance
    file of the recoded columns against the oracles, the window size handed to the covariance model (its row structure),
    block = 16: a device ring far smaller than the stream, flushed mid-stream and wrapped."""
    _ensure_driver()
    path, sites, raw, chrom, pos, X, y = _dropin_case(tmp_path, binary)
    coding = CODING_DOMINANT if name == "dominant" else CODING_RECESSIVE
    Name = "MetaDominant" if name == "dominant" else "MetaRecessive"
    env = dict(os.environ)
    if block:
        env["RVT_METACOV_BLOCK"] = str(block)
        env["RVT_METASCORE_BLOCK"] = str(block)
    rc, lines, err = _run([path, "-", "-", "%s[windowSize=%d]" % (name, window), sites], env)
    assert rc == 0, err
    sec = sections_of(lines)
    assert list(sec) == ["out.%s.assoc" % Name, "out.%sCov.assoc" % Name]
    want, _ = recode(raw, coding)
    _check_score_section(sec["out.%s.assoc" % Name], raw, want, X, y, binary)
    _check_cov_section(sec["out.%sCov.assoc" % Name], want, chrom, pos, X, y, binary, window)


def test_driver_coded_models_leave_the_additive_sections_alone(tmp_path):
    """score,cov,dominant in one invocation: the additive sections are character for character those of a run without
    `dominant`, and the coded sections those of a run of their own."""
    _ensure_driver()
    path, sites, raw, chrom, pos, X, y = _dropin_case(tmp_path, 0)
    rc, both, err = _run([path, "-", "-", "score,cov[windowSize=1200],dominant[windowSize=1200]", sites])
    assert rc == 0, err
    rc, additive, err = _run([path, "-", "-", "score,cov[windowSize=1200]", sites])
    assert rc == 0, err
    rc, coded, err = _run([path, "-", "-", "dominant[windowSize=1200]", sites])
    assert rc == 0, err
    both, additive, coded = sections_of(both), sections_of(additive), sections_of(coded)
    assert list(both) == ["out.MetaScore.assoc", "out.MetaCov.assoc", "out.MetaDominant.assoc", "out.MetaDominantCov.assoc"]
    for k in additive:
        assert both[k] == additive[k] and len(additive[k]) > 10
    for k in coded:
        assert both[k] == coded[k] and len(coded[k]) > 10


def test_driver_coded_models_refuse_a_kinship(tmp_path):
    """With a kinship decomposition the coded models fail every fit with a message: counters and NA in the score file, no row
    in the covariance file, and the run still ends well."""
    _ensure_driver()
    from test_fam_cpu import make_family_case
    N, K, U, S, X, y = make_family_case(45, 2, 61)
    raw = make_raw(N, 12, seed=5, special=False)
    path = str(tmp_path / "in.bin")
    write_input(path, y, X[:, 1:], 0, [(raw, np.zeros(12))])
    kin = str(tmp_path / "kin.bin")
    with open(kin, "wb") as f:
        f.write(struct.pack("<q", N))
        f.write(np.asfortranarray(U, dtype="<f4").tobytes(order="F"))
        f.write(np.ascontiguousarray(S, dtype="<f4").tobytes())
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        for k in range(12):
            f.write("1 %d\n" % (100 + k))
    rc, lines, err = _run([path, "-", "-", "recessive[windowSize=1000]", sites, kin])
    assert rc == 0, err
    sec = sections_of(lines)
    assert list(sec) == ["out.MetaRecessive.assoc", "out.MetaRecessiveCov.assoc"]
    rows = [r for r in sec["out.MetaRecessive.assoc"] if not r[0].startswith("##")][1:]
    assert len(rows) == 12 and all(r[-4:] == ["NA"] * 4 for r in rows)
    assert sec["out.MetaRecessiveCov.assoc"] == [COV_HEADER]
