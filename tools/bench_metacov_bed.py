#!/usr/bin/env python3
"""MetaCov's band from rows of a resident .bed matrix (rvt_cov_band_bed_dev) beside the two routes a caller has without it,
measured in one run at N = 500 000:

  bed    rvt_cov_band_bed_dev on H + w consecutive resident rows (heads per call H with w / H <= 1/4): variants/s = H / wall
         time of the call, and the call's three device timings (front stage, products + band finish, whole call)
  (a)    rvt_cov_band on a ring block whose H + w columns are already resident with their column cache: the best device route
         without the call — the fp64 columns have crossed PCIe before the clock starts
  (b)    the same including rvt_block_upload_columns of the H + w columns from host memory, a column per call as the adapter
         uploads them: what a caller with a resident matrix has to do without the call

for windows of 200 / 1 000 / 3 000 markers, on rows without a missing call and on rows with 1 % missing.  The rows are 256
distinct drawn rows repeated (the products do not look at the values).  One JSON document: profiles/metacov_bed_bench.json.

usage (GPU box): python tools/bench_metacov_bed.py [--samples 500000] [--window 200,1000,3000] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rvtests_amd  # noqa: E402
import metacov_bed_cases as cases  # noqa: E402

DISTINCT = 256


def heads_for(w):
    """heads per call: w / H <= 1/4, whole 1 024-head passes"""
    return max(1024, (4 * w + 1023) // 1024 * 1024)


def median(v):
    return float(np.median(np.asarray(v)))


def run_bed(eng, d_rows, H, W, w, band, scale, reps):
    eng.set_profiling(True)
    walls, ms = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        eng.cov_band_bed(d_rows, H, W, w, scale=scale, band=band, want_counts=True)
        t1 = time.perf_counter()
        if r:                                                  # (the first call grows the work spaces)
            walls.append(t1 - t0)
            ms.append(eng.cov_band_bed_last_timing())
    eng.set_profiling(False)
    ms = np.asarray(ms)
    return dict(path=eng.cov_band_last_path(), wall_ms=1e3 * median(walls), variants_per_s=H / median(walls),
                front_ms=median(ms[:, 0]), products_ms=median(ms[:, 1]), call_device_ms=median(ms[:, 2]),
                rows_prepared_per_head=W / H)


def run_ring(eng, G, H, W, w, band, scale, reps):
    """(a) and (b): the columns uploaded a column per call (timed once: b), then rvt_cov_band on them (a)"""
    ring = eng.alloc_block(W)
    try:
        t0 = time.perf_counter()
        for j in range(W):
            eng.upload_columns(ring, j, G[:, j % DISTINCT])
        eng.sync()
        t_up = time.perf_counter() - t0
        walls = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            eng.cov_band(ring, W, 0, H, W, w, scale=scale, band=band)
            t1 = time.perf_counter()
            if r:
                walls.append(t1 - t0)
        t = median(walls)
        return dict(path=eng.cov_band_last_path(), a_wall_ms=1e3 * t, a_variants_per_s=H / t, upload_ms=1e3 * t_up,
                    upload_columns_per_s=W / t_up, b_wall_ms=1e3 * (t + t_up), b_variants_per_s=H / (t + t_up))
    finally:
        eng.free_block(ring)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--covariates", type=int, default=3)
    ap.add_argument("--window", default="200,1000,3000")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-ring", action="store_true", help="only the new call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metacov_bed_bench.json"))
    args = ap.parse_args()
    N, d = args.samples, args.covariates
    widths = [int(x) for x in args.window.split(",") if x]
    eng = rvtests_amd.Engine(0)
    X, y, res, v, s2 = cases.null_model(N, d, 0, seed=1)
    eng.set_null(0, X, res, v, s2)
    scale = np.float32(1.0 / N)
    cb = (N + 3) // 4
    runs = []
    for miss in [float(x) for x in args.missing.split(",") if x]:
        rng = np.random.default_rng(11)
        maf = 10 ** rng.uniform(-2.0, -0.7, DISTINCT)
        raw = rng.binomial(2, maf, size=(N, DISTINCT)).astype(np.float64)
        if miss > 0:
            raw[rng.random((N, DISTINCT)) < miss] = -9.0
        raw = np.asfortranarray(raw)
        rows = rvtests_amd.Engine.pack_bed(raw)
        G = cases.imputed(raw)
        for w in widths:
            H = heads_for(w)
            W = H + w
            band = np.zeros((H, w + 1), dtype=np.float32)
            eng.host_register(band)                            # the band lands by DMA, as the adapter's buffer does
            d_bed = eng.bed_alloc(W)
            for r0 in range(0, W, DISTINCT):
                n = min(DISTINCT, W - r0)
                eng.bed_upload(d_bed, r0, rows[:n])
            rec = dict(N=N, d=d, window=w, heads=H, rows=W, missing_rate=miss, row_bytes=cb)
            rec["bed"] = run_bed(eng, d_bed, H, W, w, band, scale, args.reps)
            eng.bed_free(d_bed)
            if not args.no_ring:
                try:
                    rec["ring"] = run_ring(eng, G, H, W, w, band, scale, args.reps)
                except rvtests_amd.RvtError as err:
                    rec["ring"] = dict(skipped=str(err))
            eng.host_unregister(band)
            print(json.dumps(rec), flush=True)
            runs.append(rec)
    eng.close()
    doc = dict(tool="tools/bench_metacov_bed.py", what="rvt_cov_band_bed_dev beside rvt_cov_band on a resident ring (a) and with its "
               "column uploads (b); wall times are medians of %d calls behind a warm-up, device times from HIP events" % args.reps,
               runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
