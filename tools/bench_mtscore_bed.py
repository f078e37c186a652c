#!/usr/bin/env python3
"""The multiple-trait score test over rows of a resident .bed matrix (rvt_mt_score_bed_dev) against rvt_mt_score_block on the same
calls.  Writes profiles/mtscore_bed_bench.json (rewritten after every configuration) and prints it.

The shapes of tools/bench_mtscore.py: V = 1024 variants per block (--distinct rows generated, repeated), N in {100 000, 500 000},
T in {16, 256, 2048} traits = tests, two covariates shared by all tests, 5 % missing phenotypes per trait (every trait its own
pattern).  Genotype rows without a missing call and with 1 % missing calls (every row then has some).
Per configuration: seconds per block (median of --reps synchronous calls after a warm-up, host clock) and the three phases of the
call (rvt_mt_last_timing: front stage, products with the combine, finishing kernel with the copy of the results), for
  bed    rvt_mt_score_bed_dev on the resident rows,
  (a)    rvt_mt_score_block on the same columns — missing calls at the mean of the called ones — as fp64 already on the device,
  (b)    (a) plus the upload of those V columns from host memory (rvt_block_upload, timed by itself),
and the ratios (a) / bed, (b) / bed and products (a) / products bed; the largest relative difference of the finite p-values of
the two routes is recorded with them.
usage (GPU box): python tools/bench_mtscore_bed.py [--samples 100000,500000] [--traits 16,256,2048] [--variants 1024] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rvtests_amd  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def upload_tiled(eng, ptr, G, V):
    """The distinct columns of G repeated into the V columns of the block at ptr."""
    ld = eng.padded_ld()
    dp = C.POINTER(C.c_double)
    for c0 in range(0, V, G.shape[1]):
        n = min(G.shape[1], V - c0)
        eng._check(eng.L.rvt_block_upload(eng.ctx, C.c_void_p(ptr + 8 * ld * c0), n, G.ctypes.data_as(dp)))


def phases(eng):
    ms = eng.mt_last_timing()
    return {"ms_front": float(ms[0]), "ms_products": float(ms[1]), "ms_finish_and_copy": float(ms[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="100000,500000")
    ap.add_argument("--traits", default="16,256,2048")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--variants", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtscore_bed_bench.json"))
    a = ap.parse_args()
    V = a.variants
    res = {"what": "rvt_mt_score_bed_dev against rvt_mt_score_block, V = %d per block, 2 shared covariates, 5 %% missing phenotypes "
                   "per trait" % V,
           "timing": "median of %d synchronous calls after a warm-up, host clock; phases from rvt_mt_last_timing" % a.reps,
           "configs": []}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    traits = [int(s) for s in a.traits.split(",")]
    for N in [int(s) for s in a.samples.split(",")]:
        eng = rvtests_amd.Engine(0)
        rng = np.random.default_rng(N)
        maf = rng.uniform(0.005, 0.5, a.distinct)
        raw0 = np.empty((N, a.distinct), dtype=np.int8, order="F")
        for j in range(a.distinct):
            raw0[:, j] = (rng.random((N, 2), dtype=np.float32) < maf[j]).sum(1)
        Z = np.asfortranarray(rng.standard_normal((N, 2)) * [1.0, 8.0] + [0.0, 50.0])
        Yall = np.empty((N, max(traits)), order="F")
        for j in range(Yall.shape[1]):
            y = rng.standard_normal(N, dtype=np.float32).astype(np.float64) * (1.0 + j % 7) + 0.3 * Z[:, 0] + 10.0 * (j % 5)
            y[rng.random(N, dtype=np.float32) < 0.05] = np.nan
            Yall[:, j] = y
        sets = []
        for rate in [float(s) for s in a.missing.split(",")]:
            raw = raw0.copy(order="F")
            if rate > 0:
                raw[rng.random(raw.shape, dtype=np.float32) < rate] = -9
            G = np.empty((N, a.distinct), order="F")                     # the columns a caller of the block route uploads
            for j in range(a.distinct):
                g = raw[:, j].astype(np.float64)
                miss = g < 0
                g[miss] = g[~miss].mean()
                G[:, j] = g
            rows = rvtests_amd.Engine.pack_bed(raw)
            sets.append((rate, np.ascontiguousarray(rows[np.arange(V) % a.distinct]), G, int((raw < 0).any(0).sum())))
        for T in traits:
            Y = Yall[:, :T]
            tests = [(j, [0, 1]) for j in range(T)]
            eng.mt_fit_null(Y, Z, tests)
            for rate, rows, G, rows_missing in sets:
                d_bed = eng.bed_alloc(V)
                eng.bed_upload(d_bed, 0, rows)
                dt_bed, out_bed = timed(lambda: eng.mt_score_bed_dev(d_bed, V, want_counts=False), a.reps)
                ph_bed = phases(eng)
                eng.bed_free(d_bed)
                ptr = eng.alloc_block(V)
                dt_up, _ = timed(lambda: upload_tiled(eng, ptr, G, V), a.reps)
                dt_blk, out_blk = timed(lambda: eng.mt_score_block(ptr, V), a.reps)
                ph_blk = phases(eng)
                eng.free_block(ptr)
                fin = np.isfinite(out_blk["p"]) & (out_blk["p"] > 0)
                cfg = {"N": N, "T": T, "V": V, "missing_rate": rate, "distinct_rows_with_a_missing_call": rows_missing,
                       "bed": dict(s_per_block=dt_bed, variant_tests_per_s=V * T / dt_bed, **ph_bed),
                       "block_a": dict(s_per_block=dt_blk, variant_tests_per_s=V * T / dt_blk, **ph_blk),
                       "s_upload_of_the_columns": dt_up,
                       "ratio_a": dt_blk / dt_bed, "ratio_b": (dt_blk + dt_up) / dt_bed,
                       "ratio_products_a": ph_blk["ms_products"] / ph_bed["ms_products"],
                       "ratio_front_a": ph_blk["ms_front"] / ph_bed["ms_front"],
                       "same_nan_pattern": bool(np.array_equal(np.isnan(out_bed["p"]), np.isnan(out_blk["p"]))),
                       "same_bits_as_block": bool(all(np.array_equal(out_bed[k].view(np.uint64), out_blk[k].view(np.uint64))
                                                      for k in ("U", "V", "p"))),
                       "max_rel_p_difference": float(np.max(np.abs(out_bed["p"][fin] - out_blk["p"][fin]) / out_blk["p"][fin]))}
                res["configs"].append(cfg)
                save()
                print(json.dumps(cfg), flush=True)
        eng.close()
    save()


if __name__ == "__main__":
    main()
