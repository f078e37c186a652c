#!/usr/bin/env python3
"""Throughput of the MetaScore single-variant statistics (rvt_score_block) at full size: one device block of V
variants, N samples, read once (8 N V algorithmic bytes).  Reports ms per block, variants per second and the
algorithmic bandwidth.  usage (GPU box): python tools/bench_metascore.py [--samples 500000] [--variants 4096]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rvtests_amd  # noqa: E402
import bench  # noqa: E402


def median_call(fn, reps):
    fn()                                                     # work spaces, digit planes
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))], out


def binary_leg(N, rows, reps, block_cols=2048, d=4, distinct=256):
    """rvt_score_bed_dev under a binary null model on `rows` resident rows (the `distinct` generated rows repeated; 1 % missing
    calls; no counts), and on the same rows: (a) rvt_score_block under the same null from an fp64 block of the imputed columns
    that is already on the device — the route a case-control cohort had before, its uploads not charged; (b) rvt_score_bed_dev
    under a quantitative null — one pass and one tile column fewer.  Also the rows with every 2 turned into a 1: no wave-part
    holds a 2, so the third pass is skipped and the difference is its cost."""
    rng = np.random.default_rng(N)
    raw = rng.binomial(2, 10 ** rng.uniform(-2.5, -0.4, distinct), size=(N, distinct)).astype(np.float32)
    raw[rng.random((N, distinct)) < 0.01] = -9.0
    X = np.asfortranarray(np.column_stack([np.ones(N)] + [rng.normal(size=N) for _ in range(d - 1)]))
    lin = X @ np.array([-1.0, 0.3, -0.2, 0.1][:d]) + 0.3 * np.maximum(raw[:, 7], 0)
    yb = (rng.random(N) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    yq = lin + rng.normal(size=N)
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_BINARY, X, yb)
    packed = eng.pack_bed(raw)
    d_bed = eng.bed_alloc(rows)
    for r0 in range(0, rows, distinct):
        eng.bed_upload(d_bed, r0, packed[:min(distinct, rows - r0)])
    no_hom = eng.pack_bed(np.where(raw == 2, 1.0, raw))
    d_bed1 = eng.bed_alloc(rows)
    for r0 in range(0, rows, distinct):
        eng.bed_upload(d_bed1, r0, no_hom[:min(distinct, rows - r0)])
    dt_b, mm_b, out_b = median_call(lambda: eng.score_bed_dev(d_bed, rows, want_counts=False), reps)
    dt_1, mm_1, out_1 = median_call(lambda: eng.score_bed_dev(d_bed1, rows, want_counts=False), reps)
    # (a) the imputed columns as doubles, uploaded before the clock starts
    nn = (raw >= 0).sum(0)
    mu = np.where(nn > 0, np.where(raw >= 0, raw, 0).sum(0, dtype=np.float64) / np.maximum(nn, 1), 0.0)
    G = np.asfortranarray(np.where(raw >= 0, raw, mu[None, :]), dtype=np.float64)
    ptr = eng.alloc_block(block_cols)
    for j in range(0, block_cols, distinct):
        eng.upload_columns(ptr, j, G[:, :min(distinct, block_cols - j)])
    dt_a, mm_a, out_a = median_call(lambda: eng.score_block(ptr, block_cols), reps)
    eng.free_block(ptr)
    k = out_a["ok"][:distinct].astype(bool) & out_b[0][:distinct].astype(bool)
    dev = {f: float(np.max(np.abs(out_b[i + 1][:distinct][k] - out_a[f][:distinct][k]) / np.abs(out_a[f][:distinct][k])))
           for i, f in enumerate(("U", "V", "effect", "se", "p"))}
    # (b) the same rows under a quantitative null
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, yq)
    dt_q, mm_q, out_q = median_call(lambda: eng.score_bed_dev(d_bed, rows, want_counts=False), reps)
    eng.bed_free(d_bed)
    eng.bed_free(d_bed1)
    eng.close()
    return {"N": N, "resident_rows": rows, "d": d, "missing": 0.01, "reps": reps,
            "binary_resident": {"ms_per_call": 1e3 * dt_b, "ms_min_max": [1e3 * t for t in mm_b], "variants_per_s": rows / dt_b,
                                "device_GBps_of_codes": (N / 4.0) * rows / dt_b / 1e9, "tested": int(out_b[0].sum())},
            "binary_resident_rows_without_a_2": {"ms_per_call": 1e3 * dt_1, "ms_min_max": [1e3 * t for t in mm_1],
                                                 "variants_per_s": rows / dt_1},
            "a_binary_fp64_block": {"columns": block_cols, "ms_per_call": 1e3 * dt_a, "ms_min_max": [1e3 * t for t in mm_a],
                                    "variants_per_s": block_cols / dt_a, "tested": int(out_a["ok"].sum())},
            "b_quantitative_resident": {"ms_per_call": 1e3 * dt_q, "ms_min_max": [1e3 * t for t in mm_q],
                                        "variants_per_s": rows / dt_q, "tested": int(out_q[0].sum())},
            "binary_over_fp64_block": (rows / dt_b) / (block_cols / dt_a),
            "faster_than_fp64_block": bool(rows / dt_b > block_cols / dt_a),   # the expectation: 1/32 of the bytes, same cores
            "binary_over_quantitative": dt_q / dt_b,
            "third_pass_share_of_call": (dt_b - dt_1) / dt_b,
            "worst_relative_deviation_from_fp64_block": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--binary", action="store_true",
                    help="resident rows under a binary null model at N = 200 000 and 500 000 -> profiles/score_bed_binary_bench.json")
    ap.add_argument("--rows", type=int, default=65536, help="--binary: resident rows per call")
    a = ap.parse_args()
    if a.binary:
        import json
        res = {"tool": "tools/bench_metascore.py --binary", "results": [binary_leg(N, a.rows, a.reps) for N in (200000, 500000)]}
        for r in res["results"]:
            print(json.dumps(r))
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_bed_binary_bench.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        slower = [r["N"] for r in res["results"] if not r["faster_than_fp64_block"]]
        if slower:                                           # a finding for DESIGN.md §3.4b, written down above; say so loudly
            sys.exit("the resident rows under a binary null are NOT faster than the fp64 blocks at N = %s" % slower)
        return
    dev = torch.device("cuda:0")
    N, V = a.samples, a.variants
    eng = rvtests_amd.Engine(0)
    ld = eng.padded_ld(N)
    X, y, res, sigma2 = bench.fit_null_qt(dev, N, 7)
    eng.set_null(rvtests_amd.TRAIT_QUANTITATIVE, np.asfortranarray(X.cpu().numpy()), res.cpu().numpy().copy(),
                 np.full(N, float(sigma2)), float(sigma2))
    blocks, Ms, afs = bench.make_genes(dev, N, ld, 1, 5, V, V)
    torch.cuda.synchronize()
    def timed(ptr):                                          # median of single calls: the pool's boxes are shared
        eng.score_block(ptr, V)
        ts = []
        for _ in range(max(a.reps, 7)):
            t0 = time.perf_counter()
            out = eng.score_block(ptr, V)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    dt, r = timed(blocks[0].data_ptr())
    print({"N": N, "V": V, "kernel": "general fp64 (content of the block unknown)", "ms_per_block": 1e3 * dt,
           "variants_per_s": V / dt, "alg_GBps": 8.0 * N * V / dt / 1e9, "tested": int(r["ok"].sum())})
    # the same block as hard calls whose content is known (rvt_block_classify; the adapters get it per column for free
    # when they upload): slices of 32 columns through the int8 kernel
    hard = torch.round(blocks[0]).contiguous()
    assert eng.classify_block(hard.data_ptr(), V)
    dt, r = timed(hard.data_ptr())
    print({"N": N, "V": V, "kernel": "hard-call int8", "ms_per_block": 1e3 * dt, "variants_per_s": V / dt,
           "alg_GBps": 8.0 * N * V / dt / 1e9, "tested": int(r["ok"].sum())})
    # the same hard calls as a RESIDENT .bed matrix (rvt_score_bed_dev): N/4 bytes per site instead of 8 N
    packed = eng.pack_bed(np.asfortranarray(hard[:256, :N].T.cpu().numpy()))
    rows = 32768
    d_bed = eng.bed_alloc(rows)
    for r0 in range(0, rows, packed.shape[0]):
        eng.bed_upload(d_bed, r0, packed[:min(packed.shape[0], rows - r0)])
    eng.score_bed_dev(d_bed, rows, want_counts=False)
    ts = []
    for _ in range(max(a.reps, 7)):
        t0 = time.perf_counter()
        out = eng.score_bed_dev(d_bed, rows)
        ts.append(time.perf_counter() - t0)
    dt = float(np.median(ts))                                 # (the pool's boxes are shared: single calls scatter by 2x)
    print({"N": N, "V": rows, "kernel": "resident .bed rows (gene_tnull_hcp<2, score>)", "ms_per_call": 1e3 * dt,
           "ms_per_call_min_max": [1e3 * min(ts), 1e3 * max(ts)],
           "variants_per_s": rows / dt, "device_GBps_of_codes": (N / 4.0) * rows / dt / 1e9,
           "alg_GBps_at_8N_per_site": 8.0 * N * rows / dt / 1e9, "tested": int(out[0].sum())})
    eng.bed_free(d_bed)


if __name__ == "__main__":
    main()
