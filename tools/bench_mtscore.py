#!/usr/bin/env python3
"""Throughput of the multiple-trait score test (rvt_mt_score_block, `--single fastmtscore`).  Writes profiles/mtscore_bench.json
(rewritten after every configuration) and prints it.

Hard calls, V = 1024 variants per block (--distinct columns generated, repeated), N in {100 000, 500 000} samples, T in {16, 256,
2048} traits = tests, two covariates shared by all tests, 5 % missing phenotypes per trait (every trait its own pattern).
Per configuration: the call's seconds (median of --reps after a warm-up, host clock around the synchronous call), variant-tests
per second, the share of the call in its three phases (rvt_mt_last_timing: genotype pass, products, finishing kernel with the
copy of the results) and the product's int8 operations per second per plane pair: 2 N V (6 R + K) operations for R = T + 2
resident rows of six planes and K patterns of one plane ("useful"), and the same with R and K rounded up to the 256-row panels the
kernel computes ("issued").
The route without this entry point, at T = 16 on complete data: one rvt_fit_null + rvt_score_block per trait over the same
block; the ratio is given with the null fits (one block per analysis) and without them (a long analysis, nulls installed once
per pass over the genotypes).
usage (GPU box): python tools/bench_mtscore.py [--samples 100000,500000] [--traits 16,256,2048] [--variants 1024] [--reps 3]"""
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


def upload_tiled(eng, G, V):
    """A block of V columns: the distinct columns of G repeated."""
    ptr = eng.alloc_block(V)
    ld = eng.padded_ld()
    dp = C.POINTER(C.c_double)
    for c0 in range(0, V, G.shape[1]):
        n = min(G.shape[1], V - c0)
        eng._check(eng.L.rvt_block_upload(eng.ctx, C.c_void_p(ptr + 8 * ld * c0), n, G.ctypes.data_as(dp)))
    return ptr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="100000,500000")
    ap.add_argument("--traits", default="16,256,2048")
    ap.add_argument("--variants", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtscore_bench.json"))
    a = ap.parse_args()
    V = a.variants
    res = {"what": "rvt_mt_score_block, hard calls, V = %d per block, 2 shared covariates, 5 %% missing phenotypes per trait" % V,
           "timing": "median of %d synchronous calls after a warm-up, host clock" % a.reps, "configs": []}

    if os.path.exists(a.out):  # (a kernel-trace summary recorded beside the rates stays with the file)
        try:
            old = json.load(open(a.out))
            if "kernel_trace" in old:
                res["kernel_trace"] = old["kernel_trace"]
        except ValueError:
            pass

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for N in [int(s) for s in a.samples.split(",")]:
        eng = rvtests_amd.Engine(0)  # (a context per sample count: the per-trait route leaves its null model behind)
        rng = np.random.default_rng(N)
        maf = rng.uniform(0.005, 0.5, a.distinct)
        G = np.empty((N, a.distinct), order="F")
        for j in range(a.distinct):
            G[:, j] = (rng.random((N, 2), dtype=np.float32) < maf[j]).sum(1)
        Z = np.asfortranarray(rng.standard_normal((N, 2)) * [1.0, 8.0] + [0.0, 50.0])
        for T in [int(s) for s in a.traits.split(",")]:
            Y = np.empty((N, T), order="F")
            for j in range(T):
                y = rng.standard_normal(N, dtype=np.float32).astype(np.float64) * (1.0 + j % 7) + 0.3 * Z[:, 0] + 10.0 * (j % 5)
                y[rng.random(N, dtype=np.float32) < 0.05] = np.nan
                Y[:, j] = y
            tests = [(j, [0, 1]) for j in range(T)]
            t0 = time.perf_counter()
            nul = eng.mt_fit_null(Y, Z, tests)
            t_null = time.perf_counter() - t0
            ptr = upload_tiled(eng, G, V)
            dt, out = timed(lambda: eng.mt_score_block(ptr, V), a.reps)
            ms = eng.mt_last_timing()
            R, K = T + 2, T
            pad = lambda n: (n + 255) // 256 * 256  # noqa: E731
            t_prod = ms[1] * 1e-3
            cfg = {"N": N, "T": T, "V": V, "patterns": K, "tests_ok": int(nul["ok"].sum()), "s_fit_null": t_null, "s_per_block": dt,
                   "variant_tests_per_s": V * T / dt,
                   "ms_genotype_pass": float(ms[0]), "ms_products": float(ms[1]), "ms_finish_and_copy": float(ms[2]),
                   "share_genotype_pass": float(ms[0] / ms.sum()), "share_products": float(ms[1] / ms.sum()),
                   "share_finish_and_copy": float(ms[2] / ms.sum()),
                   "output_tiles_value_product": (pad(R) // 256) * (pad(V) // 256),
                   "product_pops_per_plane_pair_useful": 2.0 * N * V * (6 * R + K) / t_prod / 1e15,
                   "product_pops_per_plane_pair_issued": 2.0 * N * pad(V) * (6 * pad(R) + pad(K)) / t_prod / 1e15,
                   "finite_p": int(np.isfinite(out["p"]).sum())}
            eng.free_block(ptr)
            if T == 16:
                # the route without rvt_mt_*: one null model and one pass over the block per trait, on complete data
                Yc = np.asfortranarray(np.where(np.isnan(Y), 0.0, Y))
                X = np.asfortranarray(np.column_stack([np.ones(N), Z]))
                eng.mt_fit_null(Yc, Z, tests)
                ptr = upload_tiled(eng, G, V)
                dt_mt, out_mt = timed(lambda: eng.mt_score_block(ptr, V), a.reps)
                eng.free_block(ptr)
                eng.mt_clear()
                eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, Yc[:, 0])
                ptr = upload_tiled(eng, G, V)
                eng.score_block(ptr, V)  # warm-up
                t_fit, t_score = [], []
                for _ in range(a.reps):
                    f = s = 0.0
                    for j in range(T):
                        t0 = time.perf_counter()
                        eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, Yc[:, j])
                        t1 = time.perf_counter()
                        r = eng.score_block(ptr, V)
                        s += time.perf_counter() - t1
                        f += t1 - t0
                    t_fit.append(f)
                    t_score.append(s)
                eng.free_block(ptr)
                f, s = float(np.median(t_fit)), float(np.median(t_score))
                # the two routes give the same p-values (the last trait of the last repetition)
                ok = r["ok"] == 1
                agree = float(np.nanmax(np.abs(out_mt["p"][ok, T - 1] - r["p"][ok]) / r["p"][ok]))
                cfg["per_trait_route_complete_data"] = {
                    "s_per_block_mt": dt_mt, "s_16_fit_null": f, "s_16_score_block": s,
                    "ratio_with_null_fits": (f + s) / dt_mt, "ratio_score_blocks_only": s / dt_mt,
                    "max_rel_p_difference_last_trait": agree}
            res["configs"].append(cfg)
            save()
            print(json.dumps(cfg), flush=True)
            del Y
        eng.close()
    save()


if __name__ == "__main__":
    main()
