#!/usr/bin/env python3
"""RareCover and Madsen-Browning (--burden rarecover, mb) beside Price's variable-threshold test (rvt_vtprice_blocks) on the SAME
genes and the same null 0 / 1 phenotype in the same run: shuffles/s and genes/s in both permutation modes, on the two shapes of
tools/bench_vtprice.py — N = 500 000, M ~ U{20..80}, MAF log-uniform 5e-4..5e-2, and N = 50 000, M = 30.  alpha = 1 keeps the stop
rule from ending a gene early, so every gene runs exactly nPerm shuffles in all three tests.  Three repeats each; writes
profiles/burdenperm_bench.json.
usage (GPU box): python tools/bench_burdenperm.py [--quick] [--kernel-stats rocprofv3_kernel_stats.csv [--no-run]] [--out FILE]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rvtests_amd  # noqa: E402


def make_genes(rng, N, n, mlo, mhi):
    genes = []
    for _ in range(n):
        M = int(rng.integers(mlo, mhi + 1))
        maf = np.exp(rng.uniform(np.log(5e-4), np.log(5e-2), M))
        G = np.empty((N, M), order="F")
        for j in range(M):
            G[:, j] = rng.binomial(2, maf[j], size=N)
        genes.append((G, G.sum(0) / (2.0 * N)))
    return genes


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def shape(name_of_shape, N, n_genes, mlo, mhi, nperm_counter, nperm_exact, n_exact, repeats, seed):
    rng = np.random.default_rng(seed)
    genes = make_genes(rng, N, n_genes, mlo, mhi)
    y = (rng.random(N) < 0.5).astype(np.float64)
    eng = rvtests_amd.Engine(0)
    eng.fit_null(1, np.asfortranarray(np.ones((N, 1))), y.copy())
    ptrs = [eng.upload_block(G) for G, af in genes]
    Ms, afs = [G.shape[1] for G, af in genes], [af for G, af in genes]
    rec = {"shape": name_of_shape, "N": N, "genes": n_genes, "M": Ms, "repeats": repeats}
    for mode, nperm, k in (("counter", nperm_counter, n_genes), ("exact", nperm_exact, n_exact)):
        eng.set_perm_exact(mode == "exact")
        runs = {"rarecover": lambda: eng.rarecover_blocks(ptrs[:k], Ms[:k], y, nperm, 1.0),
                "mb": lambda: eng.mb_blocks(ptrs[:k], Ms[:k], y, nperm, 1.0),
                "vt": lambda: eng.vtprice_blocks(ptrs[:k], Ms[:k], afs[:k], y, nperm, 1.0)}
        eng.rand_seed(1)
        rec[mode] = {"nperm": nperm, "genes": k}
        rates = {}
        for name, run in runs.items():
            run()                                                      # warm-up: buffers, code objects
            ts, out = timed(run, repeats)
            done = sum(r.actual_perm for r in out)
            assert done == nperm * k and all(r.fit_ok for r in out), (name, done)
            rates[name] = [done / t for t in ts]
            rec[mode][name + "_shuffles_per_s"] = rates[name]
            rec[mode][name + "_genes_per_s"] = [k / t for t in ts]
            rec[mode][name + "_spread"] = (max(rates[name]) - min(rates[name])) / float(np.median(rates[name]))
            if name == "rarecover":
                rec[mode]["carriers_per_gene"] = [int(r.n_carrier) for r in out]
                rec[mode]["selected_per_gene"] = [int(r.n_selected) for r in out]
            if name == "mb":
                rec[mode]["entries_per_gene"] = [int(r.n_entries) for r in out]
        for name in ("rarecover", "mb"):
            rec[mode][name + "_over_vt_median"] = float(np.median(rates[name]) / np.median(rates["vt"]))
        print(json.dumps({"shape": name_of_shape, "mode": mode, **{a: rec[mode][a] for a in rec[mode] if a.endswith(("_per_s", "_median"))}}),
              flush=True)
    for p in ptrs:
        eng.free_block(p)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a functional run of the tool")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of one rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burdenperm_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-run", action="store_true", help="only merge --kernel-stats into the existing --out file")
    a = ap.parse_args()
    if a.quick:
        shapes = [("quick_N20000", 20000, 3, 20, 40, 2000, 200, 2)]
    else:
        shapes = [("configs2_N500000_M20-80", 500000, 6, 20, 80, 10000, 600, 2), ("configs1_N50000_M30", 50000, 8, 30, 30, 10000, 2000, 4)]
    result = {"device": "MI355X (gfx950)", "alpha": 1.0, "trait": "null 0 / 1 phenotype, half cases", "shapes": []}
    if os.path.exists(a.out):  # keep what an earlier run recorded (the kernel times of the profiled run)
        try:
            result["kernel_stats"] = json.load(open(a.out)).get("kernel_stats")
        except ValueError:
            pass
    if a.no_run:
        result = json.load(open(a.out))
    for k, s in enumerate([] if a.no_run else shapes):
        result["shapes"].append(shape(*s, repeats=a.repeats, seed=17 + k))
    if a.kernel_stats:
        rows = []
        for r in csv.DictReader(open(a.kernel_stats)):
            if any(w in r.get("Name", "") for w in ("rc_", "mb_", "bp_", "vtp_", "perm_", "fam_", "rot_")):
                rows.append({"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                             "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])})
        result["kernel_stats"] = rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
