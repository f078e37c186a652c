#!/usr/bin/env python3
"""Price's variable-threshold permutation test (--vt price) beside the SKAT permutation test on the SAME genes in the same run:
shuffles/s and genes/s in both permutation modes, carrier entries per gene, on two shapes with a null quantitative trait —
N = 500 000, M ~ U{20..80}, MAF log-uniform 5e-4..5e-2, and N = 50 000, M = 30.  alpha = 1 keeps the stop rule from ending a
gene early, so every gene runs exactly nPerm shuffles in both tests.  Three repeats each; writes profiles/vtprice_bench.json.
usage (GPU box): python tools/bench_vtprice.py [--quick] [--kernel-stats rocprofv3_kernel_stats.csv [--no-run]] [--out FILE]"""
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


def shape(name, N, n_genes, mlo, mhi, nperm_counter, nperm_exact, n_exact, repeats, seed):
    rng = np.random.default_rng(seed)
    genes = make_genes(rng, N, n_genes, mlo, mhi)
    y = rng.normal(size=N)
    eng = rvtests_amd.Engine(0)
    eng.fit_null(0, np.asfortranarray(np.ones((N, 1))), y.copy())
    ptrs = [eng.upload_block(G) for G, af in genes]
    Ms, afs = [G.shape[1] for G, af in genes], [af for G, af in genes]
    distinct = [int((G >= 1.0).any(1).sum()) for G, af in genes]  # samples that carry at least one variant of the gene
    rec = {"shape": name, "N": N, "genes": n_genes, "M": Ms, "repeats": repeats}
    for mode, nperm, k in (("counter", nperm_counter, n_genes), ("exact", nperm_exact, n_exact)):
        eng.set_perm_exact(mode == "exact")
        prm = rvtests_amd.Params(1.0, 25.0, 1.0, 25.0, nperm, 1.0)
        run_vt = lambda: eng.vtprice_blocks(ptrs[:k], Ms[:k], afs[:k], y, nperm, 1.0)
        run_sk = lambda: eng.run_blocks(ptrs[:k], Ms[:k], afs[:k], tests=rvtests_amd.TEST_SKAT, params=prm, ids=list(range(k)))
        eng.rand_seed(1)
        run_vt(), run_sk()                                             # warm-up: buffers, code objects
        tv, ov = timed(run_vt, repeats)
        ts, os_ = timed(run_sk, repeats)
        nv = sum(r.actual_perm for r in ov)
        ns = sum(r.perm_actual_perm for r in os_)
        assert nv == ns == nperm * k, (nv, ns)
        vt_rate, sk_rate = [nv / t for t in tv], [ns / t for t in ts]
        rec[mode] = {
            "nperm": nperm, "genes": k, "nnz_per_gene": [int(r.n_carrier_entries) for r in ov],
            "distinct_carriers_per_gene": distinct[:k],
            "thresholds_per_gene": [int(r.n_threshold) for r in ov],
            "vt_shuffles_per_s": vt_rate, "vt_genes_per_s": [k / t for t in tv],
            "skat_shuffles_per_s": sk_rate, "skat_genes_per_s": [k / t for t in ts],
            "vt_spread": (max(vt_rate) - min(vt_rate)) / float(np.median(vt_rate)),
            "skat_spread": (max(sk_rate) - min(sk_rate)) / float(np.median(sk_rate)),
            "vt_over_skat_median": float(np.median(vt_rate) / np.median(sk_rate)),
        }
        if mode == "counter":  # the bar: VT at least SKAT, the only margin the run-to-run spread of the repeats
            rec[mode]["bar_vt_at_least_skat"] = bool(max(vt_rate) >= min(sk_rate)) and bool(
                np.median(vt_rate) >= np.median(sk_rate) * (1.0 - rec[mode]["vt_spread"] - rec[mode]["skat_spread"]))
        print(json.dumps({"shape": name, "mode": mode, **{a: rec[mode][a] for a in ("vt_shuffles_per_s", "skat_shuffles_per_s",
                                                                                 "vt_over_skat_median")}}), flush=True)
    for p in ptrs:
        eng.free_block(p)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a functional run of the tool")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of one rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vtprice_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-run", action="store_true", help="only merge --kernel-stats into the existing --out file")
    a = ap.parse_args()
    if a.quick:
        shapes = [("quick_N20000", 20000, 3, 20, 40, 2000, 200, 2)]
    else:
        shapes = [("configs2_N500000_M20-80", 500000, 6, 20, 80, 10000, 600, 2), ("configs1_N50000_M30", 50000, 8, 30, 30, 10000, 2000, 4)]
    result = {"device": "MI355X (gfx950)", "alpha": 1.0, "trait": "null quantitative", "shapes": []}
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
            if any(w in r.get("Name", "") for w in ("vtp_", "perm_", "k_fam_")):
                rows.append({"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                             "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])})
        result["kernel_stats"] = rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
