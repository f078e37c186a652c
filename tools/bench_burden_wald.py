#!/usr/bin/env python3
"""The analytic burden tests --burden cmcWald, zegginiWald, fp, exactCMC (rvt_burden_blocks): genes/s of each test alone at the two
shapes of tools/bench_burdenperm.py — N = 500 000 with M ~ U{20..80} and N = 50 000 with M = 30 — under a binary and a quantitative
null model (intercept only), three repeats each.  Every gene is also run through rvt_mb_blocks with nPerm = 0, whose first steps are
flipped_poly_block and a per-gene collapse: in a `rocprofv3 --kernel-trace --stats` run of this tool that gives the yardstick
(fam_flip_compact_kernel + mb_collapse_kernel) beside burden_columns_kernel.  Writes profiles/burden_wald_bench.json.
usage (GPU box): python tools/bench_burden_wald.py [--quick] [--kernel-stats kernel_stats.csv [--no-run]] [--out FILE]"""
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
from rvtests_amd import engine as E  # noqa: E402

ROOFLINE = 8e12   # bytes/s: the HBM figure the project measures against
TESTS = (("cmcwald", E.BURDEN_CMCWALD), ("zegginiwald", E.BURDEN_ZEGGINIWALD), ("fp", E.BURDEN_FP), ("exactcmc", E.BURDEN_EXACTCMC))


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


def shape(name, N, n_genes, mlo, mhi, repeats, seed):
    rng = np.random.default_rng(seed)
    genes = make_genes(rng, N, n_genes, mlo, mhi)
    ybin = (rng.random(N) < 0.3).astype(np.float64)
    yq = rng.normal(size=N)
    eng = rvtests_amd.Engine(0)
    X = np.asfortranarray(np.ones((N, 1)))
    Ms, afs = [G.shape[1] for G, af in genes], [af for G, af in genes]
    rec = {"shape": name, "N": N, "genes": n_genes, "M": Ms, "repeats": repeats}
    # what the tool itself asks of the collapse kernel: its calls, and their algorithmic bytes — one read of every gene, plus one
    # collapsed column per gene for the three tests that have a block (exactCMC writes none)
    collapse_calls, collapse_bytes, yard_calls = 0, 0, 0
    for trait, y in (("binary", ybin), ("quantitative", yq)):
        eng.fit_null(1 if trait == "binary" else 0, X, y.copy())
        ld = eng.padded_ld()
        ptrs = [eng.upload_block(G) for G, af in genes]
        rec[trait] = {}
        for k, (tname, bit) in enumerate(TESTS):
            if tname == "exactcmc" and trait != "binary":
                continue
            ts = []
            for it in range(repeats + 1):                              # the first call is the warm-up
                t0 = time.perf_counter()
                out = eng.burden_blocks(ptrs, Ms, afs, ybin, bit)
                ts.append(time.perf_counter() - t0)
                collapse_calls += 1
                collapse_bytes += 8 * ld * (sum(Ms) + (0 if tname == "exactcmc" else n_genes))
            rec[trait][tname + "_genes_per_s"] = [n_genes / t for t in ts[1:]]
            rec[trait][tname + "_ok"] = int(sum((r.cmc_wald.ok, r.zeggini_wald.ok, r.fp_ok, r.exact_ok)[k] for r in out))
        if trait == "binary":                                          # the yardstick's kernels, for the profiled run
            eng.mb_blocks(ptrs, Ms, ybin, 0, 0.05)
            yard_calls += 1
        print(json.dumps({"shape": name, "trait": trait, **rec[trait]}), flush=True)
        for p in ptrs:
            eng.free_block(p)
    rec["collapse_calls"] = collapse_calls
    rec["collapse_algorithmic_bytes"] = int(collapse_bytes)
    rec["yardstick_passes"] = yard_calls
    rec["gene_bytes_one_pass"] = int(8 * ld * sum(Ms))
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a functional run of the tool")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of one rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burden_wald_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-run", action="store_true", help="only merge --kernel-stats into the existing --out file")
    a = ap.parse_args()
    shapes = [("quick_N20000", 20000, 6, 20, 40)] if a.quick else [("N500000_M20-80", 500000, 8, 20, 80), ("N50000_M30", 50000, 32, 30, 30)]
    result = {"device": "MI355X (gfx950)", "roofline_bytes_per_s": ROOFLINE, "shapes": []}
    if a.no_run:
        result = json.load(open(a.out))
    for k, s in enumerate([] if a.no_run else shapes):
        result["shapes"].append(shape(*s, repeats=a.repeats, seed=23 + k))
    if a.kernel_stats:
        # every kernel of the run, by the names the profiler gives them; the counts below come from the CSV's Calls column and
        # from what the run itself recorded (collapse_calls, yardstick_passes), so --repeats and the shapes may be anything — but
        # the CSV has to be of a run with the same arguments as the one that wrote --out
        rows = [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                 "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])} for r in csv.DictReader(open(a.kernel_stats))]
        rows.sort(key=lambda r: -r["total_ns"])
        result["kernel_stats"] = rows[:30]
        calls = sum(s["collapse_calls"] for s in result["shapes"])
        total = sum(s["collapse_algorithmic_bytes"] for s in result["shapes"])
        one_pass = sum(s["gene_bytes_one_pass"] * s["yardstick_passes"] for s in result["shapes"])
        col = [r for r in rows if "burden_columns_kernel" in r["name"]]
        if col and col[0]["total_ns"] > 0:
            sec = col[0]["total_ns"] * 1e-9
            result["collapse_kernel"] = {"launches": col[0]["calls"], "calls_of_the_run": calls, "algorithmic_bytes": int(total), "seconds": sec,
                                         "bytes_per_s": total / sec, "fraction_of_roofline": total / sec / ROOFLINE,
                                         "seconds_per_pass_over_the_genes": sec * one_pass / max(1, total)}
        yard = [r for r in rows if "fam_flip_compact_kernel" in r["name"] or "mb_collapse_kernel" in r["name"]]
        if yard:
            ysec = sum(r["total_ns"] for r in yard) * 1e-9
            result["yardstick_flip_then_collapse"] = {"kernels": sorted(r["name"] for r in yard), "passes": sum(s["yardstick_passes"] for s in result["shapes"]),
                                                      "gene_bytes_one_pass": int(one_pass), "seconds": ysec}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
