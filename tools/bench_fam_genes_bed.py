#!/usr/bin/env python3
"""FamSKAT and the family burden tests from rows of a resident .bed matrix (rvt_run_fam_tests_bed_dev) beside the fp64 block
route (rvt_run_fam_tests), in the manner of tools/bench_fam_bed.py: warm-up, repeated timed calls, median.  Shapes: nuclear
families of 4 in the family form (members interleaved) at N = 20 000 and 100 000, and the dense rotation (the same families
through rvt_set_kinship with RVT_KINSHIP_DENSE=1) at N = 12 000; a batch of --genes genes of M ~ U{20..80} rows each, lying
anywhere in a resident matrix of --distinct hard-call rows (they overlap), d = 4, 2 % and 0 % of the calls missing; FamSKAT
alone (tests = 16) and all three tests (16 | 32 | 64).  Per shape: gene-sets/s of the new call, its front stage alone between two
HIP events (rvt_debug_fam_genes_bed_front_timed), and the two baselines on the imputed fp64 columns of the same genes —
  (a) rvt_run_fam_tests on blocks that are already on the device;
  (b) the same including the blocks' way there: rvt_block_alloc, the columns over the link, the call, rvt_block_free
— with the ratios of the new call's rate to both.

  python tools/bench_fam_genes_bed.py [--route both|bed|block] [--families 20000,100000] [--dense 12000] [--missing 0.02,0]
                                      [--label this] [--out profiles/fam_genes_bed_bench.json]

--route block measures (a) and (b) alone and needs nothing of the new call, so it also runs against the library of an earlier
commit (RVT_LIBRARY=<its librvtests_amd.so>); --route bed measures the new call alone.  The result is stored in the JSON under
--label, beside what other labels left there: the block-route figures of two commits side by side show what the cut of
rvt_run_fam_tests into front and tail costs."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the engine's library: one HIP runtime for both  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("RVT_BENCH_PACKAGE_ROOT", ROOT))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rvtests_amd  # noqa: E402
from bench_fam_families import cohort, dense_u  # noqa: E402
from bench_single import hard_calls, null_case, timed  # noqa: E402

MASKS = (("famskat", 16), ("all_three", 16 | 32 | 64))


def shape(a, N, form, missing):
    rng = np.random.default_rng(3)
    fam_ptr, members, blocks, S, u4 = cohort(N, "interleaved")
    X, y = null_case(rng, N, a.d, False)
    raw = hard_calls(rng, N, a.distinct)
    if missing > 0:
        raw[rng.random(raw.shape) < missing] = -9.0
    Ms = rng.integers(20, 81, a.genes)
    first = np.array([rng.integers(0, a.distinct - M + 1) for M in Ms])
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)                   # (rvt_bed_alloc takes the rows' pitch from it)
    if form == "dense":
        os.environ["RVT_KINSHIP_DENSE"] = "1"
        eng.set_kinship(dense_u(N, members, u4), S)
        os.environ.pop("RVT_KINSHIP_DENSE", None)
    else:
        eng.set_kinship_families(fam_ptr, members, blocks, S)
    res = {"N": N, "form": form, "missing": missing, "genes": a.genes, "rows": int(Ms.sum()), "d": a.d,
           "visited_fraction": eng.kinship_structure()}
    eng.fit_fam_null(X, y)
    d_bed = ptrs = G = None
    if a.route != "block":
        rows = eng.pack_bed(raw)
        cb = rows.shape[1]
        d_bed = eng.bed_alloc(a.distinct)
        eng.bed_upload(d_bed, 0, rows)
        addr = [d_bed + int(f) * cb for f in first]
    if a.route != "bed":
        called = raw >= 0
        mean = np.where(called, raw, 0.0).sum(0) / np.maximum(called.sum(0), 1)
        G = np.asfortranarray(np.where(called, raw, mean[None, :]))      # what a caller uploads today
        ptrs = [eng.upload_block(G[:, f:f + M]) for f, M in zip(first, Ms)]

    def through_the_link(tests):
        p = [eng.upload_block(G[:, f:f + M]) for f, M in zip(first, Ms)]
        out = eng.run_fam_blocks(p, Ms, tests=tests)
        for q in p:
            eng.free_block(q)
        return out

    for name, tests in MASKS:
        r = {}
        if a.route != "block":
            dt, out = timed(lambda: eng.run_fam_tests_bed_dev(addr, Ms, tests=tests), a.reps)
            front = sorted(eng.debug_fam_genes_bed_front_timed(addr, Ms, tests=tests) for _ in range(1 + a.reps))[:-1]
            r.update(gene_sets_per_s=a.genes / dt, ms_per_batch=1e3 * dt, front_stage_ms=float(np.median(front)),
                     famskat_ok=int(sum(q.famskat_ok for q in out)), kept_rows=int(sum(q.n_poly for q in out)),
                     bytes_in_per_row=cb)
        if a.route != "bed":
            dt_a, out = timed(lambda: eng.run_fam_blocks(ptrs, Ms, tests=tests), a.reps)
            dt_b, _ = timed(lambda: through_the_link(tests), a.link_reps)
            r.update(block_on_device_gene_sets_per_s=a.genes / dt_a, block_on_device_ms_per_batch=1e3 * dt_a,
                     block_with_upload_gene_sets_per_s=a.genes / dt_b, block_bytes_in_per_row=8 * N,
                     block_famskat_ok=int(sum(q.famskat_ok for q in out)))
        if a.route == "both":
            r.update(ratio_to_a=dt_a / dt, ratio_to_b=dt_b / dt)
        res[name] = r
    for q in ptrs or []:
        eng.free_block(q)
    if d_bed is not None:
        eng.bed_free(d_bed)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="20000,100000")
    ap.add_argument("--dense", default="12000")
    ap.add_argument("--missing", default="0.02,0")
    ap.add_argument("--genes", type=int, default=64)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--link-reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=256, help="rows of the resident matrix (generated on the host)")
    ap.add_argument("--route", default="both", choices=["both", "bed", "block"])
    ap.add_argument("--label", default="this", help="key of this run in the JSON (e.g. parent_block for an earlier commit's library)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fam_genes_bed_bench.json"))
    a = ap.parse_args()
    shapes = [(int(x) // 4 * 4, "families") for x in a.families.split(",") if x]
    shapes += [(int(x) // 4 * 4, "dense") for x in a.dense.split(",") if x]
    run = {"route": a.route, "genes": a.genes, "d": a.d, "shapes": []}
    for N, form in shapes:
        for missing in (float(x) for x in a.missing.split(",")):
            run["shapes"].append(shape(a, N, form, missing))
            print(json.dumps(run["shapes"][-1]), flush=True)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = run
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
