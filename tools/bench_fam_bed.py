#!/usr/bin/env python3
"""famScore and famLRT from rows of a resident .bed matrix (rvt_score_bed_dev_fam, rvt_lrt_bed_dev_fam) beside the fp64 block
route, in the manner of tools/bench_fam_families.py: warm-up, repeated timed calls, median.  Shapes: nuclear families of 4 in
the family form (members interleaved) at N = 20 000 and 100 000, and the dense rotation (the same families through
rvt_set_kinship with RVT_KINSHIP_DENSE=1) at N = 12 000; V = 4 096 hard-call variants, d = 4, 2 % and 0 % of the calls missing.
Per shape: variants/s of both calls and the front stage alone between two HIP events (rvt_debug_rotate_bed_timed), and the two
baselines measured in the same run on the imputed fp64 columns of the same calls —
  (a) rvt_score_block_fam / rvt_lrt_block_fam / rvt_debug_rotate_timed on a block that is already on the device;
  (b) the same including the block's way there: rvt_block_alloc, the columns over the link (rvt_block_upload_columns), the call,
      rvt_block_free
— with the ratios of the new calls' rates to both.  Writes profiles/fam_bed_bench.json (and prints a line per shape).

  python tools/bench_fam_bed.py [--families 20000,100000] [--dense 12000] [--missing 0.02,0] [--out profiles/fam_bed_bench.json]
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_fam_bed.py --route bed|block --reps 3 --families N --dense "" --missing m

--route bed / block: one route alone (its input only, 1 + reps timed rotations, then 1 + reps famScore calls) and nothing
written — for a kernel trace, where both routes would otherwise share the names of the kernels behind the front stage."""
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
from bench_single import hard_calls, null_case, timed, upload  # noqa: E402


def shape(a, N, form, missing):
    rng = np.random.default_rng(3)
    V, d = a.variants, a.d
    fam_ptr, members, blocks, S, u4 = cohort(N, "interleaved")
    X, y = null_case(rng, N, d, False)
    raw = hard_calls(rng, N, min(V, a.distinct))
    if missing > 0:
        raw[rng.random(raw.shape) < missing] = -9.0
    called = raw >= 0
    mean = np.where(called, raw, 0.0).sum(0) / np.maximum(called.sum(0), 1)
    G = np.asfortranarray(np.where(called, raw, mean[None, :]))          # what a caller uploads today
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)                   # (rvt_bed_alloc takes the rows' pitch from it)
    if form == "dense":
        os.environ["RVT_KINSHIP_DENSE"] = "1"
        eng.set_kinship(dense_u(N, members, u4), S)
        os.environ.pop("RVT_KINSHIP_DENSE", None)
    else:
        eng.set_kinship_families(fam_ptr, members, blocks, S)
    res = {"N": N, "form": form, "missing": missing, "V": V, "d": d, "visited_fraction": eng.kinship_structure()}
    eng.fit_fam_null(X, y)
    rows = eng.pack_bed(raw)
    cb = rows.shape[1]
    d_bed = ptr = None
    if a.route != "block":
        d_bed = eng.bed_alloc(V)
        for v0 in range(0, V, rows.shape[0]):
            eng.bed_upload(d_bed, v0, rows[:min(rows.shape[0], V - v0)])
    if a.route != "bed":
        ptr = upload(eng, G, V)

    def med(fn):
        return float(np.median(sorted(fn() for _ in range(1 + a.reps))[:-1]))   # (the first call allocates)

    def through_the_link(call):
        p = upload(eng, G, V)
        out = call(p)
        eng.free_block(p)
        return out

    if a.route != "both":   # one route alone, for a kernel trace: 1 + reps front stages / rotations, 1 + reps famScore calls
        if a.route == "bed":
            res["rotation_ms"] = med(lambda: eng.debug_rotate_bed_timed(d_bed, V))
            res["famScore_s"] = timed(lambda: eng.score_bed_dev_fam(d_bed, V, 0, want_counts=False), a.reps)[0]
        else:
            res["rotation_ms"] = med(lambda: eng.debug_rotate_timed(ptr, V))
            res["famScore_s"] = timed(lambda: eng.score_block_fam(ptr, V, 0), a.reps)[0]
        eng.close()
        return res
    new = {"famScore": lambda: eng.score_bed_dev_fam(d_bed, V, 0, want_counts=False),
           "famLRT": lambda: eng.lrt_bed_dev_fam(d_bed, V, want_counts=False)}
    base = {"famScore": lambda p: eng.score_block_fam(p, V, 0), "famLRT": lambda p: eng.lrt_block_fam(p, V)}
    for name in new:
        dt, _ = timed(new[name], a.reps)
        dt_a, _ = timed(lambda: base[name](ptr), a.reps)
        dt_b, _ = timed(lambda: through_the_link(base[name]), a.link_reps)
        res[name] = {"variants_per_s": V / dt, "block_on_device_variants_per_s": V / dt_a,
                     "block_with_upload_variants_per_s": V / dt_b, "ratio_to_a": dt_a / dt, "ratio_to_b": dt_b / dt}
    ms = med(lambda: eng.debug_rotate_bed_timed(d_bed, V))
    ms_a = med(lambda: eng.debug_rotate_timed(ptr, V))
    res["rotation"] = {"ms_per_block": ms, "block_on_device_ms_per_block": ms_a, "ratio_to_a": ms_a / ms,
                       "bytes_in_per_column": cb, "block_bytes_in_per_column": 8 * N}
    eng.free_block(ptr)
    eng.bed_free(d_bed)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="20000,100000")
    ap.add_argument("--dense", default="12000")
    ap.add_argument("--missing", default="0.02,0")
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--link-reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=256, help="distinct rows generated on the host")
    ap.add_argument("--route", default="both", choices=["both", "bed", "block"],
                    help="bed / block: that route's rotation and famScore calls alone, nothing written (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fam_bed_bench.json"))
    a = ap.parse_args()
    shapes = [(int(x) // 4 * 4, "families") for x in a.families.split(",") if x]
    shapes += [(int(x) // 4 * 4, "dense") for x in a.dense.split(",") if x]
    out = {"V": a.variants, "d": a.d, "shapes": []}
    for N, form in shapes:
        for missing in (float(x) for x in a.missing.split(",")):
            out["shapes"].append(shape(a, N, form, missing))
            print(json.dumps(out["shapes"][-1]), flush=True)
    if a.route != "both":
        return
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
