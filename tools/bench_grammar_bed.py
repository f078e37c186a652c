#!/usr/bin/env python3
"""famGrammarGamma from rows of a resident .bed matrix (rvt_grammar_bed_dev) beside the fp64 block route, in the manner of
tools/bench_fam_bed.py.  Shapes: nuclear families of 4 in the family form (members interleaved) at N = 20 000, 100 000 and
500 000 with af=mean, and the dense rotation (the same families through rvt_set_kinship with RVT_KINSHIP_DENSE=1) at N = 12 000
with af=kinship; V = 4 096 hard-call variants, d = 4, 0 % and 2 % of the calls missing.  Per shape, each `--repeats` times (the
minimum and the median of the repeats' seconds are reported; a repeat is itself the median of `--reps` calls behind a warm-up):
  new  rvt_grammar_bed_dev on the resident rows, and its product kernel alone between two HIP events
       (rvt_debug_grammar_bed_timed) with the bytes of codes it reads per second;
  (a)  rvt_grammar_block on the imputed fp64 columns of the same calls, already on the device;
  (b)  the same including the block's way there: rvt_block_alloc, the columns over the link, the call, rvt_block_free;
  (c)  rvt_score_bed_dev (the linear score test under the ordinary quantitative null model) on the same rows.
`beats_a` says whether the new call's slowest repeat is faster than (a)'s fastest, i.e. by more than the spread of the repeats.
Writes profiles/grammar_bed_bench.json (and prints a line per shape).

  python tools/bench_grammar_bed.py [--families 20000,100000,500000] [--dense 12000] [--missing 0,0.02] [--out ...]"""
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
    kin = 1 if form == "dense" else 0
    fam_ptr, members, blocks, S, u4 = cohort(N, "interleaved")
    X, y = null_case(rng, N, d, False)
    raw = hard_calls(rng, N, min(V, a.distinct))
    if missing > 0:
        raw[rng.random(raw.shape) < missing] = -9.0
    called = raw >= 0
    mean = np.where(called, raw, 0.0).sum(0) / np.maximum(called.sum(0), 1)
    G = np.asfortranarray(np.where(called, raw, mean[None, :]))          # what a caller uploads today
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)                   # (rvt_bed_alloc takes the rows' pitch from it; (c))
    if form == "dense":
        os.environ["RVT_KINSHIP_DENSE"] = "1"
        eng.set_kinship(dense_u(N, members, u4), S)
        os.environ.pop("RVT_KINSHIP_DENSE", None)
    else:
        eng.set_kinship_families(fam_ptr, members, blocks, S)
    eng.fit_fam_null(X, y)                                               # (the block route's layout; af=kinship)
    eng.fit_grammar_null(X, y)
    rows = eng.pack_bed(raw)
    cb = rows.shape[1]
    d_bed = eng.bed_alloc(V)
    for v0 in range(0, V, rows.shape[0]):
        eng.bed_upload(d_bed, v0, rows[:min(rows.shape[0], V - v0)])
    ptr = upload(eng, G, V)

    def through_the_link():
        p = upload(eng, G, V)
        out = eng.grammar_block(p, V, kin)
        eng.free_block(p)
        return out

    def repeats(fn, reps):
        ts = [timed(fn, reps)[0] for _ in range(a.repeats)]
        return {"s_min": min(ts), "s_median": float(np.median(ts)), "s_max": max(ts), "variants_per_s": V / float(np.median(ts))}

    res = {"N": N, "form": form, "af": "kinship" if kin else "mean", "missing": missing, "V": V, "d": d}
    res["new"] = repeats(lambda: eng.grammar_bed_dev(d_bed, V, kin, want_counts=False), a.reps)
    res["a_block_on_device"] = repeats(lambda: eng.grammar_block(ptr, V, kin), a.reps)
    res["b_block_with_upload"] = repeats(through_the_link, a.link_reps)
    res["c_score_bed_dev"] = repeats(lambda: eng.score_bed_dev(d_bed, V, want_counts=False), a.reps)
    ms = [float(np.median(sorted(eng.debug_grammar_bed_timed(d_bed, V) for _ in range(1 + a.reps))[:-1])) for _ in range(a.repeats)]
    res["product_kernel"] = {"ms_min": min(ms), "ms_median": float(np.median(ms)), "bytes_of_codes": cb * V,
                             "codes_bytes_per_s": cb * V / (float(np.median(ms)) * 1e-3),
                             "variants_per_s": V / (float(np.median(ms)) * 1e-3)}
    res["ratio_to_a"] = res["a_block_on_device"]["s_median"] / res["new"]["s_median"]
    res["ratio_to_b"] = res["b_block_with_upload"]["s_median"] / res["new"]["s_median"]
    res["ratio_to_c"] = res["c_score_bed_dev"]["s_median"] / res["new"]["s_median"]
    res["beats_a"] = res["new"]["s_max"] < res["a_block_on_device"]["s_min"]
    res["no_slower_than_c"] = res["new"]["s_median"] <= res["c_score_bed_dev"]["s_median"]
    eng.free_block(ptr)
    eng.bed_free(d_bed)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="20000,100000,500000")
    ap.add_argument("--dense", default="12000")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--link-reps", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=256, help="distinct rows generated on the host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_bed_bench.json"))
    a = ap.parse_args()
    shapes = [(int(x) // 4 * 4, "families") for x in a.families.split(",") if x]
    shapes += [(int(x) // 4 * 4, "dense") for x in a.dense.split(",") if x]
    out = {"V": a.variants, "d": a.d, "repeats": a.repeats, "shapes": []}
    for N, form in shapes:
        for missing in (float(x) for x in a.missing.split(",")):
            out["shapes"].append(shape(a, N, form, missing))
            print(json.dumps(out["shapes"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
