#!/usr/bin/env python3
"""The related-sample tests on a kinship installed family by family (rvt_set_kinship_families), in the manner of
tools/bench_single.py --fam: nuclear families of 4, listed contiguously and interleaved (member r of family i is sample
i + r N/4), d = 4, blocks of 4 096 hard-call variants, at N = 20 000, 100 000 and 500 000.  Per N and layout: seconds and device
memory of the installation, seconds of rvt_fit_fam_null, variants/s of famScore, famLRT and famGrammarGamma (af=mean,
af=kinship), FamSKAT gene-sets/s on the shape of tools/bench_famskat.py (128 genes of 30 variants), and the rotation alone —
HIP events directly around it (rvt_debug_rotate_timed) — as milliseconds per 4 096 columns and the bytes/s that is at the
ideal 16 N bytes per column.  The unrelated quantitative score pass on the same block is timed beside them.

  python tools/bench_fam_families.py [--samples 20000,100000,500000] [--parent parent.json] [--out profiles/fam_families_bench.json]
  python tools/bench_fam_families.py --dense --samples N --layout interleaved|contiguous [--rotate-calls K]

--dense: the same cohort through a DENSE installation of the equivalent U (rvt_set_kinship) — what a commit without the family
form has to do; one JSON line with the installation, the FamSKAT rate and, where the library has the hook, the rotation's
milliseconds; --rotate-calls K runs rvt_debug_rotate on the 4 096 columns K times (for a kernel trace of a library without the
hook).  --parent FILE: a JSON object with such figures measured on the parent commit, stored under "parent"."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("RVT_BENCH_PACKAGE_ROOT", ROOT))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rvtests_amd  # noqa: E402
from bench_single import hard_calls, null_case, timed, upload  # noqa: E402

BLK = np.array([[1, 0, .5, .5], [0, 1, .5, .5], [.5, .5, 1, .5], [.5, .5, .5, 1]])


def cohort(N, layout):
    """fam_ptr, members, the eigenvector blocks (column-major per family) and S of N / 4 nuclear families."""
    n_fam = N // 4
    s4, u4 = np.linalg.eigh(BLK)
    fam_ptr = np.arange(0, N + 1, 4, dtype=np.int64)
    if layout == "contiguous":
        members = np.arange(N, dtype=np.int32)
    else:
        members = (np.arange(n_fam)[:, None] + n_fam * np.arange(4)[None, :]).astype(np.int32).ravel()
    blocks = np.tile(u4.ravel(order="F").astype(np.float32), n_fam)
    return fam_ptr, members, blocks, np.tile(s4, n_fam).astype(np.float32), u4


def dense_u(N, members, u4):
    U = np.zeros((N, N), dtype=np.float32, order="F")
    for f in range(N // 4):
        U[members[4 * f:4 * f + 4], 4 * f:4 * f + 4] = u4
    return U


def famskat_rate(eng, N, genes, variants, reps):
    rng = np.random.default_rng(4)
    dev = torch.device("cuda:0")
    ld = eng.padded_ld(N)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    blocks = []
    for _ in range(genes):
        maf = torch.tensor(10 ** rng.uniform(np.log10(5e-4), np.log10(5e-2), variants), device=dev, dtype=torch.float32)
        G = torch.zeros((variants, ld), dtype=torch.float64, device=dev)
        for _h in range(2):
            G[:, :N] += (torch.rand((variants, N), generator=g, device=dev) < maf[:, None]).to(torch.float64)
        blocks.append(G)
    torch.cuda.synchronize()
    ptrs, Ms = [b.data_ptr() for b in blocks], [variants] * genes
    dt, out = timed(lambda: eng.run_fam_blocks(ptrs, Ms), reps)
    return {"genes": genes, "M": variants, "ms_per_batch": 1e3 * dt, "gene_sets_per_s": genes / dt,
            "ok": int(sum(r.famskat_ok for r in out))}


def mem_free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def leg(a, N, layout, dense=False):
    rng = np.random.default_rng(3)
    V, d = a.variants, a.d
    fam_ptr, members, blocks, S, u4 = cohort(N, layout)
    X, y = null_case(rng, N, d, False)
    eng = rvtests_amd.Engine(0)
    res = {"N": N, "layout": layout, "d": d, "V": V, "form": "dense" if dense else "families"}
    U = dense_u(N, members, u4) if dense else None
    free0 = mem_free()
    t0 = time.perf_counter()
    if dense:
        eng.set_kinship(U, S)
    else:
        eng.set_kinship_families(fam_ptr, members, blocks, S)
    res["install_s"] = time.perf_counter() - t0
    res["install_device_bytes"] = int(free0 - mem_free())
    res["visited_fraction"] = eng.kinship_structure()
    del U
    t0 = time.perf_counter()
    eng.fit_fam_null(X, y)
    res["fit_fam_null_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    eng.fit_grammar_null(X, y)
    res["fit_grammar_null_s"] = time.perf_counter() - t0
    G = hard_calls(rng, N, min(V, a.distinct))
    ptr = upload(eng, G, V)
    if hasattr(eng, "debug_rotate_timed"):
        ms = sorted(eng.debug_rotate_timed(ptr, V) for _ in range(1 + a.reps))[:-1]   # (the first call allocates)
        res["rotation"] = {"ms_per_block": float(np.median(ms)), "ms_all": ms,
                           "ideal_bytes_per_s": 16.0 * N * V / (1e-3 * float(np.median(ms)))}
    for _ in range(a.rotate_calls):
        eng.debug_rotate(ptr, V)
    if not a.rotation_only:
        runs = {"famScore": lambda: eng.score_block_fam(ptr, V, 0), "famLRT": lambda: eng.lrt_block_fam(ptr, V),
                "famGrammarGamma_mean": lambda: eng.grammar_block(ptr, V, 0),
                "famGrammarGamma_kinship": lambda: eng.grammar_block(ptr, V, 1)}
        for name, fn in runs.items():
            dt, _ = timed(fn, a.reps)
            res[name] = {"s_per_block": dt, "variants_per_s": V / dt}
    eng.free_block(ptr)
    if not a.rotation_only:
        res["FamSKAT"] = famskat_rate(eng, N, a.genes, a.gene_variants, a.reps)
    eng.close()
    if not dense and not a.rotation_only:
        eng = rvtests_amd.Engine(0)   # the unrelated quantitative score pass on the same columns
        eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)
        ptr = upload(eng, G, V)
        dt, _ = timed(lambda: eng.score_block(ptr, V), a.reps)
        res["unrelated_score"] = {"s_per_block": dt, "variants_per_s": V / dt}
        eng.free_block(ptr)
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="20000,100000,500000")
    ap.add_argument("--layout", default="interleaved,contiguous")
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=256, help="distinct columns generated on the host")
    ap.add_argument("--genes", type=int, default=128)
    ap.add_argument("--gene-variants", type=int, default=30)
    ap.add_argument("--dense", action="store_true", help="a dense installation of the equivalent U instead")
    ap.add_argument("--dense-beside", default="20000", help="N at which the families run also times the dense installation")
    ap.add_argument("--rotate-calls", type=int, default=0)
    ap.add_argument("--rotation-only", action="store_true")
    ap.add_argument("--parent", help="JSON file of the parent commit's figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fam_families_bench.json"))
    a = ap.parse_args()
    Ns = [int(x) // 4 * 4 for x in a.samples.split(",")]
    layouts = a.layout.split(",")
    if a.dense:
        print(json.dumps(leg(a, Ns[0], layouts[0], dense=True)))
        return
    beside = [int(x) for x in a.dense_beside.split(",") if x]
    out = {"V": a.variants, "d": a.d, "legs": [], "dense_install_this_commit": []}
    for N in Ns:
        for layout in layouts:
            out["legs"].append(leg(a, N, layout))
            print(json.dumps(out["legs"][-1]), flush=True)
            if N in beside:
                out["dense_install_this_commit"].append(leg(a, N, layout, dense=True))
                print(json.dumps(out["dense_install_this_commit"][-1]), flush=True)
    if a.parent:
        out["parent"] = json.load(open(a.parent))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
