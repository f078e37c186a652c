#!/usr/bin/env python3
"""Throughput of the single-variant Wald test (rvt_wald_block).  Prints one JSON line:
  binary:       V hard-call variants (MAF U(0.005, 0.5)) (--distinct of them, repeated) at N samples and d columns of X (batched per-variant IRLS,
                wald_logistic.hip.h): variants per second, mean rounds, device time per round
  quantitative: the same shape at --qt-samples (closed form of the score partials): variants per second
  cpu:          one core of the oracle's LogisticRegression::FitLogisticModel on a few of the same variants
usage (GPU box): python tools/bench_single.py [--samples 200000] [--qt-samples 500000] [--variants 4096] [--d 4]

--fam: the single-variant tests for related samples instead (famScore = rvt_score_block_fam, famLRT = rvt_lrt_block_fam,
famGrammarGamma = rvt_grammar_block with af=mean and af=kinship) on nuclear families of 4 at --fam-samples and on the same
kinship forced through the dense path (RVT_KINSHIP_DENSE=1, every panel of U visited) at --dense-samples; variants per second,
and for GrammarGamma af=mean its HBM fraction (8 N bytes per variant over 8 TB/s) beside the unrelated quantitative score pass.
rvt_set_kinship takes U as a dense N x N float matrix, which this script builds on the host: 1.6 GB at N = 20 000, 40 GB at the
N = 100 000 of a large pedigree, hence the default.  visited_fraction: rvt_kinship_structure (1.0 = every panel of U is read).
usage (GPU box): python tools/bench_single.py --fam [--fam-samples 20000] [--dense-samples 12000] [--variants 4096]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rvtests_amd  # noqa: E402
import orc  # noqa: E402


def null_case(rng, N, d, binary):
    X = np.ones((N, d))
    X[:, 1:] = rng.standard_normal((N, d - 1))
    if binary:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(X @ (0.2 * rng.standard_normal(d)) - 0.5)))).astype(float)
    else:
        y = X @ rng.standard_normal(d) + rng.standard_normal(N)
    return np.asfortranarray(X), y


def hard_calls(rng, N, V):
    maf = rng.uniform(0.005, 0.5, V)
    G = np.empty((N, V), order="F")
    for j in range(V):
        G[:, j] = (rng.random((N, 2)) < maf[j]).sum(1)
    return G


def upload(eng, G, V):
    """A block of V columns: the distinct columns of G repeated (each fit depends on its column alone)."""
    ptr = eng.alloc_block(V)
    for c0 in range(0, V, G.shape[1]):
        eng.upload_columns(ptr, c0, G[:, :min(G.shape[1], V - c0)])
    return ptr


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--qt-samples", type=int, default=500000)
    ap.add_argument("--variants", type=int, default=4096)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-variants", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=256, help="distinct columns generated on the host")
    ap.add_argument("--binary-only", action="store_true", help="the binary leg alone (kernel profiles)")
    ap.add_argument("--fam", action="store_true", help="the related-sample single-variant tests")
    ap.add_argument("--fam-samples", type=int, default=20000)
    ap.add_argument("--dense-samples", type=int, default=12000)
    ap.add_argument("--fam-d", type=int, default=4)
    a = ap.parse_args()
    if a.fam:
        return fam_main(a)
    rng = np.random.default_rng(1)
    V, d = a.variants, a.d
    out = {"V": V, "d": d}
    eng = rvtests_amd.Engine(0)

    N = a.samples
    X, y = null_case(rng, N, d, True)
    G = hard_calls(rng, N, min(V, a.distinct))
    eng.fit_null(rvtests_amd.TRAIT_BINARY, X, y)
    ptr = upload(eng, G, V)
    dt, r = timed(lambda: eng.wald_block(ptr, V), a.reps)
    fitted = r["ok"] != 0
    rounds = r["rounds"][fitted]
    # rounds of the lockstep batch: the longest fit; every round streams the variants still active
    out["binary"] = {"N": N, "s_per_block": dt, "variants_per_s": V / dt, "mean_rounds": float(rounds.mean()),
                     "max_rounds": int(rounds.max()), "active_variant_rounds": int(rounds.sum()),
                     "ms_per_round": 1e3 * dt / max(int(rounds.max()), 1),
                     "fitted": int((r["ok"] == 1).sum()), "failed": int((r["ok"] == -1).sum())}
    eng.free_block(ptr)

    cpu_t = []
    for j in range(a.cpu_variants):
        A = np.column_stack([X[:, :1], G[:, j], X[:, 1:]])
        t0 = time.perf_counter()
        orc.fit_logistic(A, y)
        cpu_t.append(time.perf_counter() - t0)
    out["cpu_one_core"] = {"N": N, "variants_per_s": 1.0 / float(np.mean(cpu_t)), "variants": a.cpu_variants}
    del G
    if a.binary_only:
        eng.close()
        print(json.dumps(out))
        return

    Nq = a.qt_samples
    X, y = null_case(rng, Nq, d, False)
    G = hard_calls(rng, Nq, min(V, a.distinct))
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)
    ptr = upload(eng, G, V)
    dtq, rq = timed(lambda: eng.wald_block(ptr, V), a.reps)
    out["quantitative"] = {"N": Nq, "s_per_block": dtq, "variants_per_s": V / dtq, "fitted": int((rq["ok"] == 1).sum())}
    eng.free_block(ptr)
    eng.close()
    print(json.dumps(out))


def family_kinship(N):
    """Nuclear families of 4: U block diagonal (the eigenvectors of one family's kinship), S tiled."""
    blk = np.array([[1, 0, .5, .5], [0, 1, .5, .5], [.5, .5, 1, .5], [.5, .5, .5, 1]])
    s4, u4 = np.linalg.eigh(blk)
    U = np.zeros((N, N), dtype=np.float32, order="F")
    for f in range(N // 4):
        U[4 * f:4 * f + 4, 4 * f:4 * f + 4] = u4
    return U, np.tile(s4, N // 4).astype(np.float32)


def fam_leg(a, N, dense):
    rng = np.random.default_rng(3)
    N = N // 4 * 4
    V, d = a.variants, a.fam_d
    U, S = family_kinship(N)
    X, y = null_case(rng, N, d, False)
    if dense:
        os.environ["RVT_KINSHIP_DENSE"] = "1"
    eng = rvtests_amd.Engine(0)
    eng.set_kinship(U, S)  # (rvt_set_kinship reads RVT_KINSHIP_DENSE)
    os.environ.pop("RVT_KINSHIP_DENSE", None)
    res_struct = eng.kinship_structure()
    del U
    t0 = time.perf_counter()
    eng.fit_fam_null(X, y)
    t_fam_null = time.perf_counter() - t0
    t0 = time.perf_counter()
    eng.fit_grammar_null(X, y)
    t_gg_null = time.perf_counter() - t0
    G = hard_calls(rng, N, min(V, a.distinct))
    ptr = upload(eng, G, V)
    res = {"N": N, "d": d, "dense_path": dense, "visited_fraction": res_struct, "s_fam_null": t_fam_null, "s_grammar_null": t_gg_null}
    runs = {"famScore": lambda: eng.score_block_fam(ptr, V, 0), "famLRT": lambda: eng.lrt_block_fam(ptr, V),
            "famGrammarGamma_mean": lambda: eng.grammar_block(ptr, V, 0),
            "famGrammarGamma_kinship": lambda: eng.grammar_block(ptr, V, 1)}
    for name, fn in runs.items():
        dt, _ = timed(fn, a.reps)
        res[name] = {"s_per_block": dt, "variants_per_s": V / dt}
    res["famGrammarGamma_mean"]["hbm_fraction"] = 8.0 * N * V / res["famGrammarGamma_mean"]["s_per_block"] / 8e12
    res["lrt_over_score"] = res["famLRT"]["s_per_block"] / res["famScore"]["s_per_block"]
    eng.free_block(ptr)
    eng.close()
    return res


def fam_main(a):
    out = {"V": a.variants, "families": fam_leg(a, a.fam_samples, False), "dense": fam_leg(a, a.dense_samples, True)}
    # the unrelated quantitative score pass at the family leg's N, for the HBM comparison
    rng = np.random.default_rng(5)
    N = a.fam_samples // 4 * 4
    X, y = null_case(rng, N, a.fam_d, False)
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)
    ptr = upload(eng, hard_calls(rng, N, min(a.variants, a.distinct)), a.variants)
    dt, _ = timed(lambda: eng.score_block(ptr, a.variants), a.reps)
    out["unrelated_score"] = {"N": N, "s_per_block": dt, "variants_per_s": a.variants / dt,
                              "hbm_fraction": 8.0 * N * a.variants / dt / 8e12}
    eng.free_block(ptr)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
