#!/usr/bin/env python3
"""rvt_kinship_from_bed: what the empirical kinship costs on the device.  Writes profiles/kinship_bench.json (and prints it).
  shapes : N in --samples (4096, 12000, 20000) x V = --sites (65536) rows of a resident .bed matrix, --missing (1 %) of the calls
           missing, both methods; per shape the device milliseconds of the three stages (HIP events: site pass, Gram product,
           finish with the copy of K to the host), the call's wall time and the useful operation rate of the product —
           N (N + 1) / 2 pairs x V sites, 2 operations per pair and site for BN (one fp64 multiply-add), 6 for IBS (three int8
           multiply-adds: n n' + u u' + h h')
  BN     : the ratio to tools/gemm64_bench (gemm_f64.hip.h, the fp64 matrix-core product of this project) on the symmetric product
           of the same shape — N outputs a side over V along the contraction.  That tool holds 64 K-slices of partial results
           (512 N^2 bytes): shapes whose partials exceed --gemm-partials-gb take the rate of the largest shape that ran
  IBS    : the ratio to the int8 rate tools/rotgemm_bench reports for rot_gemm.hip.h (per plane pair, 20 000 x 20 000 x 3840)
  host   : for the first N only, the wall time of the same kinship through numpy's BLAS (planes / z matrix, then matrix products)
Every GPU step is a child process under its own `timeout`; nothing here uses more than the 16 CPUs of a job.
usage (GPU box): python tools/bench_kinship.py [--samples 4096,12000,20000] [--sites 65536]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEMM64 = os.path.join(ROOT, "tools", "gemm64_bench")
ROTGEMM = os.path.join(ROOT, "tools", "rotgemm_bench")


def draw_calls(rng, N, V, missing):
    f = rng.uniform(0.01, 0.5, V)
    G = rng.binomial(2, f, size=(N, V)).astype(np.int8)
    G[rng.random((N, V)) < missing] = -9
    return G


def useful_ops(N, V, method):
    return (6.0 if method == "ibs" else 2.0) * (N * (N + 1) / 2.0) * V


def device_leg(a):
    import rvtests_amd
    N, V = a.n, a.sites
    rng = np.random.default_rng(N)
    X = np.asfortranarray(np.column_stack([np.ones(N), rng.normal(size=N)]))
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, rng.normal(size=N))
    distinct = min(V, a.distinct)
    rows = eng.pack_bed(draw_calls(rng, N, distinct, a.missing))   # (the cost does not depend on the calls: the sites repeat)
    d_bed = eng.bed_alloc(V)
    for v0 in range(0, V, distinct):
        eng.bed_upload(d_bed, v0, rows[:min(distinct, V - v0)])
    out = {"N": N, "V": V, "missing": a.missing}
    for method in ("bn", "ibs"):
        eng.kinship_from_bed(d_bed, min(V, 1024), method=method)    # warm-up: code objects, first allocations
        t0 = time.perf_counter()
        K, info = eng.kinship_from_bed(d_bed, V, method=method)
        wall = time.perf_counter() - t0
        ops = useful_ops(N, V, method)
        out[method] = {"ms_stats": info.ms_stats, "ms_product": info.ms_product, "ms_finish": info.ms_finish,
                       "call_wall_s": wall, "sites_used": info.sites_used, "useful_ops": ops,
                       "useful_ops_per_s_of_the_product": ops / (1e-3 * info.ms_product),
                       "useful_ops_per_s_of_the_call": ops / wall}
        del K
    eng.bed_free(d_bed)
    eng.close()
    print(json.dumps(out))


def host_leg(a):
    """the same kinship with numpy's BLAS on the host (no filters: min_maf = 0, max_missing = 1), wall seconds"""
    N, V = a.n, a.sites
    rng = np.random.default_rng(N)
    distinct = min(V, a.distinct)
    G = np.tile(draw_calls(rng, N, distinct, a.missing), (1, (V + distinct - 1) // distinct))[:, :V]
    out = {"N": N, "V": V}
    t0 = time.perf_counter()
    called = G >= 0
    cnt = called.sum(0)
    s = np.where(called, G, 0).sum(0).astype(np.float64)
    keep = (s > 0) & (s < 2.0 * cnt)
    mean = s[keep] / cnt[keep]
    scale = np.sqrt(1.0 / (1.0 - mean / 2.0) / mean)
    Z = np.where(called[:, keep], (G[:, keep] - mean) * scale, 0.0)
    K = Z @ Z.T / keep.sum()
    out["bn_wall_s"] = time.perf_counter() - t0
    del Z, K
    t0 = time.perf_counter()
    keep = s > 0
    n = called[:, keep].astype(np.float32)            # (fp32 sums of 0 / +-1 products are exact below 2^24 > 2 V)
    u = np.where(called[:, keep], G[:, keep] - 1, 0).astype(np.float32)
    h = (G[:, keep] == 1).astype(np.float32)
    c = (n @ n.T).astype(np.float64)
    k = c + (u @ u.T) + (h @ h.T)
    K = np.divide(k, c, out=np.zeros_like(k), where=c > 0)
    out["ibs_wall_s"] = time.perf_counter() - t0
    print(json.dumps(out))


def child(cmd, limit):
    """one step: a fresh process under its own time limit; returns its stdout"""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("step failed (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-2000:]))
    print("%.1f s: %s" % (time.perf_counter() - t0, " ".join(cmd[-6:])), file=sys.stderr, flush=True)
    return p.stdout


def last_json(text):
    return json.loads(text.strip().splitlines()[-1])


def build_tool(path):
    if not os.path.exists(path):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", path + ".hip", "-o", path])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4096,12000,20000")
    ap.add_argument("--sites", type=int, default=65536)
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--distinct", type=int, default=4096, help="distinct sites generated on the host")
    ap.add_argument("--gemm-partials-gb", type=float, default=100.0, help="largest partial-result buffer gemm64_bench may allocate")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--leg", default="", help="(internal) device | host: run that leg in this process")
    ap.add_argument("--n", type=int, default=0, help="(internal) the leg's sample count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinship_bench.json"))
    a = ap.parse_args()
    if a.leg == "device":
        return device_leg(a)
    if a.leg == "host":
        return host_leg(a)
    me = [sys.executable, os.path.abspath(__file__), "--sites", str(a.sites), "--missing", str(a.missing), "--distinct", str(a.distinct)]
    sizes = [int(t) for t in a.samples.split(",")]
    res = {"sites": a.sites, "missing": a.missing, "shapes": []}
    build_tool(GEMM64)
    build_tool(ROTGEMM)
    m = re.search(r"bench n=20000 T=3840: [0-9.]+ ms per plane pair, ([0-9.]+) POP/s", child([ROTGEMM, "bench"], 300))
    rot_ops = float(m.group(1)) * 1e15
    res["rot_gemm_int8_ops_per_s"] = rot_ops
    gemm_rate = None
    for N in sizes:
        shape = last_json(child(me + ["--leg", "device", "--n", str(N)], 600))
        # the fp64 product of the same shape: outputs N x N (symmetric), contraction V
        if 512.0 * N * N / 1e9 <= a.gemm_partials_gb:
            g = last_json(child([GEMM64, "bench", str(a.sites), str(N)], 300))
            gemm_rate = g["band_TFLOPs"] * 1e12
            shape["gemm64_bench"] = {"ms": g["ms"], "useful_flops_per_s": gemm_rate, "slices": g["slices"], "same_shape": True}
        elif gemm_rate is not None:
            shape["gemm64_bench"] = {"useful_flops_per_s": gemm_rate, "same_shape": False}
        if gemm_rate is not None:
            shape["bn"]["product_rate_over_gemm64_bench"] = shape["bn"]["useful_ops_per_s_of_the_product"] / gemm_rate
        shape["ibs"]["product_rate_over_rot_gemm"] = shape["ibs"]["useful_ops_per_s_of_the_product"] / rot_ops
        res["shapes"].append(shape)
    if not a.skip_host:
        res["host_numpy_blas"] = last_json(child(me + ["--leg", "host", "--n", str(sizes[0])], 900))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
