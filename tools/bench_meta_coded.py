#!/usr/bin/env python3
"""The dominant / recessive meta models: what the recoding costs.  Writes profiles/meta_coded_bench.json (and prints it).
  kernels: rvt_block_recode (fp64 columns, out of place) and rvt_bed_recode_block (rows of a resident .bed matrix) alone, at
           --samples x --columns with --missing of the calls missing: device milliseconds per call from HIP events (count pass,
           write / expand pass; rvt_recode_last_timing), the call's wall time, and bytes/s against the algorithmic bytes —
           24 N per fp64 column (8 N read by the count pass, 8 N read + 8 N written by the write pass), N/2 + 8 N per .bed row
  driver:  sites/s of `--meta dominant` through host_driver --synthetic-meta --coding dominant against `--meta score` +
           `--meta cov` on the same columns (--coding additive: the additive path is what the parent commit runs), and their ratio
Every GPU step is a child process under its own `timeout`; nothing here uses more than the 16 CPUs of a job.
usage (GPU box): python tools/bench_meta_coded.py [--samples 500000] [--columns 1024] [--variants 8000] [--window 200]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRIVER = os.path.join(ROOT, "rvtests_amd", "csrc", "host", "host_driver")


def raw_columns(rng, N, V, missing):
    maf = rng.uniform(0.05, 0.45, V)
    G = np.empty((N, V), order="F")
    for j in range(V):
        G[:, j] = (rng.random((N, 2)) < maf[j]).sum(1)
        G[rng.random(N) < missing, j] = -9.0
    return G


def kernels_leg(a):
    import rvtests_amd
    rng = np.random.default_rng(1)
    N, V = a.samples, a.columns
    X = np.ones((N, 3), order="F")
    X[:, 1:] = rng.standard_normal((N, 2))
    y = X @ rng.standard_normal(3) + rng.standard_normal(N)
    G = raw_columns(rng, N, min(V, a.distinct), a.missing)
    eng = rvtests_amd.Engine(0)
    eng.fit_null(rvtests_amd.TRAIT_QUANTITATIVE, X, y)
    eng.set_profiling(True)
    src, dst = eng.alloc_block(V), eng.alloc_block(V)
    for c0 in range(0, V, G.shape[1]):
        eng.upload_columns(src, c0, G[:, :min(G.shape[1], V - c0)])
    eng.sync()
    cb = (N + 3) // 4
    rows = eng.pack_bed(G)
    d_bed = eng.bed_alloc(V)
    for c0 in range(0, V, G.shape[1]):
        eng.bed_upload(d_bed, c0, rows[:min(G.shape[1], V - c0)])
    out = {"N": N, "columns": V, "missing": a.missing, "reps": a.reps}
    for name, coding in (("dominant", rvtests_amd.CODING_DOMINANT), ("recessive", rvtests_amd.CODING_RECESSIVE)):
        for kind, call, nbytes in (("block_recode", lambda: eng.block_recode(dst, 0, src, 0, V, coding, want_counts=False), 24.0 * N * V),
                                   ("bed_recode_block", lambda: eng.bed_recode_block(d_bed, V, coding, dst, 0, want_counts=False),
                                    (2.0 * cb + 8.0 * N) * V)):
            call()
            ev, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                ev.append(eng.recode_last_timing())
            cnt_ms, wr_ms = float(np.median([e[0] for e in ev])), float(np.median([e[1] for e in ev]))
            out["%s_%s" % (kind, name)] = {
                "count_pass_ms": cnt_ms, "write_pass_ms": wr_ms, "passes_ms": cnt_ms + wr_ms,
                "call_wall_ms": 1e3 * float(np.median(wall)),   # (with the columns' bookkeeping pass behind the recoding)
                "algorithmic_bytes": nbytes, "bytes_per_s_of_the_passes": nbytes / (1e-3 * (cnt_ms + wr_ms))}
    eng.bed_free(d_bed)
    eng.free_block(src)
    eng.free_block(dst)
    eng.close()
    print(json.dumps(out))


def child(cmd, limit):
    """one GPU step: a fresh process under its own time limit; its last stdout line is its JSON result"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("step failed (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64, help="distinct columns generated on the host")
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", type=int, default=8000)
    ap.add_argument("--window", type=int, default=200, help="markers per covariance window")
    ap.add_argument("--leg", default="", help="(internal) kernels: run the in-process leg")
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_coded_bench.json"))
    a = ap.parse_args()
    if a.leg == "kernels":
        return kernels_leg(a)
    res = {"kernels": child([sys.executable, os.path.abspath(__file__), "--leg", "kernels", "--samples", str(a.samples), "--columns",
                             str(a.columns), "--distinct", str(a.distinct), "--missing", str(a.missing), "--reps", str(a.reps)], 300)}
    if not a.skip_driver:
        drv = {}
        for coding in ("additive", "dominant"):
            r = child([DRIVER, "--synthetic-meta", str(a.samples), str(a.variants), str(a.window), "--missing", str(a.missing),
                       "--coding", coding], 300)
            drv[coding] = {k: r[k] for k in ("mode", "N", "variants", "window_markers", "variants_per_s",
                                             "variants_per_s_after_the_first", "seconds", "seconds_in_fit", "assoc_lines")}
        drv["dominant_over_additive"] = drv["dominant"]["variants_per_s_after_the_first"] / drv["additive"]["variants_per_s_after_the_first"]
        k = res["kernels"]["block_recode_dominant"]
        # the recode passes of both coded models (score block and covariance ring) as a share of the coded run
        per_site_ms = 2.0 * k["passes_ms"] / res["kernels"]["columns"] * (a.samples / res["kernels"]["N"])
        drv["recode_passes_share_of_the_time"] = per_site_ms * 1e-3 * drv["dominant"]["variants_per_s_after_the_first"]
        res["driver"] = drv
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
