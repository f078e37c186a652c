#!/usr/bin/env python3
"""Every route of the kinship eigendecomposition (rvt_kinship_decompose, rvt_kinship_decompose_families) on fixed matrices that
sit on the route switches, the results as SHA-256 of the U and S bytes and hex doubles: what two builds of the engine must
agree on bit for bit when the solver code is rearranged.

    python tools/dump_decompose.py OUT.json                   # run on the GPU: one JSON document
    python tools/dump_decompose.py --peak OUT.json            # the highest device memory in use during a dense N = 24 000
    python tools/dump_decompose.py --compare A.json B.json [--parent-again A2.json] [--commits PARENT BRANCH] [--out RESULT.json]

RVT_LIBRARY chooses the build.  --parent-again: a second run of the parent; a case whose two parent runs differ is reported
as not repeatable and left out of the comparison."""
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _info(info):
    return {name: (float(getattr(info, name)).hex() if isinstance(getattr(info, name), float) else int(getattr(info, name)))
            for name, _ in type(info)._fields_}


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            del os.environ[k]


# ---- the matrices (those of tests/test_gpu_decompose.py and tests/test_gpu_kinship_families.py) ------------------------------
def dense_matrix(N, kind):
    rng = np.random.default_rng(N)
    if kind == "grm":
        Z = rng.standard_normal((N, 3 * N))
        K = Z @ Z.T / (3 * N)
    elif kind == "psd":
        Z = rng.standard_normal((N, N // 2))
        K = Z @ Z.T / N
    elif kind == "indefinite":
        A = rng.standard_normal((N, N))
        K = (A + A.T) / 2
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
        lam = np.concatenate([np.linspace(0.5, 3.0, N // 2), -np.linspace(0.5, 3.0, N // 2)])
        K = (Q * lam) @ Q.T
    return ((K + K.T) / 2).astype(np.float32)


def batch_matrix():
    rng = np.random.default_rng(5)
    N = 700
    Z = rng.standard_normal((N, 2 * N))
    K32 = ((Z @ Z.T) / (2 * N)).astype(np.float32)
    return (K32 + K32.T) / 2


def block_kinship(rng, sizes):
    N = int(np.sum(sizes))
    K = np.zeros((N, N))
    o = 0
    for sz in sizes:
        A = rng.uniform(0.05, 0.5, (sz, sz))
        K[o:o + sz, o:o + sz] = (A + A.T) / 2 + np.eye(sz)
        o += sz
    return K


def family_mix():
    """The 260 families of sizes 1..9 with the zeroed row 7: in order, shuffled, and the matrix with families of 70."""
    rng = np.random.default_rng(12)
    sizes = rng.choice([1, 2, 3, 4, 6, 9], size=260)
    K = block_kinship(rng, sizes)
    K[7, :] = 0.0
    K[:, 7] = 0.0
    K32 = K.astype(np.float32)
    perm = rng.permutation(K.shape[0])
    Kp = np.ascontiguousarray(K32[np.ix_(perm, perm)])
    big = block_kinship(rng, [70, 3, 4, 2, 5] * 20).astype(np.float32)
    return K32, Kp, big


def family_blocks(sizes, seed, shuffle=True):
    """fam_ptr, members and the flat column-major blocks, every block filled as block_kinship fills it."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    fam_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(fam_ptr[-1])
    members = (rng.permutation(N) if shuffle else np.arange(N)).astype(np.int32)
    blocks = []
    for sz in sizes:
        A = rng.uniform(0.05, 0.5, (sz, sz))
        blocks.append(((A + A.T) / 2 + np.eye(sz)).astype(np.float32).ravel(order="F"))
    return fam_ptr, members, np.concatenate(blocks)


def phenotype(N, seed):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N), rng.standard_normal(N)])
    return X, 0.3 * X[:, 1] + rng.standard_normal(N)


# ---- one case = one engine -------------------------------------------------------------------------------------------------
def installed(e, X, y):
    import synth
    N = X.shape[0]
    out = {"kinship_structure": float(e.kinship_structure()).hex()}
    e.fit_fam_null(X, y)
    G = synth.make_gene(N, 8, seed=508, missing=0.02, common=True)[1]
    r = e.run_fam_blocks([e.upload_block(G)], [8])[0]
    out["famskat_ok"], out["famskat_Q"], out["famskat_p"] = int(r.famskat_ok), float(r.famskat_Q).hex(), float(r.famskat_p).hex()
    return out


def dense_case(K32, install=False, Xy=None, **env):
    import rvtests_amd
    e = rvtests_amd.Engine(0)
    try:
        with Env(**env):
            U, S, info = e.kinship_decompose(K32, install=install, want_vectors=not install)
        out = {"U": None if U is None else _sha(U), "S": _sha(S), "info": _info(info)}
        if install:
            out.update(installed(e, *Xy))
        return out
    except rvtests_amd.RvtError as err:
        return {"error": str(err)}
    finally:
        e.close()


def blocks_case(fam_ptr, members, blocks, install, want_u):
    import ctypes as C
    import rvtests_amd
    from rvtests_amd.engine import DecomposeInfo, family_form
    e = rvtests_amd.Engine(0)
    try:
        N, n_fam, fam_ptr, members, blocks, _ = family_form(fam_ptr, members, blocks)
        U = np.zeros(blocks.size if want_u else 0, dtype=np.float32)
        S = np.zeros(N, dtype=np.float32)
        info = DecomposeInfo()
        fp = C.POINTER(C.c_float)
        e._check(e.L.rvt_kinship_decompose_families(
            e.ctx, N, n_fam, fam_ptr.ctypes.data_as(C.POINTER(C.c_int64)), members.ctypes.data_as(C.POINTER(C.c_int32)),
            blocks.ctypes.data_as(fp), U.ctypes.data_as(fp) if want_u else None, S.ctypes.data_as(fp), 1 if install else 0,
            C.cast(C.byref(info), C.c_void_p)))
        out = {"U": _sha(U) if want_u else None, "S": _sha(S), "info": _info(info)}
        if install:
            e.N = N
            out.update(installed(e, *phenotype(N, 9)))
        return out
    except rvtests_amd.RvtError as err:
        return {"error": str(err)}
    finally:
        e.close()


def run():
    from test_fam_cpu import make_family_case
    doc = {}

    def case(name, fn, *a, **kw):
        t0 = time.perf_counter()
        doc[name] = fn(*a, **kw)
        print("%-58s %.2f s" % (name, time.perf_counter() - t0), flush=True)

    N75, K75, _, _, X75, y75 = make_family_case(75, 2, 7)
    K75 = K75.astype(np.float32)
    mix, mix_shuffled, big = family_mix()
    grm = dense_matrix(1000, "grm")
    opposite = dense_matrix(130, "opposite")
    case("family/nuclear-75", dense_case, K75)
    case("family/mix-260", dense_case, mix)
    case("family/mix-260-shuffled", dense_case, mix_shuffled)
    case("family-refused/families-of-70", dense_case, big)
    case("tridiag/grm-1000", dense_case, grm)
    case("tridiag/indefinite-257", dense_case, dense_matrix(257, "indefinite"))
    case("tridiag/opposite-130", dense_case, opposite)
    case("tridiag/grm-128", dense_case, dense_matrix(128, "grm"))
    case("switch/grm-127", dense_case, dense_matrix(127, "grm"))
    case("tridiag/grm-700-batch-64", dense_case, batch_matrix(), RVT_TRIDIAG_BATCH="64")
    case("tridiag-declines/psd-300", dense_case, dense_matrix(300, "psd"))
    case("jacobi/grm-1000", dense_case, grm, RVT_KINSHIP_JACOBI="1")
    case("jacobi/opposite-130-shift", dense_case, opposite, RVT_KINSHIP_JACOBI="1")
    case("jacobi/grm-65", dense_case, dense_matrix(65, "grm"), RVT_KINSHIP_JACOBI="1")
    case("dense-forced/nuclear-75", dense_case, K75, RVT_KINSHIP_DENSE="1")
    case("installed/nuclear-75", dense_case, K75, install=True, Xy=(X75, y75))
    case("installed/grm-1000", dense_case, grm, install=True, Xy=phenotype(1000, 9))
    fm = family_blocks(np.random.default_rng(8).choice([1, 2, 3, 4, 6], size=260), 41)
    two_passes = family_blocks([64] * 2100, 43)
    for install in (False, True):
        for want_u in (True, False):
            tag = "install=%d/U=%d" % (install, want_u)
            case("blocks/mix-260/" + tag, blocks_case, *fm, install, want_u)
            case("blocks/2100-tiles/" + tag, blocks_case, *two_passes, install, want_u)
    bad = grm.copy()
    bad[3, 5] = np.nan
    case("error/nan", dense_case, bad)
    bad = grm.copy()
    bad[3, 5] += 1.0
    case("error/asymmetric", dense_case, bad)
    case("error/order-1", dense_case, np.ones((1, 1), dtype=np.float32))
    case("error/family-of-65", blocks_case, np.array([0, 65, 70], dtype=np.int64), np.arange(70, dtype=np.int32),
         np.ones(65 * 65 + 25, dtype=np.float32), False, True)
    return doc


# ---- the peak of the dense route ---------------------------------------------------------------------------------------------
def peak(N=24000):
    import torch
    import rvtests_amd
    g = torch.Generator(device="cuda").manual_seed(1)
    Z = torch.randn((N, 2 * N), dtype=torch.float32, device="cuda", generator=g)
    K = (Z @ Z.T) / (2 * N)
    K = ((K + K.T) / 2).cpu().numpy()
    del Z
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    e = rvtests_amd.Engine(0)
    free0, total = torch.cuda.mem_get_info()
    high, stop = [total - free0], threading.Event()

    def sample():      # (the engine's call is a ctypes call: it runs without the interpreter lock)
        while not stop.is_set():
            high[0] = max(high[0], total - torch.cuda.mem_get_info()[0])
            time.sleep(0.02)

    th = threading.Thread(target=sample)
    th.start()
    t0 = time.perf_counter()
    try:
        U, S, info = e.kinship_decompose(K, want_vectors=False)
    finally:
        stop.set()
        th.join()
    dt = time.perf_counter() - t0
    e.close()
    return {"N": N, "seconds": dt, "sweeps": int(info.sweeps), "in_use_before_bytes": int(total - free0),
            "peak_in_use_bytes": int(high[0]), "peak_above_start_bytes": int(high[0] - (total - free0)),
            "twenty_N2_bytes": 20 * N * N, "S": _sha(S)}


def compare(path_a, path_b, path_a2, commits, out_path):
    def load(p):
        with open(p, "rb") as f:
            raw = f.read()
        return json.loads(raw), hashlib.sha256(raw).hexdigest()

    (a, sha_a), (b, sha_b) = load(path_a), load(path_b)
    a2 = load(path_a2)[0] if path_a2 else a
    not_repeatable = sorted(k for k in a if a[k] != a2.get(k))
    compared = sorted(k for k in set(a) | set(b) if k not in not_repeatable)
    differing = [k for k in compared if a.get(k) != b.get(k)]
    result = {"identical": not differing, "differing_cases": differing, "not_repeatable_at_the_parent": not_repeatable,
              "parent_run_twice": bool(path_a2), "cases_compared": compared,
              "fields_compared": sum(len(a[k]) + len(a[k].get("info", {})) for k in compared if k in a),
              "sha256": {"parent": sha_a, "branch": sha_b},
              "commits": {"parent": commits[0], "branch": commits[1]} if commits else None,
              "parent": {k: a[k] for k in compared if k in a}}
    text = json.dumps(result, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if not differing else 1


def main(argv):
    def opt(name, n=1):
        return argv[argv.index(name) + 1:argv.index(name) + 1 + n] if name in argv else None

    if argv and argv[0] == "--compare":
        again, out = opt("--parent-again"), opt("--out")
        return compare(argv[1], argv[2], again[0] if again else None, opt("--commits", 2), out[0] if out else None)
    doc = peak() if argv[0] == "--peak" else run()
    with open(argv[-1], "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
    print("wrote", argv[-1], len(doc), "entries")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
