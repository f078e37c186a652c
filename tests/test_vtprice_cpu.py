"""CPU: a plain numpy restatement of the reference's VariableThresholdPrice::fit (src/Model.h:1745-1882 over
makeVariableThreshodlGenotype / zegginiCollapse, src/Model.cpp:132-148,301-382; permute / centerVector / getRowVariance,
src/LinearAlgebra.h; Permutation, src/Permutation.h:48-158) in fp64 and sample order, driven by the glibc stream the oracle
exports — the yardstick of tests/test_gpu_vtprice.py — and the checks that need no GPU: the statement against a brute-force
dense form and against the carrier-list / prefix-sum form the kernels use, its stop rule against the oracle's, its shuffle
against the C library's rand(), the ABI entry and its record, the `--vt price[...]` parser entry and the header line."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "rvtests_amd", "csrc", "host", "host_driver")
PERM_HEADER = "NumPerm\tActualPerm\tStat\tNumGreater\tNumEqual\tPermPvalue"


# ---- the statement -----------------------------------------------------------------------------------------------------------
def seq_sum(v):
    """left-to-right double sum, as the reference's loops run"""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def groups(af):
    """groupFrequency (src/Model.cpp:254-261): std::map of ceil(1e6 f) / 1e6 -> column indices, ascending keys"""
    g = {}
    for j, f in enumerate(af):
        g.setdefault(math.ceil(1000000. * float(f)) / 1000000, []).append(j)
    keys = sorted(g)
    return keys, [g[k] for k in keys]


def carries(Gf):
    """(int)g > 0 of zegginiCollapse (src/Model.cpp:142-145): truncation towards zero"""
    return np.trunc(Gf).astype(np.int64) > 0


def collapsed_rows(Gf, af):
    """sortedBurden after transposeInPlace: row t = per-sample count of carried variants over the cumulative columns
    (makeVariableThreshodlGenotype, src/Model.cpp:311-338).  af[j] belongs to column j of the flipped, polymorphic block."""
    freq, grp = groups(af[:Gf.shape[1]])
    Cm = carries(Gf)
    rows, cum = [], []
    for cols in grp:
        cum += cols
        rows.append(Cm[:, cum].sum(1).astype(np.float64))
    return freq, np.array(rows).reshape(len(freq), Gf.shape[0])


def row_sd(b):
    """sqrt(getRowVariance) (src/LinearAlgebra.h:183-191), in fp64"""
    avg = seq_sum(b) / len(b)
    return math.sqrt(seq_sum((b - avg) ** 2) / len(b))


def calc_z(yv, rows, sds, freq):
    """calculateZ (src/Model.h:1832-1850) with zmax = -999 on entry: (zmax, optFreq, all |z_t|)"""
    zmax, opt, zs = -999.0, None, []
    for t in range(rows.shape[0]):
        z = seq_sum(rows[t] * yv)
        if sds[t] != 0:
            z /= sds[t]
        zs.append(abs(z))
        if abs(z) > zmax or t == 0:
            zmax, opt = abs(z), freq[t]
    return zmax, opt, zs


def calc_z_binary(y01, rows, freq):
    """The engine's form for a 0 / 1 phenotype: sum b (y - ybar) from the exact integers (cases among the carriers, sum b) with one
    fixed formula, sd^2 = (N sum b^2 - (sum b)^2) / N^2 from exact integers — equal configurations give bit-equal z."""
    N = len(y01)
    ybar = seq_sum(y01) / float(N)
    zmax, opt = -999.0, None
    for t in range(rows.shape[0]):
        bi = rows[t].astype(np.int64)
        s1, s2, cases = int(bi.sum()), int((bi * bi).sum()), int(bi[y01 == 1.0].sum())
        sd = math.sqrt(float(N * s2 - s1 * s1) / (float(N) * float(N)))
        z = float(cases) - ybar * float(s1)
        if sd != 0:
            z = z / sd
        if abs(z) > zmax or t == 0:
            zmax, opt = abs(z), freq[t]
    return zmax, opt


def permute(v, rand):
    """permute (src/LinearAlgebra.h:8-21)"""
    for i in range(len(v) - 1, 0, -1):
        j = rand() % (i + 1)
        if i != j:
            v[i], v[j] = v[j], v[i]


class Stop:
    """Permutation (src/Permutation.h:69-98); threshold is an INT member"""

    def __init__(self, nperm, alpha, obs):
        self.nperm, self.obs, self.threshold = nperm, obs, int(1.0 * nperm * alpha * 2)
        self.actual = self.num_x = self.num_eq = 0

    def next(self):
        return not (self.actual >= self.nperm or self.num_x + self.num_eq >= self.threshold)

    def add(self, s):
        self.actual += 1
        self.num_x += s > self.obs
        self.num_eq += s == self.obs

    def pvalue(self):
        return 1.0 if self.actual == 0 else 1.0 * (self.num_x + 0.5 * self.num_eq) / self.actual


def orc_rand():
    return int(orc.lib().orc_rand())


def statement(G, af, y, nperm, alpha, rand=orc_rand, binary_exact=False, obs=None, keep=False):
    """VariableThresholdPrice::fit on the unflipped block G.  binary_exact: the engine's integer form for a 0 / 1 phenotype.
    obs: compare the permuted statistics with this observed value instead (the device's), as tests/test_gpu_perm.py does.
    Returns a dict; fit_ok False when no column is polymorphic (nothing drawn)."""
    Gf = orc.flip_poly(np.asfortranarray(G, dtype=np.float64))[0]
    if Gf.shape[1] == 0:
        return {"fit_ok": False}
    freq, rows = collapsed_rows(Gf, af)
    y = np.asarray(y, dtype=np.float64)
    if binary_exact:
        yv = y.copy()
        zmax, opt = calc_z_binary(yv, rows, freq)
        stat = lambda v: calc_z_binary(v, rows, freq)[0]
    else:
        yv = y - seq_sum(y) / len(y)
        sds = [row_sd(b) for b in rows]
        zmax, opt, _ = calc_z(yv, rows, sds, freq)
        stat = lambda v: calc_z(v, rows, sds, freq)[0]
    st = Stop(nperm, alpha, zmax if obs is None else obs)
    perms = []
    while st.next():
        permute(yv, rand)
        s = stat(yv)
        st.add(s)
        if keep:
            perms.append(s)
    nnz = int(carries(Gf).sum())
    return {"fit_ok": True, "n_poly": Gf.shape[1], "n_threshold": len(freq), "nnz": nnz, "opt_freq": opt, "zmax": zmax,
            "actual": st.actual, "num_x": int(st.num_x), "num_eq": int(st.num_eq), "pvalue": st.pvalue(), "perms": perms,
            "rows": rows, "yc": y - seq_sum(y) / len(y), "sds": None if binary_exact else sds}


def zmax_bound(res):
    """forward bound of a reordered sum on the observed zmax: max_t nnz 2^-52 sum |b_i y_i| / sd_t"""
    worst = 0.0
    for t, b in enumerate(res["rows"]):
        sd = res["sds"][t] if res["sds"][t] != 0 else 1.0
        worst = max(worst, res["nnz"] * 2.0 ** -52 * float(np.abs(b * res["yc"]).sum()) / sd)
    return worst


def float_to_string(v):
    """floatToString (base/TypeConversion.h:100-105): %g with 6 significant digits"""
    return "%g" % v


def format_row(res, nperm, last):
    """writeOutput (src/Model.h:1814-1819) without the site columns: a failed fit prints the Permutation fields after reset() and
    the OptFreq / Zmax left by the last successful fit (`last`, (-1, -1) before the first)"""
    if not res["fit_ok"]:
        return "\t%g\t%g\t%d\t0\t%s\t0\t0\t%s" % (last[0], last[1], nperm, float_to_string(0.0), float_to_string(1.0))
    return "\t%g\t%g\t%d\t%d\t%s\t%d\t%d\t%s" % (res["opt_freq"], res["zmax"], nperm, res["actual"], float_to_string(res["zmax"]),
                                                res["num_x"], res["num_eq"], float_to_string(res["pvalue"]))


# ---- the form the kernels use ------------------------------------------------------------------------------------------------
def carrier_list_z(Gf, af, yv):
    """entries (sample, group) ordered by group, a sample carrying k variants of a group k times; z_t from the prefix sums of the
    per-group sums; sd from the exact integers sum b, sum b^2"""
    N = Gf.shape[0]
    freq, grp = groups(af[:Gf.shape[1]])
    Cm = carries(Gf)
    P, zs, b = 0.0, [], np.zeros(N, dtype=np.int64)
    for cols in grp:
        ent = np.concatenate([np.nonzero(Cm[:, j])[0] for j in cols])
        P += float(yv[ent].sum())
        np.add.at(b, ent, 1)
        s1, s2 = int(b.sum()), int((b * b).sum())
        sd = math.sqrt(float(N * s2 - s1 * s1) / (float(N) * float(N)))
        zs.append(abs(P / sd) if sd != 0 else abs(P))
    return freq, zs


def _gene(rng, N, M, ties=False, flip=False, imputed=False):
    maf = 10 ** rng.uniform(-2.2, -0.9, M)
    G = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    if ties:
        G[:, 1::3] = G[rng.permutation(N)][:, 0::3][:, :G[:, 1::3].shape[1]]      # equal allele counts: one frequency group
    if flip:
        G[:, 0] = 2.0 - G[:, 0]
    if imputed:                                                                   # imputed means on both sides of 1
        G[rng.random(N) < 0.02, M - 1] = 0.37
        G[rng.random(N) < 0.02, M - 2] = 1.25
    return np.asfortranarray(G), G.sum(0) / (2.0 * N)


def test_statement_agrees_with_dense_rows_and_with_the_carrier_list_form():
    rng = np.random.default_rng(5)
    for N, M, kw in ((300, 12, dict(ties=True)), (257, 9, dict(flip=True, imputed=True)), (120, 1, {}), (400, 70, dict(ties=True))):
        G, af = _gene(rng, N, M, **kw)
        Gf, fl, kp = orc.flip_poly(G)
        if kw.get("flip"):
            assert fl[0] == 1
        afm = af[:Gf.shape[1]]
        freq, rows = collapsed_rows(Gf, afm)
        # brute force: every collapsed row built explicitly, element by element, as zegginiCollapse does
        keys = sorted(set(math.ceil(1000000. * f) / 1000000 for f in afm))
        assert keys == freq and (len(freq) < Gf.shape[1]) == bool(kw.get("ties"))
        for t, f in enumerate(keys):
            brute = np.zeros(N)
            for p in range(N):
                for j in range(Gf.shape[1]):
                    if math.ceil(1000000. * afm[j]) / 1000000 <= f and int(Gf[p, j]) > 0:
                        brute[p] += 1.0
            assert (brute == rows[t]).all()
        if kw.get("imputed"):
            Cm = carries(Gf)
            assert not Cm[Gf == 0.37].any() and Cm[Gf == 1.25].all() and (Gf == 0.37).any() and (Gf == 1.25).any()
        y = rng.normal(size=N)
        yc = y - seq_sum(y) / N
        zmax, opt, zs = calc_z(yc, rows, [row_sd(b) for b in rows], freq)
        f2, z2 = carrier_list_z(Gf, afm, yc)
        assert f2 == freq and np.allclose(z2, zs, rtol=1e-11, atol=1e-12)
        assert zmax == max(zs) and opt == freq[int(np.argmax(zs))]
        if M == 1:
            assert len(freq) == 1                                   # a single group is computed like any other
        yb = (rng.random(N) < 0.4).astype(np.float64)
        zb, ob = calc_z_binary(yb, rows, freq)
        zq, oq, _ = calc_z(yb - seq_sum(yb) / N, rows, [row_sd(b) for b in rows], freq)
        assert abs(zb - zq) <= 1e-10 * max(zq, 1.0)
    assert statement(np.zeros((50, 3)), np.zeros(3), rng.normal(size=50), 10, 0.5)["fit_ok"] is False       # M = 0 after filtering


def test_stop_rule_agrees_with_the_oracle():
    O = orc.lib()
    O.orc_perm_stop_run.restype = C.c_double
    O.orc_perm_stop_run.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    rng = np.random.default_rng(3)
    for nperm, alpha in ((300, 0.05), (300, 0.0333), (100, 0.001), (50, 0.5), (0, 0.05), (40, 0.0)):
        for obs in (0.3, 1.5, 2.0):
            stats = np.round(np.abs(rng.normal(size=400)), 1)      # (rounded: ties with the observed value occur)
            st = Stop(nperm, alpha, obs)
            k = 0
            while st.next() and k < len(stats):
                st.add(stats[k])
                k += 1
            b = (C.c_int * 3)()
            p = O.orc_perm_stop_run(nperm, alpha, obs, stats.ctypes.data_as(C.POINTER(C.c_double)), len(stats), b)
            assert [st.actual, st.num_x, st.num_eq] == list(b) and st.pvalue() == p


def test_shuffle_agrees_with_the_c_library():
    libc = C.CDLL("libc.so.6")
    libc.srand(7)
    orc.rand_seed(7)
    a, b = list(range(23)), list(range(23))
    for _ in range(5):
        permute(a, orc_rand)
        permute(b, lambda: int(libc.rand()))
    assert a == b and a != list(range(23))
    orc.rand_seed(1)


def test_library_exports_the_entry_and_the_record_layout_matches_the_header():
    import rvtests_amd
    L = rvtests_amd.load_library()
    assert hasattr(L, "rvt_vtprice_blocks")
    R = rvtests_amd.VtPriceResult
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rvtests_amd.h"\nint main(void) {\n  printf("%zu", sizeof(rvt_vtprice_result));\n'
    names = [f[0] for f in R._fields_]
    assert names == ["fit_ok", "n_poly", "n_threshold", "n_carrier_entries", "opt_freq", "zmax", "num_perm", "actual_perm",
                     "num_greater", "num_equal", "perm_pvalue"]
    for n in names:
        src += '  printf(" %%zu", offsetof(rvt_vtprice_result, %s));\n' % n
    src += "  return 0;\n}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(R)] + [getattr(R, n).offset for n in names]


def _ensure_driver():
    if not os.path.exists(DRIVER):
        import __graft_entry__ as g
        g.build()


def _write_input(path, y, binary, genes):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<qiii", len(y), 0, int(binary), len(genes)))
        f.write(np.ascontiguousarray(y, dtype="<f8").tobytes())
        for G, af in genes:
            f.write(struct.pack("<i", G.shape[1]))
            f.write(np.ascontiguousarray(af, dtype="<f8").tobytes())
            f.write(np.asfortranarray(G, dtype="<f8").tobytes(order="F"))


def run_vt_driver(path, spec, perm_exact=None):
    env = dict(os.environ)
    env.pop("RVT_PERM_EXACT", None)
    if perm_exact is not None:
        env["RVT_PERM_EXACT"] = "1" if perm_exact else "0"
    env["RVT_DRIVER_VT"] = spec
    p = subprocess.run([DRIVER, path, "-", "-"], capture_output=True, text=True, timeout=600, env=env)
    return p.returncode, p.stdout, p.stderr


def test_model_manager_accepts_vt_price_and_the_header_is_the_reference_s(tmp_path):
    _ensure_driver()
    rng = np.random.default_rng(1)
    G, af = _gene(rng, 60, 4)
    path = str(tmp_path / "in.bin")
    _write_input(path, rng.normal(size=60), 0, [(G, af)])
    rc, out, err = run_vt_driver(path, "price[nPerm=200,alpha=0.1]")
    assert rc == 0, err
    lines = out.split("\n")
    assert lines[0] == "== out.VariableThresholdPrice.assoc"
    # writeHeaderTab's tab, then "\tOptFreq\tZmax\t", Permutation::writeHeader, "\n" (src/Model.h:1807-1812): an empty column
    assert lines[1] == "Range\tN_INFORMATIVE\tNumVar\tNumPolyVar\t" + "\tOptFreq\tZmax\t" + PERM_HEADER
    row = lines[2].split("\t")
    assert len(row) == len(lines[1].split("\t")) and row[4] == "" and row[7] == "200"     # NumPerm from the parsed nPerm
    rc, out, err = run_vt_driver(path, "price")
    assert rc == 0 and out.split("\n")[2].split("\t")[7] == "10000"                     # default nPerm
    rc, out, err = run_vt_driver(path, "nosuchvt")
    assert rc == 1 and "Unknown model name: nosuchvt" in err

