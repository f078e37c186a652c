"""Inputs, routes, references and error bounds of the tests that walk every integer kernel along the covariate count d
(test_null_width_cases_cpu.py, test_gpu_null_width.py).

Every fast kernel multiplies genotypes with a null tile — [X | rr] under a quantitative trait, [v o X | res | v] under a binary
one — whose width d decides the kernel (expected_route) and, inside the digit-plane kernels, strides, lane gates and one scale
per column.  The models here are built so that the columns do NOT look alike (make_model), the references are long-double
statements of the same products (ref_suffstat) and the bounds are derived from the formats the engine documents (t_bound,
s_bound), per route and per entry."""
import numpy as np

import orc

U53 = 2.0 ** -53          # unit roundoff of fp64

# the widths at which a route changes (suffstat_hc.hip.h kHcMaxD, suffstat_hcw.hip.h kHcwMaxD, suffstat_hcx.hip.h
# kHcxStageCols - 2, suffstat_fdx.hip.h (kFdxStageCols - 3) / 2)
HC_MAX_D = 13
HCX_MAX_D = 6
FDX_MAX_D = 6
# fixed-point bits of a digit-plane column below the power of two above TWICE its largest entry
B_HCX = 42                # six balanced base-128 digits (rvt_set_null)
B_PLANES = 56             # eight (ensure_hcp_planes)

# (N, d, binary) of every model the GPU file installs: test_null_width_cases_cpu.py checks each of them without a GPU
MODELS = sorted(set(
    [(2003, d, 1) for d in (5, 6, 7, 13, 14, 16)] +            # binary blocks: hcx, hcw, fp64
    [(61, d, 1) for d in (2, 6, 7)] +                          # one ragged group: hcx, hcw; d = 2: the context walk
    [(2003, d, 0) for d in (1, 2, 4, 6, 7, 8, 12, 13, 14)] +   # quantitative blocks, host rows, resident rows, score, lattice, float
    [(61, d, 0) for d in (2, 4, 7)] +                          # one ragged group: hc, host rows, resident planes, fdx; d = 2: the walk
    [(20011, 13, 0)]))                                         # several wave-parts on the planes


def model_seed(N, d, binary):
    return 1000 * d + 10 * (N % 97) + binary


def make_model(N, d, binary, seed, G_effect=None):
    """(X, y, res, v, sigma2) as Engine.set_null takes them, fitted by the oracle.  Columns, as far as d reaches: the
    intercept; a 0/1 indicator (p = 0.45); an uncentred age-like column (50 +- 12); a PC-like column (sd 0.01); a normal
    column whose largest |entry| is 4 (1 - 2^-30) — just under a power of two: frexp gives e = 2, mx 2^shift = 2^(B-1) (1 - 2^-30)
    exceeds the 0.98 2^(B-1) cut and the shift is decremented; a normal column whose largest |entry| is exactly 8.0 — a power
    of two: e = 4, mx 2^shift = 2^(B-2), no decrement; then normals of scale 10^U(-1, 1)."""
    rng = np.random.default_rng(seed)
    cols = [np.ones(N)]
    if d > 1:
        cols.append((rng.random(N) < 0.45).astype(np.float64))
    if d > 2:
        cols.append(50.0 + 12.0 * rng.normal(size=N))
    if d > 3:
        cols.append(0.01 * rng.normal(size=N))
    for target in (4.0 * (1.0 - 2.0 ** -30), 8.0)[:max(0, min(2, d - 4))]:
        z = rng.normal(size=N)
        i = int(np.argmax(np.abs(z)))
        c = z * (target / abs(z[i]))
        c[i] = np.sign(z[i]) * target                       # (exactly: the product above may round beside it)
        c = np.clip(c, -target, target)
        assert np.max(np.abs(c)) == target
        cols.append(c)
    for _ in range(max(0, d - 6)):
        cols.append(10.0 ** rng.uniform(-1.0, 1.0) * rng.normal(size=N))
    X = np.asfortranarray(np.column_stack(cols))
    assert X.shape == (N, d)
    lin = np.zeros(N)
    if d > 1:
        lin += 0.3 * X[:, 1]
    if d > 2:
        lin += 0.02 * (X[:, 2] - 50.0)
    if d > 4:
        lin -= 0.1 * X[:, 4]
    if G_effect is not None:
        lin += G_effect
    if binary:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(-1.0 + lin)))).astype(np.float64)
        rc, beta, p, v = orc.fit_logistic(X, y)
        assert rc == 0
        return X, y, y - p, v, 1.0
    y = lin + rng.normal(size=N)
    rc, beta, pred, res, s2 = orc.fit_linear(X, y)
    assert rc == 0
    return X, y, res, np.full(N, s2), s2


def null_tile(X, res, v, binary):
    """The tile the integer kernels multiply with, as rvt_set_null forms it in fp64: [X | rr] (rr = res), or
    [v o X | res | v] under a binary trait.  Column d is the one behind u = G'res in both."""
    if binary:
        return np.asfortranarray(np.column_stack([v[:, None] * X, res, v]))
    return np.asfortranarray(np.column_stack([X, res]))


def expected_route(d, binary, input_kind):
    """The route table by d.  input_kind: 'block' (an fp64 block of hard calls), 'bed' (rvt_submit_gene_bed), 'bed_dev'
    (rvt_submit_gene[s]_bed_dev), 'score_bed_dev', 'lattice', 'float'."""
    if input_kind == "block":
        if d > HC_MAX_D:
            return "fp64"
        if not binary:
            return "gene_suffstat_hc"
        return "gene_suffstat_hcx" if d <= HCX_MAX_D else "gene_suffstat_hcw"
    if input_kind == "bed":
        return "gene_suffstat_hcp" if (d <= HC_MAX_D and not binary) else "expanded"
    if input_kind == "bed_dev":
        return "gene_tnull_hcp" if (d <= HC_MAX_D and not binary) else "expanded"
    if input_kind == "score_bed_dev":
        return "planes" if d <= HC_MAX_D else "refused"
    if input_kind == "lattice":
        return "gene_suffstat_lat" if (d <= HC_MAX_D and not binary) else "fp64"
    if input_kind == "float":
        return "gene_suffstat_fdx" if (d <= FDX_MAX_D and not binary) else "fp64"
    raise ValueError(input_kind)


def column_scale_ratio(tile):
    """Per column: the largest magnitude over the median of the non-zero magnitudes — column_scale_ok's quantity (the upper
    median, nth_element at size / 2); 0 for a zero column."""
    tile = np.asarray(tile, dtype=np.float64).reshape(len(tile), -1)
    out = np.zeros(tile.shape[1])
    for k in range(tile.shape[1]):
        mag = np.sort(np.abs(tile[:, k][tile[:, k] != 0.0]))
        if mag.size:
            out[k] = mag[-1] / mag[mag.size // 2]
    return out


def quantise(col, B):
    """(q, shift): the integers the digit planes of one tile column encode, q_i = rint(col_i 2^shift), under the shift rule of
    rvt_set_null (B = 42) / ensure_hcp_planes (B = 56): mx = f 2^e with 0.5 <= f < 1, shift = B - (e + 1), one less when
    mx 2^shift > 0.98 2^(B - 1) — the balanced digits end at 0.496 2^B.  A zero column: shift 0."""
    col = np.asarray(col, dtype=np.float64)
    mx = float(np.max(np.abs(col)))
    if mx == 0.0:
        return np.zeros(col.shape, dtype=np.int64), 0
    f, e = np.frexp(mx)
    shift = B - (int(e) + 1)
    if np.ldexp(mx, shift) > 0.98 * 2.0 ** (B - 1):
        shift -= 1
    q = np.rint(np.ldexp(col, shift))                      # (llrint: to nearest, ties to even; exact in fp64 below 2^63)
    assert np.max(np.abs(q)) <= 63 * sum(128 ** p for p in range(B // 7))
    return q.astype(np.int64), shift


FP64_ROUTES = ("fp64", "gene_suffstat_hc", "gene_suffstat_hcw", "gene_suffstat_hcp", "gene_suffstat_lat")
PLANE_BITS = {"gene_suffstat_hcx": B_HCX, "gene_tnull_hcp": B_PLANES}


def t_bound(G, tile, route):
    """(M, ncols) bounds on |T_jk - ref| for T = G'tile (column d: u), G the mean-imputed matrix.
    a_jk = sum_i |g_ij z_ik|, c_j = sum_i |g_ij|.
    fp64 product routes: N u a_jk — any order of N fp64 multiply-adds.
    Digit-plane routes: c_j max_i |z_ik| 2^-(B-2) + 8 u a_jk.  The first term: an entry of the quantised column is off by at most
    half a unit, 2^-shift / 2, and 2^-shift <= max |z_k| 2^-(B-3) after the decrement; the sum over the samples is an exact integer.
    A mean-imputed column is H + mu m with both operands on the planes: c_j over the IMPUTED column, c(H) + |mu| c(m), is that
    bound on the H operand plus |mu| times it on the mask operand.  The second term: the integer sums of the wave-parts turned
    into doubles, scaled and added."""
    A = np.abs(G).T @ np.abs(tile)
    if route in FP64_ROUTES:
        return G.shape[0] * U53 * A
    B = PLANE_BITS[route]
    c = np.abs(G).sum(0)
    return c[:, None] * np.max(np.abs(tile), axis=0)[None, :] * 2.0 ** -(B - 2) + 8.0 * U53 * A


def s_bound(G, w, binary, imputed):
    """(M, M) bounds on |S_jl - ref| for S = G' diag(w) G.  Quantitative hard calls without imputed entries: 0 — the int8 Gram
    matrix is an integer and exact.  Binary: sum_i g_ij g_il 2^-43 (the weights rounded to 42 fractional bits) + N u sum_i v_i
    g_ij g_il.  Quantitative with imputed entries, and every fp64 kernel: N u sum_i |g_ij g_il| — the integer parts are exact
    and mu enters through a few fp64 products and sums of non-negative terms; N of them bound any such order."""
    GG = np.abs(G).T @ np.abs(G)
    if binary:
        return GG * 2.0 ** -43 + G.shape[0] * U53 * ((np.abs(G) * w[:, None]).T @ np.abs(G))
    if not imputed:
        return np.zeros_like(GG)
    return G.shape[0] * U53 * GG


def ref_suffstat(G, w, tile):
    """(S, T) = (G' diag(w) G, G' tile) in long double (64-bit significand: 2^-11 of fp64's rounding per operation)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "long double is not wider than double on this machine"
    Gl = np.asarray(G, dtype=np.longdouble)
    S = (Gl * np.asarray(w, dtype=np.longdouble)[:, None]).T @ Gl
    T = Gl.T @ np.asarray(tile, dtype=np.longdouble)
    return S, T


def emulate_planes(raw, tile, B):
    """T = G'tile of raw hard calls (negative = missing) as a digit-plane route forms it: H'q and m'q in Python integers
    (exact), turned into doubles, scaled by 2^-shift and combined with the imputed value — what the kernels add in fp64
    behind their exact integer sums."""
    raw = np.asarray(raw)
    G = orc.impute_mean(np.asfortranarray(raw, dtype=np.float64))
    H = np.where(raw < 0, 0, raw).astype(np.int64).astype(object)
    m = (raw < 0).astype(np.int64).astype(object)
    out = np.zeros((raw.shape[1], tile.shape[1]))
    for k in range(tile.shape[1]):
        q, shift = quantise(tile[:, k], B)
        qo = q.astype(object)
        hq, mq = H.T.dot(qo), m.T.dot(qo)
        for j in range(raw.shape[1]):
            mu = float(G[raw[:, j] < 0, j][0]) if (raw[:, j] < 0).any() else 0.0
            out[j, k] = np.ldexp(float(int(hq[j])), -shift) + mu * np.ldexp(float(int(mq[j])), -shift)
    return G, out


def raw_gene(N, M, seed, missing=0.01):
    """Raw hard calls (-9 = missing) with the columns that go wrong: a flipped column (sum > N), one value plus missing calls
    (monomorphic), an all-zero column, nothing but missing calls, an imputed value >= 1.  missing = 0: no missing call at all
    (the special columns keep their called part)."""
    rng = np.random.default_rng(seed)
    maf = 10 ** rng.uniform(-2.7, -0.5, M)
    raw = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    if missing > 0:
        raw[rng.random((N, M)) < missing] = -9.0
    if M > 3:
        raw[:, 1] = np.where(raw[:, 1] < 0, -9.0, rng.binomial(2, 0.9, size=N))
    if M > 6:
        raw[:, 4] = np.where(rng.random(N) < 0.1, -9.0, 1.0) if missing > 0 else 1.0
    if M > 8:
        raw[:, 7] = 0.0
    if M > 10 and missing > 0:
        raw[:, 9] = -9.0
    if M > 12:
        raw[:, 11] = np.where(rng.random(N) < (0.3 if missing > 0 else 0.0), -9.0, rng.binomial(2, 0.7, size=N))
    return np.asfortranarray(raw)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def gene(N, M, missing=True):
    """(raw, G, af) of THE gene of M variants at N samples — raw_gene, the oracle's imputation and counter frequencies; built
    once and shared (nobody writes into them).  missing=False: the same columns without a missing call."""
    def make():
        raw = raw_gene(N, M, seed=100 + M, missing=0.01 if missing else 0.0)
        return raw, orc.impute_mean(raw), orc.counter_af(raw)
    return _cached(("gene", N, M, missing), make)


def masked_gene(N, M, rate=0.2):
    """(raw, G, af): common variants with `rate` of the calls missing in EVERY column.  rate = 0.2: a slice of 64 samples holds
    about 13 M masked entries, many rounds of gene_suffstat_hcx's list of 48, and every lane of the wave holds one at once;
    rate = 0.02 at M = 80: few entries, but spread over five tiles — most lanes hold one."""
    def make():
        rng = np.random.default_rng(7000 + M)
        raw = rng.binomial(2, rng.uniform(0.05, 0.4, M), size=(N, M)).astype(np.float64)
        raw[rng.random((N, M)) < rate] = -9.0
        raw = np.asfortranarray(raw)
        assert np.all((raw < 0).sum(0) > 0)
        return raw, orc.impute_mean(raw), orc.counter_af(raw)
    return _cached(("masked", N, M, rate), make)


def lattice_gene(N, M, den=1000):
    """(K, G, af): decimal dosages K / den as a VCF DS field prints them — hard calls blurred by the imputation; one flipped
    column; G the double nearest to K / den."""
    def make():
        rng = np.random.default_rng(8000 + M)
        H = rng.binomial(2, 10 ** rng.uniform(-2.7, -0.7, M), size=(N, M))
        blur = np.rint(np.abs(rng.normal(0.0, 0.04, size=(N, M))) * den).astype(np.int64)
        blur[rng.random((N, M)) < 0.7] = 0
        K = np.where(H == 2, 2 * den - blur, np.where(H == 1, den + blur * rng.choice([-1, 1], size=(N, M)), blur))
        Hc = rng.binomial(2, 0.85, size=N)
        K[:, 2] = np.clip(Hc * den - blur[:, 2] * (Hc > 0), 0, 2 * den)
        K = np.clip(K, 0, 2 * den).astype(np.int64)
        G = np.asfortranarray(K.astype(np.float64) / float(den))
        return K, G, G.sum(0) / (2.0 * N)
    return _cached(("lattice", N, M, den), make)


def float_gene(N, M):
    """(G, af): dosages as an 8-bit BGEN block gives them, p = float32(v) float32(1 / 255), dosage = p1 + 2 p2 in double —
    multiples of 2^-37."""
    def make():
        rng = np.random.default_rng(9000 + M)
        s = np.float32(1.0 / 255.0)
        carrier = rng.random((N, M)) < 0.05
        doubt = rng.random((N, M)) < 0.1
        v1 = np.where(carrier, 255 - rng.integers(0, 32, (N, M)), np.where(doubt, rng.integers(0, 8, (N, M)), 0))
        v2 = np.where(carrier, rng.integers(0, 16, (N, M)), np.where(doubt, rng.integers(0, 2, (N, M)), 0))
        v1 = np.minimum(v1, 255 - v2)
        G = np.asfortranarray((v1.astype(np.float32) * s).astype(np.float64) + 2.0 * (v2.astype(np.float32) * s).astype(np.float64))
        return G, np.clip(G.mean(0) / 2, 1e-6, 1.0)
    return _cached(("float", N, M), make)


def case_model(N, d, binary):
    """THE model of (N, d, binary): make_model with the gene of 33 variants planted (three of its rare columns carry an
    effect) — what both test files install."""
    def make():
        G = gene(N, 33)[1]
        return make_model(N, d, binary, model_seed(N, d, binary), G_effect=0.4 * G[:, [0, 2, 3]].sum(1))
    return _cached(("model", N, d, binary), make)
