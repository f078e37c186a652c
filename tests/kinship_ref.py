"""A literal numpy fp64 restatement of `vcf2kinship --ibs` / `--bn` on hard calls (vcfUtils/vcf2kinship.cpp): the site loop
of :943-960 and IBSKinship / BaldingNicolsKinship addGenotype + calculate (:138-266), site by site, in the reference's order.
Written with per-site loops over what the reference adds — NOT with the plane identity the device uses — so that the
identity is what the comparison tests.

G: (N, V) integer calls 0 / 1 / 2, negative = missing.  kinship(G, method, min_maf, max_missing) -> (K, info) with
info = dict(sites, sites_used, filtered_missing, filtered_maf, monomorphic).  The one stated difference from the reference is
carried here too: a BN site whose calls are all 2 (scale = inf, the reference's K turns NaN) is skipped as monomorphic."""
import numpy as np


def site_filter(g, min_maf, max_missing):
    """The category of one site: None (used), or the first filter of :943-960 that drops it."""
    N = len(g)
    called = g >= 0
    n_miss = int(N - called.sum())
    if n_miss > 1.0 * max_missing * N:                    # :943  nMiss > maxMissing, maxMissing = 1.0 * FLAG_maxMissing * N (:805)
        return "filtered_missing"
    ac = int(g[called].sum())
    total_ac = 2 * int(called.sum())
    af = 1.0 * ac / total_ac if total_ac > 0 else 0.0     # :949-952
    if af < min_maf or af > 1.0 - min_maf:                # :953
        return "filtered_maf"
    if not (g[called] != 0).any():                        # :957  !hasVariant
        return "monomorphic"
    return None


def kinship(G, method, min_maf=0.0, max_missing=1.0):
    G = np.asarray(G)
    N, V = G.shape
    info = dict(sites=V, sites_used=0, filtered_missing=0, filtered_maf=0, monomorphic=0)
    k = np.zeros((N, N))
    count = np.zeros((N, N))
    n = 0
    for v in range(V):
        g = G[:, v].astype(np.int64)
        cat = site_filter(g, min_maf, max_missing)
        if cat is not None:
            info[cat] += 1
            continue
        called = g >= 0
        if method == "ibs":
            # addGenotype :150-157: if (g[i] >= 0 && g[j] >= 0) { k[i][j] += 2.0 - abs(g[i] - g[j]); ++count[i][j]; }
            # (the N x N terms of a site as int8 — they are 0, 1 or 2 — then added to the fp64 sums, as the reference adds them)
            g8 = g.astype(np.int8)
            both = np.logical_and.outer(called, called)
            term = np.int8(2) - np.abs(np.subtract.outer(g8, g8))
            np.add(k, term * both, out=k)
            np.add(count, both, out=count)
            n += 1
        else:
            s = float(g[called].sum())
            non_miss = int(called.sum())
            if s == 0.0:                                  # :214 (cannot happen behind :957; kept as written)
                info["monomorphic"] += 1
                continue
            if s == 2.0 * non_miss:                       # every call 2: scale = inf in the reference — skipped here
                info["monomorphic"] += 1
                continue
            mean = s / non_miss                           # :219
            scale = np.sqrt(1.0 / (1.0 - mean / 2.0) / mean)   # :220
            geno = np.where(called, (g.astype(np.float64) - mean) * scale, 0.0)   # :224-231
            k += np.outer(geno, geno)                     # :236-241 (a zero geno[i] adds nothing)
            n += 1
    if method == "ibs":
        K = np.zeros((N, N))
        np.divide(k, count, out=K, where=count > 0)       # calculate :160-170: entries with count == 0 stay 0
    else:
        K = k / n if n > 0 else k                         # calculate :246-254
    info["sites_used"] = n
    return K, info
