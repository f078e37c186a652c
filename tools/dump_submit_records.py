#!/usr/bin/env python3
"""Every entry point of the gene submission path, with a fixed seed, records and returned frequencies written as hex doubles:
what two builds of the engine must agree on bit for bit when the submission path is rearranged.

    python tools/dump_submit_records.py OUT.json              # run on the GPU: one JSON document
    python tools/dump_submit_records.py --compare A.json B.json [--commits PARENT BRANCH] [--out RESULT.json]

Entry points: submit_gene, _raw, _i8, _bed, _bed_dev, _vcf (genotype and dosage text), _bgen; submit_genes kinds 1, 2, 3, 7;
score_bed_dev under a quantitative and a binary trait.  N in {130, 4099} (below / above the size from which int8 and fp64
blocks are packed on the way), M in {1, 17, 40}, with and without the frequencies returned, all on ONE engine per N so that
blocks are reused across entry points and widths."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NS = (130, 4099)
MS = (1, 17, 40)


def _hex(x):
    return [float(v).hex() for v in np.asarray(x, dtype=np.float64).ravel()]


def _record(r):
    out = {}
    for name, _ in type(r)._fields_:
        v = getattr(r, name)
        out[name] = float(v).hex() if isinstance(v, float) else int(v)
    return out


def _raw_gene(rng, N, M):
    maf = 10 ** rng.uniform(-2.0, -0.5, M)
    raw = rng.binomial(2, maf, size=(N, M)).astype(np.float64)
    raw[rng.random((N, M)) < 0.03] = -9.0
    raw[N // 2, :] = -9.0
    return np.asfortranarray(raw)


def _dosage_record(rng, n_file, pos):
    cols = [b"./.:." if rng.random() < 0.03 else b"0/1:%.3f" % rng.uniform(0, 2) for _ in range(n_file)]
    return b"\t".join([b"1", b"%d" % pos, b".", b"A", b"G", b"50", b"PASS", b".", b"GT:DS"]) + b"\t" + b"\t".join(cols)


def run(N):
    import rvtests_amd
    import bgengen
    import orc
    import synth
    import vcfgen
    rng = np.random.default_rng(20240 + N)
    e = rvtests_amd.Engine(0)
    X, y, res, v, s2 = synth.make_null(N, 2, 0, seed=17)
    e.set_null(0, X, res, v, s2)
    e.vcf_set_samples(np.arange(N, dtype=np.int32))
    e.vcf_set_filters(0, 0, 0, 0)
    out = {}
    gid = [0]

    def collect(name, afs):
        recs = e.collect()
        out[name] = {"af": [None if a is None else _hex(a) for a in afs], "records": [_record(r) for r in recs]}

    genes = {M: _raw_gene(rng, N, M) for M in MS}
    beds = {M: e.pack_bed(genes[M]) for M in MS}
    cb = (N + 3) // 4
    d_bed = e.bed_alloc(sum(MS) + 4)
    e.bed_upload(d_bed, 0, np.full((3, cb), 0x55, dtype=np.uint8))
    first, at = {}, 3
    for M in MS:
        e.bed_upload(d_bed, at, beds[M])
        first[M], at = d_bed + at * cb, at + M
    vcf = {M: [vcfgen.make_record(rng, N, fmt=[b"GT", b"GT:DP"][j & 1], edge=0.03, pos=10 * M + j) for j in range(M)] for M in MS}
    dos = {M: [_dosage_record(rng, N, 10 * M + j) for j in range(M)] for M in MS}
    bgen = {M: [bgengen.layout2_block_fast(rng, N, bits=(8, 16, 32)[j % 3], missing=0.02) for j in range(M)] for M in MS}

    def each(name, submit):
        for want_af in (True, False):
            afs = []
            for M in MS:
                gid[0] += 1
                afs.append(submit(gid[0], M, want_af))
            collect("%s/want_af=%d" % (name, want_af), afs)

    gene_af = {M: orc.counter_af(genes[M]) for M in MS}
    imputed = {M: orc.impute_mean(genes[M]) for M in MS}
    afs = []
    for M in MS:
        gid[0] += 1
        e.submit_gene(gid[0], imputed[M], gene_af[M])
        afs.append(None)
    collect("submit_gene", afs)
    each("submit_gene_raw", lambda g, M, w: e.submit_gene_raw(g, genes[M], want_af=w))
    each("submit_gene_i8", lambda g, M, w: e.submit_gene_raw(g, genes[M].astype(np.int8), want_af=w))
    each("submit_gene_bed", lambda g, M, w: e.submit_gene_bed(g, beds[M], M, want_af=w))
    each("submit_gene_bed_dev", lambda g, M, w: e.submit_gene_bed_dev(g, first[M], M, want_af=w))
    each("submit_gene_vcf", lambda g, M, w: e.submit_gene_vcf(g, vcf[M], want_af=w))
    e.vcf_set_dosage(True)
    each("submit_gene_vcf_dosage", lambda g, M, w: e.submit_gene_vcf_dosage(g, dos[M], b"DS", want_af=w))
    e.vcf_set_dosage(False)
    each("submit_gene_bgen", lambda g, M, w: e.submit_gene_bgen(g, bgen[M], 2, want_af=w))
    ids = [1000 + k for k in range(len(MS))]
    for kind, arrays in ((1, [genes[M] for M in MS]), (2, [np.asfortranarray(genes[M].astype(np.int8)) for M in MS]),
                         (3, [beds[M] for M in MS])):
        e.submit_genes(kind, ids, arrays, list(MS))
        collect("submit_genes/kind=%d" % kind, [None] * len(MS))
    e.submit_genes_bed_dev(ids, [first[M] for M in MS], list(MS))
    collect("submit_genes/kind=7", [None] * len(MS))
    V = sum(MS)
    out["score_bed_dev/quantitative"] = [_hex(a) for a in e.score_bed_dev(first[MS[0]], V)]
    Xb, yb, resb, vb, s2b = synth.make_null(N, 2, 1, seed=17)
    e.set_null(1, Xb, resb, vb, s2b)
    out["score_bed_dev/binary"] = [_hex(a) for a in e.score_bed_dev(first[MS[0]], V)]
    e.bed_free(d_bed)
    e.close()
    return out


def compare(path_a, path_b, commits, out_path):
    docs = []
    for p in (path_a, path_b):
        with open(p, "rb") as f:
            raw = f.read()
        docs.append((json.loads(raw), hashlib.sha256(raw).hexdigest()))
    (a, sha_a), (b, sha_b) = docs
    for doc in (a, b):      # (the AnalyticVT block is written only when that test is requested: not part of these records)
        for v in doc.values():
            if isinstance(v, dict):
                v["records"] = [{k: x for k, x in r.items() if not k.startswith("vt_")} for r in v["records"]]
    differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    doubles = sum(len(x) for v in a.values() for x in (v if isinstance(v, list) else v["af"]) if x) + \
        sum(len(r) for v in a.values() if isinstance(v, dict) for r in v["records"])
    result = {"identical": not differing, "differing_entries": differing, "entries": sorted(a), "values_compared": doubles,
              "sha256": {"parent": sha_a, "branch": sha_b},
              "commits": {"parent": commits[0], "branch": commits[1]} if commits else None}
    text = json.dumps(result, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if not differing else 1


def main(argv):
    if argv and argv[0] == "--compare":
        commits = argv[argv.index("--commits") + 1:argv.index("--commits") + 3] if "--commits" in argv else None
        out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
        return compare(argv[1], argv[2], commits, out_path)
    doc = {}
    for N in NS:
        for k, v in run(N).items():
            doc["N=%d/%s" % (N, k)] = v
    with open(argv[0], "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
    print("wrote", argv[0], len(doc), "entries")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
