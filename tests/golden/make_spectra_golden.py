#!/usr/bin/env python3
"""Fixture for the M = 512 gene of tests/test_spectra_cpu.py / tests/test_gpu_spectra.py: the oracle's SKAT on
spectra_designs.make_plain_case(512, N=1200).  The oracle's dense eigensolver needs about ten seconds at this width, too
long for a test that every later change runs again, so its Q and p-value are recorded here once, with a SHA-256 digest of the
(integer-valued) genotype block and the residual sum of squares they belong to: a seeded generator that drifts fails that
check, not the comparison.
Run from the repository root after the oracle is built: python tests/golden/make_spectra_golden.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import orc                      # noqa: E402
import spectra_designs as sd    # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def main():
    c = sd.make_plain_case(512, N=1200)
    rc, a = orc.skat(c["G"], c["af"], c["X"], c["res"], c["v"], 0)
    assert rc == 0
    out = {"case": "spectra_designs.make_plain_case(512, N=1200)", "G_sha256": digest(c["G"].T), "rss": repr(float(c["res"] @ c["res"])),
           "n_poly": a.n_poly, "n_lambda": a.n_lambda, "skat_Q": repr(a.Q), "skat_p": repr(a.pvalue)}
    with open(os.path.join(HERE, "spectra_wide512.json"), "w") as fo:
        json.dump(out, fo, indent=1)
    print(out)


if __name__ == "__main__":
    main()
