#!/usr/bin/env python3
"""Generate tests/golden/ref_live.npz: the outputs of the COMPILED REFERENCE fragments under oracle/_ref (`make -C oracle
ref`, which needs the reference tree) for the tests that compare the oracle / the adapters with them — Davies / Liu / qf(),
GenotypeCounter + SNPHWE, the RingMemoryPool window walk, the Permutation stop rule, ModelParser, floatToString, the libVcf
genotype parsers and MVTDST.  Each test's REF_LIVE function makes the calls; a machine without the reference reads the
recorded outputs instead (orc.ref_outputs), one with it compares the live outputs with them.  Run where oracle/_ref is built."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
import test_oracle_ref  # noqa: E402
import test_vcf_cpu  # noqa: E402
import test_vt_cpu  # noqa: E402


def main():
    assert orc.ref() is not None and orc.ref_counter() is not None and orc.ref_vcf() is not None and \
        orc.ref_mvt() is not None and test_oracle_ref._ref_host() is not None, "build oracle/_ref first (make -C oracle ref)"
    arrays = {}
    for mod in (test_oracle_ref, test_vcf_cpu, test_vt_cpu):
        for key, live in mod.REF_LIVE.items():
            for name, v in live().items():
                arrays["%s/%s" % (key, name)] = np.asarray(v)
    out = os.path.join(HERE, "ref_live.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, len(arrays), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
