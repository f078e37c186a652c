"""CPU: rvt_burden_blocks is exported and the ctypes mirror of rvt_burden_more_result has the header's size and offsets."""
import ctypes as C
import os
import subprocess

import rvtests_amd
from rvtests_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_burden_blocks_is_exported():
    L = rvtests_amd.load_library()
    assert hasattr(L, "rvt_burden_blocks") and hasattr(L, "rvt_burden_last_columns")
    assert (engine.BURDEN_CMCWALD, engine.BURDEN_ZEGGINIWALD, engine.BURDEN_FP, engine.BURDEN_EXACTCMC) == (1, 2, 4, 8)


def test_record_layout_matches_the_header(tmp_path):
    R, W = engine.BurdenMoreResult, engine.BurdenWaldFit
    names = [f[0] for f in R._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rvtests_amd.h"\nint main(){\n'
    src += '  printf("%zu %zu %u %u %u %u %d", sizeof(rvt_burden_more_result), sizeof(rvt_burden_wald_fit), RVT_BURDEN_CMCWALD, ' \
           'RVT_BURDEN_ZEGGINIWALD, RVT_BURDEN_FP, RVT_BURDEN_EXACTCMC, RVT_MAX_COV);\n'
    for n in names:
        src += '  printf(" %%zu", offsetof(rvt_burden_more_result, %s));\n' % n
    for n in ("ok", "rounds", "beta", "se", "pvalue"):
        src += '  printf(" %%zu", offsetof(rvt_burden_wald_fit, %s));\n' % n
    src += "  return 0;\n}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    want = [C.sizeof(R), C.sizeof(W), 1, 2, 4, 8, engine.MAX_COV] + [getattr(R, n).offset for n in names] + \
           [getattr(W, n).offset for n in ("ok", "rounds", "beta", "se", "pvalue")]
    assert got == want
