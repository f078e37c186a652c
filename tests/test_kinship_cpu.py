"""CPU: the numpy restatement of vcf2kinship's IBS / Balding-Nichols kinship (tests/kinship_ref.py) against values worked by
hand, the plane identity the device product is built on, and the C ABI / binding of rvt_kinship_from_bed (no compute calls:
there is no GPU here)."""
import ctypes as C
import os
import subprocess

import numpy as np

import kinship_ref
import rvtests_amd
from rvtests_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rvtests_amd.h")

# four samples A B C D, three sites; D is missing at the second site; the third site has mean 0.5
G43 = np.array([[0, 2, 0],
                [1, 2, 1],
                [2, 0, 1],
                [1, -9, 0]])


def sym(n, entries):
    K = np.zeros((n, n))
    for (i, j), v in entries.items():
        K[i, j] = K[j, i] = v
    return K


def test_ibs_by_hand():
    # per site 2 - |g_i - g_j| (the table's entries 2 / 1 / 0), summed over the sites where both are called, over their number:
    #   AB 1 + 2 + 1 over 3, AC 0 + 0 + 1 over 3, AD 1 + 2 over 2 (D missing at site 2), BC 1 + 0 + 2, BD 2 + 1 over 2, CD 1 + 1 over 2
    want = sym(4, {(0, 0): 2.0, (1, 1): 2.0, (2, 2): 2.0, (3, 3): 2.0, (0, 1): 4.0 / 3.0, (0, 2): 1.0 / 3.0, (0, 3): 3.0 / 2.0,
                   (1, 2): 3.0 / 3.0, (1, 3): 3.0 / 2.0, (2, 3): 2.0 / 2.0})
    K, info = kinship_ref.kinship(G43, "ibs")
    assert (K == want).all()
    assert info == dict(sites=3, sites_used=3, filtered_missing=0, filtered_maf=0, monomorphic=0)


def test_ibs_pair_never_called_together_is_zero():
    G = np.array([[0, -9], [-9, 1], [1, 1]])
    K, _ = kinship_ref.kinship(G, "ibs")
    assert K[0, 1] == 0.0 and K[1, 0] == 0.0
    assert K[0, 0] == 2.0 and K[0, 2] == 1.0 and K[1, 2] == 2.0


def test_bn_site_with_mean_one_half_by_hand():
    # g = 0 1 1 0: mean 1/2, scale = sqrt(1 / (1 - 1/4) / (1/2)) = sqrt(8/3), z = -+ sqrt(8/3) / 2, z z' = +- 2/3
    K, info = kinship_ref.kinship(G43[:, 2:3], "bn")
    s = np.array([-1.0, 1.0, 1.0, -1.0])
    np.testing.assert_allclose(K, np.outer(s, s) * 2.0 / 3.0, rtol=4e-16, atol=0)
    assert info["sites_used"] == 1


def test_bn_three_sites_by_hand():
    # site 1: mean 1, scale sqrt 2, z = sqrt 2 (-1 0 1 0); site 2: mean 4/3 over the three calls, scale 3/2, z = (1 1 -2 0);
    # site 3 as above; K = sum z z' / 3
    want = sym(4, {(0, 0): 11.0, (0, 1): 1.0, (0, 2): -14.0, (0, 3): 2.0, (1, 1): 5.0, (1, 2): -4.0, (1, 3): -2.0, (2, 2): 20.0,
                   (2, 3): -2.0, (3, 3): 2.0}) / 9.0
    K, info = kinship_ref.kinship(G43, "bn")
    np.testing.assert_allclose(K, want, rtol=0, atol=2e-15)   # a handful of roundings of sums below 8 (ulp 8.9e-16), then / 3
    assert (K == K.T).all() and info["sites_used"] == 3


def test_site_filters_in_the_reference_order():
    # 10 samples.  site 0: 4 missing (> 0.3 * 10) and monomorphic -> counted as filtered_missing, the first filter
    # site 1: af = 1/20 < 0.1 -> filtered_maf;  site 2: af = 19/20 > 0.9 -> filtered_maf;  site 3: nothing called (3 allowed
    # missing exceeded) -> filtered_missing;  site 4: kept (af = 4/20);  site 5: all 2 -> af = 1 -> filtered_maf
    G = np.zeros((10, 6), dtype=np.int64)
    G[:4, 0] = -9
    G[0, 1] = 1
    G[:, 2] = 2
    G[0, 2] = 1
    G[:, 3] = -9
    G[:4, 4] = 1
    G[:, 5] = 2
    for method in ("ibs", "bn"):
        _, info = kinship_ref.kinship(G, method, min_maf=0.1, max_missing=0.3)
        assert info == dict(sites=6, sites_used=1, filtered_missing=2, filtered_maf=3, monomorphic=0), method
    # nothing filtered: the all-zero site 0 and the uncalled site 3 are monomorphic; BN also skips the all-2 site 5
    _, info = kinship_ref.kinship(G, "ibs")
    assert info == dict(sites=6, sites_used=4, filtered_missing=0, filtered_maf=0, monomorphic=2)
    K, info = kinship_ref.kinship(G, "bn")
    assert info == dict(sites=6, sites_used=3, filtered_missing=0, filtered_maf=0, monomorphic=3)
    assert np.isfinite(K).all()
    # everything dropped: K stays zero
    K, info = kinship_ref.kinship(G, "bn", min_maf=0.5)
    assert info["sites_used"] == 0 and (K == 0).all()


def test_plane_identity_over_the_nine_pairs():
    """2 - |a - b| = 1 + (a - 1)(b - 1) + [a = 1][b = 1]: the n n' + u u' + h h' of the device product for two called samples"""
    for a in (0, 1, 2):
        for b in (0, 1, 2):
            assert 2 - abs(a - b) == 1 + (a - 1) * (b - 1) + int(a == 1) * int(b == 1), (a, b)


def test_abi_declares_exports_and_binds_kinship_from_bed(tmp_path):
    src = open(HEADER).read()
    assert "int rvt_kinship_from_bed(rvt_ctx* ctx, const unsigned char* d_rows, int64_t V, int method" in src
    assert "#define RVT_KINSHIP_IBS 0" in src and "#define RVT_KINSHIP_BN  1" in src
    rvtests_amd.build_library()
    lib = rvtests_amd.load_library()
    assert hasattr(lib, "rvt_kinship_from_bed")
    fn = lib.rvt_kinship_from_bed
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double),
                                 C.POINTER(engine.KinshipInfo)]
    assert callable(getattr(engine.Engine, "kinship_from_bed"))
    assert (engine.KINSHIP_IBS, engine.KINSHIP_BN) == (0, 1)
    # the ctypes mirror of rvt_kinship_info has the header's size and field offsets
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rvtests_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                    'sizeof(rvt_kinship_info),offsetof(rvt_kinship_info,monomorphic),offsetof(rvt_kinship_info,ms_stats),'
                    'offsetof(rvt_kinship_info,ms_finish));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(exe)])
    a, b, c, d = map(int, subprocess.check_output([str(exe)]).split())
    KI = engine.KinshipInfo
    assert (a, b, c, d) == (C.sizeof(KI), KI.monomorphic.offset, KI.ms_stats.offset, KI.ms_finish.offset)
