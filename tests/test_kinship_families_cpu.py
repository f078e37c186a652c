"""CPU: the host-only parts of the family-form kinship — rvt_kinship_components against a plain union-find, the new
symbols in the header and the library, and the Python wrappers' checks, which run before any device call."""
import re

import numpy as np
import pytest

import rvtests_amd
from rvtests_amd import engine
from test_abi import HEADER, declared_functions

NEW = ["rvt_set_kinship_families", "rvt_kinship_decompose_families", "rvt_kinship_components",
       "rvt_group_set_kinship_families"]


def plain_components(N, i, j):
    """Connected components by repeated relabelling: families in the order of their first member, members ascending."""
    label = list(range(N))
    changed = True
    while changed:
        changed = False
        for a, b in zip(i, j):
            lo = min(label[a], label[b])
            if label[a] != lo or label[b] != lo:
                label[a] = label[b] = lo
                changed = True
        for k in range(N):                       # path to the smallest label of the component
            if label[label[k]] != label[k]:
                label[k] = label[label[k]]
                changed = True
    fams = {}
    for k in range(N):
        fams.setdefault(label[k], []).append(k)
    return [fams[r] for r in sorted(fams, key=lambda r: fams[r][0])]


@pytest.mark.parametrize("N,n_pairs,seed", [(1, 0, 0), (7, 0, 1), (50, 30, 2), (400, 250, 3), (400, 2000, 4), (1000, 600, 5)])
def test_components_match_a_plain_union_find(N, n_pairs, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, N, n_pairs).astype(np.int32)
    j = rng.integers(0, N, n_pairs).astype(np.int32)
    if n_pairs >= 30:
        i[:5] = j[:5]                            # self-pairs
        i[5:15], j[5:15] = i[15:25], j[15:25]    # repeats
        j[25:30], i[25:30] = i[15:20], j[15:20]  # the same pairs the other way round
    fam_ptr, members = rvtests_amd.kinship_components(N, i, j)
    want = plain_components(N, i.tolist(), j.tolist())
    assert fam_ptr.dtype == np.int64 and members.dtype == np.int32
    assert fam_ptr[0] == 0 and fam_ptr[-1] == N and len(fam_ptr) == len(want) + 1
    got = [members[fam_ptr[f]:fam_ptr[f + 1]].tolist() for f in range(len(fam_ptr) - 1)]
    assert got == want
    assert sorted(members.tolist()) == list(range(N))
    firsts = [g[0] for g in got]
    assert firsts == sorted(firsts) and all(g == sorted(g) for g in got)
    if n_pairs < N:
        assert any(len(g) == 1 for g in got)     # isolated samples are families of their own


def test_components_are_not_capped_at_64():
    N = 200
    fam_ptr, members = rvtests_amd.kinship_components(N, np.arange(N - 1, dtype=np.int32), np.arange(1, N, dtype=np.int32))
    assert fam_ptr.tolist() == [0, N] and members.tolist() == list(range(N))


def test_components_refuse_bad_pairs():
    with pytest.raises(rvtests_amd.RvtError):
        rvtests_amd.kinship_components(5, [0, 5], [1, 2])
    with pytest.raises(rvtests_amd.RvtError):
        rvtests_amd.kinship_components(5, [0, -1], [1, 2])
    with pytest.raises(rvtests_amd.RvtError):
        rvtests_amd.kinship_components(0, [], [])
    with pytest.raises(TypeError):
        rvtests_amd.kinship_components(5, [0.5], [1.0])
    with pytest.raises(ValueError):
        rvtests_amd.kinship_components(5, [0, 1], [1])


def test_new_symbols_are_declared_documented_and_exported():
    names = declared_functions()
    lib = rvtests_amd.load_library()
    src = open(HEADER).read()
    for n in NEW:
        assert n in names and hasattr(lib, n)
        # documented like its neighbours: a comment block ends directly in front of the declaration
        assert re.search(r"\*/\s*int\s+" + n + r"\s*\(", src), n


class NoDevice:
    """Stands where the loaded library would: any call through it is a device call made too early."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached the library (%s) before it had checked its arguments" % name)


def bare(cls):
    e = cls.__new__(cls)
    e.L = NoDevice()
    e.ctx = e.g = None
    return e


GOOD = dict(fam_ptr=np.array([0, 2, 3], dtype=np.int64), members=np.array([2, 0, 1], dtype=np.int32),
            blocks=np.arange(5, dtype=np.float32), S=np.ones(3, dtype=np.float32))


def test_family_form_accepts_and_converts():
    N, n_fam, fp, mem, blk, S = rvtests_amd.family_form([0, 2, 3], [2, 0, 1], np.arange(5.0), np.ones(3))
    assert (N, n_fam) == (3, 2)
    assert fp.dtype == np.int64 and mem.dtype == np.int32 and blk.dtype == np.float32 and S.dtype == np.float32
    assert all(a.flags.c_contiguous for a in (fp, mem, blk, S))


@pytest.mark.parametrize("change,err", [
    (dict(fam_ptr=np.array([0.0, 2.0, 3.0])), TypeError),
    (dict(members=np.array([2.0, 0.0, 1.0])), TypeError),
    (dict(blocks=np.arange(5)), TypeError),
    (dict(S=np.ones(3, dtype=np.int32)), TypeError),
    (dict(fam_ptr=np.array([[0, 2, 3]])), ValueError),
    (dict(fam_ptr=np.array([0])), ValueError),
    (dict(members=np.array([[2, 0, 1]])), ValueError),
    (dict(blocks=np.zeros((5, 1), dtype=np.float32)), ValueError),
    (dict(blocks=np.zeros(4, dtype=np.float32)), ValueError),
    (dict(blocks=np.zeros(6, dtype=np.float32)), ValueError),
    (dict(S=np.ones(4, dtype=np.float32)), ValueError),
    (dict(S=np.ones((3, 1), dtype=np.float32)), ValueError),
    (dict(members=np.array([2, 0, -1])), ValueError),
])
def test_wrappers_reject_wrong_dtypes_and_shapes_before_any_device_call(change, err):
    args = dict(GOOD, **change)
    for obj in (bare(engine.Engine), bare(engine.Group)):
        with pytest.raises(err):
            obj.set_kinship_families(args["fam_ptr"], args["members"], args["blocks"], args["S"])
    if "S" not in change:
        with pytest.raises(err):
            bare(engine.Engine).kinship_decompose_families(args["fam_ptr"], args["members"], args["blocks"])


def test_wrappers_reach_the_library_only_with_checked_arguments():
    with pytest.raises(AssertionError, match="rvt_set_kinship_families"):
        bare(engine.Engine).set_kinship_families(**{("U_blocks" if k == "blocks" else k): v for k, v in GOOD.items()})
