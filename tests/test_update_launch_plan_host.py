"""The geometry of a per-class update launch (update_launch_plan in csrc/kernels.hip) through its
test entry smi_update_launch_plan_test: a pure host function, no device needed.

Sizes of the kernel that the checks need (csrc/common.h, csrc/kernels.hip): class c has
NPL[c] pixels per lane and TEAM[c] threads per component; a one-wavefront class packs up to
4 * waves-per-SIMD wavefronts into a workgroup; a wavefront's image takes (TEAM * NPL + 4)
floats of dynamic LDS; the kernel's static LDS is 256 B per packed wavefront plus 64 B; a
CU has 160 KB of LDS.
"""

import ctypes

import numpy as np
import pytest

NPL = [7, 16, 27, 42, 59, 16, 27, 42, 59]
TEAM = [64] * 5 + [256] * 4
PACK_MAX = [16, 16, 12, 8, 8, 1, 1, 1, 1]
LDS = 160 * 1024
PACK_LIMIT = 1024  # kUpdatePackLimit
CUS = 256
# ring plan bytes of the order of the standard boxes' (41^2: the workgroup's 105 KB less its
# twelve images; 61^2: 49 KB)
STAGE = {0: 6000, 2: 24000, 4: 49000}
NONE, TRAILING, IN_GRID, SEPARATE = 0, 1, 2, 3
CASES = [(2, 1024), (2, 1025), (2, 3072), (2, 3073), (2, 3413), (2, 10240), (4, 4096)]


@pytest.fixture(scope="module")
def plan():
    from scarlet_amd import _lib

    lib = _lib.load()

    def get(n_items, cls, stage_bytes, pending, cus=CUS, ranges=1, range_items=None):
        out = np.zeros(8, dtype=np.int64)
        _lib.check(lib.smi_update_launch_plan_test(
            n_items, cls, stage_bytes, cus, n_items if range_items is None else range_items,
            int(pending), ranges, _lib.ptr(out, ctypes.c_int64)))
        keys = ("pack", "blocks", "persistent", "stage", "lds", "lds_table", "gather_off", "fold")
        return dict(zip(keys, (int(x) for x in out)))

    return get


def static_lds(cls):
    return PACK_MAX[cls] * 256 + 64


def shares(p, n_items):
    """[lo, hi) of every updating workgroup (include/scarlet_amd.h)."""
    if p["persistent"]:
        q, r = divmod(n_items, p["blocks"])
        return [(i * q + min(i, r), i * q + min(i, r) + q + (i < r)) for i in range(p["blocks"])]
    return [(i * p["pack"], min((i + 1) * p["pack"], n_items)) for i in range(p["blocks"])]


@pytest.mark.parametrize("cls,n_items", CASES)
@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("ranges", [1, 3])
def test_shares_lds_table_and_bookkeeping(plan, cls, n_items, pending, ranges):
    p = plan(n_items, cls, STAGE[cls], pending, ranges=ranges)
    per_wave = (TEAM[cls] * NPL[cls] + 4) * 4
    assert p["stage"] == 1 and 4 <= p["pack"] <= PACK_MAX[cls]
    # the shares cover the list exactly once, none is empty
    sh = shares(p, n_items)
    assert sh[0][0] == 0 and sh[-1][1] == n_items
    assert all(a[1] == b[0] for a, b in zip(sh, sh[1:])) and all(lo < hi for lo, hi in sh)
    # the LDS: images + plan (+ table) + static within a CU's 160 KB
    assert p["lds"] == p["pack"] * per_wave + STAGE[cls]
    assert max(p["lds"], p["lds_table"]) + static_lds(cls) <= LDS
    # the gather table costs no wavefront (the pack is what the plan alone allows) and no
    # workgroup of the CU, and lies behind images and plan
    fit = (LDS - (PACK_MAX[cls] * 256 + 64 + STAGE[cls])) // per_wave
    assert p["pack"] == min(PACK_MAX[cls], fit)
    if p["gather_off"] >= 0:
        assert p["gather_off"] % 16 == 0 and p["gather_off"] >= p["lds"]
        assert p["lds_table"] == p["gather_off"] + TEAM[cls] * NPL[cls] * 4
        assert LDS // (p["lds_table"] + static_lds(cls)) == LDS // (p["lds"] + static_lds(cls))
    else:
        assert p["lds_table"] == p["lds"]
    assert (p["gather_off"] >= 0) == (cls == 2)  # (61^2: seven images and the plan fill the LDS)
    # persistent exactly when the full workgroups outnumber what the chip holds at once; the
    # grid is then the chip, or half of it for a range that shares the chip with other ranges
    # where a workgroup fills a CU
    per_cu = max(1, LDS // (p["lds"] + static_lds(cls)))
    resident = CUS * per_cu
    full = -(-n_items // p["pack"])
    assert per_cu == 1
    assert p["persistent"] == int(full > resident)
    assert p["blocks"] == ((resident // 2 if ranges > 1 else resident) if p["persistent"] else full)
    # the bookkeeping travels exactly once: in the grid of a persistent launch, as trailing
    # workgroups of a small one, else as a kernel of its own -- and not at all if none is pending
    if not pending:
        assert p["fold"] == NONE
    elif p["persistent"]:
        assert p["fold"] == IN_GRID
        for nb in (1, p["blocks"] - 1, p["blocks"], 342, 1024):
            taken = sorted(b for i in range(p["blocks"]) for b in range(i, nb, p["blocks"]))
            assert taken == list(range(nb))
    else:
        assert p["fold"] == (TRAILING if n_items <= PACK_LIMIT else SEPARATE)
    # the geometry does not depend on the bookkeeping
    q = plan(n_items, cls, STAGE[cls], not pending, ranges=ranges)
    assert {k: v for k, v in p.items() if k != "fold"} == {k: v for k, v in q.items() if k != "fold"}


def test_expected_numbers_of_the_flagship_range(plan):
    """3 413 boxes of 41^2 (a third of 1024 blends of ten), one workgroup of twelve wavefronts per
    CU: alone 256 workgroups with shares of 13 and 14, as one of three ranges 128 with shares of
    26 and 27."""
    p = plan(3413, 2, STAGE[2], True)
    assert (p["pack"], p["blocks"], p["persistent"], p["fold"]) == (12, 256, 1, IN_GRID)
    assert sorted({hi - lo for lo, hi in shares(p, 3413)}) == [13, 14]
    p = plan(3413, 2, STAGE[2], True, ranges=3)
    assert (p["pack"], p["blocks"], p["persistent"], p["fold"]) == (12, 128, 1, IN_GRID)
    assert sorted({hi - lo for lo, hi in shares(p, 3413)}) == [26, 27]
    # the boundary is that of the persistent launch, whatever the number of ranges; an odd chip
    # rounds its half up
    for ranges in (2, 3, 4):
        assert plan(3072, 2, STAGE[2], True, ranges=ranges)["blocks"] == 256
        assert plan(3073, 2, STAGE[2], True, ranges=ranges)["blocks"] == 128
    assert plan(3073, 2, STAGE[2], True, cus=255, ranges=2)["blocks"] == 128
    assert plan(3073, 2, STAGE[2], True, cus=255, ranges=1)["blocks"] == 255
    assert plan(3072, 2, STAGE[2], True)["persistent"] == 0
    assert plan(3073, 2, STAGE[2], True)["persistent"] == 1
    # a smaller chip turns persistent earlier
    assert plan(1025, 2, STAGE[2], True, cus=64)["fold"] == IN_GRID


def test_gather_table_is_left_out_where_it_would_cost_a_workgroup(plan):
    """21^2 class, 16 wavefronts of 1 808 B: with 7 072 B of plan four workgroups share a CU
    (40 160 B each) and the table's 1 792 B would make it three; with 6 000 B it fits."""
    p = plan(2000, 0, 7072, False)
    assert p["pack"] == 16 and p["lds"] == 36000 and p["gather_off"] == -1 and p["lds_table"] == 36000
    assert LDS // (36000 + static_lds(0)) == 4 and LDS // (36000 + 1792 + static_lds(0)) == 3
    p = plan(2000, 0, 6000, False)
    assert p["gather_off"] == 16 * 1808 + 6000 and p["lds_table"] == p["gather_off"] + 1792


def test_shared_ranges_keep_the_full_grid_where_workgroups_share_a_cu(plan):
    """21^2 class: four workgroups of sixteen wavefronts per CU, so half a grid would still sit
    on every CU."""
    n = 16 * 4 * CUS + 1
    one, three = plan(n, 0, STAGE[0], True), plan(n, 0, STAGE[0], True, ranges=3)
    assert one == three and one["persistent"] == 1 and one["blocks"] == 4 * CUS
    assert plan(n - 1, 0, STAGE[0], True, ranges=3)["persistent"] == 0


def test_small_first_class_of_a_large_range_gets_no_trailing_workgroups(plan):
    """300 boxes of 61^2 in a range of 3 413 components: the launch is small, the range is not --
    the bookkeeping stays a kernel of its own; geometry as for the class alone."""
    alone, mixed = plan(300, 4, STAGE[4], True), plan(300, 4, STAGE[4], True, range_items=3413)
    assert alone["fold"] == TRAILING and mixed["fold"] == SEPARATE
    assert dict(alone, fold=0) == dict(mixed, fold=0)
    assert plan(300, 4, STAGE[4], True, range_items=PACK_LIMIT)["fold"] == TRAILING
    assert plan(300, 4, STAGE[4], True, range_items=PACK_LIMIT + 1)["fold"] == SEPARATE
    # a persistent first class carries it whatever the range holds besides
    assert plan(3413, 2, STAGE[2], True, range_items=5000)["fold"] == IN_GRID
    with pytest.raises(Exception):
        plan(300, 4, STAGE[4], True, range_items=299)


def test_classes_without_a_staged_plan(plan):
    """No ring plan, or a four-wavefront team: packed while small, one component per workgroup
    beyond, never persistent; the bookkeeping trails a small launch and is a kernel of its own
    in front of a large one."""
    for cls, stage in ((2, -1), (6, 24000), (6, -1)):
        per = (TEAM[cls] * NPL[cls] + 4) * 4
        small, large = plan(PACK_LIMIT, cls, stage, True), plan(PACK_LIMIT + 1, cls, stage, True)
        assert small["pack"] == PACK_MAX[cls] and large["pack"] == 1
        assert small["blocks"] == -(-PACK_LIMIT // PACK_MAX[cls]) and large["blocks"] == PACK_LIMIT + 1
        for p in (small, large):
            assert (p["stage"], p["persistent"], p["gather_off"]) == (0, 0, -1)
            assert p["lds"] == p["lds_table"] == p["pack"] * per
            assert p["lds"] + static_lds(cls) <= LDS
        assert small["fold"] == TRAILING and large["fold"] == SEPARATE


def test_bad_arguments_are_refused(plan):
    from scarlet_amd._lib import ScarletAmdError

    for args in ((0, 2, 24000), (10, 9, 24000), (10, -1, 24000)):
        with pytest.raises(ScarletAmdError):
            plan(*args, True)
    with pytest.raises(ScarletAmdError):
        plan(10, 2, 24000, True, cus=0)
    with pytest.raises(ScarletAmdError):
        plan(10, 2, 24000, True, ranges=0)
