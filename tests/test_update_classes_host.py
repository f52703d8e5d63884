"""CPU preconditions of tests/test_gpu_update_classes.py: the case table of
tests/update_class_cases.py is annotated correctly (size class and sweep plan of every box), its
starting images give every chain work to do, and the numpy restatement of the kernels' maximum
normalisation lies within one ulp of the oracle's division.  No GPU."""

import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import update_class_cases as cases
from conftest import ROOT

WEIGHTINGS = sorted({(c.weighting, c.min_gradient) for c in cases.CHAINS.values()}
                    | {("flat", 0.1), ("nearest", 0.0), ("angle", 0.0)})
ALL_BLENDS = cases.register_blends() + cases.general_blends()


def _common_h(name):
    text = open(os.path.join(ROOT, "scarlet_amd", "csrc", "common.h")).read()
    m = re.search(r"constexpr int %s\[kNumUpdateClasses\] = \{([^}]*)\};" % name, text)
    assert m, name
    return tuple(int(x) for x in m.group(1).split(","))


def test_the_restated_size_classes_are_those_of_common_h():
    """If this fails the classes have moved: revisit the table of update_class_cases.py (which
    boxes fill a class, which are the first of the next), then restate the numbers there."""
    text = open(os.path.join(ROOT, "scarlet_amd", "csrc", "common.h")).read()
    assert _common_h("kUpdateNpl") == cases.UPDATE_NPL
    assert _common_h("kUpdateTeam") == cases.UPDATE_TEAM
    assert re.search(r"constexpr int kMaxRegisterBox = 256 \* 59;", text)
    assert re.search(r"constexpr int kNumSmallClasses = 5;", text)
    assert cases.MAX_REGISTER_BOX == cases.UPDATE_NPL[-1] * cases.UPDATE_TEAM[-1]
    # (the slot layout's limit, csrc/batch.hip)
    assert "h * w <= %d" % cases.FAST_SLOT_PIXELS in open(
        os.path.join(ROOT, "scarlet_amd", "csrc", "batch.hip")).read()


def test_every_row_has_the_class_it_is_annotated_with():
    full = [n * t for n, t in zip(cases.UPDATE_NPL, cases.UPDATE_TEAM)]
    seen = {}
    for (h, w), n_pix, cls, _ in cases.BOXES:
        assert h * w == n_pix, (h, w)
        assert cases.update_class(n_pix) == cls, (h, w)
        assert h <= cases.H and w <= cases.W
        seen.setdefault(cls, []).append(n_pix)
    # every class and the general kernel; every class has the box that fills it exactly, and
    # every class but the first a box within 64 pixels (one slot per lane of a wavefront) of its
    # lower edge
    assert sorted(seen) == [cases.GENERAL] + list(range(9))
    for cls in range(9):
        assert full[cls] in seen[cls], cls
        if cls:
            assert min(seen[cls]) - full[cls - 1] <= 64, cls
    assert min(seen[cases.GENERAL]) - cases.MAX_REGISTER_BOX <= 64
    assert max(n for n in seen[cases.GENERAL] if n <= cases.FAST_SLOT_PIXELS) > 16000
    assert max(seen[cases.GENERAL]) > cases.FAST_SLOT_PIXELS
    # the overhanging copies: classes 0, 3, 5 and 7, top and left edge only, frame smaller than box
    over = [b for b in cases.register_blends() if b.name.endswith("_over")]
    assert sorted(b.cls for b in over) == [0, 3, 5, 7]
    for b in over:
        (h, w), (oy, ox), (fh, fw) = b.shape, b.origin, b.frame
        assert oy < 0 and ox < 0 and fh < h and fw < w and oy + h <= fh and ox + w <= fw
    assert len(cases.register_blends()) == 30 and len(cases.general_blends()) == 3
    assert len({b.name for b in ALL_BLENDS}) == len(ALL_BLENDS)


@pytest.mark.parametrize("weighting", ["angle", "flat", "nearest"])
def test_every_row_has_the_sweep_plan_it_is_annotated_with(weighting):
    """The library's own plan builder (csrc/sweep_plan.cpp) on the tables of every box, and the
    conditions under which the update kernels take a ring schedule (refresh_view in
    csrc/batch.hip, update_component in csrc/kernels.hip)."""
    import ring_model
    from oracle import proxops
    from scarlet_amd import operator

    for (h, w), n_pix, cls, plan in cases.BOXES:
        weights, offsets, didx = operator.monotonic_tables((h, w), weighting, (h // 2, w // 2))
        # the oracle's tables are the library's (so both sweep the same operator) ...
        ow, odidx, ooff = proxops.monotonic_operator((h, w), weighting, (h // 2, w // 2))
        assert_array_equal(ow, weights)
        assert_array_equal(odidx, didx)
        assert_array_equal(ooff, offsets)
        # ... of at most four terms per pixel: the slot layout exists for every box it has room for
        assert (weights > 0).sum(axis=0).max() <= 4
        ring = ring_model.ring_plan((h, w), weights, offsets, didx)
        one_plane_stream = ring is not None and ring["stream_bytes"] > 0 and ring["planes"] == 1
        if n_pix > cases.FAST_SLOT_PIXELS:
            want = cases.LEVEL_NO_SLOTS
        elif one_plane_stream and 0 <= cls < cases.NUM_SMALL_CLASSES:
            want = cases.RING_LATE if ring["n_nat"] < ring["n_pad"] else cases.RING
        else:
            want = cases.LEVEL
        assert plan == want, ((h, w), weighting, ring and {k: ring[k] for k in (
            "planes", "n_nat", "n_pad", "rmax", "stream_bytes")})
        # the boundaries named in the table
        if (h, w) == (47, 47):
            assert ring["rmax"] == 23 and ring["n_nat"] == ring["n_pad"]
        if (h, w) == (49, 49):
            assert ring["rmax"] == 24 and ring["n_nat"] < ring["n_pad"]
        if (h, w) == (63, 63):
            assert one_plane_stream and ring["rmax"] == 31
        if (h, w) == (65, 65):
            assert ring["planes"] == 2 and ring["rmax"] == 32


@pytest.mark.parametrize("blend", ALL_BLENDS, ids=lambda b: b.name)
def test_the_chain_has_work_to_do(blend):
    """A condition, not a measurement: the oracle's prox_monotonic changes at least 10 % of the
    pixels of the starting image under every weighting in use, positivity at least one -- no
    case passes because its chain had nothing to do.  (A box that does not meet it gets another
    noise seed in update_class_cases.SEEDS; the threshold stays.)"""
    from oracle import lite as olite
    from oracle import proxops

    x0 = cases.start_image(blend)
    assert x0.dtype == np.float32 and abs(x0.max() - 1) > 1e-3 and (x0 < 0).any()
    for weighting, g in WEIGHTINGS:
        swept = proxops.prox_monotonic(x0.copy(), 0, weighting, g)
        assert (swept != x0).mean() >= 0.10, (weighting, g, (swept != x0).mean())
        assert (proxops.prox_positivity(swept, 0, np.float32(0)) != swept).sum() >= 1
    swept = olite.monotonicity(x0.copy(), 1, "angle", 0.0)
    assert (swept != x0).mean() >= 0.10
    # the other links of the table's chains bite as well
    sed = cases.start_spectrum(blend)
    for name, chain in cases.CHAINS.items():
        got = cases.oracle_chain(x0, chain, sed)
        assert got.dtype == np.float32 and np.isfinite(got).all(), name
    base = cases.oracle_chain(x0, cases.CHAINS["no_norm"], sed)
    for name in ("symmetry_1", "symmetry_0.5", "l0_absolute", "l1_absolute"):
        assert (cases.oracle_chain(x0, cases.CHAINS[name], sed) != base).mean() >= 0.10, name
    lite = cases.oracle_chain(x0, cases.CHAINS["lite_bg_thresh"], sed)
    fit = cases.oracle_chain(x0, cases.CHAINS["no_norm_lite_fit_center"], sed)
    assert ((lite == 0) & (fit > 0)).sum() >= 1  # the background threshold removes positive pixels


@pytest.mark.parametrize("blend", ALL_BLENDS, ids=lambda b: b.name)
def test_the_scene_is_well_conditioned(blend):
    """A condition on the scene, taken from the oracle alone: its answer with float64 moments (the
    reference, what the device is compared with) and with float32 moments (what any float32 kernel
    holds) agree to a fifth of each bound of the device test -- 2e-6 after the first iteration,
    2e-5 after three, 2e-4 for v_morph -- so four fifths of a bound are left for the kernel's own
    rounding.  A starting image with a centre pixel below 0.5 fails it: the maximum normalisation
    then scales the outer pixels up in each of the ten sub-iterations, by 1 / 0.33 for the
    default seed of the 128^2 box, and the two oracle runs are 1.8e-4 apart after ONE iteration.
    (A box that does not meet it gets another noise seed in update_class_cases.SEEDS; the
    thresholds stay.)"""
    for case in cases.PGM_KEYWORDS:
        a = cases.oracle_steps(blend, case)
        b = cases.oracle_steps(blend, case, state_dtype=np.float32)
        assert np.abs(a["first"][1] - b["first"][1]).max() < 2e-6, case
        assert np.abs(a["last"][1] - b["last"][1]).max() < 2e-5, case
        assert np.abs(a["last"][2] - b["last"][2]).max() < 2e-4 * np.abs(a["last"][2]).max(), case


def test_some_fitted_centres_are_not_the_box_centre():
    """The fit-centre chains take one of nine plans per box: the table must reach others than
    the middle one."""
    from oracle import lite as olite

    moved = 0
    for blend in ALL_BLENDS:
        x0 = cases.start_image(blend)
        h, w = blend.shape
        moved += olite.get_center(x0, (h // 2, w // 2), 1) != (h // 2, w // 2)
    assert moved >= len(ALL_BLENDS) // 3, moved


@pytest.mark.parametrize("blend", ALL_BLENDS, ids=lambda b: b.name)
def test_reciprocal_normalisation_is_within_one_ulp_of_the_division(blend):
    """u * (1 / max) with the maximum set to 1 -- what the kernels compute -- against the oracle's
    u / max: at most one float32 ulp apart, pixel by pixel (both correctly rounded, the reciprocal
    product within 1.5 ulp of the quotient), exactly 1 at the maximum, nothing negative."""
    from oracle import proxops

    chain = cases.CHAINS["norm_max"]
    u = cases.oracle_chain(cases.start_image(blend), chain, upto_norm=True)
    got = cases.reciprocal_max_normalisation(u)
    ref = proxops.prox_normalization(u.copy(), 0, "max")
    assert ref.dtype == np.float32
    assert cases.ulp_distance(got, ref).max() <= 1
    assert got.max() == 1.0 and got.min() >= 0.0
    assert (got != ref).any() or u.size < 500  # (the relation is not vacuous on the larger boxes)
