"""What ``fit_blends`` decides for blends with low-resolution observations, without a device:
groups, keys, reasons, operator bytes, cuts, and the slicing of the batched transforms."""

import ctypes

import numpy as np
import pytest

import multires_batch_cases as mc
import scarlet_amd.fitting as fitting
from scarlet_amd import _lib
from scarlet_amd.fitting import plan_fit_blends


def test_five_of_a_class_share_a_group_and_other_classes_have_their_own():
    groups, alone = plan_fit_blends(mc.LISTS["first"](), 25, e_rel=1e-4)
    assert alone == {}
    assert [idx for _, idx in groups] == [[0, 1, 2, 3, 4]]
    key = groups[0][0]
    assert key[0] == 3 and key[3:] == ((40, 44), ((2, 11, 11, 54, 60),), 1)

    groups, alone = plan_fit_blends(mc.LISTS["classes"](), 25, e_rel=1e-4)
    assert alone == {}
    assert [idx for _, idx in groups] == [[0, 2, 4, 6, 8], [1], [3], [5], [7]]
    assert [key[3:] for key, _ in groups] == [
        ((40, 44), ((2, 11, 11, 54, 60),), 1),
        ((36, 36), ((1, 9, 9, 48, 48),), 1),
        ((50, 46), ((3, 14, 14, 64, 60),), 1),
        ((34, 130), ((2, 10, 10, 48, 144),), 1),
        ((44, 48), ((1, 11, 11, 60, 60), (1, 8, 8, 60, 60)), 2)]


def test_single_resolution_and_psf_shift_blends_keep_their_places():
    groups, alone = plan_fit_blends(mc.LISTS["single"](), 25, e_rel=1e-4)
    assert alone == {}
    assert [idx for _, idx in groups] == [[0, 2, 3, 4, 5], [1]]
    assert len(groups[1][0]) == 3  # the key of a blend without such observations is the old one
    groups, alone = plan_fit_blends(mc.LISTS["psf_shift"](), 25, e_rel=1e-4)
    assert alone == {1: "free renderer parameters (psf_shift)"}
    assert [idx for _, idx in groups] == [[0, 2, 3, 4, 5]]


def test_reasons_for_being_fitted_alone_are_specific():
    dense = mc.make_blend("first", 7)
    dense.observations[1].renderer._dense = True  # what device_path(0) leaves behind
    assert not dense.observations[1].renderer.on_spectral_path()
    # a second high-resolution observation of the same channel: a further cube
    twice = mc.make_blend("first", 8)
    hr = twice.observations[0]
    import scarlet_amd as scarlet

    again = scarlet.Observation(hr.data.copy(), wcs=hr.wcs, psf=hr.psf, channels=["hr"],
                                weights=hr.weights.copy()).match(twice.frame)
    twice.observations = tuple(twice.observations) + (again,)
    groups, alone = plan_fit_blends([dense, mc.make_blend("first", 9), twice], 25)
    assert alone == {0: "a low-resolution observation on the dense path",
                     2: "several observations of one channel"}
    assert [idx for _, idx in groups] == [[1]]
    assert "several terms in its loss" not in alone.values()


def test_operator_bytes_and_cuts(monkeypatch):
    blends = mc.LISTS["classes"]()
    groups, _, nbytes = plan_fit_blends(blends, 25, details=True)
    each = 2 * 11 * 54 * 31 * 8  # C n_a Fy Kx complex float32
    assert nbytes == [5 * each, 1 * 9 * 48 * 25 * 8, 3 * 14 * 64 * 31 * 8, 2 * 10 * 48 * 73 * 8,
                      (11 + 8) * 60 * 31 * 8]
    for blend in blends:
        for obs in blend.observations[1:]:
            C, n_a, n_b, Fy, Fx = obs.renderer.shape_class()
            assert obs.renderer.operator_bytes() == C * n_a * Fy * (Fx // 2 + 1) * 8
    # a cap of two members and a half: 2 + 2 + 1, every part a batch under the same key
    monkeypatch.setattr(fitting, "LOWRES_OPERATOR_CAP", 2 * each + each // 2)
    cut, alone, nbytes = plan_fit_blends(blends, 25, details=True)
    assert alone == {}
    assert [idx for _, idx in cut] == [[0, 2], [4, 6], [8], [1], [3], [5], [7]]
    assert cut[0][0] == cut[1][0] == cut[2][0] == groups[0][0]
    assert nbytes[:3] == [2 * each, 2 * each, each]
    # a member beyond the cap is a batch of its own
    monkeypatch.setattr(fitting, "LOWRES_OPERATOR_CAP", 1)
    cut, _ = plan_fit_blends(blends, 25)
    assert [idx for _, idx in cut] == [[0], [2], [4], [6], [8], [1], [3], [5], [7]]
    assert fitting._cut_by_bytes([], 10) == []
    assert fitting._cut_by_bytes([4, 4, 4, 11, 1, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]


def test_key_does_not_merge_frames_or_classes():
    base = mc.make_blend("first", 11)
    run = fitting._classify(base)[1]
    key = fitting._group_key(run)
    other = fitting._group_key(fitting._classify(mc.make_blend("first", 12, offset=(0.3, 0.1)))[1])
    assert key == other  # offsets, data and components do not enter
    seen = {key}
    for kind in ("small", "three", "wide", "double"):
        k = fitting._group_key(fitting._classify(mc.make_blend(kind, 13))[1])
        assert k not in seen
        seen.add(k)
    # same frame and convolution, another class / another number of observations
    frame, (cls,), count = key[3:]
    for changed in ((frame, (cls[:1] + (12,) + cls[2:],), count), ((41, 44), (cls,), count),
                    (frame, (cls, cls), 2)):
        assert key[:3] + changed != key
    single = fitting._group_key(fitting._classify(mc.make_blend("first", 14, single=True))[1])
    assert len(single) == 3 and single not in seen


@pytest.mark.parametrize("adjoint", [0, 1])
def test_batched_transform_keeps_the_slices_of_the_single_resampler(adjoint):
    lib = _lib.load()
    names = ("tm", "tn", "bk", "kslice", "n_slices")
    shapes = {(bands, fy, fx) for _, lows, _, ffts in mc.CLASSES.values()
              for (bands, _, _), (fy, fx) in zip(lows, ffts)}
    # (and rows long enough for two and three slices; 700 x 3 bands x 40 000 members is cut)
    for C, Fy, Fx in sorted(shapes) + [(5, 150, 322), (3, 90, 700)]:
        Kx = Fx // 2 + 1
        N, K = (Fx, 2 * Kx) if adjoint else (2 * Kx, Fx)
        slices = max(Fx, 2 * Kx)
        scratch = C * Fy * slices * ((slices + 319) // 320 + 1)  # the resampler's own scratch
        single = (ctypes.c_int32 * 5)()
        assert lib.smi_gemm_plan(Fy, N, K, C, scratch, single) == 0
        single = dict(zip(names, single))
        for n in (1, 2, 7, 256, 40000):
            own, pooled = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 5)()
            _lib.check(lib.smi_lowres_gemm_plans_test(C, Fy, Fx, n, adjoint, own, pooled))
            own, pooled = dict(zip(names, own)), dict(zip(names, pooled))
            assert own == single
            assert (pooled["kslice"], pooled["n_slices"]) == (single["kslice"], single["n_slices"])
            assert pooled["n_slices"] == -(-K // pooled["kslice"])
            if n == 1:
                assert pooled == single  # the batch of one is the single launch
        assert single["n_slices"] == -(-K // 320) or Fx < 320
