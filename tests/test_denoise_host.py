"""``wavelet.plan_wavelet_denoising_batch`` and the denoising oracle, without a GPU: the groups,
the images that go one by one with their reasons, the launch count as a function of the largest
scale count and ``max_iter`` alone, the share of cases that pass the rounding-margin test, and
the oracle against the reference's own denoisings."""

import os

import numpy as np
import pytest

import denoise_cases as dc
import denoise_oracle
from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "interpolate_observation.npz"))


def formula(scales, max_iter):
    """csrc/denoise_batch.hip, header comment"""
    return (1 + 4 * scales) + 2 + (2 * scales + max_iter * max(6 * scales, 1))


def test_launch_count_is_the_documented_formula():
    from scarlet_amd import wavelet

    for scales in (0, 1, 3, 6, 30):
        for max_iter in (1, 2, 20):
            assert wavelet.denoise_launches(scales, max_iter) == formula(scales, max_iter)
    assert wavelet.denoise_launches(4, 20, wavelet.DENOISE_TRANSFORM) == 17
    assert wavelet.denoise_launches(4, 20, wavelet.DENOISE_SUPPORT) == 2
    assert wavelet.denoise_launches(4, 20, wavelet.DENOISE_ITERATE) == 8 + 20 * 24
    assert wavelet.denoise_launches(0, 3, wavelet.DENOISE_ITERATE) == 3


def test_plan_groups_by_dtype_and_names_the_images_that_go_one_by_one():
    from scarlet_amd import wavelet

    images = dc.ragged_list() + [np.ones((8, 9), np.int16), np.ones((1, 5)), np.ones((3, 4, 4))]
    groups, one_by_one = wavelet.plan_wavelet_denoising_batch(images, max_iter=20)
    n = len(dc.ragged_list())
    beyond = [i for i, im in enumerate(images[:n]) if im.shape == dc.BEYOND_SHAPE]
    assert one_by_one == [(beyond[0], "more than 65536 pixels"),
                          (n + 1, "fewer than 2 pixels along an axis"),
                          (n + 2, "not a 2-D image")]
    assert [g["dtype"] for g in groups] == [np.dtype(np.float64), np.dtype(np.float32)]
    f64 = [i for i in range(n) if images[i].dtype == np.float64 and i != beyond[0]] + [n]
    f32 = [i for i in range(n) if images[i].dtype == np.float32 and i != beyond[0]]
    assert groups[0]["images"] == f64 and groups[1]["images"] == f32  # int16 -> float64
    for g in groups:
        top = max(denoise_oracle.scales_of(images[i].shape) for i in g["images"])
        assert g["scales"] == top and g["launches"] == formula(top, 20)
    assert wavelet.plan_wavelet_denoising_batch([]) == ([], [])


def test_plan_is_the_same_for_1_and_for_50_images():
    from scarlet_amd import wavelet

    image = dc.make_image((64, 48), np.float32, 3)
    for max_iter in (1, 20):
        (one,), _ = wavelet.plan_wavelet_denoising_batch([image], max_iter)
        (fifty,), _ = wavelet.plan_wavelet_denoising_batch([image] * 50, max_iter)
        assert fifty["images"] == list(range(50))
        assert one["launches"] == fifty["launches"] == formula(4, max_iter)
        assert one["scales"] == fifty["scales"] == 4
    # smaller images beside it change nothing either
    small = dc.make_image((5, 7), np.float32, 4)
    (mixed,), _ = wavelet.plan_wavelet_denoising_batch([small, image, small], 20)
    assert mixed["launches"] == formula(4, 20)


def test_plan_cuts_groups_at_the_limits_and_takes_max_iter_below_1_out():
    from scarlet_amd import wavelet

    images = [dc.make_image((16, 16), np.float32, k) for k in range(5)]
    groups, _ = wavelet.plan_wavelet_denoising_batch(images, _max_tasks=2)
    assert [g["images"] for g in groups] == [[0, 1], [2, 3], [4]]
    # per pixel: the float32 image, 4 planes of float64 + int32 + float64, x and work
    need = 16 * 16 * (4 + 4 * 20 + 16)
    groups, _ = wavelet.plan_wavelet_denoising_batch(images, _max_bytes=3 * need)
    assert [g["images"] for g in groups] == [[0, 1, 2], [3, 4]]
    for max_iter in (0, -1):
        groups, one_by_one = wavelet.plan_wavelet_denoising_batch(images, max_iter)
        assert groups == [] and one_by_one == [(k, "max_iter < 1") for k in range(5)]


def test_space_images_and_wrong_sigma_lists_are_refused_before_any_device_call():
    from scarlet_amd import wavelet

    image = dc.make_image((8, 8), np.float64, 1)
    with pytest.raises(NotImplementedError):
        wavelet.apply_wavelet_denoising(image, image_type="space")
    with pytest.raises(NotImplementedError):
        wavelet.apply_wavelet_denoising_batch([image], image_type="space")
    with pytest.raises(ValueError):
        wavelet.apply_wavelet_denoising_batch([image, image], sigma=[1.0, 2.0, 3.0])
    assert wavelet.apply_wavelet_denoising_batch([]) == []


def test_cases_cover_the_issue_and_most_pass_the_rounding_margin():
    shapes = {c.image.shape for c in dc.CASES}
    assert shapes >= set(dc.SMALL_SHAPES) | {dc.LIMIT_SHAPE, dc.BEYOND_SHAPE}
    assert dc.LIMIT_SHAPE[0] * dc.LIMIT_SHAPE[1] == 65536
    assert {c.image.dtype for c in dc.CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {(c.sigma is None, c.positive, c.max_iter, c.k) for c in dc.CASES} >= {
        (s, p, i, k) for s in (True, False) for p in (True, False) for i in (1, 2, 20)
        for k in (1, 3)}
    exact = dc.exact_cases()
    print("cases %d, of which %d pass the rounding margin" % (len(dc.CASES), len(exact)))
    assert 4 * len(exact) >= 3 * len(dc.CASES)
    names = {c.name for c in exact}
    assert "zeros" in names and "limit_float32" in names and "beyond_float64" in names


def test_oracle_equals_the_reference_denoisings(golden):
    """within 1e-12 of the largest value, the tolerance tests/test_gpu_wavelet.py has for the
    same quantity"""
    for tag in ("a", "b"):
        image, ref = golden["denoise_img_" + tag], golden["denoise_" + tag]
        x = denoise_oracle.denoise(image)
        assert x.shape == ref.shape and x.dtype == np.float64
        err = np.abs(x - ref).max()
        print(tag, image.shape, image.dtype, "max error", err, "of", np.abs(ref).max())
        assert err <= 1e-12 * np.abs(ref).max()
    detect = np.load(os.path.join(ROOT, "tests", "golden", "detect.npz"))
    x = denoise_oracle.denoise(detect["denoise_img"])
    assert np.abs(x - detect["denoise"]).max() <= 1e-12 * np.abs(detect["denoise"]).max()
