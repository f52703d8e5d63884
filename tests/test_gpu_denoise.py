"""``wavelet.apply_wavelet_denoising`` and ``apply_wavelet_denoising_batch``
(csrc/denoise_batch.hip): every image of a ragged list equals its own call, the call equals the
loop over the public functions it replaces, and both equal the CPU restatement
tests/denoise_oracle.py bit for bit where ``wavelet_oracle.rounding_margin_ok`` holds.  The
cases are those of tests/denoise_cases.py."""

import os

import numpy as np
import pytest

import denoise_cases as dc
from conftest import ROOT
from wavelet_oracle import same_bits

pytestmark = pytest.mark.gpu

_singles = {}


def host(result):
    return result.cpu().numpy() if hasattr(result, "cpu") else result


def single(image, **options):
    """``apply_wavelet_denoising`` of one image, computed once per image and options"""
    from scarlet_amd import wavelet

    key = (id(image), tuple(sorted(options.items())))
    if key not in _singles:  # (the image is kept, so that its id stays its own)
        x = wavelet.apply_wavelet_denoising(image, **options)
        x.setflags(write=False)
        _singles[key] = (image, x)
    return _singles[key][1]


def replaced_loop(image, sigma=None, k=3, epsilon=1e-1, max_iter=20, positive=True):
    """the loop ``apply_wavelet_denoising`` was, written out with the public functions"""
    from scarlet_amd import wavelet

    image_coeffs = wavelet.starlet_transform(image)
    if sigma is None:
        sigma = np.median(np.absolute(image - np.median(image)))
    support = wavelet.get_multiresolution_support(image, image_coeffs.copy(), sigma, k, epsilon,
                                                  max_iter, "ground")
    x = wavelet.starlet_reconstruction(image_coeffs)
    for _ in range(max_iter):
        coeffs = wavelet.starlet_transform(x)
        x = x + wavelet.starlet_reconstruction(support * (image_coeffs - coeffs))
        if positive:
            x[x < 0] = 0
    return x


IMAGES = dc.ragged_list()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_image_of_a_ragged_list_equals_its_own_call(device):
    """float32 and float64 mixed, zero to six scales, the image beyond the batch limit in the
    middle; then the same images in another order"""
    from scarlet_amd import wavelet

    got = wavelet.apply_wavelet_denoising_batch(IMAGES, device=device)
    assert len(got) == len(IMAGES)
    for g, im in zip(got, IMAGES):
        g = host(g)
        assert g.dtype == np.float64 and g.shape == im.shape
        assert same_bits(g, single(im)) and np.array_equal(g, single(im)), im.shape
    order = [5, 0, 7, 3, 1, 6, 2, 4]
    got = wavelet.apply_wavelet_denoising_batch([IMAGES[i] for i in order], device=device)
    for g, i in zip(got, order):
        assert same_bits(host(g), single(IMAGES[i])), IMAGES[i].shape


def test_options_reach_every_image_and_sigma_may_be_a_list():
    from scarlet_amd import wavelet

    images = IMAGES[:3] + IMAGES[4:7]
    sigmas = [0.3 + 0.1 * n for n in range(len(images))]
    got = wavelet.apply_wavelet_denoising_batch(images, sigma=sigmas, k=1, max_iter=2,
                                                positive=False)
    for g, im, s in zip(got, images, sigmas):
        assert same_bits(g, single(im, sigma=s, k=1, max_iter=2, positive=False)), im.shape
    got = wavelet.apply_wavelet_denoising_batch(images, sigma=0.4, epsilon=0.5)
    for g, im in zip(got, images):
        assert same_bits(g, single(im, sigma=0.4, epsilon=0.5)), im.shape


def test_device_tensors_and_other_dtypes_are_accepted():
    import torch
    from scarlet_amd import wavelet

    ints = np.arange(48, dtype=np.int16).reshape(6, 8) % 7
    images = [torch.from_numpy(IMAGES[4]).to("cuda"), ints, torch.from_numpy(IMAGES[5]).to("cuda")]
    got = wavelet.apply_wavelet_denoising_batch(images)
    assert same_bits(got[0], single(IMAGES[4])) and same_bits(got[2], single(IMAGES[5]))
    assert same_bits(got[1], wavelet.apply_wavelet_denoising(ints.astype(np.float64)))
    # sigma and its first rounding are those of the image as given, as in the loop replaced
    assert same_bits(got[1], replaced_loop(ints))
    assert same_bits(wavelet.apply_wavelet_denoising(ints, sigma=1.3), replaced_loop(ints, 1.3))
    halves = IMAGES[4].astype(np.float16)
    assert same_bits(wavelet.apply_wavelet_denoising(halves), replaced_loop(halves))
    assert same_bits(wavelet.apply_wavelet_denoising_batch([halves, ints], sigma=0.7)[0],
                     replaced_loop(halves, 0.7))


@pytest.mark.parametrize("case", dc.CASES, ids=[c.name for c in dc.CASES])
def test_call_equals_the_loop_it_replaces_and_the_oracle(case):
    from scarlet_amd import wavelet

    options = dict(sigma=case.sigma, k=case.k, max_iter=case.max_iter, positive=case.positive)
    got = wavelet.apply_wavelet_denoising(case.image, **options)
    assert got.dtype == np.float64 and got.shape == case.image.shape
    loop = replaced_loop(case.image, **options)
    assert np.array_equal(got, loop, equal_nan=True) and same_bits(got, loop)
    if np.isfinite(case.image).all():
        assert np.array_equal(got, loop)
    if dc.margin_ok(case):
        assert same_bits(got, dc.oracle_result(case))
    if case.positive and np.isfinite(case.image).all():
        assert (got >= 0).all()


def test_cases_in_one_batch_equal_the_oracle():
    """the default-option cases of every shape as one ragged list"""
    from scarlet_amd import wavelet

    cases = [c for c in dc.exact_cases()
             if (c.sigma, c.k, c.positive, c.max_iter) == (None, 3, True, 20)]
    assert len(cases) >= 2 * len(dc.SMALL_SHAPES)
    got = wavelet.apply_wavelet_denoising_batch([c.image for c in cases])
    for g, c in zip(got, cases):
        assert same_bits(g, dc.oracle_result(c)), c.name


def test_max_iter_below_one_keeps_the_per_image_behaviour():
    """the loop over the public functions refuses ``max_iter=0`` in the support; so does this"""
    from scarlet_amd import _lib, wavelet

    with pytest.raises(_lib.ScarletAmdError):
        replaced_loop(IMAGES[4], max_iter=0)
    with pytest.raises(_lib.ScarletAmdError):
        wavelet.apply_wavelet_denoising(IMAGES[4], max_iter=0)


def test_goldens_hold():
    """the reference's denoisings, within 1e-12 of the largest value"""
    from scarlet_amd import wavelet

    g = np.load(os.path.join(ROOT, "tests", "golden", "detect.npz"))
    den = wavelet.apply_wavelet_denoising(g["denoise_img"])
    assert np.abs(den - g["denoise"]).max() <= 1e-12 * np.abs(g["denoise"]).max()
    g = np.load(os.path.join(ROOT, "tests", "golden", "interpolate_observation.npz"))
    images = [g["denoise_img_a"], g["denoise_img_b"]]
    for den, tag in zip(wavelet.apply_wavelet_denoising_batch(images), "ab"):
        ref = g["denoise_" + tag]
        assert np.abs(den - ref).max() <= 1e-12 * np.abs(ref).max()
