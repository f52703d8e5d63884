"""Starlet transform, reconstruction, multiresolution support and detection on the GPU
against the reference's run (tests/golden/detect.npz) and a float64 NumPy restatement."""

import numpy as np
import pytest

from conftest import golden
from wavelet_oracle import bspline as np_bspline, transform as np_transform

pytestmark = pytest.mark.gpu


def unpack(bits, shape):
    return np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)


@pytest.fixture(scope="module")
def g():
    return golden("detect")


def test_transform_and_reconstruction_bit_equal_to_the_reference(g):
    from scarlet_amd import wavelet

    for tag in "ab":
        img = g["img_" + tag]
        for gen in (1, 2):
            for scales in (None, 0, 1, 3, 5):
                key = "%s_g%d_s%s" % (tag, gen, "N" if scales is None else scales)
                w = wavelet.starlet_transform(img, scales=scales, generation=gen)
                assert w.dtype == np.float64 and w.shape == g["w_" + key].shape, key
                assert np.array_equal(w, g["w_" + key]), key
                rec = wavelet.starlet_reconstruction(g["w_" + key], generation=gen)
                assert np.array_equal(rec, g["rec_" + key]), key
            st = wavelet.Starlet.from_image(img, generation=gen)
            assert np.array_equal(st.norm, g["norm_%s_g%d" % (tag, gen)])
            assert st.scales == wavelet.get_scales(img.shape)
            back = wavelet.Starlet.from_coefficients(st.coefficients, generation=gen)
            assert np.array_equal(back.image, g["rec_%s_g%d_sN" % (tag, gen)])


def test_batch_equals_one_by_one(g):
    from scarlet_amd import wavelet

    rng = np.random.default_rng(3)
    cube = rng.normal(size=(6, 45, 70)).astype(np.float32)
    for gen in (1, 2):
        batch = wavelet.transform_device(wavelet._upload(cube), 4, gen).cpu().numpy()
        for b in range(len(cube)):
            assert np.array_equal(batch[:, b], wavelet.starlet_transform(cube[b], 4, gen))
        multi = wavelet.multiband_starlet_transform(cube.astype(np.float64), 4, gen)
        assert np.array_equal(multi, batch)
        rec = wavelet.multiband_starlet_reconstruction(multi, gen)
        for b in range(len(cube)):
            assert np.array_equal(rec[b], wavelet.starlet_reconstruction(multi[:, b], gen))


@pytest.mark.parametrize("shape", [(1024, 768), (2049, 4096), (4096, 4096)])
def test_large_frames_at_maximum_scales(shape):
    """dilations up to 1024 rows / columns, bit-equal to the NumPy restatement"""
    from scarlet_amd import wavelet

    rng = np.random.default_rng(sum(shape))
    img = rng.normal(size=shape).astype(np.float32)
    scales = wavelet.get_scales(shape)
    w = wavelet.starlet_transform(img, generation=2)
    assert w.shape == (scales + 1,) + shape
    assert np.array_equal(w, np_transform(img, scales, 2))
    rec = wavelet.starlet_reconstruction(w)
    c = w[-1]
    for j in range(scales - 1, -1, -1):
        c = np_bspline(c, j) + w[j]
    assert np.array_equal(rec, c)
    if shape == (1024, 768):
        assert np.array_equal(wavelet.starlet_transform(img, generation=1),
                              np_transform(img, scales, 1))


def test_support_detection_and_denoising(g):
    from scarlet_amd import detect, wavelet

    hsc = golden("hsc_cosmos_35")
    images = hsc["images"].astype(np.float32)
    variance = (1 / hsc["weights"].astype(np.float32)).astype(np.float32)
    band = images[2]
    coeffs = wavelet.starlet_transform(band, scales=3)
    sigma = np.median(np.sqrt(variance[2]))
    M = wavelet.get_multiresolution_support(band, coeffs, sigma)
    assert M.dtype == np.int64
    assert np.array_equal(M.astype(bool), unpack(g["support_hsc2_s3"], coeffs.shape))
    for scales in (3, 5):
        det = detect.get_detect_wavelets(images, variance, scales=scales)
        shape = tuple(g["detect_shape_s%d" % scales])
        assert det.shape == shape
        mask = unpack(g["detect_mask_s%d" % scales], shape)
        assert np.array_equal(det != 0, mask)
        ref = np_transform(images.sum(axis=0), shape[0] - 1) * mask
        assert np.abs(det - ref).max() <= 1e-12 * np.abs(ref).max()
        if scales == 3:
            assert np.array_equal(det, g["detect_s3"])
        wav = detect.get_wavelets(images, variance, scales=scales)
        shape = tuple(g["wavelets_shape_s%d" % scales])
        assert wav.shape == shape
        mask = unpack(g["wavelets_mask_s%d" % scales], shape)
        assert np.array_equal(wav != 0, mask)
        ref = np.stack([np_transform(b, shape[1] - 1) for b in images]) * mask
        assert np.abs(wav - ref).max() <= 1e-12 * np.abs(ref).max()
    den = wavelet.apply_wavelet_denoising(g["denoise_img"])
    assert np.abs(den - g["denoise"]).max() <= 1e-12 * np.abs(g["denoise"]).max()


def test_peaks_equal_the_reference(g):
    """get_peaks of the multi-scale tutorial (detect * ~mask) and the lite tutorial's chain"""
    from scarlet_amd import Box, detect

    timages = g["timages"]
    n = timages.size
    tvar = np.where(np.arange(n) < n // 2, g["tvar_lo"], g["tvar_hi"]).astype(np.float32)
    tvar = tvar.reshape(timages.shape)
    tmask = unpack(g["tmask"], timages.shape[1:])
    tdetect = detect.get_detect_wavelets(timages, tvar, scales=5)
    peaks = detect.get_peaks(tdetect * ~tmask[None])
    assert peaks == [tuple(v) for v in g["tutorial_peaks"].tolist()]
    hsc = golden("hsc_cosmos_35")
    images = hsc["images"].astype(np.float32)
    variance = (1 / hsc["weights"].astype(np.float32)).astype(np.float32)
    det = detect.get_detect_wavelets(images, variance, scales=3)
    structures, middle = detect.get_blend_structures(det)
    assert len(structures) == int(g["n_structures"])
    centers = [(p.y, p.x) for box in middle.query(Box(images.shape)[1:])
               for p in box.footprint.peaks]
    assert centers == [tuple(v) for v in g["lite_centers"].tolist()]
    assert detect.get_peaks(images=images, variance=variance, bbox=Box(images.shape)) == centers


def test_reference_wavelet_cases_restated():
    """the reference's tests/test_wavelet.py: transform / inverse of a Gaussian PSF, and the
    coefficients setter path (from_coefficients after zeroing rows far from the source)"""
    import scarlet_amd as scarlet
    from numpy.testing import assert_almost_equal, assert_equal

    psf = scarlet.GaussianPSF(1, boxsize=128).get_model()[0]
    st = scarlet.Starlet.from_image(psf, scales=3)
    assert_equal(st.coefficients.shape[0], 4)
    assert_almost_equal(st.image, psf)
    assert_almost_equal(scarlet.wavelet.starlet_reconstruction(st.coefficients), psf)
    coeffs = st.coefficients
    coeffs[:, 10:20, :] = 0
    again = scarlet.Starlet.from_coefficients(coeffs)
    assert_almost_equal(again.image, st.image)
    coeffs[:, :, :] = 0
    assert_almost_equal(st.image, psf)
    assert scarlet.wavelet.get_scales((32, 32)) == 4
    assert scarlet.wavelet.get_scales((32, 32), 2) == 2
    assert scarlet.wavelet.get_scales((100, 20), 10) == 3


def test_divergences_from_the_reference():
    from scarlet_amd import wavelet

    rng = np.random.default_rng(1)
    img = rng.normal(size=(40, 36))
    st = wavelet.Starlet.from_image(img, scales=2)
    # setters keep the number of scales (the reference passes `generation` as `scales`)
    st.generation = 1
    assert st.scales == 2
    assert np.array_equal(st.coefficients, wavelet.starlet_transform(img, 2, 1))
    st.image = img * 2
    assert st.scales == 2
    assert np.array_equal(st.coefficients, wavelet.starlet_transform(img * 2, 2, 1))
    st.convolve2D = wavelet.bspline_convolve  # a user's filter: the host loop, same numbers
    assert st.scales == 2
    assert np.array_equal(st.coefficients, wavelet.starlet_transform(img * 2, 2, 1))
    # multiband_starlet_reconstruction inverts multiband_starlet_transform
    cube = rng.normal(size=(3, 40, 36))
    w = wavelet.multiband_starlet_transform(cube, scales=3)
    assert np.allclose(wavelet.multiband_starlet_reconstruction(w), cube, atol=1e-12)
    with pytest.raises(NotImplementedError, match="shape tuple"):
        wavelet.get_multiresolution_support(img, wavelet.starlet_transform(img), 1.0,
                                            image_type="space")
