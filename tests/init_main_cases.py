"""Small scenes for the tests of ``lite.init_blends_main``, shared by the host and the GPU
tests, in the style of tests/init_cases.py (whose helpers they use).

A case is an observation, centres, a detection image (None: the coadd of the images, which
with variance 1 is their sum over the bands), the options of the call and the class every
centre is meant to take (``kinds``: "psf", "one", "two"; tests/test_lite_init_main_host.py
asserts that the oracle agrees, so a case exercises what its name says).  Images are blobs on
the centres whose levels put the PSF-weighted SNR well inside a class for ``min_snr = 10``:
below 2 ``min_snr`` one component, above it bulge and disk.  A source is PSF-shaped when
nothing of its swept image is above ``thresh * mean(noise_rms) = 0.5``: a centre on empty sky.

The frames: 9 x 11 has fewer pixels than a workgroup has threads, and every (at least
21 x 21) box leaves it on all sides; 10 x 12 and 32 x 36 have even extents, where the centred
sub-array of the symmetry operator is one row and column shorter; 33 x 37 needs a sweep of
more than one wavefront per level."""

from types import SimpleNamespace

import numpy as np

from init_cases import _observation, _stamp, gauss, same_bits  # noqa: F401

MIN_SNR = 10
ONE_LEVEL, TWO_LEVEL = 14.0, 100.0  # SNR of a source alone, per class


def _build(name, frame, C, stamp, sources, dtype=np.float32, psf=(5, 5), options=None,
           paint=None, detect=None, seed=0):
    """``sources``: ``(centre, kind, level, sigma)``, a level of None leaves the sky empty.
    ``paint(images)`` edits the images afterwards; ``detect(images)`` returns the detection
    image to pass (in the images' type)."""
    rng = np.random.RandomState(seed + sum(map(ord, name)))
    H, W = frame
    images = np.zeros((C, H, W))
    colour = 1 + 0.1 * np.arange(C)
    ph, pw = psf
    psfs = np.stack([gauss(psf, (ph // 2, pw // 2), 1.0 + 0.05 * c) for c in range(C)])
    psfs /= psfs.sum(axis=(1, 2))[:, None, None]
    for center, _, level, sigma in sources:
        if level is None:
            continue
        blob = colour[:, None, None] * (0.7 * gauss(frame, center, 1.5)
                                        + 0.3 * gauss(frame, center, sigma))[None]
        # the SNR of the blob alone, PSF stamp clipped by the frame (variance 1)
        y0, x0 = center[0] - ph // 2, center[1] - pw // 2
        ys, xs = slice(max(y0, 0), y0 + ph), slice(max(x0, 0), x0 + pw)
        cut = psfs[:, ys.start - y0:min(y0 + ph, H) - y0, xs.start - x0:min(x0 + pw, W) - x0]
        images += level / (np.sum(blob[:, ys, xs] * cut) / np.sqrt(np.sum(psfs ** 2))) * blob
    images += rng.normal(0, 0.01, images.shape)
    if paint is not None:
        paint(images)
    model_psf = gauss((7, 7), (3, 3), 0.8)
    model_psf /= model_psf.sum()
    obs = _observation(images.astype(dtype), psfs, _stamp(rng, *stamp), model_psf)
    opts = dict(min_snr=MIN_SNR)
    opts.update(options or {})
    return SimpleNamespace(name=name, obs=obs, centers=[s[0] for s in sources],
                           detect=None if detect is None else detect(images).astype(dtype),
                           options=opts, kinds=[s[1] for s in sources])


def _plateau(images):
    """A 3 x 3 plateau of exactly equal values on (16, 18): the sweep meets ties."""
    images[:, 15:18, 17:20] = images[:, 15:18, 17:20].max(axis=(1, 2))[:, None, None]


def _moat(images):
    """A ring of exact zeros at Chebyshev distance 4 of (16, 18), light beyond it."""
    y, x = np.mgrid[:images.shape[1], :images.shape[2]]
    images += 0.6
    images[:, np.maximum(np.abs(y - 16), np.abs(x - 18)) == 4] = 0.0


def _negative_centre(images):
    """The first band is negative on the centre pixel: its spectrum is clipped to 0."""
    images[0, 16, 18] = -1.0


def _smooth_detect(images):
    """A detection image that is not the coadd: the blob of (16, 18) alone, without noise."""
    return 30.0 * gauss(images.shape[1:], (16, 18), 2.0) + 2.0 * gauss(images.shape[1:], (16, 18), 6.0)


def _hollow(images):
    """Images that hold the wide part of the detection image and MINUS its core: the joint fit
    clips the bulge away."""
    shape = images.shape[1:]
    images[:] = (8.0 * gauss(shape, (16, 18), 6.0) - 1.5 * gauss(shape, (16, 18), 1.2))[None]


CASES = {
    # two corners (the centred sub-array is one pixel), an edge; every box leaves the frame
    "9x11-classes": lambda: _build(
        "9x11-classes", (9, 11), 2, (2, 3, 3),
        [((0, 0), "one", 9.0, 2.5), ((4, 10), "one", 9.0, 2.5), ((5, 4), "two", 60.0, 3.0),
         ((8, 0), "one", None, None)], psf=(3, 3)),  # (the blobs overlap: lower levels)
    # nothing but noise: PSF sources in a frame smaller than their boxes
    "9x11-dark": lambda: _build(
        "9x11-dark", (9, 11), 2, (2, 3, 3),
        [((4, 5), "psf", None, None), ((0, 10), "psf", None, None)], psf=(3, 3)),
    "9x11-f64": lambda: _build(
        "9x11-f64", (9, 11), 2, (1, 3, 3),
        [((8, 10), "two", TWO_LEVEL, 3.0), ((2, 3), "one", ONE_LEVEL, 2.5)],
        dtype=np.float64, psf=(3, 3)),
    # even extents: on the centre (the shortcut), one pixel off it, a corner
    "10x12-even": lambda: _build(
        "10x12-even", (10, 12), 2, (2, 3, 3),
        [((5, 6), "two", TWO_LEVEL, 3.0), ((4, 6), "two", TWO_LEVEL, 3.0),
         ((9, 11), "one", None, None)], psf=(3, 3)),
    "32x36-even": lambda: _build(
        "32x36-even", (32, 36), 3, (3, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 5.0), ((15, 17), "two", TWO_LEVEL, 5.0),
         ((31, 35), "one", ONE_LEVEL, 3.0), ((3, 30), "one", ONE_LEVEL, 3.0)]),
    "32x36-f64": lambda: _build(
        "32x36-f64", (32, 36), 2, (2, 3, 3),
        [((16, 19), "two", TWO_LEVEL, 4.0), ((0, 0), "one", ONE_LEVEL, 3.0)], dtype=np.float64),
    # 7 x 5 stamp broadcast over five bands; on the centre of an odd frame, and one pixel off
    "33x37-centre": lambda: _build(
        "33x37-centre", (33, 37), 5, (1, 7, 5),
        [((16, 18), "two", TWO_LEVEL, 5.0), ((2, 33), "one", ONE_LEVEL, 4.0),
         ((28, 5), "one", ONE_LEVEL, 3.0), ((32, 36), "psf", None, None)]),
    "33x37-off-centre": lambda: _build(
        "33x37-off-centre", (33, 37), 2, (1, 7, 5),
        [((16, 19), "two", TWO_LEVEL, 4.0), ((17, 0), "one", ONE_LEVEL, 3.0)], psf=(7, 7)),
    "plateau": lambda: _build(
        "plateau", (33, 37), 2, (2, 3, 3), [((16, 18), "two", TWO_LEVEL, 5.0)], paint=_plateau),
    "moat": lambda: _build(
        "moat", (33, 37), 2, (2, 3, 3), [((16, 18), "one", ONE_LEVEL, 5.0)], paint=_moat),
    "negative-centre": lambda: _build(
        "negative-centre", (33, 37), 2, (2, 3, 3), [((16, 18), "one", ONE_LEVEL, 4.0)],
        paint=_negative_centre, detect=_smooth_detect),
    "passed-detect": lambda: _build(
        "passed-detect", (33, 37), 2, (2, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 4.0), ((4, 30), "psf", ONE_LEVEL, 3.0)],
        detect=_smooth_detect),
    "percentile-30": lambda: _build(
        "percentile-30", (33, 37), 2, (2, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 5.0), ((5, 5), "two", TWO_LEVEL, 3.0)],
        options=dict(percentile=30)),
    "clips-bulge": lambda: _build(
        "clips-bulge", (33, 37), 3, (3, 3, 3), [((16, 18), "two", None, None)],
        paint=_hollow, detect=_smooth_detect),
}
# Frames near the LDS limit (108 KB of float32, 120 KB of float64: beyond the 64 KiB a kernel
# gets without asking), centres in a corner and in the middle: levels of up to 480 pixels, wider
# than the workgroup.  A low threshold keeps wide boxes; compared with the loop only.
LARGE = {
    "large-f32": lambda: _build(
        "large-f32", (150, 180), 2, (2, 3, 3),
        [((0, 0), "one", ONE_LEVEL, 20.0), ((75, 90), "one", ONE_LEVEL, 30.0),
         ((149, 3), "one", ONE_LEVEL, 10.0)], options=dict(thresh=0.02)),
    "large-f64": lambda: _build(
        "large-f64", (100, 150), 2, (2, 3, 3),
        [((99, 149), "one", ONE_LEVEL, 20.0), ((50, 74), "one", ONE_LEVEL, 30.0)],
        dtype=np.float64, options=dict(thresh=0.02)),
}
# which spectrum a joint fit clips to zero in every band
CLIPPED = {"clips-bulge": 0}


def make_case(name):
    return CASES[name]()


def run_loop(case):
    from scarlet_amd import lite

    return lite.init_all_sources_main(case.obs, case.centers, detect=case.detect, **case.options)


def run_oracle(case):
    import init_main_oracle

    return init_main_oracle.of_observation(case.obs, case.centers, case.detect, **case.options)


def run_batch(cases, **extra):
    """``init_blends_main`` of cases that share their options."""
    from scarlet_amd import lite

    options = dict(cases[0].options)
    options.update(extra)
    return lite.init_blends_main([c.obs for c in cases], [c.centers for c in cases],
                                 detect=[c.detect for c in cases], **options)


# One device group (float32 images and model PSF, two bands, the default options): frames
# 10 x 12, 9 x 11 and 33 x 37, stamps 3 x 3 and 7 x 5, PSFs 3 x 3, 5 x 5 and 7 x 7, a passed
# detection image next to coadds
GROUP = ("10x12-even", "33x37-off-centre", "9x11-classes", "passed-detect", "moat")
