"""Scenes of tests/test_fit_blends_ragged_host.py and tests/test_gpu_fit_blends_ragged.py: small
blends of different frame sizes that ``fit_blends`` puts into one device batch.  Only the
starlet variant needs a GPU (for the transform of its starting image).

Scene A: four blends on frames 31 x 24, 24 x 31, 31 x 31 and 27 x 29 (three bands, an 11 x 11
difference kernel), whose own frames get the same convolution plan, and a fifth on 70 x 66,
which gets another.  Every blend holds three image components:

* ``inside``: a 9 x 9 box well inside the frame;
* ``edge``: an 11 x 11 box that crosses the bottom and the right edge of the blend's own frame
  (and lies inside the padded 31 x 31 plane of the group wherever the own frame is smaller);
* ``grower``: a 7 x 7 box over a source of sigma 2.5 pixels, 9 pixels from the bottom right
  corner, with an image step of 0.1: the pull over its edges exceeds 0.1 at the first resize
  hook (the oracle says so for all five blends), so the box grows to 21 x 21 and then crosses
  the bottom and right edges of the own frame.

The variants add one source of another kind to every blend: a ``PointSource`` 1.5 pixels from
the bottom right corner, an ``ExtendedSourceMorphology(shifting=True)`` near that corner, a
``StarletSource`` or a ``GaussianSource``.  Scene B: two ``NullRenderer`` blends of different
frames.
"""

import numpy as np

C = 3
CHANNELS = list("gri")
FRAMES = [(31, 24), (24, 31), (31, 31), (27, 29)]
OTHER_FRAME = (70, 66)  # its own convolution plan: another group
STAMP = 11
NOISE = 0.2
GROWER_STEP = 0.1
KINDS = ("image", "point", "shifting", "starlet", "profile")


def _gauss(shape, center, sigma):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return np.exp(-0.5 * ((yy - center[0]) ** 2 + (xx - center[1]) ** 2) / sigma ** 2)


def layout(frame):
    """(name, box size, centre, sigma of the true source, amplitude) of the image components."""
    h, w = frame
    return [("inside", 9, (h // 2 - 3, w // 2 - 4), 1.3, 4.0),
            ("edge", 11, (h - 3, w - 4), 1.6, 3.0),
            ("grower", 7, (h - 9, w - 9), 2.5, 6.0)]


def _psfs():
    import scarlet_amd as scarlet

    model = scarlet.GaussianPSF(sigma=(0.8,) * C)
    observed = scarlet.GaussianPSF(sigma=(1.5,) * C, boxsize=STAMP).get_model().astype(np.float32)
    return model, scarlet.ImagePSF(observed)


def make_blend(frame, seed, kind="image", null=False, nan=False):
    """One ``Blend`` on ``frame`` = (h, w).  ``null``: without PSFs (``NullRenderer``);
    ``nan``: one pixel of the data is NaN, which makes the fit fail."""
    import scarlet_amd as scarlet

    h, w = frame
    rng = np.random.default_rng(seed)
    model_psf, obs_psf = (None, None) if null else _psfs()
    truth = np.zeros((C, h, w))
    seds = []
    for _, _, center, sigma, amp in layout(frame):
        sed = amp * rng.uniform(0.5, 1.5, size=C)
        seds.append(sed)
        truth += sed[:, None, None] * _gauss(frame, center, sigma)[None]
    if kind in ("point", "shifting", "starlet", "profile"):
        extra_center = {"point": (h - 2.5, w - 2.5), "shifting": (h - 6.3, w - 5.6),
                        "starlet": (h - 4, w - 5), "profile": (h - 5.2, w - 6.4)}[kind]
        extra_sed = 8.0 * rng.uniform(0.5, 1.5, size=C)
        truth += extra_sed[:, None, None] * _gauss(
            frame, extra_center, 0.9 if kind == "point" else 1.8)[None]
    data = (truth + rng.normal(0, NOISE, size=truth.shape)).astype(np.float32)
    if nan:
        data[1, h // 2 - 3, w // 2 - 4] = np.nan
    weights = np.full(data.shape, 1 / NOISE ** 2, dtype=np.float32)
    model_frame = scarlet.Frame((C, h, w), psf=model_psf, channels=CHANNELS)
    obs = scarlet.Observation(data, psf=obs_psf, weights=weights, channels=CHANNELS).match(model_frame)
    sources = []
    for (name, size, center, sigma, _), sed in zip(layout(frame), seds):
        oy, ox = center[0] - size // 2, center[1] - size // 2
        box = scarlet.Box((C, size, size), origin=(0, oy, ox))
        image = _gauss((size, size), (size // 2, size // 2), sigma)
        image = (image * rng.uniform(0.85, 1.15, size=image.shape)).astype(np.float32)
        image[size // 2, size // 2] = image.max() * 1.05
        image /= image.max()
        spectrum = scarlet.TabulatedSpectrum(
            model_frame, (sed * rng.uniform(0.8, 1.2, size=C)).astype(np.float32), bbox=box[0],
            min_step=np.full(C, NOISE, dtype=np.float32))
        morphology = scarlet.ExtendedSourceMorphology(
            model_frame, center, image, bbox=box[1:], monotonic="angle", resizing=True)
        if name == "grower":
            morphology.parameters[0].step = GROWER_STEP
        sources.append(scarlet.FactorizedComponent(model_frame, spectrum, morphology))
    if kind == "point":
        sources.append(scarlet.PointSource(model_frame, extra_center, obs))
    elif kind in ("shifting", "starlet"):
        size = 9 if kind == "shifting" else 11
        pixel = np.round(extra_center).astype(int)
        box = scarlet.Box((C, size, size), origin=(0, pixel[0] - size // 2, pixel[1] - size // 2))
        image = _gauss((size, size), (size // 2, size // 2), 1.8).astype(np.float32)
        spectrum = scarlet.TabulatedSpectrum(
            model_frame, extra_sed.astype(np.float32), bbox=box[0],
            min_step=np.full(C, NOISE, dtype=np.float32))
        morphology = scarlet.ExtendedSourceMorphology(
            model_frame, extra_center, image, bbox=box[1:], monotonic="angle", resizing=False,
            shifting=kind == "shifting")
        seed_source = scarlet.FactorizedComponent(model_frame, spectrum, morphology)
        # (the starlet transform of the seed's image runs on the device)
        sources.append(seed_source if kind == "shifting" else
                       scarlet.StarletSource.from_source(seed_source))
    elif kind == "profile":
        sources.append(scarlet.GaussianSource(model_frame, extra_center, 1.8, np.zeros(2), obs))
    return scarlet.Blend(sources, obs)


def scene_a(kind="image", fifth=True, nan_at=None):
    """The four ragged blends of scene A (``kind``: the variant) and, with ``fifth``, the blend
    on ``OTHER_FRAME``.  ``nan_at``: the position of a blend with a NaN in its data."""
    frames = FRAMES + ([OTHER_FRAME] if fifth else [])
    return [make_blend(f, 100 + i, kind, nan=nan_at == i) for i, f in enumerate(frames)]


def scene_b():
    """Two ``NullRenderer`` blends of different frames."""
    return [make_blend(f, 200 + i, null=True) for i, f in enumerate(FRAMES[:2])]


def equal_frames(n=3):
    """``n`` blends on the frame 31 x 24."""
    return [make_blend(FRAMES[0], 300 + i) for i in range(n)]


def oracle_scene(blend):
    """``oracle.pgm.Scene`` of an image-component blend of scene A, from the blend's own cubes
    and parameters (copies)."""
    from oracle import pgm
    from scarlet_amd.blend import _flatten

    data, weights, kernel = blend._observation()
    comps = []
    for c in _flatten(blend.sources):
        spectrum, morphology = c.children
        image = morphology.parameters[0]
        comps.append(pgm.Component(
            np.array(spectrum.parameters[0], dtype=np.float32),
            np.array(image, dtype=np.float32), morphology.bbox.origin[-2:],
            sed_min_step=np.full(C, NOISE, dtype=np.float32), morph_step=float(image.step)))
    return pgm.Scene(data.shape, data.copy(), weights.copy(), kernel.copy(), comps)


def states_of(blend):
    """What the contract of ``fit_blends`` covers of a fitted blend: per parameter its name,
    values, moments, ``std`` and step, and per component the box of its morphology."""
    from scarlet_amd.blend import _flatten

    params = [(p.name, np.array(p), p.m, p.v, p.vhat, np.ma.filled(p.std, -1.0),
               None if callable(p.step) else p.step) for p in blend.parameters]
    boxes = [(tuple(c.children[1].bbox.origin), tuple(c.children[1].bbox.shape))
             for c in _flatten(blend.sources)]
    return params, boxes


def assert_same_fit(got, want, context="", last_bit=()):
    """``got`` (a blend fitted in a list) is bit for bit ``want`` (its copy fitted alone).
    ``last_bit``: names of parameters whose values and moments are held to rtol 1e-12 instead
    (the caller says why)."""
    assert len(got.loss) == len(want.loss), context
    np.testing.assert_array_equal(np.array(got.loss), np.array(want.loss), err_msg=context)
    (p_got, b_got), (p_want, b_want) = states_of(got), states_of(want)
    assert b_got == b_want, context
    assert len(p_got) == len(p_want)
    for a, b in zip(p_got, p_want):
        assert a[0] == b[0] and a[6] == b[6], (context, a[0], a[6], b[6])
        for x, y in zip(a[1:6], b[1:6]):
            assert (x is None) == (y is None), (context, a[0])
            if x is None:
                continue
            if a[0] in last_bit:
                np.testing.assert_allclose(x, y, rtol=1e-12, err_msg="%s %s" % (context, a[0]))
            else:
                np.testing.assert_array_equal(x, y, err_msg="%s %s" % (context, a[0]))
