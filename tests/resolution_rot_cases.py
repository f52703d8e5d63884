"""Scenes with a low-resolution observation on a ROTATED pixel grid (tests/test_resolution_rot_host.py,
tests/test_gpu_resolution_rot.py, tools/make_golden_resolution_rot.py): one high-resolution band
plus one square low-resolution observation whose grid is turned by ``angle`` against the
model's, in the style of tests/multires_batch_cases.py -- the pixel scale in ``pc`` with
``cdelt`` 1, one ``crval`` for all grids (so that a linear WCS and a gnomonic one give the same
pixel-to-pixel map), Gaussian PSFs of 11 x 11 (high resolution) and 9 x 9 (low resolution)
pixels, ``Frame.from_observations(..., coverage="union", model_psf=GaussianPSF(0.8))``.

The module needs NumPy only, so that the golden generator can import it under an interpreter
that has no ``scarlet_amd``; the functions that build objects take the package (``scarlet_amd``
or the reference) as an argument.

The smallest shapes at which the rotated kernels can still go wrong (frame and FFT shape are
what the set-up gives; test_resolution_rot_host.py asserts them and that this list is covered):

    turn    HR 30 x 30,  LR 1 x 9 x 9,   0.3 rad   (2, 40, 40)   54 x 54   n_a = n_b = 9 < 16, one band
    skew    HR 34 x 40,  LR 3 x 11 x 11, -0.2 rad  (4, 44, 50)   60 x 64   Fy != Fx, three bands
    odd     HR 21 x 29,  LR 2 x 5 x 5,   0.7 rad   (3, 29, 37)   45 x 50   an odd FFT length
    wide    HR 24 x 130, LR 2 x 7 x 7,   0.25 rad  (3, 34, 140)  48 x 160  Kx = 81 > 64: a second trip over k
    tiny    HR 34 x 40,  LR 2 x 11 x 11, 1e-6 rad  (3, 44, 50)   60 x 64   sin^2 > eps: still the rotated branch

The low-resolution footprints stay inside the high-resolution one, so the union frame is the
high-resolution image padded by the same margin on all four sides.
"""

import numpy as np

HR_SCALE, LR_SCALE = 5.0e-5, 1.2e-4  # degrees per pixel: a ratio of 2.4
CRVAL = (150.0, 2.0)

OFFSETS = [(0.0, 0.0), (0.3, -0.2), (-0.45, 0.1), (0.17, 0.38), (-0.05, -0.41)]

# name: HR shape, LR bands, LR side, angle (rad), sub-pixel offset of the LR grid, seed,
#       frame shape and FFT shape of the renderer (recorded from the set-up)
CASES = {
    "turn": dict(hr=(30, 30), bands=1, side=9, angle=0.3, offset=OFFSETS[1], seed=11,
                 frame=(2, 40, 40), fft=(54, 54)),
    "skew": dict(hr=(34, 40), bands=3, side=11, angle=-0.2, offset=OFFSETS[2], seed=12,
                 frame=(4, 44, 50), fft=(60, 64)),
    "odd": dict(hr=(21, 29), bands=2, side=5, angle=0.7, offset=OFFSETS[3], seed=13,
                frame=(3, 29, 37), fft=(45, 50)),
    "wide": dict(hr=(24, 130), bands=2, side=7, angle=0.25, offset=OFFSETS[4], seed=14,
                 frame=(3, 34, 140), fft=(48, 160)),
    "tiny": dict(hr=(34, 40), bands=2, side=11, angle=1.0e-6, offset=OFFSETS[1], seed=15,
                 frame=(3, 44, 50), fft=(60, 64)),
}


# Resampler-level cases: what the scenes above cannot reach with observations of 5 .. 11 pixels a
# side -- the other tile variants of the contraction (16 TI x 16 TJ outputs, TI = ceil(n / 16) up
# to 4), more than one tile along a and along b, a second 64-column chunk of the transpose, and
# slices longer than 64 terms (K = Fy Kx > 16384).  Seeded kernels and shift tables on small
# padded grids, so that the dense float64 restatement stays cheap; compared with the restatement
# alone (the reference takes square observations only).
# name: bands, n_a, n_b, Fy, Fx, seed
KERNEL_CASES = {
    "two": dict(C=1, n_a=20, n_b=20, Fy=12, Fx=14, seed=31),      # TI = TJ = 2
    "three": dict(C=2, n_a=36, n_b=33, Fy=10, Fx=12, seed=32),    # TI = TJ = 3: the tutorial's
    "mixed": dict(C=1, n_a=50, n_b=17, Fy=9, Fx=12, seed=33),     # TI = 4, TJ = 2, odd Fy
    "tiles": dict(C=1, n_a=70, n_b=130, Fy=8, Fx=10, seed=34),    # 2 x 3 tiles, three b chunks
    "long": dict(C=1, n_a=3, n_b=2, Fy=130, Fx=256, seed=35),     # K = 16770: slices of 96 terms
}


def kernel_case(name):
    """``(kernel (C, Fy, Fx) float32, h, shifts (2, n_a), other_shifts (2, n_b), model (C, Fy, Fx)
    float32, resid (C, n_a, n_b) float32)`` of a resampler-level case."""
    case = KERNEL_CASES[name]
    C, n_a, n_b, Fy, Fx = (case[k] for k in ("C", "n_a", "n_b", "Fy", "Fx"))
    rng = np.random.RandomState(case["seed"])
    y, x = np.mgrid[:Fy, :Fx]
    bump = np.exp(-((y - Fy // 2) ** 2 + (x - Fx // 2) ** 2) / (2 * 1.5 ** 2))
    kernel = (bump * (1 + 0.3 * rng.normal(0, 1, (C, Fy, Fx)))).astype(np.float32)
    shifts = np.stack((rng.uniform(-Fy / 3, Fy / 3, n_a), rng.uniform(-Fx / 3, Fx / 3, n_a)))
    other = np.stack((rng.uniform(-Fy / 3, Fy / 3, n_b), rng.uniform(-Fx / 3, Fx / 3, n_b)))
    model = rng.normal(0, 1, (C, Fy, Fx)).astype(np.float32)
    resid = rng.normal(0, 1, (C, n_a, n_b)).astype(np.float32)
    return kernel, 2.3, shifts, other, model, resid


def wcs_params(shape, scale, angle=0.0, offset=(0.0, 0.0)):
    """``(crpix, crval, pc)`` of a pixel grid of ``shape`` centred on ``CRVAL``, moved by
    ``offset`` pixels and turned by ``angle``; the scale is in ``pc`` (``cdelt`` is 1)."""
    h, w = shape
    crpix = np.array([w / 2 + offset[1], h / 2 + offset[0]])
    c, s = np.cos(angle), np.sin(angle)
    return crpix, np.array(CRVAL), scale * np.array([[c, -s], [s, c]])


def gaussian_psf(side, sigma, bands):
    y, x = np.mgrid[:side, :side] - side // 2
    stamp = np.exp(-(y * y + x * x) / (2 * sigma ** 2))
    return np.repeat((stamp / stamp.sum())[None], bands, axis=0).astype(np.float32)


def image(rng, bands, shape, n_blobs, amplitude=5.0):
    """Seeded noise plus a few blobs."""
    h, w = shape
    y, x = np.mgrid[:h, :w]
    cube = rng.normal(0, 0.05, (bands, h, w))
    for _ in range(n_blobs):
        cy, cx = rng.uniform(0.25, 0.75) * h, rng.uniform(0.25, 0.75) * w
        s = rng.uniform(1.2, 2.5) * max(1.0, min(h, w) / 20)
        blob = np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        cube += amplitude * rng.uniform(0.5, 2.0, bands)[:, None, None] * blob
    return cube.astype(np.float32)


def arrays(name):
    """The seeded data of a case: ``(HR image, HR PSF, LR image, LR PSF)``."""
    case = CASES[name]
    rng = np.random.RandomState(case["seed"])
    side = case["side"]
    return (image(rng, 1, case["hr"], 3), gaussian_psf(11, 1.6, 1),
            image(rng, case["bands"], (side, side), 2), gaussian_psf(9, 1.3, case["bands"]))


def model(name):
    """A model cube on the case's frame: white noise inside a box plus a smooth blob, so that
    there is power at both Nyquist frequencies."""
    case = CASES[name]
    C, H, W = case["frame"]
    rng = np.random.RandomState(1000 + case["seed"])
    y, x = np.mgrid[:H, :W]
    cube = np.zeros((C, H, W))
    y0, x0 = H // 5, W // 6
    box = (slice(None), slice(y0, H - y0), slice(x0, W - x0))
    cube[box] = rng.normal(0, 1.0, cube[box].shape)
    blob = np.exp(-((y - 0.45 * H) ** 2 + (x - 0.55 * W) ** 2) / (2 * (min(H, W) / 8.0) ** 2))
    cube += 4.0 * rng.uniform(0.5, 2.0, C)[:, None, None] * blob
    return cube.astype(np.float32)


def lr_channels(name):
    return ["lr_%d" % c for c in range(CASES[name]["bands"])]


def observations(name, scarlet, make_wcs, angle=None):
    """``[obs_hr, obs_lr]`` of a case built with the package ``scarlet``; ``make_wcs(crpix, crval,
    pc, shape)`` gives the WCS object; ``angle`` replaces the case's."""
    case = CASES[name]
    side = case["side"]
    angle = case["angle"] if angle is None else angle
    im_hr, psf_hr, im_lr, psf_lr = arrays(name)
    obs_hr = scarlet.Observation(
        im_hr, wcs=make_wcs(*wcs_params(case["hr"], HR_SCALE), case["hr"]),
        psf=scarlet.ImagePSF(psf_hr), channels=["hr"],
        weights=np.full(im_hr.shape, 400.0, np.float32))
    obs_lr = scarlet.Observation(
        im_lr, wcs=make_wcs(*wcs_params((side, side), LR_SCALE, angle, case["offset"]),
                            (side, side)),
        psf=scarlet.ImagePSF(psf_lr), channels=lr_channels(name),
        weights=np.full(im_lr.shape, 400.0, np.float32))
    return [obs_hr, obs_lr]


def linear_wcs(crpix, crval, pc, shape):
    import scarlet_amd as scarlet

    out = scarlet.LinearWCS(crpix, crval, pc, np.ones(2))
    out.array_shape = tuple(shape)
    return out


def scene(name, angle=None):
    """``(frame, obs_hr, obs_lr)`` of a case with ``scarlet_amd``: both observations matched to
    the union frame."""
    import scarlet_amd as scarlet

    obs = observations(name, scarlet, linear_wcs, angle)
    frame = scarlet.Frame.from_observations(obs, coverage="union",
                                            model_psf=scarlet.GaussianPSF(sigma=0.8))
    return frame, obs[0], obs[1]


def components(name, n_components=2):
    """Seeded components on the case's frame: ``[(spectrum (C,), 9 x 9 image, origin)]``."""
    rng = np.random.RandomState(2000 + CASES[name]["seed"])
    C, H, W = CASES[name]["frame"]
    out = []
    for _ in range(n_components):
        oy, ox = rng.randint(2, H - 11), rng.randint(2, W - 11)
        y, x = np.mgrid[:9, :9] - 4
        s = rng.uniform(1.0, 2.0)
        stamp = np.exp(-(y * y + x * x) / (2 * s * s)).astype(np.float32)
        out.append((rng.uniform(0.5, 2.0, C).astype(np.float32), stamp, (oy, ox)))
    return out


def make_blend(name, n_components=2, angle=None, resizing=True):
    """A blend of the case's two observations with the components of ``components``."""
    import scarlet_amd as scarlet

    frame, obs_hr, obs_lr = scene(name, angle)
    sources = []
    for sed, stamp, (oy, ox) in components(name, n_components):
        spectrum = scarlet.TabulatedSpectrum(frame, sed.copy())
        morphology = scarlet.ExtendedSourceMorphology(
            frame, (oy + 4, ox + 4), stamp.copy(), bbox=scarlet.Box((9, 9), origin=(oy, ox)),
            resizing=resizing)
        sources.append(scarlet.FactorizedComponent(frame, spectrum, morphology))
    return scarlet.Blend(sources, [obs_hr, obs_lr])
