"""Small scenes for the tests of ``lite.init_blends``, shared by the host and the GPU tests.

A case is an observation, centres, detection coefficients ``(4, Ny, Nx)`` painted by hand --
planes 0 and 1 are the bulge, plane 2 the disk with the default slices, plane 3 is never read
-- the options of the call and the component class every centre is meant to take
(``kinds``: "psf", "one", "two", "none"; tests/test_lite_init_host.py asserts that the oracle
agrees, so a case exercises what its name says).  Images are blobs on the centres whose
levels put the PSF-weighted SNR well inside a class for ``min_snr = 10``; the variance is 1.
A blob is a narrow and a wide Gaussian, so that a joint fit keeps bulge and disk.

The frames: 9 x 11 has fewer pixels than the mask kernel's workgroup has threads, 33 x 37
has 1221, so its strided loops take two trips, the second partial.  Every morphology box is
at least 21 x 21, so every box of the 9 x 11 frame leaves the frame on all sides.

Not reachable, hence without a case: the empty source of a vanishing single component.  A
single component is tried only where ``detectlets[centre] > 0``; its seed is the maximum of a
window that holds the centre, so the seed is positive, is always kept and lies inside the
(at least 21 x 21) box: the maximum of the cut-out is never <= 0."""

from types import SimpleNamespace

import numpy as np

MIN_SNR = 10
PSF_LEVEL, ONE_LEVEL, TWO_LEVEL = 3.0, 15.0, 100.0  # SNR of a source alone, per class


def gauss(shape, center, sigma):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return np.exp(-((y - center[0]) ** 2 + (x - center[1]) ** 2) / (2.0 * sigma ** 2))


def spiral(n=15):
    """Cells of a square spiral from the centre of an n x n grid, arms one cell apart."""
    y = x = n // 2
    cells, step = [(y, x)], 2
    for dy, dx in [(0, 1), (1, 0), (0, -1), (-1, 0)] * n:
        for _ in range(step):
            y, x = y + dy, x + dx
            if not (0 <= y < n and 0 <= x < n):
                return cells
            cells.append((y, x))
        if (dy, dx) in ((1, 0), (-1, 0)):
            step += 2
    return cells


def _observation(images, psfs, stamp, model_psf):
    from scarlet_amd import lite

    dtype = images.dtype
    ones = np.ones(images.shape, dtype)
    obs = lite.LiteObservation(images, ones.copy(), ones, psfs.astype(dtype), model_psf=None)
    obs.model_psf = model_psf[None].astype(dtype)
    obs.diff_kernel = SimpleNamespace(image=stamp.astype(dtype))
    return obs


def _stamp(rng, bands, kh, kw):
    stamp = rng.uniform(-0.2, 1.0, (bands, kh, kw)) / (kh * kw)
    stamp[:, kh // 2, kw // 2] += 1
    return stamp


def _build(name, frame, C, stamp, sources, dtype=np.float32, wdtype=np.float64, psf=(5, 5),
           options=None, paint=None, seed=0):
    """``sources``: ``(centre, kind, level, bulge sigma, disk sigma)``; the bulge goes to
    planes 0 and 1, the disk to plane 2 (a sigma of None leaves the planes alone).
    ``paint(planes, images)`` edits both afterwards."""
    rng = np.random.RandomState(seed + sum(map(ord, name)))
    H, W = frame
    planes = np.zeros((4, H, W))
    images = np.zeros((C, H, W))
    colour = 1 + 0.1 * np.arange(C)
    ph, pw = psf
    psfs = np.stack([gauss(psf, (ph // 2, pw // 2), 1.0 + 0.05 * c) for c in range(C)])
    psfs /= psfs.sum(axis=(1, 2))[:, None, None]
    for center, _, level, bulge, disk in sources:
        if bulge is not None:
            planes[0] += 0.6 * gauss(frame, center, bulge)
            planes[1] += 0.4 * gauss(frame, center, 1.3 * bulge)
        if disk is not None:
            planes[2] += 0.5 * gauss(frame, center, disk)
        blob = colour[:, None, None] * (0.7 * gauss(frame, center, 1.5)
                                        + 0.3 * gauss(frame, center, disk or 4.0))[None]
        # the SNR of the blob alone, PSF stamp clipped by the frame (variance 1)
        y0, x0 = center[0] - ph // 2, center[1] - pw // 2
        ys, xs = slice(max(y0, 0), y0 + ph), slice(max(x0, 0), x0 + pw)
        cut = psfs[:, ys.start - y0:min(y0 + ph, H) - y0, xs.start - x0:min(x0 + pw, W) - x0]
        images += level / (np.sum(blob[:, ys, xs] * cut) / np.sqrt(np.sum(psfs ** 2))) * blob
    planes[3] = -1.0  # negative coefficients: clipped, and the last plane is never summed
    planes[:3] -= 1e-3  # a floor below zero around the sources (clipped to exact zeros)
    images += rng.normal(0, 0.01, images.shape)
    if paint is not None:
        paint(planes, images)
    model_psf = gauss((7, 7), (3, 3), 0.8)
    model_psf /= model_psf.sum()
    obs = _observation(images.astype(dtype), psfs, _stamp(rng, *stamp), model_psf)
    opts = dict(min_snr=MIN_SNR)
    opts.update(options or {})
    return SimpleNamespace(name=name, obs=obs, centers=[s[0] for s in sources],
                           wavelets=planes.astype(wdtype), options=opts,
                           kinds=[s[1] for s in sources])


def _flat_top(planes, images):
    """A 3 x 3 plateau on (16, 18), exactly equal values: the first of the window in
    row-major order is the seed, (15, 17), and none of its equal neighbours is accepted."""
    planes[:3, 15:18, 17:20] = planes[:3, 15:18, 17:20].max(axis=(1, 2))[:, None, None]


def _moat(planes, images):
    """A ring of exact zeros at Chebyshev distance 4 of (16, 18), light beyond it."""
    y, x = np.mgrid[:planes.shape[1], :planes.shape[2]]
    ring = np.maximum(np.abs(y - 16), np.abs(x - 18)) == 4
    planes[:3] += 0.05
    planes[:3, ring] = 0.0


def _serpentine(planes, images):
    """Plane values fall along a spiral of 15 x 15 cells whose arms are walled by zeros."""
    planes[:3] = 0.0
    for k, (y, x) in enumerate(spiral(15)):
        planes[0, y, x] = 1.0 - 0.005 * k


def _spike(planes, images):
    """One positive pixel among zeros on (4, 5): a mask of one kept pixel."""
    planes[:3] = 0.0
    planes[2, 4, 5] = 0.7


def _only_last_summed(planes, images):
    """Light in plane 2 only, which with bulge_slice=[0:1] and disk_slice=[1:2] neither the
    bulge nor the disk holds: both masks are one pixel of value 0."""
    planes[:2] = 0.0


def _negative_bulge(planes, images):
    """The images hold the disk and MINUS the bulge: the joint fit clips the bulge away."""
    bulge = planes[0].clip(0) + planes[1].clip(0)
    images[:] = (2.0 * planes[2].clip(0) - 0.6 * bulge)[None] * 40.0


def _negative_disk(planes, images):
    bulge = planes[0].clip(0) + planes[1].clip(0)
    images[:] = (1.5 * bulge - 0.4 * planes[2].clip(0))[None] * 40.0


def _dark_centre(planes, images):
    """Bright images on (10, 28) where no coefficient is positive."""
    planes[:3, 8:13, 26:31] = -0.5


CASES = {
    # all three classes, a corner, an edge; every box leaves the 9 x 11 frame; masks reach
    # the frame border
    "9x11-classes": lambda: _build(
        "9x11-classes", (9, 11), 2, (2, 3, 3),
        [((0, 0), "psf", 0.5, 1.0, 2.5), ((4, 10), "one", 9.0, 1.0, 2.5),
         ((5, 4), "two", 60.0, 1.0, 3.0)], psf=(3, 3)),  # (the blobs overlap: lower levels)
    "9x11-f64": lambda: _build(
        "9x11-f64", (9, 11), 2, (1, 3, 3),
        [((8, 10), "two", TWO_LEVEL, 1.0, 3.0), ((2, 3), "one", ONE_LEVEL, 1.0, 2.5)],
        dtype=np.float64, psf=(3, 3)),
    # 7 x 5 stamp broadcast over five bands; bulge and disk boxes differ, one clipped
    "33x37-boxes": lambda: _build(
        "33x37-boxes", (33, 37), 5, (1, 7, 5),
        [((16, 18), "two", TWO_LEVEL, 1.2, 5.0), ((2, 33), "two", TWO_LEVEL, 1.2, 4.0),
         ((28, 5), "one", ONE_LEVEL, 1.2, 3.0), ((30, 30), "psf", PSF_LEVEL, 1.0, 2.0)],
        options=dict(bulge_grow=2, disk_grow=5)),
    "33x37-f32-wavelets": lambda: _build(
        "33x37-f32-wavelets", (33, 37), 2, (2, 7, 5),
        [((16, 18), "two", TWO_LEVEL, 1.2, 5.0), ((0, 20), "one", ONE_LEVEL, 1.2, 3.0)],
        wdtype=np.float32),
    # two bands like the 3 x 3 cases, but a 7 x 5 stamp and a 7 x 7 PSF: shares their group
    "33x37-wide-stamp": lambda: _build(
        "33x37-wide-stamp", (33, 37), 2, (1, 7, 5),
        [((12, 9), "two", TWO_LEVEL, 1.2, 4.0), ((25, 30), "one", ONE_LEVEL, 1.2, 3.0)],
        psf=(7, 7)),
    "flat-top": lambda: _build(
        "flat-top", (33, 37), 2, (2, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 1.5, 5.0)], paint=_flat_top),
    "flat-top-one": lambda: _build(
        "flat-top-one", (33, 37), 2, (2, 3, 3),
        [((16, 18), "one", ONE_LEVEL, 1.5, 5.0)], paint=_flat_top),
    "moat": lambda: _build(
        "moat", (33, 37), 2, (2, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 1.5, 5.0)], paint=_moat),
    "moat-one": lambda: _build(
        "moat-one", (33, 37), 2, (2, 3, 3),
        [((16, 18), "one", ONE_LEVEL, 1.5, 5.0)], paint=_moat),
    "serpentine": lambda: _build(
        "serpentine", (15, 15), 2, (2, 3, 3), [((7, 7), "one", ONE_LEVEL, None, None)],
        paint=_serpentine),
    # the disk is one kept pixel, the bulge one pixel of value 0: 2 -> 1 fallback on a
    # one-pixel mask of the detection plane
    "spike": lambda: _build(
        "spike", (9, 11), 2, (2, 3, 3),
        [((4, 5), "one", TWO_LEVEL, None, None)], paint=_spike, psf=(3, 3)),
    "both-missing": lambda: _build(
        "both-missing", (33, 37), 2, (2, 3, 3),
        [((16, 18), "none", TWO_LEVEL, None, 3.0)], paint=_only_last_summed,
        options=dict(bulge_slice=slice(0, 1), disk_slice=slice(1, 2))),
    "no-psf": lambda: _build(
        "no-psf", (33, 37), 2, (2, 3, 3),
        [((16, 18), "one", PSF_LEVEL, 1.2, 4.0), ((10, 28), "psf", TWO_LEVEL, None, None)],
        paint=_dark_centre, options=dict(use_psf=False)),
    "empties-bulge": lambda: _build(
        "empties-bulge", (33, 37), 3, (3, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 1.2, 5.0)], paint=_negative_bulge),
    "empties-disk": lambda: _build(
        "empties-disk", (33, 37), 3, (3, 3, 3),
        [((16, 18), "two", TWO_LEVEL, 1.2, 5.0)], paint=_negative_disk),
}
# which component a joint fit keeps, where it does not keep both
KEPT = {"empties-bulge": (False, True), "empties-disk": (True, False)}


def make_case(name):
    return CASES[name]()


def blob_scene(frame, C, centers, dtype, seed, stamp=(1, 5, 5)):
    """An observation whose detection coefficients come from the starlet chain itself
    (``wavelets=None``): bright and faint blobs on noise."""
    rng = np.random.RandomState(seed)
    images = rng.normal(0, 1.0, (C,) + frame)
    for k, c in enumerate(centers):
        images += (60.0 if k % 2 == 0 else 25.0) * gauss(frame, c, 2.0 + 0.5 * k)[None]
    psfs = np.stack([gauss((5, 5), (2, 2), 1.1) for _ in range(C)])
    psfs /= psfs.sum(axis=(1, 2))[:, None, None]
    model_psf = gauss((7, 7), (3, 3), 0.8)
    model_psf /= model_psf.sum()
    return _observation(images.astype(dtype), psfs, _stamp(rng, *stamp), model_psf)


# ---------------------------------------------------------------------------
# the contract of init_blends with the per-blend loop, and with the oracle
# ---------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
            and np.array_equal(np.signbit(a), np.signbit(b)))


def assert_matches_loop(batch, loop, joint):
    """Bit for bit: sources, components, centres, boxes, morphologies, dtypes, and the
    spectra of every source but those of a joint fit (``joint[i]`` true)."""
    assert len(batch) == len(loop)
    for i, (a, b) in enumerate(zip(batch, loop)):
        assert (a is None) == (b is None), i
        if a is None:
            continue
        assert np.dtype(a.dtype) == np.dtype(b.dtype), i
        assert len(a.components) == len(b.components), (i, len(a.components), len(b.components))
        for j, (ca, cb) in enumerate(zip(a.components, b.components)):
            assert tuple(ca.center) == tuple(cb.center), (i, j)
            assert ca.bbox == cb.bbox, (i, j, ca.bbox, cb.bbox)
            assert same_bits(ca.morph, cb.morph), (i, j)
            assert ca.sed.dtype == cb.sed.dtype and ca.sed.shape == cb.sed.shape, (i, j)
            if not joint[i]:
                assert same_bits(ca.sed, cb.sed), (i, j, ca.sed, cb.sed)


def assert_matches_oracle(batch, loop, oracle):
    """Boxes, morphologies and the spectra of PSF and single-component sources equal the
    oracle's bit for bit.  The spectra of a joint fit are at least as close to the float64
    oracle as the loop's, per source, component and band:
    ``|batch - oracle| <= max(|loop - oracle|, 1e-12 max|oracle|)``.  Returns the largest
    ``|batch - oracle| / max(|loop - oracle|, 1e-12 max|oracle|)`` (0 without a joint fit)."""
    worst = 0.0
    assert len(batch) == len(oracle)
    for i, (a, b, o) in enumerate(zip(batch, loop, oracle)):
        assert (a is None) == (o is None), i
        if a is None:
            continue
        assert len(a.components) == len(o["components"]), (i, o["kind"])
        for j, (ca, (origin, morph, sed)) in enumerate(zip(a.components, o["components"])):
            assert tuple(ca.bbox.origin) == tuple(origin), (i, j)
            assert tuple(ca.bbox.shape) == (len(sed),) + morph.shape, (i, j)
            assert same_bits(ca.morph, morph), (i, j)
            if o["kind"] != "two":
                assert same_bits(ca.sed, sed), (i, j, ca.sed, sed)
        if o["kind"] == "two":
            rows = [k for k in range(2) if o["kept"][k]]
            assert len(rows) == len(a.components) == len(b.components), i
            floor = 1e-12 * np.abs(o["seds64"]).max()
            for ca, cb, k in zip(a.components, b.components, rows):
                want = o["seds64"][k]
                err = np.abs(ca.sed.astype(np.float64) - want)
                allowed = np.maximum(np.abs(cb.sed.astype(np.float64) - want), floor)
                ratio = float((err / allowed).max())
                print("joint fit, source %d component %d: |batch - oracle| %.3e, |loop - oracle| "
                      "%.3e, ratio %.3g" % (i, k, err.max(), np.abs(cb.sed - want).max(), ratio))
                worst = max(worst, ratio)
                assert np.all(err <= allowed), (i, k, err, allowed)
    return worst


def run_loop(case):
    from scarlet_amd import lite

    return lite.init_all_sources_wavelets(case.obs, case.centers, wavelets=case.wavelets.copy(),
                                          **case.options)


def run_oracle(case, options=None, wavelets=None):
    import init_oracle

    return init_oracle.of_observation(case.obs, case.centers,
                                      case.wavelets if wavelets is None else wavelets,
                                      **(case.options if options is None else options))


# ---------------------------------------------------------------------------
# the mixed catalogue: four of the cases under shared options, two scenes whose coefficients
# come from the starlet chain
# ---------------------------------------------------------------------------
# One device group (float64 wavelets, float32 images and model PSF, two bands, the default
# options): frames 9 x 11, 33 x 37 and 15 x 15, stamps 3 x 3 and 7 x 5, PSFs 3 x 3, 5 x 5 and
# 7 x 7, three, two and one source
GROUP = ("9x11-classes", "33x37-wide-stamp", "serpentine", "flat-top", "moat-one")

MIXED = ("9x11-classes", "33x37-boxes", "9x11-f64", "33x37-f32-wavelets")
MIXED_OPTIONS = dict(min_snr=MIN_SNR, bulge_grow=2, disk_grow=5)
_BLOB_CENTERS = [(12, 14), (30, 25), (20, 40), (0, 3)]
BLOBS = {"blob32": ((41, 47), 3, _BLOB_CENTERS, np.float32, 5),
         "blob64": ((36, 52), 3, _BLOB_CENTERS[:3], np.float64, 6)}


def make_blob(name):
    """A case without painted coefficients (``wavelets`` is None: the chain finds them)."""
    frame, C, centers, dtype, seed = BLOBS[name]
    return SimpleNamespace(name=name, obs=blob_scene(frame, C, centers, dtype, seed),
                           centers=centers, wavelets=None, options=dict(MIXED_OPTIONS),
                           kinds=None)


def host_wavelets(obs, scales=5):
    """get_detect_wavelets restated on the CPU (tests/wavelet_oracle.py)."""
    import wavelet_oracle as wo
    from scarlet_amd import wavelet

    detect = wo.coadd(obs.images)
    w = wo.transform(detect, wavelet.get_scales(detect.shape, scales))
    return wo.support(detect.dtype, w, np.median(np.sqrt(obs.variance)))[0] * w


def configurations():
    """Every ``(label, case, options, wavelets)`` a GPU test runs: each case under its own
    options, the cases of the mixed catalogue under the shared ones, the two blob scenes."""
    for name in CASES:
        case = make_case(name)
        yield name, case, case.options, case.wavelets
    for name in MIXED:
        case = make_case(name)
        yield "mixed/" + name, case, MIXED_OPTIONS, case.wavelets
    for name in BLOBS:
        case = make_blob(name)
        yield name, case, case.options, host_wavelets(case.obs)


def group_budget(group, key):
    """A working-set budget between one chunk and one blend per chunk: what the first two
    blends of ``group`` need."""
    from scarlet_amd.lite import initialization as li

    need = [li._init_bytes(c.obs, len(c.centers), len(c.wavelets), key) for c in group]
    return need[0] + need[1]
