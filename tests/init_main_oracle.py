"""CPU restatement of scarlet.lite's main initialisation (reference
scarlet/lite/initialization.py:188-247, 321-419 with ``use_mask=False``), written from its
behaviour in NumPy and in the data type: the coadd, the symmetry about the centre, the radial
monotonicity tables, the sequential sweep as a plain loop over the pixels by radius, the trim,
the box, the split into bulge and disk and the spectra.  The centre pixel of the real-space
convolution and the float64 joint fit are those of tests/init_oracle.py.

tests/test_lite_init_main_host.py pins it to the reference's run (tests/golden/lite_init.npz);
the GPU tests compare ``lite.init_blends_main`` and the per-blend loop with it at shapes and
options the golden does not hold.

A source is a dict as in tests/init_oracle.py: ``kind`` ("psf", "one", "two"), ``components``
(list of ``(origin, morph, sed)`` with the 3-D origin of the box), and for a joint fit
``seds64`` (float64, clipped), ``kept`` and ``cond``."""

import numpy as np

import init_oracle

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def coadd(images, noise_rms):
    return np.sum(images / (noise_rms ** 2)[:, None, None], axis=0)


def centred_slices(shape, center):
    """The largest sub-array centred on ``center`` as the reference's ``uncentered_operator``
    cuts it, or None for a centre on ``shape // 2`` (the whole array is taken as it is)."""
    cy, cx = shape[0] // 2, shape[1] // 2
    if (center[0], center[1]) == (cy, cx):
        return None
    out = []
    for n, p, c in ((shape[0], center[0], cy), (shape[1], center[1], cx)):
        d = 2 * (p - c) + (1 if n % 2 == 0 else 0)
        out.append(slice(d, None) if d > 0 else (slice(None, d) if d < 0 else slice(None)))
    return tuple(out)


def symmetrise(detect, center):
    """prox_uncentered_symmetry(detect.copy(), 0, center, "sdss")"""
    out = detect.copy()
    sl = centred_slices(detect.shape, center)
    sub = out if sl is None else out[sl]
    sub[:] = np.minimum(sub, sub[::-1, ::-1].copy())
    return out


def angle_weights(shape, center):
    """(8, N) float64 'angle' weights of the radial monotonicity operator about ``center``:
    for every neighbour inside the image and strictly nearer the centre the cosine of the angle
    between the directions pixel -> centre and pixel -> neighbour, normalised to unit sum"""
    h, w = shape
    py, px = center
    Y = (np.arange(h) - py)[:, None] * np.ones((1, w), dtype=int)
    X = (np.arange(w) - px)[None, :] * np.ones((h, 1), dtype=int)
    to_peak = np.arctan2(-Y, -X)
    cosw = np.zeros((8, h, w))
    for i, (dy, dx) in enumerate(NEIGHBOURS):
        ny, nx = Y + dy, X + dx
        ok = ((ny + py >= 0) & (ny + py < h) & (nx + px >= 0) & (nx + px < w)
              & (nx * nx + ny * ny < X * X + Y * Y))
        cosw[i][ok] = np.cos(to_peak[ok] - np.arctan2(float(dy), float(dx)))
    cosw = cosw.reshape(8, h * w)
    total = cosw.sum(axis=0)
    total[total == 0] = 1
    return cosw / total[None, :]


def radial_order(shape, center):
    """Flat pixel indices by distance from ``center``, without the centre itself"""
    yy = (np.arange(shape[0]) - center[0])[:, None]
    xx = (np.arange(shape[1]) - center[1])[None, :]
    return np.argsort(np.sqrt(xx ** 2 + yy ** 2).reshape(-1), kind="stable")[1:]


def sweep(image, center):
    """prox_weighted_monotonic(shape, "angle", min_gradient=0, center) on a copy: pixel after
    pixel by radius, each clipped at the weighted sum of its neighbours nearer the centre --
    terms in neighbour order, one rounded multiply and one rounded add each, in the image's
    type"""
    h, w = image.shape
    dtype = image.dtype.type
    weights = angle_weights(image.shape, center).astype(image.dtype)
    flat = image.copy().reshape(-1)
    offsets = [dy * w + dx for dy, dx in NEIGHBOURS]
    for p in radial_order(image.shape, center):
        ref = dtype(0)
        for i in range(8):
            if weights[i, p] > 0:
                ref = dtype(ref + dtype(flat[p + offsets[i]] * weights[i, p]))
        lim = dtype(ref * dtype(1))
        if lim < flat[p]:
            flat[p] = lim
    return flat.reshape(h, w)


def trimmed_cut(morph, center, t):
    """trim_morphology: ``(origin, cut-out)`` on the standard odd box around ``center``"""
    morph = morph.copy()
    morph[~(morph > t)] = 0
    cy, cx = center
    rows, cols = np.nonzero(morph > 0)
    size = 0
    if len(rows):
        b0, b1, l0, l1 = rows.min(), rows.max() + 1, cols.min(), cols.max() + 1
        if b0 <= cy < b1 and l0 <= cx < l1:
            size = 2 * max(cy - b0, b1 - cy, cx - l0, l1 - cx)
    boxsize = 21 + 10 * int(np.ceil(max(size - 21, 0) / 10))
    half = boxsize // 2
    cut = np.zeros((boxsize, boxsize), morph.dtype)
    H, W = morph.shape
    ys, xs = slice(max(cy - half, 0), min(cy + half + 1, H)), slice(max(cx - half, 0),
                                                                   min(cx + half + 1, W))
    cut[ys.start - (cy - half):ys.stop - (cy - half),
        xs.start - (cx - half):xs.stop - (cx - half)] = morph[ys, xs]
    return (int(cy - half), int(cx - half)), cut


def init_sources(images, variance, psfs, stamp, model_psf, noise_rms, centers, detect=None,
                 min_snr=50, percentile=25, thresh=0.5):
    """``stamp``: the (1 or C, kh, kw) difference kernel; ``model_psf``: its 2-D image;
    ``detect``: None (the coadd) or a 2-D array, not modified."""
    C = images.shape[0]
    stamp = np.broadcast_to(stamp, (C,) + stamp.shape[1:])
    if detect is None:
        detect = coadd(images, noise_rms)
    py, px = model_psf.shape[0] // 2, model_psf.shape[1] // 2
    psf_sed = init_oracle.centre_taps(model_psf, stamp, (py, px)).astype(model_psf.dtype)
    t = np.mean(noise_rms) * thresh
    out = []
    for center in centers:
        cy, cx = int(center[0]), int(center[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.floor(init_oracle.snr(images, variance, psfs, (cy, cx))) / min_snr
        origin, cut = trimmed_cut(sweep(symmetrise(detect, (cy, cx)), (cy, cx)), (cy, cx), t)
        peak = np.max(cut)
        if peak == 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                sed = images[:, cy, cx] / psf_sed
            sed[sed < 0] = 0
            out.append(dict(kind="psf", components=[((0, cy - py, cx - px),
                                                     model_psf / np.max(model_psf), sed)]))
            continue
        morph = cut / peak
        if n >= 2:
            level = morph.dtype.type(percentile / 100)
            bulge = np.maximum(morph - level, 0)
            disk = np.minimum(morph, level)
            bulge, disk = bulge / np.max(bulge), disk / np.max(disk)
            box = (origin, morph.shape)
            seds, cond = init_oracle.joint_fit(images, stamp, [box, box], [bulge, disk])
            seds64 = np.where(seds < 0, 0, seds)
            seds = seds.astype(images.dtype)
            seds[seds < 0] = 0
            out.append(dict(kind="two", cond=cond, seds64=seds64, kept=(True, True),
                            components=[((0,) + origin, bulge, seds[0]),
                                        ((0,) + origin, disk, seds[1])]))
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                sed = images[:, cy, cx] / init_oracle.centre_taps(detect, stamp, (cy, cx))
            sed[sed < 0] = 0
            out.append(dict(kind="one", components=[((0,) + origin, morph, sed * peak)]))
    return out


def of_observation(obs, centers, detect=None, **options):
    """``init_sources`` on the data of a ``LiteObservation``."""
    return init_sources(obs.images, obs.variance, obs.psfs, np.asarray(obs.diff_kernel.image),
                        np.asarray(obs.model_psf)[0], np.asarray(obs.noise_rms), centers, detect,
                        **options)
