"""CPU restatement of scarlet.lite's wavelet initialisation (reference
scarlet/lite/initialization.py:422-605) from given detection coefficients, written from its
behaviour: NumPy, ``oracle.proxops.prox_monotonic_mask`` for the masks, the tap loop of the
reference's ``apply_filter`` for the centre pixel of the real-space convolution, a direct
float64 convolution and a float64 ``lstsq`` for the joint fit of bulge and disk.

tests/test_lite_init_host.py pins it to the reference's run (tests/golden/detect.npz); the
GPU tests compare ``lite.init_blends`` and the per-blend loop with it at shapes and options
the golden does not hold.

A source is None (neither bulge nor disk), or a dict: ``kind`` ("psf", "one", "two", "empty"),
``components`` (list of ``(origin, morph, sed)`` with the 3-D origin of the box), and for a
joint fit ``cond``, the condition number of the worst band's design matrix."""

import numpy as np
from scipy.signal import convolve2d

from oracle import proxops


def snr(images, variance, psfs, center):
    """calculate_snr: PSF stamp on the centre, zero outside the frame, the images' type"""
    C, ph, pw = psfs.shape
    y0, x0 = center[0] - ph // 2, center[1] - pw // 2
    img, var = np.zeros(psfs.shape, images.dtype), np.zeros(psfs.shape, variance.dtype)
    _, H, W = images.shape
    ys, xs = slice(max(y0, 0), min(y0 + ph, H)), slice(max(x0, 0), min(x0 + pw, W))
    sub = (slice(None), slice(ys.start - y0, ys.stop - y0), slice(xs.start - x0, xs.stop - x0))
    img[sub], var[sub] = images[:, ys, xs], variance[:, ys, xs]
    return np.sum(img * psfs) / np.sqrt(np.sum(psfs * var * psfs))


def centre_taps(plane, stamp, center):
    """The centre pixel of apply_filter, band by band: accumulator from 0, taps in row-major
    order, one rounded multiply and add per tap in the plane's type, taps outside skipped."""
    dtype = np.float64 if plane.dtype == np.float64 else np.float32
    plane = plane.astype(dtype, copy=False)
    C, kh, kw = stamp.shape
    out = np.zeros(C, dtype)
    H, W = plane.shape
    for c in range(C):
        k = stamp[c].astype(dtype)
        acc = dtype(0)
        for ky in range(kh):
            y = center[0] - (ky - kh // 2)
            if not 0 <= y < H:
                continue
            for kx in range(kw):
                x = center[1] - (kx - kw // 2)
                if 0 <= x < W:
                    acc = dtype(acc + dtype(k[ky, kx] * plane[y, x]))
        out[c] = acc
    return out


def monotonic_morph(plane, center, grow):
    """init_monotonic_morph(use_mask=True): ``(origin, morph)`` of the normalised cut-out on
    its standard odd box around ``center``, or None when only a zero seed is left"""
    plane = np.ascontiguousarray(plane)
    valid, _, bounds = proxops.prox_monotonic_mask(plane, 0, center, max_iter=0)
    morph = np.where(valid, plane, 0).astype(plane.dtype)  # (not a product: -0 stays out)
    b0, b1, l0, l1 = (int(v) for v in bounds)
    if (b0, l0) == (b1, l1) and morph[b0, l0] == 0:
        return None
    if grow is not None and grow > 0:
        b0, b1, l0, l1 = b0 - grow, b1 + grow, l0 - grow, l1 + grow
    cy, cx = center
    inside = b0 <= cy <= b1 and l0 <= cx <= l1
    size = 2 * max(cy - b0, b1 + 1 - cy, cx - l0, l1 + 1 - cx) if inside else 0
    boxsize = 21 + 10 * int(np.ceil(max(size - 21, 0) / 10))
    half = boxsize // 2
    cut = np.zeros((boxsize, boxsize), plane.dtype)
    H, W = plane.shape
    for i in range(boxsize):
        y = cy - half + i
        if 0 <= y < H:
            xs = slice(max(cx - half, 0), min(cx + half + 1, W))
            cut[i, xs.start - (cx - half):xs.stop - (cx - half)] = morph[y, xs]
    with np.errstate(divide="ignore", invalid="ignore"):
        cut = cut / np.max(cut)
    return (cy - half, cx - half), cut


def joint_fit(images, stamp, boxes, morphs):
    """multifit_seds in float64: ``(seds (2, C) float64 before the clip, cond)``; the design
    is each morphology on the union box, convolved there (zero outside) with the band's stamp"""
    C, H, W = images.shape
    y0 = min(o[0] for o, _ in boxes)
    x0 = min(o[1] for o, _ in boxes)
    y1 = max(o[0] + s[0] for o, s in boxes)
    x1 = max(o[1] + s[1] for o, s in boxes)
    img = np.zeros((C, y1 - y0, x1 - x0))
    ys, xs = slice(max(y0, 0), min(y1, H)), slice(max(x0, 0), min(x1, W))
    img[:, ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = images[:, ys, xs]
    full = []
    for (o, s), m in zip(boxes, morphs):
        f = np.zeros(img.shape[1:])
        f[o[0] - y0:o[0] - y0 + s[0], o[1] - x0:o[1] - x0 + s[1]] = m
        full.append(f)
    seds, cond = np.zeros((len(morphs), C)), 0.0
    for c in range(C):
        k = stamp[c if stamp.shape[0] > 1 else 0].astype(np.float64)
        design = np.stack([convolve2d(f, k, mode="same").reshape(-1) for f in full], axis=1)
        seds[:, c] = np.linalg.lstsq(design, img[c].reshape(-1), rcond=None)[0]
        sv = np.linalg.svd(design, compute_uv=False)
        cond = max(cond, sv[0] / sv[-1] if sv[-1] > 0 else np.inf)
    return seds, cond


def init_sources(images, variance, psfs, stamp, model_psf, centers, wavelets, min_snr=50,
                 bulge_grow=5, disk_grow=5, use_psf=True, bulge_slice=slice(None, 2),
                 disk_slice=slice(2, -1)):
    """``stamp``: the (1 or C, kh, kw) difference kernel; ``model_psf``: its 2-D image;
    ``wavelets``: (S, Ny, Nx), not modified."""
    wavelets = np.where(wavelets < 0, 0, wavelets).astype(wavelets.dtype)
    C = images.shape[0]
    stamp = np.broadcast_to(stamp, (C,) + stamp.shape[1:])

    def plane_sum(stack):
        if len(stack) == 0:
            return np.zeros(wavelets.shape[1:], wavelets.dtype)
        acc = stack[0].copy()
        for p in stack[1:]:
            acc = acc + p
        return acc

    detect, bulges, disks = (plane_sum(wavelets[s]) for s in (slice(None, -1), bulge_slice,
                                                              disk_slice))
    py, px = model_psf.shape[0] // 2, model_psf.shape[1] // 2
    psf_sed = centre_taps(model_psf, stamp, (py, px)).astype(model_psf.dtype)
    out = []
    for center in centers:
        cy, cx = int(center[0]), int(center[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.floor(snr(images, variance, psfs, (cy, cx))) / min_snr

        def psf_source():
            with np.errstate(divide="ignore", invalid="ignore"):
                sed = images[:, cy, cx] / psf_sed
            sed[sed < 0] = 0
            return dict(kind="psf", components=[((0, cy - py, cx - px),
                                                 model_psf / np.max(model_psf), sed)])

        def single():
            found = monotonic_morph(detect, (cy, cx), disk_grow)
            if found is None or np.max(found[1]) <= 0:
                return dict(kind="empty", components=[])
            with np.errstate(divide="ignore", invalid="ignore"):
                sed = images[:, cy, cx] / centre_taps(detect, stamp, (cy, cx))
            sed[sed < 0] = 0
            return dict(kind="one", components=[((0,) + found[0], found[1] / np.max(found[1]),
                                                 sed)])

        if (n < 1 and use_psf) or detect[cy, cx] <= 0:
            out.append(psf_source())
        elif n < 2:
            out.append(single())
        else:
            bulge = monotonic_morph(bulges, (cy, cx), bulge_grow)
            disk = monotonic_morph(disks, (cy, cx), disk_grow)
            if bulge is None and disk is None:
                out.append(None)
            elif bulge is None or disk is None:
                out.append(single())
            else:
                seds, cond = joint_fit(images, stamp, [(bulge[0], bulge[1].shape),
                                                       (disk[0], disk[1].shape)],
                                       [bulge[1], disk[1]])
                seds64 = seds.copy()
                seds = seds.astype(images.dtype)
                seds[seds < 0] = 0
                comps = []
                if np.count_nonzero(seds[0]):
                    comps.append(((0,) + bulge[0], bulge[1], seds[0]))
                if np.sum(seds[1]) != 0:
                    comps.append(((0,) + disk[0], disk[1], seds[1]))
                out.append(dict(kind="two", components=comps, cond=cond,
                                seds64=np.where(seds64 < 0, 0, seds64),
                                kept=(bool(np.count_nonzero(seds[0])), bool(np.sum(seds[1]) != 0))))
    return out


def of_observation(obs, centers, wavelets, **options):
    """``init_sources`` on the data of a ``LiteObservation``."""
    return init_sources(obs.images, obs.variance, obs.psfs, np.asarray(obs.diff_kernel.image),
                        np.asarray(obs.model_psf)[0], centers, np.asarray(wavelets), **options)
