"""NumPy restatement of ``scarlet.lite``'s ``weight_sources`` (reference
scarlet/lite/measure.py:39-91 with lite/models.py:521-535, 302-324 and the tap loop of
operators_pybind11.cc:39-56), in the dtype of its inputs.

The convolution is the reference's tap loop written as shifted block adds: the result starts
at zero and every tap of the odd stamp, in row-major order, adds ``value * image`` on the
block where the shifted image stays inside the array -- one rounded multiply and one rounded
add per pixel and tap, the order per pixel fixed.  NumPy neither fuses nor reorders these, so
the arrays are what the native loop gives bit for bit.
"""

import numpy as np


def convolve(cube, stamp):
    """Zero-boundary convolution of a (C, h, w) cube with a (1 or C, kh, kw) stamp of odd
    sides; ``stamp=None``: no convolution."""
    if stamp is None:
        return cube
    kh, kw = stamp.shape[1:]
    if kh % 2 == 0 or kw % 2 == 0:
        raise ValueError("ambiguous centre: the stamp must have odd height and width")
    C, h, w = cube.shape
    out = np.zeros_like(cube)
    for c in range(C):
        values = np.asarray(stamp[c if stamp.shape[0] > 1 else 0], dtype=cube.dtype)
        for ky in range(kh):
            dy = ky - kh // 2
            if abs(dy) >= h:
                continue
            ys, ye = max(dy, 0), max(-dy, 0)
            for kx in range(kw):
                dx = kx - kw // 2
                if abs(dx) >= w:
                    continue
                xs, xe = max(dx, 0), max(-dx, 0)
                out[c, ys:h - ye, xs:w - xe] += values[ky, kx] * cube[c, ye:h - ys, xe:w - xs]
    return out


def _overlap(a0, a1, b0, b1):
    """[lo, hi) common to [a0, a1) and [b0, b1); hi = lo when they miss."""
    lo = max(a0, b0)
    return lo, max(min(a1, b1), lo)


def _add(dest, dest_origin, sub, sub_origin):
    """dest += sub on the overlap of the two 2-D placements (cubes: leading band axis)."""
    y0, y1 = _overlap(dest_origin[0], dest_origin[0] + dest.shape[1], sub_origin[0],
                      sub_origin[0] + sub.shape[1])
    x0, x1 = _overlap(dest_origin[1], dest_origin[1] + dest.shape[2], sub_origin[1],
                      sub_origin[1] + sub.shape[2])
    dest[:, y0 - dest_origin[0]:y1 - dest_origin[0], x0 - dest_origin[1]:x1 - dest_origin[1]] += \
        sub[:, y0 - sub_origin[0]:y1 - sub_origin[0], x0 - sub_origin[1]:x1 - sub_origin[1]]


def reweight(images, weights, psf_half, stamp, components, sources, mask_footprint=True,
             origin=(0, 0), stats=None):
    """Fluxes of ``weight_sources``.

    images, weights: (C, H, W); psf_half: (py, px), the half sizes of the observed PSFs;
    stamp: the difference kernel (1 or C, kh, kw) or None; components: ``(sed, morph, (oy,
    ox))`` in the order the scene adds them, positions in the coordinates ``origin`` (the
    frame's corner) lives in; sources: lists of component indices.

    Returns per source ``(flux, (band, y, x) origin of its box)``; a null source gives
    ``(0, None)``.  ``stats``: a dict whose counts ``clamped`` (ratio > 1), ``zeroed`` (total
    == 0) and ``masked`` (weight 0 inside a flux box) are incremented."""
    dtype = images.dtype
    C, H, W = images.shape
    py, px = psf_half
    fy, fx = origin
    masked = images * (weights > 0) if mask_footprint else images.copy()
    total = np.zeros((C, H, W), dtype)
    for sed, morph, o in components:
        _add(total, (fy, fx), sed[:, None, None] * morph[None, :, :], o)
    total = convolve(total, stamp)
    total[total < 0] = 0
    out = []
    for members in sources:
        if len(members) == 0:
            out.append((0, None))
            continue
        boxes = [(components[k][2][0], components[k][2][1]) + components[k][1].shape
                 for k in members]
        y0, x0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
        y1, x1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
        model = np.zeros((C, y1 - y0, x1 - x0), dtype)
        for k in members:
            sed, morph, o = components[k]
            _add(model, (y0, x0), sed[:, None, None] * morph[None, :, :], o)
        grown = np.zeros((C, y1 - y0 + 2 * py, x1 - x0 + 2 * px), dtype)
        grown[:, py:py + y1 - y0, px:px + x1 - x0] = model
        gy, gx = y0 - py, x0 - px
        model = convolve(grown, stamp)
        model[model < 0] = 0
        a0, a1 = _overlap(fy, fy + H, gy, gy + grown.shape[1])
        b0, b1 = _overlap(fx, fx + W, gx, gx + grown.shape[2])
        in_box = (slice(None), slice(a0 - gy, a1 - gy), slice(b0 - gx, b1 - gx))
        in_obs = (slice(None), slice(a0 - fy, a1 - fy), slice(b0 - fx, b1 - fx))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = model[in_box] / total[in_obs]
        zero = total[in_obs] == 0
        ratio[zero] = 0
        high = ratio > 1
        ratio[high] = 1
        if stats is not None:
            stats["clamped"] = stats.get("clamped", 0) + int(high.sum())
            stats["zeroed"] = stats.get("zeroed", 0) + int(zero.sum())
            stats["masked"] = stats.get("masked", 0) + int((weights[in_obs] <= 0).sum())
        out.append((ratio * masked[in_obs], (0, a0, b0)))
    return out
