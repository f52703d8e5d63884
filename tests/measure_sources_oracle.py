"""Float64 NumPy oracle of csrc/measure_sources.hip, on the plans of ``measure.plan_blend``
(spectra, images, boxes, stamps and weights: no scarlet object): the model by the kernel's rule,
the rendered model by direct zero-boundary convolution, and every sum together with the sum of
the absolute values of its terms."""

import numpy as np


def model_cube(rect, comps, C):
    """(C, h, w): the rounded products sed[c] * image of the components, added to zero in order."""
    y0, x0, h, w = rect
    cube = np.zeros((C, h, w), np.float64)
    for (cy, cx, ch, cw), sed, image in comps:
        part = np.asarray(sed, np.float64)[:, None, None] * np.asarray(image, np.float64)[None]
        cube[:, cy - y0:cy - y0 + ch, cx - x0:cx - x0 + cw] += part
    return cube


def placed(rect, plane, shape):
    """The plane of a box in a zero frame of ``shape``; what leaves the frame is cut."""
    y0, x0, h, w = rect
    H, W = shape
    out = np.zeros(shape, np.float64)
    ys, ye, xs, xe = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ye > ys and xe > xs:
        out[ys:ye, xs:xe] = plane[ys - y0:ye - y0, xs - x0:xe - x0]
    return out


def convolve(plane, stamp):
    """Zero-boundary "same" convolution by direct taps, rows then columns ascending:
    out[y, x] = sum K[ky, kx] plane[y + kh // 2 - ky, x + kw // 2 - kx]."""
    H, W = plane.shape
    kh, kw = stamp.shape
    pad = np.zeros((H + kh - 1, W + kw - 1), np.float64)
    pad[kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = plane
    out = np.zeros((H, W), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            out += np.float64(stamp[ky, kx]) * pad[kh - 1 - ky:kh - 1 - ky + H,
                                                   kw - 1 - kx:kw - 1 - kx + W]
    return out


def _sum(terms):
    """A sum and the sum of the absolute values of its terms."""
    return float(terms.sum()), float(np.abs(terms).sum())


def source(rect, comps, bands, shape):
    """Everything the device forms for one source: ``records`` (C, 8) and ``rendered``
    (observed bands, 3) as smi_measure_sources_f32 lays them out, ``records_abs`` (C, 6) and
    ``rendered_abs`` with the absolute sums, ``R`` the rendered cubes, ``cube`` the model."""
    C, H, W = shape
    y0, x0, h, w = rect
    cube = model_cube(rect, comps, C)
    y, x = np.indices((h, w), dtype=np.float64)
    records, records_abs = np.zeros((C, 8)), np.zeros((C, 6))
    for c in range(C):
        m = cube[c]
        for k, weight in enumerate((None, y, x, y * y, y * x, x * x)):
            records[c, k], records_abs[c, k] = _sum(m if weight is None else weight * m)
        records[c, 6], records[c, 7] = m.max(), int(np.argmax(m))
    rendered, rendered_abs = np.zeros((len(bands), 3)), np.zeros((len(bands), 3))
    R = np.zeros((len(bands), H, W))
    for b, (channel, stamp, weight) in enumerate(bands):
        R[b] = convolve(placed(rect, cube[channel], (H, W)), np.asarray(stamp))
        var = 1.0 / np.asarray(weight, np.float64)
        for q, terms in enumerate((R[b], R[b] * R[b], (R[b] * R[b]) * var)):
            rendered[b, q], rendered_abs[b, q] = _sum(terms)
    return dict(records=records, records_abs=records_abs, rendered=rendered,
                rendered_abs=rendered_abs, R=R, cube=cube)


def blend(plan):
    """``source`` for every source with components of a plan (None for the others)."""
    return [source(rect, comps, plan["bands"], plan["shape"]) if comps else None
            for rect, comps in plan["sources"]]


def region_pixels(rect, shape, kh, kw):
    """Frame pixels the rendered model reaches: the box grown by the stamp's half, clipped."""
    y0, x0, h, w = rect
    _, H, W = shape
    gh = max(min(y0 + h + kh // 2, H) - max(y0 - kh // 2, 0), 0)
    gw = max(min(x0 + w + kw // 2, W) - max(x0 - kw // 2, 0), 0)
    return gh * gw
