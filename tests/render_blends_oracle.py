"""Float64 NumPy oracle of csrc/render_sources.hip, on the plans of ``rendering.plan_blend``
(spectra, images, boxes, stamps, weights and data: no scarlet object), built on
tests/measure_sources_oracle.py: the scene by the kernel's rule (the rounded products
sed[c] * image of all components, added to zero in order, cut to the frame), every rendering by
direct zero-boundary convolution, the ratio rules of the reference's weight_sources, and the error
bounds the GPU test holds the device to."""

import numpy as np

import measure_sources_oracle as mo

U = 2.0 ** -52    # unit roundoff of a float64 sum's term (as tests/test_gpu_measure_blends.py)
U32 = 2.0 ** -24  # float32, round to nearest
TINY32 = 2.0 ** -149


def scene_cube(plan, absolute=False):
    """(C, H, W): every component of the blend added into a zero frame, in order."""
    C, H, W = plan["shape"]
    cube = np.zeros((C, H, W), np.float64)
    for _, comps in plan["sources"]:
        for (cy, cx, ch, cw), sed, image in comps:
            part = np.asarray(sed, np.float64)[:, None, None] * np.asarray(image, np.float64)[None]
            if absolute:
                part = np.abs(part)
            ys, ye, xs, xe = max(cy, 0), min(cy + ch, H), max(cx, 0), min(cx + cw, W)
            if ye > ys and xe > xs:
                cube[:, ys:ye, xs:xe] += part[:, ys - cy:ye - cy, xs - cx:xe - cx]
    return cube


def _render(cube, plan):
    """(bands, H, W): band b is ``cube[channel_b]`` convolved with its stamp."""
    return np.stack([mo.convolve(cube[channel], np.asarray(stamp, np.float64))
                     for channel, stamp, _ in plan["bands"]])


def _render_abs(cube_abs, plan):
    return np.stack([mo.convolve(cube_abs[channel], np.abs(np.asarray(stamp, np.float64)))
                     for channel, stamp, _ in plan["bands"]])


def ratio(R_k, R_tot):
    """max(R_k, 0) / max(R_tot, 0), 0 where the denominator is 0, 1 where it exceeds 1."""
    num = np.where(R_k < 0, 0.0, R_k)
    den = np.where(R_tot < 0, 0.0, R_tot)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / den
    out[den == 0] = 0
    out[out > 1] = 1
    return out


def ratio_bound(R_k, R_tot, d_k, d_tot):
    """How far the ratio can move when R_k moves by at most d_k and R_tot by at most d_tot.  The
    ratio does not fall when R_k grows, and for R_tot > 0 does not grow when R_tot grows: its
    extremes over the two intervals lie at their ends -- except that at R_tot <= 0 it is 0 and
    just above it is 1 (or 0 while R_k <= 0), so an interval of R_tot that holds 0 reaches both."""
    here = ratio(R_k, R_tot)
    lo = ratio(R_k - d_k, R_tot + d_tot)
    hi = ratio(R_k + d_k, R_tot - d_tot)
    crosses = R_tot - d_tot <= 0
    lo = np.where(crosses, 0.0, lo)
    hi = np.where(crosses, np.where((R_k + d_k > 0) & (R_tot + d_tot > 0), 1.0, 0.0), hi)
    return np.maximum(hi - here, here - lo)


def blend(plan, key, mask_footprint=True):
    """Everything the device forms for one blend, bands of all observations in a row:

    ``R`` (bands, H, W) the float64 scene and ``R_bound`` what a float64 tap loop in another order
    may differ from it by: (kh kw K + 4) 2^-52 sum |terms|, K the components -- recursive summation
    of the same rounded terms in two orders, as ``_bounds`` of tests/test_gpu_measure_blends.py;
    ``rendered_bound`` = one float32 rounding of the value on top; ``chi2`` (bands,) with
    ``chi2_bound`` = sum w (2 |R - d| e + e^2), e = R_bound, + (H W + 8) 2^-52 sum |terms|: the
    moved terms, three roundings per term and two orders of a sum of H W terms; ``image``; and
    ``sources``: per source None or a dict of ``region``, ``R`` (bands, H, W), ``R_bound``,
    ``rendered_bound`` (both on the region), ``flux`` and ``flux_bound`` = |image| times
    ``ratio_bound`` + |flux| (2^-24 + 2 x 2^-52): the moved ratio, the division, the product and
    the one float32 rounding more."""
    from scarlet_amd import rendering

    C, kh, kw = key
    _, H, W = plan["shape"]
    taps = kh * kw
    n_comp = sum(len(comps) for _, comps in plan["sources"])
    R = _render(scene_cube(plan), plan)
    R_bound = (taps * n_comp + 4) * U * _render_abs(scene_cube(plan, absolute=True), plan)
    d = np.stack([np.asarray(image, np.float64) for image in plan["data"]])
    w = np.stack([np.asarray(weight, np.float64) for _, _, weight in plan["bands"]])
    terms = w * (R - d) ** 2
    chi2 = terms.sum(axis=(1, 2))
    chi2_bound = ((w * (2 * np.abs(R - d) * R_bound + R_bound ** 2)).sum(axis=(1, 2))
                  + (H * W + 8) * U * np.abs(terms).sum(axis=(1, 2)))
    image32 = np.stack([np.asarray(image, np.float32) for image in plan["data"]])
    if mask_footprint:
        image32 = image32 * (np.stack([wt for _, _, wt in plan["bands"]]) > 0)
    image = image32.astype(np.float64)
    sources = []
    for (rect, comps), region in zip(plan["sources"], plan["regions"]):
        if not comps:
            sources.append(None)
            continue
        assert tuple(region) == tuple(rendering.region_of(rect, (H, W), kh, kw))
        y0, x0, h, wd = region
        crop = (slice(None), slice(y0, y0 + h), slice(x0, x0 + wd))
        cube = mo.model_cube(rect, comps, C)
        cube_abs = mo.model_cube(rect, [(r, np.abs(s), np.abs(i)) for r, s, i in comps], C)
        R_k = np.stack([mo.convolve(mo.placed(rect, cube[channel], (H, W)),
                                    np.asarray(stamp, np.float64))
                        for channel, stamp, _ in plan["bands"]])
        A_k = np.stack([mo.convolve(mo.placed(rect, cube_abs[channel], (H, W)),
                                    np.abs(np.asarray(stamp, np.float64)))
                        for channel, stamp, _ in plan["bands"]])
        # (outside the region the source's rendering is exactly zero)
        outside = np.ones((H, W), bool)
        outside[y0:y0 + h, x0:x0 + wd] = False
        assert not R_k[:, outside].any()
        Rk_bound = (taps * len(comps) + 4) * U * A_k
        flux = ratio(R_k[crop], R[crop]) * image[crop]
        flux_bound = (np.abs(image[crop]) * ratio_bound(R_k[crop], R[crop], Rk_bound[crop],
                                                        R_bound[crop])
                      + np.abs(flux) * (U32 + 2 * U) + TINY32)
        sources.append(dict(region=tuple(region), R=R_k, R_bound=Rk_bound[crop],
                            rendered_bound=Rk_bound[crop] + U32 * np.abs(R_k[crop]) + TINY32,
                            flux=flux, flux_bound=flux_bound))
    return dict(R=R, R_bound=R_bound, rendered_bound=R_bound + U32 * np.abs(R) + TINY32,
                chi2=chi2, chi2_bound=chi2_bound, image=image, sources=sources, data=d,
                weights=w)
