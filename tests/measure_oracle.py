"""What ``lite.measure_blends`` sums, restated for the tests: per source the reweighted flux
cube f and the convolved model M clipped at 0 (both from ``reweight_oracle``, in the dtype of
the data), and per band the eight sums of the table with ``math.fsum`` over float64 terms --
the correctly rounded sum of the very products the device adds, so the only thing that
separates the two is the order of the additions."""

import math

import numpy as np

import reweight_cases
import reweight_oracle

U = 2.0 ** -53
NAMES = ("model_flux", "model_sq", "flux", "y", "x", "yy", "yx", "xx")


def models(blend):
    """Per source the ``model[in_box]`` of ``weight_sources`` -- the source's model on its box
    grown by the PSF half sizes, convolved with the stamp, clipped at 0, cut to the frame --
    or None for a null source.  The steps are those of ``reweight_oracle.reweight``."""
    obs = blend.observation
    dtype = obs.images.dtype
    C, H, W = obs.images.shape
    py, px = obs.psfs.shape[-2] // 2, obs.psfs.shape[-1] // 2
    fy, fx = obs.bbox.origin[1:]
    kernel = obs.diff_kernel
    stamp = None if kernel is None else np.asarray(kernel.image)
    out = []
    for src in blend.sources:
        if len(src.components) == 0:
            out.append(None)
            continue
        boxes = [tuple(c.bbox.origin[1:]) + c.morph.shape for c in src.components]
        y0, x0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
        y1, x1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
        model = np.zeros((C, y1 - y0, x1 - x0), dtype)
        for c in src.components:
            reweight_oracle._add(model, (y0, x0), c.sed[:, None, None] * c.morph[None, :, :],
                                 tuple(c.bbox.origin[1:]))
        grown = np.zeros((C, y1 - y0 + 2 * py, x1 - x0 + 2 * px), dtype)
        grown[:, py:py + y1 - y0, px:px + x1 - x0] = model
        gy, gx = y0 - py, x0 - px
        model = reweight_oracle.convolve(grown, stamp)
        model[model < 0] = 0
        a0, a1 = reweight_oracle._overlap(fy, fy + H, gy, gy + grown.shape[1])
        b0, b1 = reweight_oracle._overlap(fx, fx + W, gx, gx + grown.shape[2])
        out.append(model[:, a0 - gy:a1 - gy, b0 - gx:b1 - gx])
    return out


def cubes(blend, mask_footprint=True):
    """Per source ``(flux, model, origin)``; ``(0, None, None)`` for a null source."""
    out = []
    for (flux, origin), model in zip(reweight_cases.oracle(blend, mask_footprint), models(blend)):
        if origin is None:
            out.append((0, None, None))
        else:
            assert model.shape == flux.shape
            out.append((flux, model, origin))
    return out


def terms(flux, model):
    """The eight ``(C, h, w)`` float64 term arrays of a source, in the order of ``NAMES``.
    The coordinate weights are exact integers; a product is exact for float32 data and rounded
    once for float64 data, here as on the device."""
    f, m = np.asarray(flux, np.float64), np.asarray(model, np.float64)
    y, x = np.indices(f.shape[1:], dtype=np.float64)
    return (m, m * m, f, y * f, x * f, (y * y) * f, (y * x) * f, (x * x) * f)


def exact_sums(flux, model):
    """``(sums, bound)``, both ``(C, 8)``: the ``fsum`` of every band's terms, and ``(N + 1)
    2^-53 sum |t|`` with N the pixels of the box (see ``test_gpu_measure``)."""
    C, h, w = flux.shape
    sums, bound = np.zeros((C, 8)), np.zeros((C, 8))
    for k, t in enumerate(terms(flux, model)):
        for b in range(C):
            flat = t[b].reshape(-1).tolist()
            sums[b, k] = math.fsum(flat)
            bound[b, k] = (h * w + 1) * U * math.fsum(abs(v) for v in flat)
    return sums, bound


def table_sums(row):
    """The eight sums of a table row as ``(C, 8)``, in the order of ``NAMES``."""
    return np.concatenate([row["model_flux"][:, None], row["model_sq"][:, None],
                           row["flux"][:, None], row["sums"]], axis=1)


def first_peak(flux):
    """``(index, value)`` of the first maximum in (band, y, x) order."""
    at = np.unravel_index(np.argmax(flux), flux.shape)
    return tuple(int(v) for v in at), float(flux[at])


def reference_snr(model, noise_rms):
    """Reference scarlet/measure.py:89-102 for one observation whose rendered model is
    ``model`` (C, h, w) and whose ``noise_rms`` is one number per band."""
    M = model.reshape(-1)
    W = (model / (model.sum(axis=(-2, -1))[:, None, None])).reshape(-1)
    noise_var = (np.asarray(noise_rms) ** 2)[:, None, None] * np.ones(model.shape)
    var = noise_var.reshape(-1)
    return (M * W).sum() / np.sqrt(((var * W) * W).sum())
