"""Blends for the ``lite.measure_blends`` tests that ``reweight_cases`` lacks: its source
rectangles all fit one 32 x 32 tile of the kernel.

``make_blend``: a 64 x 65 frame with a 5 x 5 stamp that has negative lobes, images of both
signs, a block of zero weights, and four sources -- two components whose flux box is 35 x 64
(2 x 2 ragged tiles), one whose flux box is the 33 x 33 corner of the frame (one pixel over a
tile both ways, its own box overhanging), a null source, and a small one inside a tile.

``flat_blend``: the known-answer construction -- no stamp, 1 x 1 PSFs (the flux box is the
source's box), one single-component source with morphology 1 and integer spectrum, positive
weights, images that are 1 except where a test plants maxima: the ratio is exactly 1, so f is
the image and M the spectrum."""

from types import SimpleNamespace

import numpy as np

FRAME = (64, 65)
PSF_HALF = (2, 2)
# per source the (oy, ox, h, w) of its components; flux box = union grown by PSF_HALF, in frame
BOXES = [
    [(10, 3, 20, 30), (25, 20, 16, 43)],   # union rows 10..41, columns 3..63 -> 35 x 64 at (8, 1)
    [(33, 34, 40, 40)],                    # rows 33.., columns 34.. -> 33 x 33 at (31, 32)
    [],                                    # null source
    [(3, 50, 7, 9)],                       # 11 x 13 at (1, 48)
]
FLUX_BOXES = [(8, 1, 35, 64), (31, 32, 33, 33), None, (1, 48, 11, 13)]


def make_blend(dtype=np.float32, C=3, seed=0, corner=(0, 0)):
    """Deterministic: two calls give equal blends."""
    from scarlet_amd import Box, lite
    from scarlet_amd.lite.parameters import FistaParameter

    rng = np.random.RandomState(1000 + seed)
    H, W = FRAME
    py, px = PSF_HALF
    fy, fx = corner
    images = rng.normal(0.5, 1.0, (C, H, W)).astype(dtype)
    weights = np.ones((C, H, W), dtype)
    weights[:, 20:23, 30:36] = 0
    weights[0, H - 2:, W - 3:] = 0
    psfs = np.ones((C, 2 * py + 1, 2 * px + 1), dtype)
    obs = lite.LiteObservation(images, (1 / np.maximum(weights, 1)).astype(dtype), weights, psfs,
                               model_psf=None, bbox=Box((C, H, W), origin=(0, fy, fx)))
    stamp = rng.uniform(-0.6, 1.0, (C, 5, 5)) / 25
    stamp[:, 2, 2] += 1
    obs.diff_kernel = SimpleNamespace(image=stamp.astype(dtype))
    sources = []
    for boxes in BOXES:
        comps = []
        for oy, ox, h, w in boxes:
            sed = rng.uniform(0.5, 2.0, C).astype(dtype)
            morph = rng.uniform(0.05, 1.0, (h, w)).astype(dtype)
            bbox = Box((C, h, w), origin=(0, oy + fy, ox + fx))
            comps.append(lite.LiteFactorizedComponent(
                FistaParameter(sed, step=0.1), FistaParameter(morph, step=0.1),
                (oy + fy + h // 2, ox + fx + w // 2), bbox, obs.bbox, obs.noise_rms, bg_thresh=0.25))
        sources.append(lite.LiteSource(comps, dtype))
    return lite.LiteBlend(sources, obs)


def flat_blend(h, w, origin=(0, 0), planted=(), dtype=np.float32, sed=(1, 2, 3)):
    """One source on the (h, w) box at ``origin`` of a 64 x 65 frame; ``planted``: ``((band,
    y, x), value)`` in box coordinates, written into the images."""
    from scarlet_amd import Box, lite
    from scarlet_amd.lite.parameters import FistaParameter

    C = len(sed)
    H, W = FRAME
    oy, ox = origin
    images = np.ones((C, H, W), dtype)
    for (b, y, x), value in planted:
        images[b, oy + y, ox + x] = value
    weights = np.ones((C, H, W), dtype)
    psfs = np.ones((C, 1, 1), dtype)
    obs = lite.LiteObservation(images, np.ones((C, H, W), dtype), weights, psfs, model_psf=None,
                               bbox=Box((C, H, W)))
    comp = lite.LiteFactorizedComponent(
        FistaParameter(np.array(sed, dtype), step=0.1), FistaParameter(np.ones((h, w), dtype), step=0.1),
        (oy + h // 2, ox + w // 2), Box((C, h, w), origin=(0, oy, ox)), obs.bbox, obs.noise_rms,
        bg_thresh=0.25)
    return lite.LiteBlend([lite.LiteSource([comp], dtype)], obs)
