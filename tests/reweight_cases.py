"""Synthetic lite blends for the reweighting tests, and the bridge from a ``LiteBlend`` to
``reweight_oracle.reweight``.  Positive spectra and morphologies, images of both signs, a
stamp with negative lobes (so the clamps at 0 act), a block of zero weights, boxes across
each of the four frame edges, one wholly outside, a two-component source whose boxes differ
and a null source.  The frames sit one pixel either side of the kernel's 32 x 32 tile."""

from types import SimpleNamespace

import numpy as np

import reweight_oracle

#           name            frame     C  stamp (bands, kh, kw) or None   psf half  frame corner
CASES = {
    "7x5-none":   dict(frame=(7, 5), C=3, stamp=None, psf_half=(1, 2)),
    "7x5-3x3":    dict(frame=(7, 5), C=3, stamp=(3, 3, 3), psf_half=(1, 1)),
    "7x5-5x9":    dict(frame=(7, 5), C=3, stamp=(3, 5, 9), psf_half=(2, 4)),
    "7x5-15x15":  dict(frame=(7, 5), C=3, stamp=(3, 15, 15), psf_half=(7, 7)),
    "33x31-bcast": dict(frame=(33, 31), C=3, stamp=(1, 5, 5), psf_half=(3, 2)),
    "64x65-C1":   dict(frame=(64, 65), C=1, stamp=(1, 7, 5), psf_half=(2, 3)),
    "33x31-C7":   dict(frame=(33, 31), C=7, stamp=(7, 3, 5), psf_half=(4, 4), corner=(3, -2)),
    "31x33-big-psf": dict(frame=(31, 33), C=2, stamp=(2, 3, 3), psf_half=(5, 6)),
}


def _boxes(H, W):
    """Per source the (oy, ox, h, w) of its components, relative to the frame's corner."""
    return [
        [(2, 1, 5, 5), (4, 2, 3, 7)],          # two components, different boxes
        [(-2, W // 2 - 2, 5, 5)],              # across the top edge
        [(H // 2 - 2, -3, 5, 5)],              # left
        [(H - 3, 1, 5, 5)],                    # bottom
        [(1, W - 2, 5, 5)],                    # right
        [(H + 20, 0, 3, 3)],                   # wholly outside, grown box included
        [],                                    # null source
        [(H - 2, W - 2, 7, 7)],                # across the corner
    ]


def make_blend(name, dtype=np.float32, mixed=False, seed=0):
    """The ``LiteBlend`` of a case; deterministic, so two calls give equal blends.
    ``mixed``: float64 morphologies on float32 images (takes the per-blend path)."""
    from scarlet_amd import Box, lite
    from scarlet_amd.lite.parameters import FistaParameter

    case = CASES[name]
    rng = np.random.RandomState(seed + sum(map(ord, name)))
    (H, W), C = case["frame"], case["C"]
    py, px = case["psf_half"]
    fy, fx = case.get("corner", (0, 0))
    images = rng.normal(0.5, 1.0, (C, H, W)).astype(dtype)
    weights = np.ones((C, H, W), dtype)
    weights[:, 1:3, 0:2] = 0
    weights[0, H - 2:, W - 3:] = 0
    psfs = np.ones((C, 2 * py + 1, 2 * px + 1), dtype)
    obs = lite.LiteObservation(images, (1 / np.maximum(weights, 1)).astype(dtype), weights, psfs,
                               model_psf=None, bbox=Box((C, H, W), origin=(0, fy, fx)))
    if case["stamp"] is not None:
        kb, kh, kw = case["stamp"]
        stamp = rng.uniform(-0.6, 1.0, (kb, kh, kw)) / (kh * kw)
        stamp[:, kh // 2, kw // 2] += 1
        obs.diff_kernel = SimpleNamespace(image=stamp.astype(dtype))
    sources = []
    for boxes in _boxes(H, W):
        comps = []
        for oy, ox, h, w in boxes:
            sed = rng.uniform(0.5, 2.0, C).astype(dtype)
            morph = rng.uniform(0.05, 1.0, (h, w)).astype(np.float64 if mixed else dtype)
            bbox = Box((C, h, w), origin=(0, oy + fy, ox + fx))
            comps.append(lite.LiteFactorizedComponent(
                FistaParameter(sed, step=0.1), FistaParameter(morph, step=0.1),
                (oy + fy + h // 2, ox + fx + w // 2), bbox, obs.bbox, obs.noise_rms, bg_thresh=0.25))
        sources.append(lite.LiteSource(comps, dtype))
    return lite.LiteBlend(sources, obs)


def oracle(blend, mask_footprint=True, stats=None):
    """``reweight_oracle.reweight`` on the data of a ``LiteBlend``."""
    obs = blend.observation
    index = {id(c): k for k, c in enumerate(blend.components)}
    comps = [(c.sed, c.morph, tuple(c.bbox.origin[1:])) for c in blend.components]
    kernel = obs.diff_kernel
    return reweight_oracle.reweight(
        obs.images, obs.weights, (obs.psfs.shape[-2] // 2, obs.psfs.shape[-1] // 2),
        None if kernel is None else np.asarray(kernel.image), comps,
        [[index[id(c)] for c in s.components] for s in blend.sources], mask_footprint,
        origin=tuple(obs.bbox.origin[1:]), stats=stats)


def fluxes(blend):
    """What a reweighting left on the sources: ``(flux, origin or None)`` like the oracle."""
    out = []
    for s in blend.sources:
        if s.is_null:
            assert s.flux == 0 and s.flux_box.shape == (0, 0, 0)
            out.append((0, None))
        else:
            assert s.flux.shape == s.flux_box.shape
            out.append((s.flux, tuple(s.flux_box.origin)))
    return out


def assert_same(got, want):
    """Bit for bit: dtypes, shapes, origins, values."""
    assert len(got) == len(want)
    for i, ((a, ao), (b, bo)) in enumerate(zip(got, want)):
        assert ao == bo, i
        if ao is None:
            assert a == 0 and b == 0
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert np.array_equal(a, b), (i, np.abs(a - b).max())


# relative to each array's largest absolute value: the oracle's measured worst case on the
# reference's fluxes, 2.6e-6, with four-fold room
GOLDEN_TOL = 1e-5


def check_against_golden(fluxes, g):
    """Shapes and origins equal, values within GOLDEN_TOL of each array's largest absolute
    value; returns the worst relative deviation."""
    worst = 0.0
    for i, (flux, origin) in enumerate(fluxes):
        want = g["flux_%d" % i]
        assert tuple(origin) == tuple(g["flux_origin_%d" % i]), i
        assert flux.shape == want.shape, i
        err = np.abs(flux - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err < GOLDEN_TOL, (i, err)
    return worst
