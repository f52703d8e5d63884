"""Synthetic lite blends for the tests of ``lite.fit_spectra_blends``, and the bridge from a
``LiteBlend`` to ``init_oracle.joint_fit``.

The eight blends of ``reweight_cases`` (small frames under 3 x 3 to 15 x 15 stamps, no kernel, a
broadcast stamp, 1 and 7 bands, a frame corner, boxes across every edge, one wholly outside, a
null and a two-component source, images of both signs), then blends whose union boxes sit one
pixel either side of the kernel's 16 x 16 tile and span three tiles, one component, two on one
box, two whose grown boxes do not meet, and blends at and past each limit of the kernel."""

from types import SimpleNamespace

import numpy as np

import init_oracle
import reweight_cases

T = 16  # tile side of csrc/lite_spectra.hip (scarlet_amd.lite.spectra.TILE)


def _grid(n_side, pitch, jitter, seed):
    """``n_side ** 2`` boxes of 5 x 5 on a jittered grid, a source each."""
    rng = np.random.RandomState(seed)
    return [[(int(i * pitch + rng.randint(0, jitter + 1)), int(j * pitch + rng.randint(0, jitter + 1)),
              5, 5)] for i in range(n_side) for j in range(n_side)]


def _scattered(n, frame, seed):
    """``n`` boxes of 5 x 5 at random positions inside a square frame, a source each."""
    rng = np.random.RandomState(seed)
    return [[(int(rng.randint(0, frame - 4)), int(rng.randint(0, frame - 4)), 5, 5)]
            for _ in range(n)]


# name -> frame, bands, stamp (bands, kh, kw) or None, per source the (oy, ox, h, w) of its
# components relative to the frame's corner
OWN = {
    # union boxes of T - 1, T, T + 1 pixels, and T - 1 by T + 1
    "union-15": dict(frame=(20, 20), C=2, stamp=(2, 3, 3), boxes=[[(1, 2, 9, 9)], [(7, 8, 9, 9)]]),
    "union-16": dict(frame=(20, 20), C=2, stamp=(2, 3, 3), boxes=[[(1, 2, 9, 9)], [(8, 9, 9, 9)]]),
    "union-17": dict(frame=(20, 20), C=2, stamp=(2, 3, 3), boxes=[[(1, 2, 9, 9)], [(9, 10, 9, 9)]]),
    "union-15x17": dict(frame=(20, 20), C=2, stamp=(1, 5, 3),
                        boxes=[[(1, 2, 9, 9)], [(7, 10, 9, 9)]]),
    # three tiles on each axis, the last one partial (37 x 35)
    "three-tiles": dict(frame=(40, 38), C=3, stamp=(3, 5, 5), corner=(-4, 7),
                        boxes=[[(0, 1, 11, 11)], [(13, 12, 11, 11), (9, 6, 15, 13)],
                               [(26, 25, 11, 11)]]),
    "one-component": dict(frame=(12, 12), C=3, stamp=(3, 3, 3), boxes=[[(3, 2, 7, 7)]]),
    "same-box": dict(frame=(14, 14), C=3, stamp=(3, 3, 3), boxes=[[(2, 3, 9, 9), (2, 3, 9, 9)]]),
    # grown boxes [-1, 6) and [19, 26) along x never meet: their Gram entry is an exact 0
    "disjoint": dict(frame=(8, 26), C=2, stamp=(2, 3, 3), boxes=[[(1, 0, 5, 5)], [(2, 20, 5, 5)]]),
    # ---- at the limits: 32 components present on one tile, 64 components, a 63 x 63 stamp
    "present-32": dict(frame=(14, 14), C=2, stamp=(2, 3, 3), boxes=_scattered(32, 14, 5)),
    "components-64": dict(frame=(42, 42), C=2, stamp=(2, 3, 3), boxes=_grid(8, 5, 2, 7)),
    "stamp-63": dict(frame=(9, 11), C=1, stamp=(1, 63, 63), boxes=[[(1, 1, 5, 5)], [(3, 4, 5, 7)]]),
}
# ---- one past each limit: these take LiteBlend.fit_spectra
PAST = {
    "present-33": dict(frame=(14, 14), C=2, stamp=(2, 3, 3), boxes=_scattered(33, 14, 6)),
    "components-65": dict(frame=(42, 42), C=2, stamp=(2, 3, 3),
                          boxes=_grid(8, 5, 2, 7) + [[(17, 19, 5, 5)]]),
    "stamp-65": dict(frame=(9, 11), C=1, stamp=(1, 65, 65), boxes=[[(1, 1, 5, 5)], [(3, 4, 5, 7)]]),
}
PAST_REASON = {"present-33": "on one", "components-65": "more than 64 components",
               "stamp-65": "stamp beyond"}
NAMES = list(reweight_cases.CASES) + list(OWN)


def make_blend(name, dtype=np.float32, seed=0):
    """The ``LiteBlend`` of a case; deterministic, so two calls give equal blends."""
    from scarlet_amd import Box, lite
    from scarlet_amd.lite.parameters import FistaParameter

    if name in reweight_cases.CASES:
        return reweight_cases.make_blend(name, dtype, seed=seed)
    case = OWN[name] if name in OWN else PAST[name]
    rng = np.random.RandomState(seed + sum(map(ord, name)))
    (H, W), C = case["frame"], case["C"]
    fy, fx = case.get("corner", (0, 0))
    images = rng.normal(0.5, 1.0, (C, H, W)).astype(dtype)
    weights = np.ones((C, H, W), dtype)
    obs = lite.LiteObservation(images, weights.copy(), weights, np.ones((C, 3, 3), dtype),
                               model_psf=None, bbox=Box((C, H, W), origin=(0, fy, fx)))
    kb, kh, kw = case["stamp"]
    stamp = rng.uniform(-0.6, 1.0, (kb, kh, kw)) / (kh * kw)
    stamp[:, kh // 2, kw // 2] += 1
    obs.diff_kernel = SimpleNamespace(image=stamp.astype(dtype))
    sources = []
    for boxes in case["boxes"]:
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


def hsc_blend(hsc, g):
    """The reference's fitted FISTA state on hsc_cosmos_35 (``g``: golden lite_fista), built
    the way test_gpu_facade.py::test_lite_postprocessing_matches_the_reference builds it."""
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images = hsc["images"].astype(np.float32)
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    obs = lite.LiteObservation(images, (1 / hsc["weights"]).astype(np.float32),
                               hsc["weights"].astype(np.float32), hsc["psfs"].astype(np.float32),
                               model_psf=model_psf[0][None])
    sources = []
    for k in range(int(g["n_comp"])):
        morph = g["b_morph_%d" % k].astype(np.float32)
        oy, ox = (int(v) for v in g["b_origin_%d" % k])
        h, w = morph.shape
        bbox = scarlet.Box((5, h, w), origin=(0, oy, ox))
        comp = lite.init_fista_component((oy + h // 2, ox + w // 2), bbox,
                                         g["b_sed_%d" % k].astype(np.float32).copy(), morph.copy(),
                                         obs, bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    return lite.LiteBlend(sources, obs)


def oracle(blend):
    """``init_oracle.joint_fit`` on the data of a ``LiteBlend``: ``(seds (K, C) float64 before
    the clip, cond, pixels of the union box)``."""
    obs = blend.observation
    _, fy, fx = obs.bbox.origin
    kernel = obs.diff_kernel
    stamp = np.ones((1, 1, 1)) if kernel is None else np.asarray(kernel.image)
    boxes = [((c.bbox.origin[1] - fy, c.bbox.origin[2] - fx), c.morph.shape)
             for c in blend.components]
    seds, cond = init_oracle.joint_fit(obs.images, stamp, boxes, [c.morph for c in blend.components])
    fh = max(o[0] + s[0] for o, s in boxes) - min(o[0] for o, _ in boxes)
    fw = max(o[1] + s[1] for o, s in boxes) - min(o[1] for o, _ in boxes)
    return seds, cond, fh * fw


def sums_of_tables(packed, key):
    """What smi_lite_spectra_* returns for the packed tables of a chunk, by NumPy from the
    tables alone (float64, one sum per entry: the bits differ from the device's)."""
    from scipy.signal import convolve2d

    _, C, kh, kw = key
    out = np.zeros(packed["n_out"])
    for bl in packed["blends"]:
        K, fh, fw = int(bl["n_comp"]), int(bl["fh"]), int(bl["fw"])
        stamp = packed["stamps"][bl["stamp_off"]:bl["stamp_off"] + C * kh * kw].reshape(C, kh, kw)
        frame = packed["images"][bl["image_off"]:bl["image_off"] + C * bl["h"] * bl["w"]]
        frame = frame.reshape(C, bl["h"], bl["w"]).astype(np.float64)
        data = np.zeros((C, fh, fw))
        ys = slice(max(bl["y0"], 0), min(bl["y0"] + fh, bl["h"]))
        xs = slice(max(bl["x0"], 0), min(bl["x0"] + fw, bl["w"]))
        if ys.stop > ys.start and xs.stop > xs.start:
            data[:, ys.start - bl["y0"]:ys.stop - bl["y0"],
                 xs.start - bl["x0"]:xs.stop - bl["x0"]] = frame[:, ys, xs]
        full = []
        for d in packed["comps"][bl["comp0"]:bl["comp0"] + K]:
            f = np.zeros((fh, fw))
            m = packed["morphs"][d["morph_off"]:d["morph_off"] + d["h"] * d["w"]]
            f[d["y0"] - bl["y0"]:d["y0"] - bl["y0"] + d["h"],
              d["x0"] - bl["x0"]:d["x0"] - bl["x0"] + d["w"]] = m.reshape(d["h"], d["w"])
            full.append(f)
        sums = out[bl["out_off"]:bl["out_off"] + C * (K * K + K)].reshape(C, K * K + K)
        for c in range(C):
            design = np.stack([convolve2d(f, stamp[c], mode="same").reshape(-1) for f in full])
            sums[c, :K * K] = (design @ design.T).reshape(-1)
            sums[c, K * K:] = design @ data[c].reshape(-1)
    return out


def expected(seds64, dtype):
    """The oracle's spectra as ``multifit_seds`` hands them on: cast, then clipped."""
    seds = seds64.astype(dtype)
    seds[seds < 0] = 0
    return seds


def ratio_to_bound(got, seds64, cond, n_pix, dtype):
    """Largest ``|got - oracle|`` over the bound ``max(eps, 8 cond^2 n 2^-53) max_k |oracle[k,
    band]|``, band by band, for spectra after ``fit_spectra(clip=False)``.  Inputs are
    converted to double exactly on both sides, so only the order of the sums and the solve of
    the normal equations differ: cond^2 n u is that solve's first-order error, 8 the margin;
    eps = 2^-23 is the one rounding of a float32 result, 0 for float64."""
    eps = 2.0 ** -23 if np.dtype(dtype) == np.float32 else 0.0
    bound = max(eps, 8 * cond ** 2 * n_pix * 2.0 ** -53) * np.abs(seds64).max(axis=0)
    want = np.maximum(expected(seds64, dtype), np.dtype(dtype).type(1e-20))  # prox_sed
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / bound).max())


def state(blend):
    """Everything but the spectra: per source the identities of its components, and per
    component of the blend (morphology, box, optimizer state) as bytes / tuples."""
    per_source = [[id(c) for c in s.components] for s in blend.sources]
    comps = []
    for c in blend.components:
        opt = []
        for p in (c._sed, c._morph):
            for k, v in sorted(vars(p).items()):
                if p is c._sed and v is p.x:  # (a fresh FistaParameter's z is its x)
                    opt.append((k, "the spectrum array"))
                    continue
                if isinstance(v, np.ndarray):
                    opt.append((k, v.dtype.str, v.shape, v.tobytes()))
                elif isinstance(v, dict):
                    opt.append((k, sorted((n, np.asarray(a).tobytes()) for n, a in v.items())))
                elif not callable(v):
                    opt.append((k, repr(v)))
        comps.append((c.morph.tobytes(), tuple(c.bbox.origin), tuple(c.bbox.shape), opt))
    return per_source, comps
