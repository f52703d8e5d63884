"""Seconds ``scarlet_amd.fit_blends`` takes for a catalogue of two-resolution blends (one
high-resolution band plus a ``ResolutionRenderer`` observation on a coarser grid), the device
batches it opens and the bytes of the transformed operators they hold.  Prints one JSON document.

    python tools/fit_blends_multires_time.py [--blends 256] [--scene small|large] [--iters 100]
                                             [--repeats 3] [--distinct 16] [--loop]
                                             [--label NAME] [--out F]

``--scene small``: the first class of tests/multires_batch_cases.py (HR 30 x 34 at 0.05, two LR
bands of 11 x 11 at 0.12: frame (3, 40, 44), operators on 54 x 60).  ``--scene large``: near the
multi-resolution tutorial's size (HR 90 x 90, five LR bands of 36 x 36: frame (6, 100, 100),
operators on 120 x 120).  In both the low-resolution grid lies inside the high-resolution
footprint, so the sub-pixel offsets leave the union frame alone and the catalogue is one group.  ``--distinct`` scenes are built from scratch, each with its own
sub-pixel offset, data and 1 to 4 components (the NumPy set-up of a large ResolutionRenderer
takes most of a second); the rest of the catalogue are copies of them with fresh noise on both
observations.  A timed call fits
fresh deep copies of the catalogue (``fit_blends(blends, iters, e_rel=1e-4)``, the median of
``--repeats`` after one warm-up call); building the catalogue -- the NumPy set-up of every
``ResolutionRenderer`` -- is not timed.  ``--loop``: ``[b.fit(iters, e_rel=1e-4) for b in
blends]`` instead, the loop of single fits.  The script uses nothing but the public interface,
so it runs unchanged from a checkout of an earlier commit (there ``fit_blends`` is that loop);
to compare two commits run it from a checkout of each, in a process of its own, with ``--label``,
on fewer blends where the loop is long (the time per blend does not depend on their number).
"""
import argparse
import copy
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"small": ((30, 34), 2, 11), "large": ((90, 90), 5, 36)}
HR_SCALE, LR_SCALE = 0.05, 0.12


def make_blend(scene, seed):
    import scarlet_amd as scarlet

    hr_shape, bands, side = SCENES[scene]
    rng = np.random.RandomState(seed)

    def wcs(shape, scale, offset=(0.0, 0.0)):
        h, w = shape
        out = scarlet.LinearWCS(np.array([w / 2 + offset[1], h / 2 + offset[0]]), np.zeros(2),
                                np.eye(2) * scale, np.ones(2))
        out.array_shape = (h, w)
        return out

    def psf(n, sigma, c):
        y, x = np.mgrid[:n, :n] - n // 2
        stamp = np.exp(-(y * y + x * x) / (2 * sigma ** 2))
        return np.repeat((stamp / stamp.sum())[None], c, axis=0).astype(np.float32)

    def image(c, shape, n_blobs):
        h, w = shape
        y, x = np.mgrid[:h, :w]
        cube = rng.normal(0, 0.05, (c, h, w))
        for _ in range(n_blobs):
            cy, cx = rng.uniform(0.25, 0.75) * h, rng.uniform(0.25, 0.75) * w
            s = rng.uniform(1.2, 2.5) * max(1.0, min(h, w) / 20)
            cube += 5.0 * rng.uniform(0.5, 2.0, c)[:, None, None] * np.exp(
                -((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        return cube.astype(np.float32)

    obs_hr = scarlet.Observation(image(1, hr_shape, 3), wcs=wcs(hr_shape, HR_SCALE),
                                 psf=scarlet.ImagePSF(psf(11, 1.6, 1)), channels=["hr"],
                                 weights=np.full((1,) + hr_shape, 400.0, np.float32))
    obs_lr = scarlet.Observation(image(bands, (side, side), 2),
                                 wcs=wcs((side, side), LR_SCALE, rng.uniform(-0.45, 0.45, 2)),
                                 psf=scarlet.ImagePSF(psf(9, 1.3, bands)),
                                 channels=["lr%d" % c for c in range(bands)],
                                 weights=np.full((bands, side, side), 400.0, np.float32))
    observations = [obs_hr, obs_lr]
    frame = scarlet.Frame.from_observations(observations, coverage="union",
                                            model_psf=scarlet.GaussianPSF(sigma=0.8))
    C, H, W = frame.shape
    sources = []
    for _ in range(1 + seed % 4):
        oy, ox = rng.randint(2, H - 11), rng.randint(2, W - 11)
        y, x = np.mgrid[:9, :9] - 4
        s = rng.uniform(1.0, 2.0)
        sources.append(scarlet.FactorizedComponent(
            frame, scarlet.TabulatedSpectrum(frame, rng.uniform(0.5, 2.0, C).astype(np.float32)),
            scarlet.ExtendedSourceMorphology(
                frame, (oy + 4, ox + 4), np.exp(-(y * y + x * x) / (2 * s * s)).astype(np.float32),
                bbox=scarlet.Box((9, 9), origin=(oy, ox)))))
    return scarlet.Blend(sources, observations)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--scene", choices=sorted(SCENES), default="small")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import scarlet_amd as scarlet
    from scarlet_amd import fitting

    assert torch.cuda.is_available(), "needs a GPU"
    t0 = time.perf_counter()
    catalogue = [make_blend(args.scene, 1000 + i) for i in range(min(args.blends, args.distinct))]
    for i in range(len(catalogue), args.blends):
        blend = copy.deepcopy(catalogue[i % args.distinct])
        rng = np.random.RandomState(5000 + i)
        for obs in blend.observations:
            obs.data += rng.normal(0, 0.05, obs.data.shape).astype(np.float32)
        catalogue.append(blend)
    t_setup = time.perf_counter() - t0

    opened = [0]
    real = fitting.BlendBatch

    def counted(*a, **k):
        opened[0] += 1
        return real(*a, **k)

    fitting.BlendBatch = counted
    has_report = "_report" in inspect.signature(scarlet.fit_blends).parameters
    report = {}

    def run():
        blends = copy.deepcopy(catalogue)  # (not timed; no blend holds a device handle yet)
        opened[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.loop:
            out = [b.fit(args.iters, e_rel=1e-4) for b in blends]
        else:
            extra = dict(_report=report) if has_report else {}
            out = scarlet.fit_blends(blends, args.iters, e_rel=1e-4, **extra)
        return time.perf_counter() - t0, out

    run()  # warm-up: code objects, sweep plans, the caches of the shapes
    times, fitted = [], None
    for _ in range(args.repeats):
        t, fitted = run()
        times.append(t)
    iterations = int(sum(n for n, _ in fitted))
    blend = catalogue[0]
    renderer = blend.observations[1].renderer
    out = dict(
        metric="fit_blends_multires_seconds", label=args.label, scene=args.scene,
        mode="loop of Blend.fit" if args.loop else "fit_blends", blends=args.blends,
        frame=[int(n) for n in blend.frame.shape],
        fft_shape=[int(n) for n in renderer._fft_shape], iters=args.iters, repeats=args.repeats,
        seconds=round(float(np.median(times)), 4),
        seconds_min_max=[round(min(times), 4), round(max(times), 4)],
        iterations=iterations,
        blend_iterations_per_s=round(iterations / float(np.median(times)), 1),
        batches=opened[0], setup_s=round(t_setup, 2))
    if has_report and not args.loop:
        out.update(groups=len(report["groups"]), alone=len(report["alone"]),
                   batches_reported=report["batches"],
                   operator_bytes=report.get("operator_bytes"))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
