"""Seconds ``scarlet_amd.fit_blends`` takes for a catalogue whose blends all have frames of their
own size, and the number of device batches it opens for them.  Prints one JSON document.

    python tools/fit_blends_ragged_time.py [--blends 256] [--lo 96] [--hi 128] [--iters 100]
                                           [--repeats 3] [--label NAME] [--out F]

The scenes are those of ``tools/init_time.py:synthetic_scene`` (``synthetic.make_blend``: five
bands, a 41 x 41 stamp), each cut to its own frame: sides drawn from ``--lo`` .. ``--hi``
pixels with a seeded generator, the sources whose centres lie 8 pixels inside the cut.  The
catalogue goes through ``init_blends`` once; every timed call fits fresh deep copies of its
blends (``fit_blends(blends, iters, e_rel=1e-4)``, the median of ``--repeats`` after one warm-up
call on the same shapes).  ``batches``: the ``BlendBatch`` objects the call's groups opened,
counted by a wrapper around the class as ``scarlet_amd.fitting`` sees it, so the script runs
unchanged on a commit whose ``fit_blends`` has no ``_report``; where it has one, ``groups`` and
``alone`` come from it.  To compare two commits run the script from a checkout of each, in a
process of its own, with ``--label``.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ragged_scenes(n, lo, hi, seed0=1234):
    """(frames, centers, observations, options) of ``n`` scenes cut to frames of their own."""
    import scarlet_amd as scarlet
    from init_time import synthetic_scene

    rng = np.random.default_rng(seed0)
    frames, centers, observations = [], [], []
    kw = None
    for i in range(n):
        full_frame, full_obs, full_centers, kw = synthetic_scene(seed0 + i)
        h, w = (int(v) for v in rng.integers(lo, hi + 1, size=2))
        channels = list(full_frame.channels)
        frame = scarlet.Frame((len(channels), h, w), psf=full_frame.psf, channels=channels)
        obs = scarlet.Observation(
            np.ascontiguousarray(full_obs.data[:, :h, :w]), psf=full_obs.psf,
            weights=np.ascontiguousarray(full_obs.weights[:, :h, :w]), channels=channels).match(frame)
        frames.append(frame)
        observations.append(obs)
        centers.append([c for c in full_centers if 8 <= c[0] < h - 8 and 8 <= c[1] < w - 8])
    return frames, centers, observations, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--lo", type=int, default=96)
    ap.add_argument("--hi", type=int, default=128)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import scarlet_amd as scarlet
    from scarlet_amd import fitting
    from scarlet_amd import initialization as init

    assert torch.cuda.is_available(), "needs a GPU"
    frames, centers, observations, kw = ragged_scenes(args.blends, args.lo, args.hi)
    t0 = time.perf_counter()
    results = init.init_blends(frames, centers, observations,
                               **dict(kw, fallback=True, silent=True, set_spectra=True))
    t_init = time.perf_counter() - t0
    catalogue = [scarlet.Blend(sources, obs) for (sources, _), obs in zip(results, observations)]

    opened = [0]
    real = fitting.BlendBatch

    def counted(*a, **k):
        opened[0] += 1
        return real(*a, **k)

    fitting.BlendBatch = counted
    has_report = "_report" in inspect.signature(scarlet.fit_blends).parameters
    report = {}

    def run():
        blends = copy.deepcopy(catalogue)  # (not timed)
        opened[0] = 0
        extra = dict(_report=report) if has_report else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = scarlet.fit_blends(blends, args.iters, e_rel=1e-4, **extra)
        return time.perf_counter() - t0, out

    run()  # warm-up: code objects, rocFFT plans, sweep plans of the shapes
    times, fitted = [], None
    for _ in range(args.repeats):
        t, fitted = run()
        times.append(t)
    shapes = [tuple(f.shape[1:]) for f in frames]
    iterations = int(sum(n for n, _ in fitted))
    out = dict(
        metric="fit_blends_ragged_seconds", label=args.label, blends=args.blends,
        frame_sides=[args.lo, args.hi], distinct_frames=len(set(shapes)),
        sources=sum(len(b.sources) for b in catalogue), iters=args.iters, repeats=args.repeats,
        fit_blends_s=round(float(np.median(times)), 4),
        fit_blends_min_max_s=[round(min(times), 4), round(max(times), 4)],
        batches=opened[0], iterations=iterations,
        blend_iterations_per_s=round(iterations / float(np.median(times)), 1),
        failed=len(scarlet.fit_blends.errors), init_blends_s=round(t_init, 3))
    if has_report:
        out.update(groups=[[list(map(str, key)), len(idx)] for key, idx in report["groups"]],
                   alone=len(report["alone"]), batches_reported=report["batches"])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
