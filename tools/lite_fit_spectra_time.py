"""Seconds ``scarlet_amd.lite.fit_spectra_blends`` takes for a catalogue of lite blends, against
the per-blend loop ``for b in blends: b.fit_spectra()`` and against the fit of the same
catalogue (``fit_blends(..., reweight=False)``).  Prints one JSON line.

    python tools/lite_fit_spectra_time.py --blends 256 --iters 50 [--loop-blends 16] [--repeats 3]

The blends are those of ``tools/lite_batch_time.py``.  All three timings come from one
process and the same fitted blends.  Both paths return with the spectra in host arrays, so
each call ends with the device idle: the host clock around them is the time a caller waits.
The spectra are no input of the fit, so repeated runs do the same work.  The loop is timed on
the first ``--loop-blends`` blends and scaled per blend (its time per blend does not depend on
how many there are); every timing is the median of ``--repeats`` runs after a warm-up run of
the same shapes.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lite_batch_time import CROPS, make_blends  # noqa: E402


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop-blends", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e-rel", type=float, default=1e-9)
    args = ap.parse_args()

    import numpy as np
    import torch

    from scarlet_amd import lite

    assert torch.cuda.is_available(), "needs a GPU"
    # warm-up of the fit: plans, code objects, the monotonicity plan cache of every box size
    warm = make_blends(len(CROPS), seed0=1)
    lite.fit_blends(warm, 2, e_rel=args.e_rel, resize=10, reweight=False)

    blends = make_blends(args.blends)
    t0 = time.perf_counter()
    lite.fit_blends(blends, args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_fit = time.perf_counter() - t0

    groups, fallback = lite.plan_fit_spectra_blends(blends)
    loop = blends[:min(args.loop_blends, len(blends))]
    # warm-up of both paths on the shapes they are timed on; the loop last, so that the batch
    # is compared with it on the blends both ran
    lite.fit_spectra_blends(blends)
    for b in loop:
        b.fit_spectra()
    want = [np.stack([c.sed for c in b.components]) for b in loop]
    lite.fit_spectra_blends(blends)
    far = max(float(np.abs(np.stack([c.sed for c in b.components]) - w).max() / np.abs(w).max())
              for b, w in zip(loop, want))

    t_batch = timed(lambda: lite.fit_spectra_blends(blends), args.repeats)
    t_loop = timed(lambda: [b.fit_spectra() for b in loop], args.repeats)
    loop_scaled = t_loop[0] / len(loop) * len(blends)
    print(json.dumps(dict(
        metric="lite_fit_spectra_blends_seconds", blends=len(blends), iters=args.iters,
        components=sum(len(b.components) for b in blends),
        bands=int(blends[0].observation.images.shape[0]),
        stamp=list(blends[0].observation.diff_kernel.image.shape[1:]),
        frame_shapes=len({b.observation.images.shape for b in blends}),
        device_groups=len(groups), fallback_blends=len(fallback), repeats=args.repeats,
        fit_spectra_blends_s=round(t_batch[0], 4),
        fit_spectra_blends_min_max_s=[round(t_batch[1], 4), round(t_batch[2], 4)],
        loop_blends=len(loop), loop_s=round(t_loop[0], 4),
        loop_min_max_s=[round(t_loop[1], 4), round(t_loop[2], 4)],
        loop_scaled_s=round(loop_scaled, 3), speedup=round(loop_scaled / t_batch[0], 1),
        fit_blends_s=round(t_fit, 3),
        spectra_share_of_fit_loop=round(loop_scaled / t_fit, 2),
        spectra_share_of_fit_batch=round(t_batch[0] / t_fit, 3),
        largest_distance_from_loop=far)))


if __name__ == "__main__":
    main()
