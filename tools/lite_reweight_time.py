"""Seconds ``scarlet_amd.lite.weight_blends`` takes to reweight a fitted catalogue of lite
blends, against the per-blend loop ``for b in blends: weight_sources(b)`` and against the fit
of the same catalogue (``fit_blends(..., reweight=False)``).  Prints one JSON line.

    python tools/lite_reweight_time.py --blends 256 --iters 50 [--loop-blends 16] [--repeats 3]

The blends are those of ``tools/lite_batch_time.py``.  All three timings come from one
process and the same fitted blends.  ``weight_blends`` and ``weight_sources`` return host
arrays, so each call ends with the device idle: the host clock around them is the time a
caller waits.  The loop is timed on the first ``--loop-blends`` blends and scaled per blend
(its time per blend does not depend on how many there are); every timing is the median of
``--repeats`` runs after a warm-up run of the same shapes.
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
    from scarlet_amd.lite import measure

    assert torch.cuda.is_available(), "needs a GPU"
    # warm-up of the fit: plans, code objects, the monotonicity plan cache of every box size
    warm = make_blends(len(CROPS), seed0=1)
    lite.fit_blends(warm, 2, e_rel=args.e_rel, resize=10, reweight=False)

    blends = make_blends(args.blends)
    t0 = time.perf_counter()
    lite.fit_blends(blends, args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_fit = time.perf_counter() - t0

    groups, fallback = measure.plan_blends(blends)
    loop = blends[:min(args.loop_blends, len(blends))]
    # warm-up of both reweighting paths on the shapes they are timed on
    lite.weight_blends(blends)
    for b in loop:
        lite.weight_sources(b)
    # the batch is compared with the loop on the blends both ran
    want = [[np.array(s.flux) for s in b.sources] for b in loop]
    lite.weight_blends(blends)
    same = all(np.array_equal(s.flux, w) for b, ws in zip(loop, want) for s, w in zip(b.sources, ws))

    t_batch = timed(lambda: lite.weight_blends(blends), args.repeats)
    t_loop = timed(lambda: [lite.weight_sources(b) for b in loop], args.repeats)
    loop_per_blend = t_loop[0] / len(loop)
    loop_scaled = loop_per_blend * len(blends)
    print(json.dumps(dict(
        metric="lite_weight_blends_seconds", blends=len(blends), iters=args.iters,
        sources=sum(len(b.sources) for b in blends),
        bands=int(blends[0].observation.images.shape[0]),
        stamp=list(blends[0].observation.diff_kernel.image.shape[1:]),
        frame_shapes=len({b.observation.images.shape for b in blends}),
        device_groups=len(groups), fallback_blends=len(fallback), repeats=args.repeats,
        weight_blends_s=round(t_batch[0], 4), weight_blends_min_max_s=[round(t_batch[1], 4),
                                                                       round(t_batch[2], 4)],
        loop_blends=len(loop), loop_s=round(t_loop[0], 4),
        loop_min_max_s=[round(t_loop[1], 4), round(t_loop[2], 4)],
        loop_scaled_s=round(loop_scaled, 3), speedup=round(loop_scaled / t_batch[0], 1),
        fit_blends_s=round(t_fit, 3),
        reweight_share_of_fit_loop=round(loop_scaled / t_fit, 2),
        reweight_share_of_fit_batch=round(t_batch[0] / t_fit, 3),
        bit_identical_to_loop=bool(same))))


if __name__ == "__main__":
    main()
