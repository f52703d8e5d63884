"""Seconds ``scarlet_amd.detect.get_detect_wavelets_batch`` takes for the detection
coefficients of a catalogue of blends, against the per-blend loop
``[get_detect_wavelets(im, var, scales) for im, var in ...]`` -- what ``lite.init_blends`` ran
per chunk before it had the batch -- in the same run.  Prints one JSON line.

    python tools/detect_batch_time.py --blends 256 [--scales 5] [--repeats 3]

The blends are those of ``tools/lite_batch_time.py``.  Both paths return host arrays, so each
call ends with the device idle: the host clock around them is the time a caller waits.  Both
are warmed up on the shapes they are timed on, then timed ``--repeats`` times, alternating.
``identical_to_loop``: every blend's array equals the loop's in shape, dtype and bits (NaN
positions and zero signs included).  ``split_s``: one more batch call with its steps clocked
from outside, each ending with the device idle -- the host medians of ``sqrt(variance)``,
packing the images and their one upload per group, the device chain, and the rest (the
download and the per-blend views).
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

from lite_batch_time import make_blends  # noqa: E402


def same_bits(a, b):
    import numpy as np

    return (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
            and np.array_equal(np.signbit(a), np.signbit(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from scarlet_amd import detect, wavelet

    assert torch.cuda.is_available(), "needs a GPU"
    blends = make_blends(args.blends)
    images = [b.observation.images for b in blends]
    variance = [b.observation.variance for b in blends]

    def batch():
        return detect.get_detect_wavelets_batch(images, variance, scales=args.scales)

    def loop():
        return [detect.get_detect_wavelets(im, var, scales=args.scales)
                for im, var in zip(images, variance)]

    groups, fallback = detect.plan_detect_wavelets_batch(images, variance, scales=args.scales)
    got, want = batch(), loop()  # warm-up of both paths, and the comparison
    same = len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))
    t_batch, t_loop = [], []
    for _ in range(args.repeats):
        for fn, out in ((batch, t_batch), (loop, t_loop)):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)

    split = {}

    def clocked(name, fn):
        def run(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            split[name] = split.get(name, 0.0) + time.perf_counter() - t0
            return out
        return run

    steps = (("sigma_medians_s", detect, "_batch_sigmas"),
             ("pack_upload_s", detect, "_batch_upload"),
             ("device_s", wavelet, "detect_wavelets_batch_device"))
    saved = [(mod, f, getattr(mod, f)) for _, mod, f in steps]
    for name, mod, f in steps:
        setattr(mod, f, clocked(name, getattr(mod, f)))
    try:
        t0 = time.perf_counter()
        batch()
        total = time.perf_counter() - t0
    finally:
        for mod, f, fn in saved:
            setattr(mod, f, fn)
    split["download_views_s"] = total - sum(split.values())

    shapes = sorted({im.shape[1:] for im in images}, key=lambda s: s[0] * s[1])
    print(json.dumps(dict(
        metric="detect_wavelets_batch_seconds", blends=len(blends), scales=args.scales,
        bands=int(images[0].shape[0]), frame_shapes=len(shapes),
        smallest_frame=list(shapes[0]), largest_frame=list(shapes[-1]),
        planes=sorted({len(g) for g in got}), device_groups=len(groups),
        device_calls=sum(len(c) for c in groups.values()), fallback_blends=len(fallback),
        repeats=args.repeats,
        batch_s=round(statistics.mean(t_batch), 4),
        batch_min_max_s=[round(min(t_batch), 4), round(max(t_batch), 4)],
        loop_s=round(statistics.mean(t_loop), 4),
        loop_min_max_s=[round(min(t_loop), 4), round(max(t_loop), 4)],
        speedup=round(statistics.mean(t_loop) / statistics.mean(t_batch), 1),
        slowest_batch_beats_fastest_loop=max(t_batch) < min(t_loop),
        split_s={k: round(v, 4) for k, v in split.items()},
        identical_to_loop=same)))


if __name__ == "__main__":
    main()
