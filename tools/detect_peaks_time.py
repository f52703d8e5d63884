"""Seconds ``scarlet_amd.detect.get_peaks_batch`` takes for the peaks of a catalogue of blends
whose detection coefficients are on the device, against the per-blend loop
``[detect.get_peaks(c) for c in coeffs]`` in the same run.  Prints one JSON line.

    python tools/detect_peaks_time.py --blends 256 [--repeats 3]

The blends are those of ``tools/lite_batch_time.py``; the coefficients come from
``get_detect_wavelets_batch(..., scales=3, device=True)`` and stay where they are.  Both paths
are warmed up on the catalogue, then timed ``--repeats`` times, alternating, with the device
idle before and after the timed region; the fastest and the slowest of each are kept.
``identical_to_loop``: every blend's list of ``(y, x)`` equals the loop's, in order.
``split_s``: one more batch call with its two library calls (label and fetch, with the
allocation of their buffers) clocked from outside; the rest is host assembly -- the plan, the
``Footprint`` objects, the quad trees and their queries.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lite_batch_time import make_blends  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from scarlet_amd import detect, detect_pybind11

    assert torch.cuda.is_available(), "needs a GPU"
    blends = make_blends(args.blends)
    images = [b.observation.images for b in blends]
    variance = [b.observation.variance for b in blends]
    coeffs = detect.get_detect_wavelets_batch(images, variance, scales=3, device=True)

    def batch():
        return detect.get_peaks_batch(coeffs)

    def loop():
        return [detect.get_peaks(c) for c in coeffs]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    got, want = batch(), loop()  # warm-up of both paths, and the comparison
    same = got == want
    t_batch, t_loop = [], []
    for _ in range(args.repeats):
        t_batch.append(timed(batch))
        t_loop.append(timed(loop))

    split = {}

    def clocked(name, fn):
        def run(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            split[name] = split.get(name, 0.0) + time.perf_counter() - t0
            return out
        return run

    steps = (("label_call_s", "label_batch_device"), ("fetch_call_s", "fetch_batch_device"))
    saved = [(f, getattr(detect_pybind11, f)) for _, f in steps]
    for name, f in steps:
        setattr(detect_pybind11, f, clocked(name, getattr(detect_pybind11, f)))
    stats = []
    plain = detect_pybind11.get_footprints_batch
    detect.get_footprints_batch = lambda *a, **k: plain(*a, _stats=stats, **k)
    try:
        total = timed(batch)
    finally:
        detect.get_footprints_batch = plain
        for f, fn in saved:
            setattr(detect_pybind11, f, fn)
    split["host_assembly_s"] = total - sum(split.values())

    shapes = sorted({tuple(c.shape[1:]) for c in coeffs}, key=lambda s: s[0] * s[1])
    print(json.dumps(dict(
        metric="detect_peaks_batch_seconds", blends=len(blends), frame_shapes=len(shapes),
        smallest_frame=list(shapes[0]), largest_frame=list(shapes[-1]),
        peaks=sum(len(p) for p in got), device_chunks=len(stats),
        launches=sum(a[0] + b[0] for a, b in stats),
        synchronisations=sum(a[1] + b[1] for a, b in stats), repeats=args.repeats,
        batch_min_max_s=[round(min(t_batch), 4), round(max(t_batch), 4)],
        loop_min_max_s=[round(min(t_loop), 4), round(max(t_loop), 4)],
        speedup_fastest=round(min(t_loop) / min(t_batch), 1),
        batch_not_slower=min(t_batch) <= min(t_loop),
        split_s={k: round(v, 4) for k, v in split.items()},
        identical_to_loop=same)))


if __name__ == "__main__":
    main()
