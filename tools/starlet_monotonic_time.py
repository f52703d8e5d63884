"""Time the iterations of a batch of blends with monotonic starlet sources against the same
batch with thresholded ones.

    python tools/starlet_monotonic_time.py [--blends 64] [--iters 20] [--repeats 5]
                                           [--mode both|monotonic|thresholded]

Every blend is the fixture scene of ``tests/golden/starlet_source.npz`` on the observation of
``tests/golden/hsc_cosmos_35.npz``: five extended sources, sources 0 and 2 as starlet sources
(5 planes of 41 x 41) and the full-frame starlet source (5 planes of 58 x 48).  Spectra are
scaled per blend so that the blends differ.  The batch goes through ``BlendBatch.step`` (no
resizing, no host hook), so the time is that of the device loop.  Prints one JSON line: per mode
the milliseconds per iteration of the whole batch (median of the repeats after one warm-up) and
the ratio.  Under ``rocprofv3 --kernel-trace --stats`` (with ``--mode monotonic`` or
``--mode thresholded``: one mode per run) the per-launch times of ``starlet_step_kernel<true>`` /
``<false>`` stand next to those of the other kernels of the iteration."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def specs_of(amd, g, scale, monotonic):
    starlet = set(int(k) for k in g["starlet_of"])
    specs = []
    for k in range(int(g["n_sources"])):
        kw = dict(sed_min_step=g["sed_step_minimum_%d" % k],
                  sed_rel_step=float(g["sed_step_factor_%d" % k]))
        if float(g["sed_zero_%d" % k]) != 1e-20:
            kw["sed_floor"] = float(g["sed_zero_%d" % k])
        sed = g["sed_%d" % k] * scale
        if k in starlet:
            coeffs = g["coeffs_%d" % k]
            rule = amd.MonotonicPlanes(1, 0.0, 3) if monotonic else g["thresh_%d" % k]
            specs.append(amd.ComponentSpec(sed, np.zeros(coeffs.shape[1:]), g["origin_%d" % k],
                                           morph_step=1e-2, prox_flags=0, starlet=(coeffs, rule),
                                           **kw))
        else:
            specs.append(amd.ComponentSpec(sed, g["morph_%d" % k], g["origin_%d" % k], **kw))
    return specs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "monotonic", "thresholded"), default="both")
    args = ap.parse_args()
    import scarlet_amd as amd

    golden = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(golden, "starlet_source.npz"))
    hsc = np.load(os.path.join(golden, "hsc_cosmos_35.npz"))
    scales = 1 + 0.3 * np.sin(np.arange(args.blends))
    images = np.stack([hsc["images"]] * args.blends)
    weights = np.stack([hsc["weights"]] * args.blends)

    def run(monotonic):
        batch = amd.BlendBatch(images, weights, [specs_of(amd, g, s, monotonic) for s in scales],
                               kernel=hsc["diff_kernel"], max_iter=args.iters)
        batch.states()  # (everything uploaded and the queue empty)
        t0 = time.perf_counter()
        batch.step(0, args.iters, e_rel=1e-3)
        states = batch.states()  # synchronises
        seconds = time.perf_counter() - t0
        assert np.all(states == 0), states
        batch.close()
        return seconds

    out = dict(tool="starlet_monotonic_time", blends=args.blends, iterations=args.iters,
               starlet_components_per_blend=len(g["starlet_of"]))
    modes = ("monotonic", "thresholded") if args.mode == "both" else (args.mode,)
    for mode in modes:
        run(mode == "monotonic")  # warm-up: library load, plans, LDS configuration
        times = [run(mode == "monotonic") for _ in range(args.repeats)]
        out[mode + "_ms_per_iteration"] = 1e3 * float(np.median(times)) / args.iters
        out[mode + "_all_ms"] = [1e3 * t / args.iters for t in times]
    if len(modes) == 2:
        out["ratio"] = out["monotonic_ms_per_iteration"] / out["thresholded_ms_per_iteration"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
