"""Seconds ``scarlet_amd.init_blends`` takes to initialise a catalogue of main-API blends,
against the per-blend loop ``[init_all_sources(f, c, o) for ...]`` and against
``fit_blends(100)`` of the same catalogue in the same process.  Prints one JSON document.

    python tools/init_blends_time.py [--blends 256] [--loop-blends 16] [--repeats 3] [--out F]

The scenes are those of ``tools/init_time.py:synthetic_scene`` (``synthetic.make_blend``:
5 x 128 x 128, ten sources).  ``init_blends`` is the median of ``--repeats`` runs after a warm-up
on the same shapes; the loop is timed on the first ``--loop-blends`` scenes and scaled per blend.
``split_s``: the seconds of one ``init_blends`` call by step -- packing on the host (the
detection cubes and pixel spectra), the uploads with psf_snr and sweep and their download, the
host's decisions with the crop launch and its download, the assembly of the source objects,
the spectra (packing, uploads, the two launches, the download and the K x K solves), and the
blends the loop took.  ``identical_to_loop``: classes, boxes, centres and morphologies equal bit
for bit on the scenes both ran; ``spectra_max_rel_diff``: the largest difference of a spectrum
from the loop's, relative to the component's largest band."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from init_time import synthetic_scene  # noqa: E402


def scenes(n, seed0=1234):
    made = [synthetic_scene(seed0 + i) for i in range(n)]
    return [m[0] for m in made], [m[2] for m in made], [m[1] for m in made], made[0][3]


def compare(a, b):
    """Raise AssertionError unless two results ``(sources, skipped)`` have the same classes,
    boxes, centres and morphology bits; returns the largest relative spectrum difference."""
    import scarlet_amd as scarlet

    (sa, ka), (sb, kb) = a, b
    assert list(ka) == list(kb), "skipped"
    assert [type(s) for s in sa] == [type(s) for s in sb], "classes"
    worst = 0.0
    for s, t in zip(sa, sb):
        assert np.array_equal(np.asarray(s.center), np.asarray(t.center)), "centre"
        cs = s.children if isinstance(s, scarlet.CombinedComponent) else [s]
        ct = t.children if isinstance(t, scarlet.CombinedComponent) else [t]
        assert len(cs) == len(ct), "components"
        for c, d in zip(cs, ct):
            assert c.bbox == d.bbox, "box"
            mc, md = (np.asarray(x.children[1].parameters[0]) for x in (c, d))
            assert mc.dtype == md.dtype and np.array_equal(mc, md), "morphology"
            qc, qd = (np.asarray(x.children[0].parameters[0], np.float64) for x in (c, d))
            worst = max(worst, float(np.abs(qc - qd).max() / np.abs(qd).max()))
    return worst


def timed(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--loop-blends", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fit-iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import scarlet_amd as scarlet
    from scarlet_amd import initialization as init

    assert torch.cuda.is_available(), "needs a GPU"
    frames, centers, observations, kw = scenes(args.blends)
    opts = dict(kw, fallback=True, silent=True, set_spectra=True)
    n_loop = min(args.loop_blends, args.blends)

    report = {}

    def batch():
        report.clear()
        return init.init_blends(frames, centers, observations, _report=report, **opts)

    def loop():
        return [init.init_all_sources(f, c, o, **opts)
                for f, c, o in zip(frames[:n_loop], centers[:n_loop], observations[:n_loop])]

    groups, fallback = init.plan_init_blends(frames, centers, observations, **opts)
    got, want = batch(), loop()  # warm-up of both paths, and the comparison
    identical, differing, spectra_diff = True, [], 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        try:
            spectra_diff = max(spectra_diff, compare(a, b))
        except AssertionError as exc:
            identical = False
            differing.append((i, str(exc)[:200]))
    t_batch = timed(batch, args.repeats)
    times = dict(report["times"])  # (of the last timed call)
    launches = list(report["launches"])
    fallback = report["fallback"]
    t_loop = timed(loop, args.repeats)
    results = batch()
    blends = [scarlet.Blend(sources, obs) for (sources, _), obs in zip(results, observations)]
    t0 = time.perf_counter()
    fitted = scarlet.fit_blends(blends, args.fit_iters, e_rel=1e-4)
    t_fit = time.perf_counter() - t0
    loop_scaled = t_loop[0] / n_loop * args.blends
    total = sum(times.values()) or 1.0
    out = dict(
        metric="init_blends_seconds", blends=args.blends, frame=list(frames[0].shape),
        sources=sum(len(c) for c in centers), device_groups=len(groups),
        fallback_blends=len(fallback), repeats=args.repeats,
        launches_per_chunk=len(launches), launches=launches,
        init_blends_s=round(t_batch[0], 4),
        init_blends_min_max_s=[round(t_batch[1], 4), round(t_batch[2], 4)],
        loop_blends=n_loop, loop_s=round(t_loop[0], 4),
        loop_min_max_s=[round(t_loop[1], 4), round(t_loop[2], 4)],
        loop_scaled_s=round(loop_scaled, 3), speedup=round(loop_scaled / t_batch[0], 2),
        fit_blends_s=round(t_fit, 3), fit_iters=args.fit_iters,
        fit_iterations_mean=round(float(np.mean([n for n, _ in fitted])), 1),
        init_share_of_fit_loop=round(loop_scaled / t_fit, 2),
        init_share_of_fit_batch=round(t_batch[0] / t_fit, 2),
        split_s={k: round(v, 4) for k, v in times.items()},
        split_share={k: round(v / total, 3) for k, v in times.items()},
        identical_to_loop=identical, differing=differing[:5],
        spectra_max_rel_diff=float("%.3g" % spectra_diff))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
