"""Seconds ``scarlet_amd.render_blends`` takes to turn a fitted catalogue of main-API blends into
its images -- with defaults (scene, residual, chi^2), with ``sources=True`` and with
``reweight=True`` --, against the host loop of ``Observation.render`` calls
(``rendering.render_blend_host``), and beside ``fit_blends`` of the same catalogue in the same
process.  Prints one JSON document.

    python tools/render_blends_time.py [--blends 256] [--loop-blends 16] [--repeats 3] [--out F]

The scenes are those of ``tools/measure_blends_time.py`` (``synthetic.make_blend``: 5 x 128 x 128,
ten sources, 41 x 41 stamp), initialised by ``init_blends`` and fitted once.  Every mode of
``render_blends`` is the median of ``--repeats`` runs after a warm-up on the same shapes; the loop
is timed on the first ``--loop-blends`` blends, once without and once with the sources and
fluxes, and scaled per blend.  ``launch_ms``: the device time of the scene, sources and reduce
launches between events around them, summed over the chunks of the last timed call;
``split_s``: the host's seconds of that call by step (the plan with the flattening of the
sources, the packing, the C call with uploads, launches and downloads, the result dicts, the
blends the loop took).  ``max_diff_from_loop``: the largest difference of a scene, of a source's
rendering and of a flux from the loop's, which renders in float32 through the FFT, relative to
the largest value of the loop's image, on the blends both ran; ``flux_lit``: the same for the
flux on the pixels where the loop's scene exceeds 1e-4 of its largest value -- below that the
loop's ratio divides the rounding noise of two float32 FFTs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from init_blends_time import scenes, timed  # noqa: E402

MODES = (("default", {}), ("sources", dict(sources=True)), ("reweight", dict(reweight=True)))


def _rel(a, b):
    scale = float(np.abs(b).max()) if np.size(b) else 0.0
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / scale if scale else 0.0


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
    from scarlet_amd import rendering

    assert torch.cuda.is_available(), "needs a GPU"
    frames, centers, observations, kw = scenes(args.blends)
    results = init.init_blends(frames, centers, observations,
                               **dict(kw, fallback=True, silent=True, set_spectra=True))
    blends = [scarlet.Blend(sources, obs) for (sources, _), obs in zip(results, observations)]
    t0 = time.perf_counter()
    fitted = scarlet.fit_blends(blends, args.fit_iters, e_rel=1e-4)
    t_fit = time.perf_counter() - t0
    n_loop = min(args.loop_blends, args.blends)
    groups, refused = scarlet.plan_render_blends(blends)

    def loop(**options):
        return [rendering.render_blend_host(b, **options) for b in blends[:n_loop]]

    modes = {}
    for name, options in MODES:
        report = {}

        def batch():
            report.clear()
            return scarlet.render_blends(blends, _report=report, **options)

        got = batch()  # warm-up
        t = timed(batch, args.repeats)
        modes[name] = dict(
            seconds=round(t[0], 4), min_max_s=[round(t[1], 4), round(t[2], 4)],
            chunks=report["chunks"], fallback_blends=len(report["fallback"]),
            launch_ms=dict(zip(("scene", "sources", "reduce"),
                               (round(float(v), 3) for v in report["launch_ms"]))),
            launch_share=round(sum(report["launch_ms"]) * 1e-3 / t[0], 3),
            split_s={k: round(v, 4) for k, v in report["times"].items()},
            share_of_fit=round(t[0] / t_fit, 3))
    want = loop(reweight=True)  # warm-up of the loop, and the comparison with the last mode
    diff = dict(rendered=0.0, source_rendered=0.0, flux=0.0, flux_lit=0.0, log_likelihood=0.0)
    for a, b in zip(got, want):
        diff["rendered"] = max([diff["rendered"]] + [_rel(x, y) for x, y in
                                                     zip(a["rendered"], b["rendered"])])
        diff["log_likelihood"] = max(diff["log_likelihood"],
                                     abs(a["log_likelihood"] - b["log_likelihood"])
                                     / abs(b["log_likelihood"]))
        for s, t in zip(a["sources"], b["sources"]):
            assert s["region"] == t["region"]
            for key, field in (("source_rendered", "rendered"), ("flux", "flux")):
                diff[key] = max([diff[key]] + [_rel(x, y) for x, y in zip(s[field], t[field])])
            y0, x0, h, w = t["region"]
            for x, y, R in zip(s["flux"], t["flux"], b["rendered"]):
                lit = R[:, y0:y0 + h, x0:x0 + w] > 1e-4 * np.abs(R).max()
                scale = float(np.abs(y).max())
                if lit.any() and scale:
                    off = float(np.abs(x.astype(np.float64) - y)[lit].max())
                    diff["flux_lit"] = max(diff["flux_lit"], off / scale)
    t_scene = timed(loop, args.repeats)
    t_full = timed(lambda: loop(reweight=True), args.repeats)
    scaled = dict(default=t_scene[0] / n_loop * args.blends,
                  reweight=t_full[0] / n_loop * args.blends)
    renderer = blends[0].observations[0].renderer
    out = dict(
        metric="render_blends_seconds", blends=args.blends, frame=list(frames[0].shape),
        stamp=list(np.shape(renderer.diff_kernel.image)[1:]),
        sources=sum(len(b.sources) for b in blends), device_groups=len(groups),
        refused_blends=len(refused), repeats=args.repeats, launches_per_chunk=3,
        render_blends=modes, loop_blends=n_loop,
        loop_s=dict(default=round(t_scene[0], 4), reweight=round(t_full[0], 4)),
        loop_min_max_s=dict(default=[round(t_scene[1], 4), round(t_scene[2], 4)],
                            reweight=[round(t_full[1], 4), round(t_full[2], 4)]),
        loop_scaled_s={k: round(v, 3) for k, v in scaled.items()},
        speedup=dict(default=round(scaled["default"] / modes["default"]["seconds"], 1),
                     reweight=round(scaled["reweight"] / modes["reweight"]["seconds"], 1)),
        fit_blends_s=round(t_fit, 3), fit_iters=args.fit_iters,
        fit_iterations_mean=round(float(np.mean([n for n, _ in fitted])), 1),
        loop_share_of_fit={k: round(v / t_fit, 2) for k, v in scaled.items()},
        max_diff_from_loop={k: float("%.3g" % v) for k, v in diff.items()})
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
