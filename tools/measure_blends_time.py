"""Seconds ``scarlet_amd.measure_blends`` takes to turn a fitted catalogue of main-API blends into
its tables, against the per-source loop of ``measure.flux``, ``centroid``, ``max_pixel`` and
``snr``, and beside ``fit_blends`` of the same catalogue in the same process.  Prints one JSON
document.

    python tools/measure_blends_time.py [--blends 256] [--loop-blends 16] [--repeats 3] [--out F]

The scenes are those of ``tools/init_time.py:synthetic_scene`` (``synthetic.make_blend``:
5 x 128 x 128, ten sources, 41 x 41 stamp), initialised by ``init_blends`` and fitted once.
``measure_blends`` is the median of ``--repeats`` runs after a warm-up on the same shapes; the
loop is timed on the first ``--loop-blends`` blends and scaled per blend.  ``launch_ms``: the
device time of the model, render and reduce launches between events around them
(``smi_measure_sources_last_launch_ms``), summed over the chunks of the last timed call;
``split_s``: the host's seconds of that call by step (the plan with the flattening of the
sources, the packing, the C call with uploads, launches and downloads, the tables, the blends the
per-source functions took).  ``snr_max_rel_diff``: the largest relative difference of ``snr``
from the loop's ``measure.snr``, which renders in float32 through the FFT, on the blends both
ran; ``flux_max_rel_diff`` likewise; ``peaks_equal``: every ``max_pixel`` is the table's."""
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


def loop_rows(blends):
    """The per-source loop a caller wrote for a catalogue before ``measure_blends``."""
    from scarlet_amd import measure

    return [[(measure.flux(s), measure.centroid(s), measure.max_pixel(s),
              measure.snr(s, b.observations)) for s in b.sources] for b in blends]


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
    from scarlet_amd import measure

    assert torch.cuda.is_available(), "needs a GPU"
    frames, centers, observations, kw = scenes(args.blends)
    results = init.init_blends(frames, centers, observations,
                               **dict(kw, fallback=True, silent=True, set_spectra=True))
    blends = [scarlet.Blend(sources, obs) for (sources, _), obs in zip(results, observations)]
    t0 = time.perf_counter()
    fitted = scarlet.fit_blends(blends, args.fit_iters, e_rel=1e-4)
    t_fit = time.perf_counter() - t0
    n_loop = min(args.loop_blends, args.blends)

    # device milliseconds of the three launches, summed over the chunks of a call
    launch_ms = np.zeros(3)
    run_chunk = measure._run_chunk

    def counted(*a, **k):
        out = run_chunk(*a, **k)
        launch_ms[:] += measure.last_launch_ms()
        return out

    measure._run_chunk = counted
    report = {}

    def batch():
        report.clear()
        launch_ms[:] = 0
        return scarlet.measure_blends(blends, _report=report)

    groups, refused = scarlet.plan_measure_blends(blends)
    tables, rows = batch(), loop_rows(blends[:n_loop])  # warm-up of both paths, the comparison
    snr_diff = flux_diff = centroid_diff = 0.0
    peaks_equal = True
    for table, blend_rows in zip(tables, rows):
        for row, (flux, centre, peak, snr) in zip(table, blend_rows):
            snr_diff = max(snr_diff, abs(row["snr"] - snr) / abs(snr))
            flux_diff = max(flux_diff, float((np.abs(row["flux"] - flux) / np.abs(flux)).max()))
            centroid_diff = max(centroid_diff, float(np.abs(row["centroid"] - centre).max()))
            peaks_equal &= tuple(row["peak"]) == tuple(peak)
    t_batch = timed(batch, args.repeats)
    times = dict(report["times"])  # (of the last timed call)
    launches = launch_ms.copy()
    t_loop = timed(lambda: loop_rows(blends[:n_loop]), args.repeats)
    loop_scaled = t_loop[0] / n_loop * args.blends
    renderer = blends[0].observations[0].renderer
    out = dict(
        metric="measure_blends_seconds", blends=args.blends, frame=list(frames[0].shape),
        stamp=list(np.shape(renderer.diff_kernel.image)[1:]),
        sources=sum(len(b.sources) for b in blends), device_groups=len(groups),
        fallback_blends=len(report["fallback"]), repeats=args.repeats,
        launches_per_chunk=report.get("launches", 0),
        measure_blends_s=round(t_batch[0], 4),
        measure_blends_min_max_s=[round(t_batch[1], 4), round(t_batch[2], 4)],
        launch_ms=dict(zip(("model", "render", "reduce"), (round(float(v), 3) for v in launches))),
        launch_share=round(float(launches.sum()) * 1e-3 / t_batch[0], 3),
        split_s={k: round(v, 4) for k, v in times.items()},
        loop_blends=n_loop, loop_s=round(t_loop[0], 4),
        loop_min_max_s=[round(t_loop[1], 4), round(t_loop[2], 4)],
        loop_scaled_s=round(loop_scaled, 3), speedup=round(loop_scaled / t_batch[0], 1),
        fit_blends_s=round(t_fit, 3), fit_iters=args.fit_iters,
        fit_iterations_mean=round(float(np.mean([n for n, _ in fitted])), 1),
        loop_share_of_fit=round(loop_scaled / t_fit, 2),
        measure_blends_share_of_fit=round(t_batch[0] / t_fit, 3),
        snr_max_rel_diff=float("%.3g" % snr_diff), flux_max_rel_diff=float("%.3g" % flux_diff),
        centroid_max_abs_diff=float("%.3g" % centroid_diff), peaks_equal=bool(peaks_equal))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
