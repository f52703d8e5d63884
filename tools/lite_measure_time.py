"""Seconds ``scarlet_amd.lite.measure_blends`` takes to turn a fitted catalogue of lite blends
into its table of fluxes, centroids, moments, peaks and signal-to-noise, with and without the
flux cubes, against what there was before it: ``weight_blends`` followed by a loop over the
sources with ``scarlet_amd.measure`` (flux, centroid, max_pixel, moments; its ``snr`` does not
take a lite source, so the loop lacks that column and the model sums).  Prints one JSON line.

    python tools/lite_measure_time.py --blends 256 --iters 50 [--loop-blends 16] [--repeats 3]

The blends are those of ``tools/lite_reweight_time.py``, fitted once; all timings come from
one process.  Every call returns host arrays, so the host clock around it is the time a caller
waits.  The NumPy loop is timed on the first ``--loop-blends`` blends and scaled per blend;
every timing is the median of ``--repeats`` runs after a warm-up run of the same shapes.  The
share of the three launches is the device time between events around them
(``smi_lite_measure_last_launch_ms``), summed over the chunks of a call.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lite_batch_time import CROPS, make_blends  # noqa: E402
from lite_reweight_time import timed  # noqa: E402


def numpy_rows(blends):
    """The per-source loop a caller of ``weight_blends`` wrote for a catalogue."""
    from scarlet_amd import measure

    rows = []
    for b in blends:
        for s in b.sources:
            if s.is_null or s.flux.size == 0:
                rows.append(None)
                continue
            centre = measure.centroid(s.flux)
            rows.append((measure.flux(s.flux), centre, measure.max_pixel(s.flux),
                         measure.moments(s.flux, N=2, centroid=(centre[2], centre[1]))))
    return rows


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

    from scarlet_amd import _lib, lite
    from scarlet_amd.lite import catalog

    assert torch.cuda.is_available(), "needs a GPU"
    warm = make_blends(len(CROPS), seed0=1)
    lite.fit_blends(warm, 2, e_rel=args.e_rel, resize=10, reweight=False)
    blends = make_blends(args.blends)
    t0 = time.perf_counter()
    lite.fit_blends(blends, args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_fit = time.perf_counter() - t0

    groups, fallback = lite.plan_measure_blends(blends)
    loop = blends[:min(args.loop_blends, len(blends))]

    # device milliseconds of the launches, summed over the chunks of a call
    launch_ms = [0.0]
    run_chunk = catalog._run_chunk

    def counted(*a, **k):
        out = run_chunk(*a, **k)
        ms = ctypes.c_double()
        _lib.check(_lib.load().smi_lite_measure_last_launch_ms(ctypes.byref(ms)))
        launch_ms[0] += ms.value
        return out

    catalog._run_chunk = counted

    # warm-up, and the tables agree: with = without cubes, and the loop's numbers
    tables = lite.measure_blends(blends)
    kept = lite.measure_blends(blends, keep_flux=True)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(tables, kept))
    rows = iter(numpy_rows(loop))
    worst, peaks_equal = 0.0, True
    for table in tables[:len(loop)]:
        for row in table:
            want = next(rows)
            if want is None:
                continue
            flux, centre, peak, _ = want
            worst = max(worst, float(np.abs(row["flux"] - flux).max() / np.abs(flux).max()),
                        float(np.abs(row["centroid"] - centre[1:] - row["box"][:2]).max()))
            y0, x0 = row["box"][:2]
            peaks_equal &= (row["peak"][0], row["peak"][1] - y0, row["peak"][2] - x0) == tuple(peak)
    lite.weight_blends(blends)

    def with_launches(fn):
        shares = []

        def run():
            launch_ms[0] = 0.0
            t0 = time.perf_counter()
            fn()
            shares.append(launch_ms[0] * 1e-3 / (time.perf_counter() - t0))
        t = timed(run, args.repeats)
        return t, sorted(shares)[len(shares) // 2], launch_ms[0] * 1e-3

    t_plain, share_plain, launches_plain = with_launches(lambda: lite.measure_blends(blends))
    t_kept, share_kept, _ = with_launches(lambda: lite.measure_blends(blends, keep_flux=True))
    t_weight = timed(lambda: lite.weight_blends(blends), args.repeats)
    t_loop = timed(lambda: numpy_rows(loop), args.repeats)
    loop_scaled = t_loop[0] / len(loop) * len(blends)
    before = t_weight[0] + loop_scaled
    print(json.dumps(dict(
        metric="lite_measure_blends_seconds", blends=len(blends), iters=args.iters,
        sources=sum(len(b.sources) for b in blends),
        bands=int(blends[0].observation.images.shape[0]),
        stamp=list(blends[0].observation.diff_kernel.image.shape[1:]),
        device_groups=len(groups), fallback_blends=len(fallback), repeats=args.repeats,
        measure_blends_s=round(t_plain[0], 4),
        measure_blends_min_max_s=[round(t_plain[1], 4), round(t_plain[2], 4)],
        measure_blends_keep_flux_s=round(t_kept[0], 4),
        measure_blends_keep_flux_min_max_s=[round(t_kept[1], 4), round(t_kept[2], 4)],
        launches_s=round(launches_plain, 5), launch_share=round(share_plain, 3),
        launch_share_keep_flux=round(share_kept, 3),
        weight_blends_s=round(t_weight[0], 4),
        weight_blends_min_max_s=[round(t_weight[1], 4), round(t_weight[2], 4)],
        loop_blends=len(loop), numpy_loop_s=round(t_loop[0], 4),
        numpy_loop_scaled_s=round(loop_scaled, 3), weight_blends_plus_loop_s=round(before, 3),
        speedup_over_weight_blends_plus_loop=round(before / t_plain[0], 1),
        measure_over_weight_blends=round(t_plain[0] / t_weight[0], 2),
        fit_blends_s=round(t_fit, 3), measure_share_of_fit=round(t_plain[0] / t_fit, 3),
        tables_identical_with_and_without_cubes=bool(same),
        peaks_equal_to_loop=bool(peaks_equal), worst_deviation_from_float32_loop=worst)))


if __name__ == "__main__":
    main()
