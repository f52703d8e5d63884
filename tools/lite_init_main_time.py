"""Seconds ``scarlet_amd.lite.init_blends_main`` takes to initialise a catalogue of lite blends
the way scarlet main does, against the per-blend loop
``[init_all_sources_main(o, c) for o, c in ...]`` and against the 50-iteration fit of the
same catalogue (``fit_blends(..., reweight=False)``).  Prints one JSON line.

    python tools/lite_init_main_time.py --blends 256 [--loop-blends 16] [--repeats 3]

The blends are those of ``tools/lite_batch_time.py``: each blend's observation, and the
centres of its sources.  Both paths compute their own detection images (``detect=None``) and
return host arrays, so each call ends with the device idle: the host clock around them is the
time a caller waits.  The loop is timed on the first
``--loop-blends`` blends and scaled per blend (its time per blend does not depend on how many
there are); every timing is the median of ``--repeats`` runs after a warm-up run of the same
shapes.  ``launches``: the kernel launches of the batch's last chunk, which do not depend on
the number of blends or sources; ``split_s``: the seconds of one batch call inside the device
steps up to the sweep's results (packing, uploads, five launches, the download), the host's
decisions on class and box, the cut-outs and the joint fits (three launches and the download,
which waits for them), and the assembly of the sources.  ``identical_to_loop``: boxes, morphologies, dtypes and the spectra of PSF and
single-component sources equal bit for bit on the blends both ran; ``joint_sed_rel_diff`` is
the largest difference of a jointly fitted spectrum, relative to the spectrum's largest value
(the loop fits it through a float32 FFT convolution, the batch in float64).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lite_batch_time import CROPS, make_blends  # noqa: E402
from lite_init_time import compare, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop-blends", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e-rel", type=float, default=1e-9)
    ap.add_argument("--min-snr", type=float, default=50)
    args = ap.parse_args()

    import torch

    from scarlet_amd import _catalog, lite
    from scarlet_amd.lite import initialization

    assert torch.cuda.is_available(), "needs a GPU"
    warm = make_blends(len(CROPS), seed0=1)
    lite.fit_blends(warm, 2, e_rel=args.e_rel, resize=10, reweight=False)

    blends = make_blends(args.blends)
    observations = [b.observation for b in blends]
    centers = [[tuple(int(v) for v in s.center) for s in b.sources] for b in blends]
    t0 = time.perf_counter()
    lite.fit_blends(blends, args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_fit = time.perf_counter() - t0

    def batch(obs=observations, cs=centers):
        return lite.init_blends_main(obs, cs, min_snr=args.min_snr)

    n_loop = min(args.loop_blends, len(blends))

    def loop():
        return [lite.init_all_sources_main(o, c, min_snr=args.min_snr)
                for o, c in zip(observations[:n_loop], centers[:n_loop])]

    groups, fallback = lite.plan_init_blends_main(observations, centers)
    # warm-up of both paths on the shapes they are timed on, and the comparison
    got, want = batch(), loop()
    same, differ, joint_diff = compare(got[:n_loop], want, observations, centers, args.min_snr)
    kinds = {}
    for ss in got:
        for s in ss:
            k = len(s.components)
            kinds[k] = kinds.get(k, 0) + 1

    t_batch = timed(batch, args.repeats)
    t_loop = timed(loop, args.repeats)
    launches = list(_catalog.Launcher.last.launches)
    # one more batch call with clocks inside: the device steps up to the host's decisions (the
    # sweep's download ends with the device idle), the decisions, the rest of the launches with
    # their download, the assembly
    split = {}
    saved_launches, saved_assemble = initialization._main_launches, initialization._main_assemble

    def clocked_launches(ch, key, blends_, opts):
        real_cpu, real_call = ch.torch.Tensor.cpu, type(ch).call
        marks, crop_at = [], []

        def call(self, entry, *a, **k):
            if k.get("tag") == "crop":
                crop_at.append(time.perf_counter())
            return real_call(self, entry, *a, **k)

        def cpu(self, *a, **k):
            out = real_cpu(self, *a, **k)
            marks.append(time.perf_counter())
            return out

        t0 = time.perf_counter()
        ch.torch.Tensor.cpu, type(ch).call = cpu, call
        try:
            out = saved_launches(ch, key, blends_, opts)
        finally:
            ch.torch.Tensor.cpu, type(ch).call = real_cpu, real_call
        t1 = time.perf_counter()
        # the first five downloads bring the SNR sums, the taps and the sweep's results
        for name, dt in (("device_steps_s", marks[4] - t0), ("host_decisions_s", crop_at[0] - marks[4]),
                         ("cutouts_and_fits_s", t1 - crop_at[0])):
            split[name] = split.get(name, 0.0) + dt
        return out

    def clocked_assemble(*a, **k):
        t0 = time.perf_counter()
        out = saved_assemble(*a, **k)
        split["assembly_s"] = split.get("assembly_s", 0.0) + time.perf_counter() - t0
        return out

    initialization._main_launches, initialization._main_assemble = clocked_launches, clocked_assemble
    try:
        batch()
    finally:
        initialization._main_launches, initialization._main_assemble = saved_launches, saved_assemble
    loop_scaled = t_loop[0] / n_loop * len(blends)
    print(json.dumps(dict(
        metric="lite_init_blends_main_seconds", blends=len(blends), iters=args.iters,
        sources=sum(len(c) for c in centers), components_per_source=kinds,
        bands=int(observations[0].images.shape[0]),
        stamp=list(observations[0].diff_kernel.image.shape[1:]),
        frame_shapes=len({o.images.shape for o in observations}),
        device_groups=len(groups), fallback_blends=len(fallback), repeats=args.repeats,
        launches_per_chunk=len(launches), launches=launches,
        init_blends_main_s=round(t_batch[0], 4),
        init_blends_main_min_max_s=[round(t_batch[1], 4), round(t_batch[2], 4)],
        loop_blends=n_loop, loop_s=round(t_loop[0], 4),
        loop_min_max_s=[round(t_loop[1], 4), round(t_loop[2], 4)],
        loop_scaled_s=round(loop_scaled, 3), speedup=round(loop_scaled / t_batch[0], 1),
        fit_blends_s=round(t_fit, 3),
        init_share_of_fit_loop=round(loop_scaled / t_fit, 2),
        init_share_of_fit_batch=round(t_batch[0] / t_fit, 3),
        split_s={k: round(v, 4) for k, v in split.items()},
        identical_to_loop=same, differing=differ, joint_sed_rel_diff=float("%.3g" % joint_diff))))


if __name__ == "__main__":
    main()
