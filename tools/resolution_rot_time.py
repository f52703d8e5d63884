"""Device time of the rotated resampler (path 2, scarlet_amd/csrc/resample_rot.hip) at the size
of the multi-resolution tutorial: a 100 x 100 model frame and five bands of 36 x 36
low-resolution pixels on a grid turned by 0.3 rad.

    python tools/resolution_rot_time.py [--out profiles/resolution_rot_time.json]

Timed with device events around back-to-back calls on resident arrays, no host transfers
(``smi_resampler_time`` for the rendering, ``smi_resampler_time_adjoint`` for the transpose),
several windows each.  Beside it, in the same process and alternating with it, the unrotated
spectral path (path 1) on the same shapes at angle 0, for scale: that is existing code, not the
code under test.  Needs a GPU; there is no pass mark.

What the rotated rendering needs, from the shapes: ``C n_a n_b Fy Kx`` complex terms (8 flop
each) and one read of ``E`` (``C n_a Fy Kx`` complex float32).  The JSON names, for each, the time
the hardware would need at its peak, and which of the two the measured time is closer to.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_GBS = 8000.0           # HBM3E peak of the MI355X, AMD's published specification
FP64_VECTOR_TFLOPS = 78.6  # peak FP64 vector rate of the MI355X, AMD's published specification

FRAME, BANDS, SIDE, ANGLE = (100, 100), 5, 36, 0.3


def renderer(scarlet, cases, angle):
    channels = ["hr"] + ["lr_%d" % c for c in range(BANDS)]
    wcs = cases.linear_wcs(*cases.wcs_params(FRAME, cases.HR_SCALE), FRAME)
    frame = scarlet.Frame((len(channels),) + FRAME, wcs=wcs, psf=scarlet.GaussianPSF(sigma=0.8),
                          channels=channels)
    rng = np.random.RandomState(5)
    obs = scarlet.Observation(
        cases.image(rng, BANDS, (SIDE, SIDE), 2),
        wcs=cases.linear_wcs(*cases.wcs_params((SIDE, SIDE), cases.LR_SCALE, angle, (0.3, -0.2)),
                             (SIDE, SIDE)),
        psf=scarlet.ImagePSF(cases.gaussian_psf(9, 1.3, BANDS)), channels=channels[1:])
    obs.match(frame)
    model = rng.normal(0, 1, frame.shape).astype(np.float32)
    obs.render(model)  # the model is resident from here on
    return obs.renderer


def windows(lib, _lib, fn, handle, n_rep, n_windows):
    out = []
    for _ in range(n_windows):
        t = ctypes.c_double()
        _lib.check(fn(handle, n_rep, ctypes.byref(t)))
        out.append(t.value * 1e3)  # us
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolution_rot_time.json"))
    parser.add_argument("--reps", type=int, default=2000)
    parser.add_argument("--windows", type=int, default=5)
    args = parser.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU (no CPU fallback)"
    import resolution_rot_cases as cases
    import scarlet_amd as scarlet
    from scarlet_amd import _lib

    lib = _lib.load()
    rot, flat = renderer(scarlet, cases, ANGLE), renderer(scarlet, cases, 0.0)
    assert rot.device_path() == 2 and flat.device_path() == 1
    assert rot.shape_class() == flat.shape_class()
    C, n_a, n_b, Fy, Fx = rot.shape_class()
    Kx = Fx // 2 + 1
    times = {"rotated": {"render": [], "adjoint": []}, "spectral": {"render": [], "adjoint": []}}
    for _ in range(args.windows):  # alternating, so that both see the same neighbours
        for tag, r in (("rotated", rot), ("spectral", flat)):
            handle = r._resampler()[1]
            times[tag]["render"] += windows(lib, _lib, lib.smi_resampler_time, handle, args.reps, 1)
            times[tag]["adjoint"] += windows(lib, _lib, lib.smi_resampler_time_adjoint, handle,
                                             args.reps, 1)

    def summary(v):
        return dict(median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2),
                    max_us=round(max(v), 2), windows_us=[round(x, 2) for x in v])

    flops = 8.0 * C * n_a * n_b * Fy * Kx
    e_bytes = 8.0 * C * n_a * Fy * Kx
    bytes_render = e_bytes + 8.0 * n_b * Fy * Kx + 4.0 * C * Fy * Fx + 4.0 * C * n_a * n_b
    t_flops, t_bytes = flops / (FP64_VECTOR_TFLOPS * 1e12) * 1e6, bytes_render / (HBM_GBS * 1e9) * 1e6
    measured = float(np.median(times["rotated"]["render"]))
    result = {
        "what": "device time per call of the rotated resampler (path 2) and, for scale, of the "
                "unrotated spectral path (path 1, existing code) on the same shapes",
        "shape": dict(frame=FRAME, bands=C, n_a=n_a, n_b=n_b, Fy=Fy, Fx=Fx, Kx=Kx,
                      angle_rad=ANGLE),
        "measured": "HIP events around %d back-to-back calls on resident arrays, %d windows per "
                    "entry, rotated and spectral alternating in one process" % (args.reps,
                                                                               args.windows),
        "device": "MI355X",
        "device_name_reported": torch.cuda.get_device_name(0),
        "rotated": {k: summary(v) for k, v in times["rotated"].items()},
        "spectral_for_scale": {k: summary(v) for k, v in times["spectral"].items()},
        "rotated_render_needs": {
            "flops": flops, "bytes": bytes_render, "E_bytes": e_bytes,
            "at_fp64_vector_peak_us": round(t_flops, 2), "at_hbm_peak_us": round(t_bytes, 2),
            "peaks": {"fp64_vector_tflops": FP64_VECTOR_TFLOPS, "hbm_gbs": HBM_GBS},
            "achieved_gflops": round(flops / measured / 1e3, 1),
            "achieved_gbs": round(bytes_render / measured / 1e3, 1),
            "closer_to": "arithmetic" if abs(np.log(measured / t_flops)) < abs(
                np.log(measured / t_bytes)) else "the read of E",
        },
        "not_measured": "per-kernel times (no profiler run), the transpose's share of a fit "
                        "iteration, other sizes",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
