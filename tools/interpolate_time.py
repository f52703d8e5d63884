"""Seconds ``scarlet_amd.interpolation.interpolate_observations`` takes for a catalogue of
observations, with and without ``wave_filter``, against the same products in NumPy on the host.
Prints one JSON line.

    python tools/interpolate_time.py [--blends 256] [--bands 5] [--size 64] [--frame 128]
                                     [--parent DIR]

Every call returns host arrays, so it ends with the device idle; the median of ``--repeats``
calls after a warm-up.  Baselines: for the plain case ``Sy @ X @ Sx.T`` per band in NumPy
(float64, the matrices formed once per blend, as the device path forms them); for
``wave_filter=True`` the host loop around device calls that ``apply_wavelet_denoising`` was
(``tools/denoise_time.py``: in a process of its own, the tree ``--parent`` if given, timed on
``--baseline-images`` bands and scaled to all of them) followed by those products.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import denoise_time  # noqa: E402


class Grid:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Scene(Grid):
    """an observation on a grid ``scale`` times coarser than the frame's"""

    def __init__(self, data, scale, offset):
        super().__init__(data.shape)
        self.data, self.scale, self.offset = data, scale, offset

    def convert_pixel_to(self, target, pixel=None):
        import numpy as np

        return np.asarray(pixel, dtype=np.float64) * self.scale + self.offset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--frame", type=int, default=128)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-images", type=int, default=16)
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from scarlet_amd import interpolation

    assert torch.cuda.is_available(), "needs a GPU"
    bands = denoise_time.make_images(args.blends * args.bands, args.size)
    scale = args.frame / args.size
    scenes = [Scene(np.stack(bands[k * args.bands:(k + 1) * args.bands]), scale, 0.25 * (k % 4))
              for k in range(args.blends)]
    frames = [Grid((args.bands, args.frame, args.frame))] * args.blends

    def host_products():
        out = []
        for obs, frame in zip(scenes, frames):
            sy, sx = interpolation.sinc_matrices(*interpolation.observation_grid(obs, frame),
                                                 frame.shape[1:])
            out.append(np.stack([sy @ band.astype(np.float64) @ sx.T for band in obs.data]))
        return out

    result = dict(metric="interpolate_observations_seconds", blends=args.blends,
                  bands=args.bands, observation=[args.size] * 2, frame=[args.frame] * 2,
                  repeats=args.repeats)
    want = host_products()
    for wave_filter in (False, True):
        def run():
            return interpolation.interpolate_observations(scenes, frames, wave_filter=wave_filter)
        got = run()  # warm-up
        times = denoise_time.timed(run, args.repeats)
        tag = "wave_filter" if wave_filter else "plain"
        result[tag + "_s"] = round(statistics.median(times), 4)
        result[tag + "_min_max_s"] = [round(min(times), 4), round(max(times), 4)]
        if not wave_filter:
            result["plain_max_error_vs_numpy"] = float(max(np.abs(g - w).max()
                                                           for g, w in zip(got, want)))
    t_host = statistics.median(denoise_time.timed(host_products, args.repeats))
    result["numpy_products_s"] = round(t_host, 4)
    result["plain_speedup"] = round(t_host / result["plain_s"], 1)
    base = denoise_time.baseline(args, os.path.abspath(args.parent) if args.parent else ROOT,
                                 args.parent is not None)
    scaled = base["list_s"] * len(bands) / args.baseline_images
    result["denoise_baseline"] = ("parent commit" if args.parent
                                  else "this tree's loop over the public functions")
    result["denoise_baseline_scaled_s"] = round(scaled, 4)
    result["wave_filter_baseline_s"] = round(scaled + t_host, 4)
    result["wave_filter_speedup"] = round((scaled + t_host) / result["wave_filter_s"], 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
