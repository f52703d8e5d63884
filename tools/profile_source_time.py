"""Time a batch of blends with profile sources through ``fit_blends``.

    python tools/profile_source_time.py [--blends 64] [--iters 30] [--repeats 3]

Every blend is the quickstart scene (``tests/golden/hsc_cosmos_35.npz``) with its sources from
``init_all_sources(max_components=1)``; the first two become ``GaussianSource``s and the third a
``SpergelSource`` at the same catalogue positions, the rest stay ``ExtendedSource``s.  Spectra
are scaled per blend so that the blends differ.  Prints one JSON line: seconds per ``fit_blends``
call (median of the repeats after one warm-up call), iterations run, blends.  Under
``rocprofv3 --kernel-trace --stats`` the per-launch times of ``profile_step_kernel`` and of the
update kernels of the same batch stand side by side."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_blend(scarlet, hsc, scale):
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    centers = [tuple(c) for c in hsc["centers"]]
    sources, _ = scarlet.initialization.init_all_sources(
        frame, centers, obs, max_components=1, min_snr=50, thresh=1, fallback=True, silent=True,
        set_spectra=True)
    sources = list(sources)
    sources[0] = scarlet.GaussianSource(frame, centers[0], 1.5, np.zeros(2), obs)
    sources[1] = scarlet.GaussianSource(frame, centers[1], 2.3, np.array([0.2, -0.1]), obs)
    sources[2] = scarlet.SpergelSource(frame, centers[2], 0.5, 2.0, np.array([0.1, 0.05]), obs)
    for src in sources:
        for p in src.parameters:
            if p.name == "spectrum":
                p[...] *= scale
    return scarlet.Blend(sources, obs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import scarlet_amd as scarlet

    hsc = np.load(os.path.join(ROOT, "tests", "golden", "hsc_cosmos_35.npz"))
    scales = 1 + 0.3 * np.sin(np.arange(args.blends))

    def run():
        blends = [make_blend(scarlet, hsc, s) for s in scales]
        t0 = time.perf_counter()
        results = scarlet.fit_blends(blends, args.iters, e_rel=1e-9)
        return time.perf_counter() - t0, sum(r[0] for r in results)

    run()  # warm-up: library load, plans, LDS configuration
    times, iterations = zip(*(run() for _ in range(args.repeats)))
    print(json.dumps(dict(tool="profile_source_time", blends=args.blends,
                          iterations=int(iterations[0]), seconds=float(np.median(times)),
                          all_seconds=[float(t) for t in times],
                          profile_sources_per_blend=3)))


if __name__ == "__main__":
    main()
