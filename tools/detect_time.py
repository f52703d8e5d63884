"""Time the detection chain get_detect_wavelets + get_blend_structures on synthetic frames.

Device stages (coadd, starlet transform, multiresolution support) with HIP events on the current
stream, after a warm-up of every shape; then separately the device-to-host copy of the detection
coefficients, the host footprints / structures, and the NumPy equivalent of the device stages (the
reference's algorithm: float64 transform, masked standard deviations) on one core; and the
footprint stage both ways from coefficients that are on the device: the device-to-host copy plus
the host ``get_footprints`` of three planes (the route of a host array) against
``get_footprints_device`` (labelling call with HIP events for one and three planes, the library's
fetch, the Python objects), and the quad trees / structures that remain on the host either way.
``--golden`` does the footprint part on the recorded coefficients of the tutorial frame
(tests/golden/detect.npz). A tree without ``get_footprints_device`` (an older commit under
comparison) reports the host route only. The bytes model beside the times counts the float64 plane
streams each stage must move at least (unmeasured estimate, compared with the ~6.3 TB/s a float4
copy reaches).

    python tools/detect_time.py [--sizes 2048 4096] [--bands 5] [--scales 5] [--golden]
                                [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BW = 6.29e12  # bytes/s, float4 copy on the MI355X


def frame(rng, bands, n):
    """seeded noise plus a few hundred Gaussian sources"""
    images = rng.normal(scale=1.0, size=(bands, n, n)).astype(np.float32)
    yy, xx = np.mgrid[:n, :n]
    for _ in range(max(50, n * n // 40000)):
        y, x = rng.uniform(0, n, 2)
        s = rng.uniform(1.0, 4.0)
        r = 15
        y0, y1 = int(max(0, y - r)), int(min(n, y + r))
        x0, x1 = int(max(0, x - r)), int(min(n, x + r))
        g = np.exp(-((yy[y0:y1, x0:x1] - y) ** 2 + (xx[y0:y1, x0:x1] - x) ** 2) / (2 * s * s))
        images[:, y0:y1, x0:x1] += (rng.uniform(5, 200) * g * rng.uniform(0.5, 1.5, (bands, 1, 1))
                                    ).astype(np.float32)
    variance = np.ones_like(images)
    return images, variance


def numpy_detect(images, variance, scales):
    """the device stages restated in NumPy, float64 (one core)"""
    taps = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)

    def one(x, d):
        n = x.shape[0]
        out = x * taps[2]
        if 2 * d < n:
            out[2 * d:] += x[:n - 2 * d] * taps[0]
        if d < n:
            out[d:] += x[:n - d] * taps[1]
            out[:n - d] += x[d:] * taps[3]
        if 2 * d < n:
            out[:n - 2 * d] += x[2 * d:] * taps[4]
        return out

    def B(x, j):
        return one(one(x, 2 ** j).T, 2 ** j).T

    sigma = np.median(np.sqrt(variance))
    c = np.sum(images, axis=0).astype(np.float64)
    w = np.zeros((scales + 1,) + c.shape)
    for j in range(scales):
        nxt = B(c, j)
        w[j] = c - B(nxt, j)
        c = nxt
    w[-1] = c
    sj = np.ones(scales + 1) * sigma
    last = sj
    for _ in range(20):
        M = np.abs(w) > 3 * sj[:, None, None]
        sj = np.std(w * ~M, axis=(1, 2))
        cut = sj > 0
        if np.all(np.abs(sj[cut] - last[cut]) / sj[cut] < 0.1):
            break
        last = sj
    return M * w


def _median_ms(fn, reps):
    """median wall time of fn() in ms between device synchronisations, after one warm-up"""
    import torch

    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def footprint_stages(d_planes, reps):
    """"coefficients on device -> list of Footprints" of the (3, H, W) device tensor both ways,
    and where the rest of the host time goes.  Times in ms: median, or (median, min, max)."""
    import torch
    from scarlet_amd import Box, detect, detect_pybind11 as dp

    d_planes = d_planes.contiguous()
    out = {"planes": int(d_planes.shape[0]), "shape": list(d_planes.shape[1:])}

    def host_route():
        host = d_planes.cpu().numpy()
        return [dp.get_footprints(p, 0, 4, 0) for p in host]

    out["host_route_ms"] = _median_ms(host_route, reps)
    out["d2h_ms"] = _median_ms(lambda: d_planes.cpu().numpy(), reps)[0]
    footprints = host_route()
    out["n_footprints"] = [len(f) for f in footprints]
    if hasattr(dp, "get_footprints_device"):
        out["device_route_ms"] = _median_ms(lambda: dp.get_footprints_device(d_planes, 0, 4, 0),
                                            reps)
        for name, planes in (("label_1_plane_ms", d_planes[:1]), ("label_3_planes_ms", d_planes)):
            ev = []
            for rep in range(reps + 1):
                a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                a.record()
                counts, work = dp.label_device(planes, 4, 0)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    ev.append(a.elapsed_time(b))
            out[name] = float(np.median(ev))
        counts, work = dp.label_device(d_planes, 4, 0)
        fetch = lambda: [dp.fetch_device(d_planes, k, 0, counts, work)  # noqa: E731
                         for k in range(len(d_planes))]
        out["fetch_ms"] = _median_ms(fetch, reps)[0]
        arrays = fetch()
        t = time.perf_counter()
        for rep in range(reps):
            got = [dp._footprint_objects(*a) for a in arrays]
        out["python_objects_ms"] = (time.perf_counter() - t) * 1e3 / reps
        pk = lambda fp: [(p.y, p.x, p.flux) for p in fp.peaks]  # noqa: E731
        same = all(tuple(a.bounds) == tuple(b.bounds) and np.array_equal(a.footprint, b.footprint)
                   and pk(a) == pk(b)
                   for fa, fb in zip(got, footprints) for a, b in zip(fa, fb))
        out["device_equals_host"] = bool(same and [len(f) for f in got] == out["n_footprints"])
    shape = tuple(d_planes.shape[1:])
    t = time.perf_counter()
    for rep in range(reps):
        low = detect.QuadTreeRegion(Box(shape), capacity=10).add_footprints(footprints[0])
        middle = detect.QuadTreeRegion(Box(shape), capacity=10).add_footprints(footprints[1])
        [detect.SingleScaleStructure(2, fp).add_scale_tree(0, low).add_scale_tree(1, middle)
         for fp in footprints[2]]
    out["trees_and_structures_ms"] = (time.perf_counter() - t) * 1e3 / reps
    return out


def run_golden(reps):
    import torch

    g = np.load(os.path.join(ROOT, "tests", "golden", "detect.npz"))
    d = torch.from_numpy(np.ascontiguousarray(g["detect_s3"][:3])).to("cuda")
    out = dict(size="tutorial", footprints=footprint_stages(d, reps))
    print(json.dumps(out), flush=True)
    return out


def run(n, bands, scales, reps, numpy_ref):
    import torch
    from scarlet_amd import detect, wavelet

    rng = np.random.default_rng(n)
    images, variance = frame(rng, bands, n)
    npix = n * n
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    d_images = wavelet._upload(images)
    sigma = np.median(np.sqrt(variance))
    s0, t0 = wavelet.initial_sigma(np.float32, scales + 1, sigma, 3)
    stages = {"coadd": [], "transform": [], "support": [], "d2h": []}
    iters = None
    for rep in range(reps + 1):  # the first round warms every shape up
        e = [ev() for _ in range(5)]
        e[0].record()
        det = wavelet.coadd_device(d_images)
        e[1].record()
        coeffs = wavelet.transform_device(det[None], scales)
        e[2].record()
        _, Mw, iters = wavelet.support_device(coeffs, s0[None], t0[None])
        e[3].record()
        host = Mw[:, 0].cpu().numpy()
        e[4].record()
        torch.cuda.synchronize()
        if rep:
            for k, name in enumerate(stages):
                stages[name].append(e[k].elapsed_time(e[k + 1]))
        d_first = Mw[:3, 0].contiguous()
        del coeffs, Mw
    med = {k: float(np.median(v)) for k, v in stages.items()}
    # bytes each stage must move at least (float64 planes of n*n): coadd reads the float32 bands
    # and writes one float32 plane; a generation-2 scale streams nine planes (four 1-D passes:
    # read + write each, plus the read of c_j for w_j); the support reads all planes twice per
    # iteration and once more to write M (int32) and M*w.
    plane = 8 * npix
    model = {"coadd": 4 * npix * (bands + 1), "transform": 9 * plane * scales + plane,
             "support": int(iters[0]) * 2 * plane * (scales + 1) + (scales + 1) * (plane + 4 * npix + plane),
             "d2h": plane * (scales + 1)}
    t0h = time.perf_counter()
    structures, middle = detect.get_blend_structures(host)
    host_fp = time.perf_counter() - t0h
    out = dict(size=n, bands=bands, scales=scales, reps=reps, support_iterations=int(iters[0]),
               device_ms=med, bytes=model,
               model_ms_at_copy_bw={k: v / COPY_BW * 1e3 for k, v in model.items() if k != "d2h"},
               host_footprints_s=host_fp, n_structures=len(structures),
               footprints=footprint_stages(d_first, reps))
    dev_total = (med["coadd"] + med["transform"] + med["support"] + med["d2h"]) / 1e3
    if numpy_ref:
        t = time.perf_counter()
        ref = numpy_detect(images, variance, scales)
        out["numpy_1core_s"] = time.perf_counter() - t
        out["max_rel_diff_vs_numpy"] = float(np.abs(ref - host).max() / np.abs(ref).max())
        out["end_to_end_speedup"] = (out["numpy_1core_s"] + host_fp) / (dev_total + host_fp)
        out["device_stages_speedup"] = out["numpy_1core_s"] / dev_total
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--golden", action="store_true",
                    help="also the footprint stages on the tutorial frame's coefficients")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("detect_time.py measures the GPU: no GPU visible")
    results = [run(n, a.bands, a.scales, a.reps, not a.no_numpy) for n in a.sizes]
    if a.golden:
        results.append(run_golden(max(a.reps, 20)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
