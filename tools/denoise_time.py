"""Seconds ``scarlet_amd.wavelet.apply_wavelet_denoising_batch`` takes for a list of images,
against the host loop around device calls that ``apply_wavelet_denoising`` was before it.
Prints one JSON line.

    python tools/denoise_time.py [--images 256] [--size 128] [--max-iter 20] [--parent DIR]

The batch is timed as the median of ``--repeats`` calls after a warm-up; every call returns
host arrays, so it ends with the device idle and the host clock is the time a caller waits.
The baseline runs in a process of its own: with ``--parent DIR`` (a built checkout of the commit
before the batch existed) that tree's ``apply_wavelet_denoising``, otherwise this tree's loop
over the same public functions (``wavelet._denoise_host_loop``); it is timed on
``--baseline-images`` images and scaled to the list.  One image alone is timed on both.
``batch_events_ms``: the device chain of one more batch call between two events.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_images(n, size, seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:size, :size]
    out = []
    for _ in range(n):
        cy, cx = rng.uniform(0, size, 2)
        blob = 20 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * (size / 16) ** 2))
        out.append((blob + rng.normal(0.0, 1.0, (size, size))).astype(np.float32))
    return out


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def child(args):
    """the baseline, in the tree ``args.root``"""
    sys.path.insert(0, args.root)
    from scarlet_amd import wavelet

    loop = wavelet.apply_wavelet_denoising if args.parent_api else \
        (lambda im, max_iter: wavelet._denoise_host_loop(im, None, 3, 1e-1, max_iter, True))
    images = make_images(args.baseline_images, args.size)
    loop(images[0], max_iter=args.max_iter)  # warm-up
    t_list = timed(lambda: [loop(im, max_iter=args.max_iter) for im in images], args.repeats)
    t_one = timed(lambda: loop(images[0], max_iter=args.max_iter), 5 * args.repeats)
    print(json.dumps(dict(list_s=statistics.median(t_list), one_s=statistics.median(t_one))))


def baseline(args, root, parent_api):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--size",
           str(args.size), "--max-iter", str(args.max_iter), "--baseline-images",
           str(args.baseline_images), "--repeats", str(args.repeats)]
    if parent_api:
        cmd.append("--parent-api")
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-images", type=int, default=16)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-api", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args)

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from scarlet_amd import wavelet

    assert torch.cuda.is_available(), "needs a GPU"
    images = make_images(args.images, args.size)

    def batch():
        return wavelet.apply_wavelet_denoising_batch(images, max_iter=args.max_iter)

    groups, one_by_one = wavelet.plan_wavelet_denoising_batch(images, args.max_iter)
    got = batch()  # warm-up
    want = [wavelet._denoise_host_loop(im, None, 3, 1e-1, args.max_iter, True)
            for im in images[:args.baseline_images]]
    same = all(np.array_equal(a, b) for a, b in zip(got, want))
    t_batch = timed(batch, args.repeats)
    t_one = timed(lambda: wavelet.apply_wavelet_denoising(images[0], max_iter=args.max_iter),
                  5 * args.repeats)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    flat = wavelet._denoise_pack(torch, images)
    table = wavelet._denoise_tables(images, [None] * len(images), 3)
    buf = wavelet._DenoiseBuffers(torch, table, flat.device)
    torch.cuda.synchronize()
    start.record()
    wavelet.denoise_device(flat, buf, wavelet.DENOISE_ALL, max_iter=args.max_iter)
    end.record()
    torch.cuda.synchronize()
    base = baseline(args, os.path.abspath(args.parent) if args.parent else ROOT,
                    args.parent is not None)
    scale = args.images / args.baseline_images
    batch_s = statistics.median(t_batch)
    print(json.dumps(dict(
        metric="wavelet_denoising_batch_seconds", images=args.images, size=args.size,
        max_iter=args.max_iter, repeats=args.repeats, device_calls=len(groups),
        launches=[g["launches"] for g in groups], one_by_one=len(one_by_one),
        batch_s=round(batch_s, 4),
        batch_min_max_s=[round(min(t_batch), 4), round(max(t_batch), 4)],
        batch_events_ms=round(start.elapsed_time(end), 3),
        baseline="parent commit" if args.parent else "this tree's loop over the public functions",
        baseline_images=args.baseline_images,
        baseline_list_s=round(base["list_s"], 4),
        baseline_scaled_s=round(base["list_s"] * scale, 4),
        speedup=round(base["list_s"] * scale / batch_s, 1),
        one_image_s=round(statistics.median(t_one), 5),
        one_image_baseline_s=round(base["one_s"], 5),
        identical_to_loop=bool(same))))


if __name__ == "__main__":
    main()
