"""Blend-iterations per second of ``scarlet_amd.lite.fit_blends`` against the loop of
``LiteBlend.fit`` on lite blends of mixed frame sizes (cropped ``scarlet_amd.synthetic``
scenes, AMSGrad components, box resizing every 10 iterations).  Prints one JSON line.

    python tools/lite_batch_time.py --blends 256 --iters 50 [--loop-blends 32]

The loop is timed on the first ``--loop-blends`` blends only (its rate does not depend on how
many blends there are); both rates count the iterations the blends actually ran.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROPS = [(64, 64), (72, 60), (80, 72), (60, 88), (96, 80), (56, 56), (88, 100)]


def make_blend(seed, h, w):
    import scarlet_amd as scarlet
    from scarlet_amd import lite, synthetic

    s = synthetic.make_blend(seed)
    images = np.ascontiguousarray(s["data"][:, :h, :w], np.float32)
    weights = np.ascontiguousarray(s["weights"][:, :h, :w], np.float32)
    psfs = np.repeat(s["obs_psf"], images.shape[0], axis=0).astype(np.float32)
    obs = lite.LiteObservation(images, (1 / weights).astype(np.float32), weights, psfs,
                               model_psf=s["model_psf"].astype(np.float32))
    sources = []
    for k in range(len(s["morphs"])):
        morph = np.asarray(s["morphs"][k], np.float32)
        oy, ox = (int(v) for v in s["origins"][k])
        mh, mw = morph.shape
        if not (0 <= oy + mh // 2 < h and 0 <= ox + mw // 2 < w):
            continue
        bbox = scarlet.Box((images.shape[0], mh, mw), origin=(0, oy, ox))
        comp = lite.init_adaprox_component((oy + mh // 2, ox + mw // 2), bbox,
                                           np.asarray(s["seds"][k], np.float32).copy(),
                                           morph.copy(), obs, bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    if not sources:
        return None
    return lite.LiteBlend(sources, obs)


def make_blends(n, seed0=1000):
    out, seed = [], seed0
    while len(out) < n:
        h, w = CROPS[seed % len(CROPS)]
        b = make_blend(seed, h, w)
        seed += 1
        if b is not None:
            out.append(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blends", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop-blends", type=int, default=32)
    ap.add_argument("--e-rel", type=float, default=1e-9)
    args = ap.parse_args()

    import torch

    from scarlet_amd import lite
    from scarlet_amd.lite.fitting import group_keys

    assert torch.cuda.is_available(), "needs a GPU"
    # warm-up: plans, code objects and the monotonicity plan cache of every box size
    warm = make_blends(len(CROPS), seed0=1)
    lite.fit_blends(warm, 2, e_rel=args.e_rel, resize=10, reweight=False)

    blends = make_blends(args.blends)
    n_groups = len(set(k for k in group_keys(blends, args.iters, args.e_rel) if k is not None))
    t0 = time.perf_counter()
    lite.fit_blends(blends, args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_batch = time.perf_counter() - t0
    it_batch = sum(b.it for b in blends)

    loop = make_blends(min(args.loop_blends, args.blends))
    t0 = time.perf_counter()
    for b in loop:
        b.fit(args.iters, e_rel=args.e_rel, resize=10, reweight=False)
    t_loop = time.perf_counter() - t0
    it_loop = sum(b.it for b in loop)

    rate_batch, rate_loop = it_batch / t_batch, it_loop / t_loop
    print(json.dumps(dict(
        metric="lite_fit_blends_blend_iters_per_s", blends=len(blends), iters=args.iters,
        frame_shapes=len({b.observation.images.shape for b in blends}), device_groups=n_groups,
        fit_blends_blend_iters_per_s=round(rate_batch, 1),
        loop_blend_iters_per_s=round(rate_loop, 1), loop_blends=len(loop),
        speedup=round(rate_batch / rate_loop, 2), fit_blends_s=round(t_batch, 3),
        loop_s=round(t_loop, 3))))


if __name__ == "__main__":
    main()
