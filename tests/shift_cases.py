"""Case table of the Fourier-shift tests (tests/test_shift_host.py, tests/test_gpu_shift.py).

NumPy only; the helpers at the end lean on ``oracle`` (NumPy as well).  What the table is
for, and what the scene tests of tests/test_gpu_parity.py leave out, is in NOTEBOOK.md
("Fourier-shift kernels, shape by shape").

Images are white noise (``rng.random``, scaled to maximum 1) and the data is ``rng.normal``:
the y-Nyquist rank-one term of the shift map, ``beta (-1)^n ah[m]``, is of the order of 1e-2 of
such an image and next to nothing of a smooth one.  Every component has ``prox_flags=0``, so no
sweep plan is needed and boxes with even sides are legal.  Frames are small and the large
boxes overhang them on both sides: every scene stays on the fused convolution path.

A box is ``(shape, origin, shift, second shift)``; ``shift=None`` is a component without a
free shift.  The second shifts are what ``set_centers`` moves a live batch to: they hold
values beyond one pixel and negative integers.
"""

import zlib
from collections import namedtuple

import numpy as np

RTOL = 1e-5  # tests/test_gpu_parity.py
DATA_SIGMA = 8.0

Box = namedtuple("Box", "shape origin shift shift2")

_SMALL = [
    Box((16, 17), (-5, 3), (0.37, -1.6), (-1.25, 0.4)),    # even h: Fy = 48; overhangs
    Box((17, 16), (20, 15), (-2.0, 3.0), (0.3, -0.7)),     # Fy = 45 odd; the integer shift
    Box((1, 9), (10, 2), (0.3, 0.2), (-0.4, -1.0)),
    Box((8, 1), (30, 30), (-0.3, 0.45), (-1.0, 0.2)),
    Box((2, 2), (12, 25), (0.25, 0.5), (-0.45, 1.3)),
    Box((1, 1), (39, 35), (0.3, -0.4), (-0.6, 0.25)),      # the frame's last pixel
]
_SMALL_B = [b._replace(shift=s) for b, s in zip(_SMALL, [
    (-0.3, 0.55), (0.6, -0.35), (-0.25, 1.0), (0.3, -0.45), (-0.3, 0.45), (-0.35, 0.3)])]

CASES = {
    # name: (bands, frame, [boxes of blend 0, boxes of blend 1, ...])
    "small": (2, (40, 36), [_SMALL]),
    # the last square box whose work arrays fit the LDS
    "lds_edge": (2, (100, 100), [[Box((95, 95), (2, 3), (0.3, -0.45), (-1.0, 1.35))]]),
    # the first square box with work arrays in global memory, a small box riding along
    "scratch_edge": (2, (100, 100), [[Box((96, 96), (-3, 5), (-0.3, 0.45), (1.4, -2.0)),
                                      Box((12, 20), (60, 70), (0.3, -0.45), (-3.0, 0.45))]]),
    # small boxes on the global path only because of a neighbour without a shift
    "pushed": (2, (100, 90), [[Box((121, 121), (-10, -15), None, None),
                               Box((12, 20), (5, 8), (0.3, 0.45), (-1.3, -1.0)),
                               Box((17, 23), (70, 60), (-0.4, 0.25), (2.0, -0.3))]]),
    # pixel counts 1, 2 and 3 modulo 4, scratch regions back to back
    "packed": (2, (100, 100), [[Box((97, 97), (-2, -4), (0.3, -0.45), (-1.0, 0.4)),
                                Box((98, 99), (1, 0), (-0.3, 0.45), (1.45, -2.0)),
                                Box((99, 101), (0, -1), (0.28, 0.45), (-0.3, -1.2))]]),
    # the 240 px limit: F = 500 on the long axes, Fy = 135 (odd) for h = 61
    "limit": (2, (72, 70), [[Box((240, 61), (-80, 4), (0.25, -0.45), (-1.3, 2.0)),
                             Box((61, 240), (5, -90), (0.45, 0.25), (-2.0, -0.4)),
                             Box((240, 240), (-100, -60), (-0.25, 0.45), (1.2, -1.0))]]),
    # the largest boxes the update kernel takes along (it keeps one image of the largest box in the
    # LDS: at most 40956 pixels), so that the backward kernel is seen at F = 500 as well:
    # ``gradient()`` refuses the 240 x 240 box of ``limit`` (NOTEBOOK.md)
    "limit_update": (2, (72, 70), [[Box((240, 61), (-80, 4), (-0.25, 0.45), (2.0, -1.3)),
                                    Box((61, 240), (5, -90), (0.3, -0.25), (-0.4, -2.0)),
                                    Box((240, 170), (-100, -60), (0.25, -0.45), (-1.0, 1.2))]]),
    # Fy = 125 and 225: no Nyquist frequency along y, shifts beyond one pixel
    "odd_fy": (2, (64, 60), [[Box((57, 20), (3, 5), (1.3, -2.6), (-3.0, 0.4)),
                              Box((107, 30), (-20, 25), (-1.75, 1.2), (0.4, -2.0))]]),
    # two blends, different data and different shifts
    "two_blends": (2, (40, 36), [_SMALL, _SMALL_B]),
}


def gaussian_kernel():
    """The difference kernel of every scene: 3 x 3, sigma 0.8, normalised, one band."""
    g = np.exp(-np.arange(-1, 2) ** 2 / (2 * 0.8**2))
    k = np.outer(g, g)
    return (k / k.sum()).astype(np.float32)[None]


def make_case(name):
    """The arrays of a case: dict with ``C, H, W, kernel, data, weights`` (per blend) and
    ``blends``: per blend a list of dicts ``sed, morph, origin, shift, shift2``."""
    C, (H, W), blends = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out = dict(name=name, C=C, H=H, W=W, kernel=gaussian_kernel(), blends=[])
    nb = len(blends)
    out["data"] = rng.normal(0.0, DATA_SIGMA, (nb, C, H, W)).astype(np.float32)
    out["weights"] = np.ones((nb, C, H, W), dtype=np.float32)
    for boxes in blends:
        comps = []
        for box in boxes:
            morph = rng.random(box.shape)
            morph = (morph / morph.max()).astype(np.float32)
            comps.append(dict(sed=rng.uniform(0.5, 2.0, C).astype(np.float32), morph=morph,
                              origin=box.origin,
                              shift=None if box.shift is None else np.array(box.shift, float),
                              shift2=None if box.shift2 is None else np.array(box.shift2, float)))
        out["blends"].append(comps)
    return out


def shifting_components(case):
    """(blend, index in the blend, component dict) of every component with a free shift."""
    return [(b, k, c) for b, comps in enumerate(case["blends"]) for k, c in enumerate(comps)
            if c["shift"] is not None]


def is_integer(s):
    return float(s) == np.round(s)


def zero_filled_roll(x, shift):
    """``x`` moved by the integer ``shift`` = (dy, dx), zeros moving in."""
    dy, dx = int(shift[0]), int(shift[1])
    h, w = x.shape
    out = np.zeros_like(x)
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = x[ys, xs]
    return out


def forward_bound(op, x):
    """Elementwise bound of the float32 evaluation of ``Dr x Tx^T - Di x Hx^T``: two chained
    float32 dot products of lengths w and h with rounded operands,

        (h + w + 4) 2^-24 (|Dr| |x| |Tx|^T + |Di| |x| |Hx|^T) + 1e-10 max|x|
    """
    h, w = x.shape
    ax = np.abs(x)
    mag = np.abs(op.Dr) @ ax @ np.abs(op.Tx).T + np.abs(op.Di) @ ax @ np.abs(op.Hx).T
    return (h + w + 4) * 2.0**-24 * mag + 1e-10 * ax.max()


def without(op, *names):
    """Copy of a ShiftOperator with the named matrices zeroed."""
    import copy

    out = copy.copy(op)
    for name in names:
        setattr(out, name, np.zeros_like(getattr(op, name)))
    return out


def oracle_scene(case, b, which="shift"):
    """float64 ``oracle.pgm.Scene`` of blend ``b`` (the float32 inputs promoted), the components
    without constraint like ``prox_flags=0``; ``which``: "shift" or "shift2"."""
    from oracle import pgm

    comps = []
    for c in case["blends"][b]:
        oc = pgm.Component(c["sed"].astype(np.float64), c["morph"].astype(np.float64), c["origin"],
                           shift=None if c[which] is None else c[which].copy())
        oc.morph_prox = lambda x, step: x
        comps.append(oc)
    shape = (case["C"], case["H"], case["W"])
    return pgm.Scene(shape, case["data"][b].astype(np.float64),
                     case["weights"][b].astype(np.float64),
                     case["kernel"].astype(np.float64), comps, dtype=np.float64)


def boxed_gradient(sc, c, G):
    """``G`` (C, H, W) cut to the box of component ``c``, zero outside the frame."""
    h, w = c.morph.shape
    boxed = np.zeros((sc.frame_shape[0], h, w))
    fs, bs = sc.box_slices(c)
    boxed[bs] = G[fs]
    return boxed


def grad_scales(sc):
    """``grad_scales`` of tests/test_gpu_parity.py restated: (max_c sum |G| |morph|,
    max_yx sum_c |sed| |G|) per component, the magnitudes the float32 sums run over."""
    G = np.abs(sc.model_gradient(sc.render(sc.get_model())))
    out = []
    for c in sc.components:
        boxed = boxed_gradient(sc, c, G)
        out.append((np.einsum("cyx,yx->c", boxed, np.abs(c.morph)).max(),
                    np.einsum("c,cyx->yx", np.abs(c.sed), boxed).max()))
    return out


def upstream_gradients(sc):
    """d(-logL)/d(shifted image) per component: ``sum_c sed_c G_c`` over the box."""
    G = sc.model_gradient(sc.render(sc.get_model()))
    return [np.einsum("c,cyx->yx", c.sed, boxed_gradient(sc, c, G)) for c in sc.components]


# ---- kernel-shift scenes -------------------------------------------------------------------
# name: (C, frame, batch kernel (ph, pw), stamp (h0, w0), kernel bands, shifts per blend)
KERNEL_CASES = {
    "inner_stamp": (2, (20, 24), (15, 15), (9, 13), 2, [(0.3, -0.45)]),   # (a)
    "shared_band": (3, (20, 24), (11, 7), (11, 7), 1, [(-0.35, 0.3)]),    # (b)
    "per_band": (3, (20, 24), (11, 7), (11, 7), 3, [(0.4, 0.25)]),        # (c)
    "short_frame": (2, (5, 30), (7, 9), (7, 9), 2, [(0.3, -0.4)]),        # (d) < one slab
    "partial_slab": (2, (21, 19), (7, 9), (7, 9), 1, [(-0.3, 0.35)]),     # (d) 21 = 2 x 8 + 5
    "two_blends": (2, (20, 24), (9, 7), (9, 7), 2, [(0.35, -0.3), (-0.35, 0.3)]),  # (e)
    "integer": (2, (20, 24), (9, 9), (9, 9), 2, [(-1.0, 2.0)]),           # (f)
}


def make_kernel_case(name):
    """dict with ``C, H, W, ph, pw, stamps (nb, bands, h0, w0), shifts (nb, 2), fft_shape, data,
    weights`` and per blend two components without shift (``sed, morph, origin``)."""
    from oracle import fftconv

    C, (H, W), (ph, pw), (h0, w0), bands, shifts = KERNEL_CASES[name]
    rng = np.random.default_rng(zlib.crc32(("kernel " + name).encode()))
    nb = len(shifts)
    stamps = rng.random((nb, bands, h0, w0))
    stamps = (stamps / stamps.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)
    blends = []
    for _ in range(nb):
        comps = []
        for shape, origin in (((min(H, 7), 9), (0, 3)), ((min(H, 11), 8), (H - min(H, 11), W - 10))):
            morph = rng.random(shape)
            comps.append(dict(sed=rng.uniform(0.5, 2.0, C).astype(np.float32),
                              morph=(morph / morph.max()).astype(np.float32), origin=origin))
        blends.append(comps)
    return dict(name=name, C=C, H=H, W=W, ph=ph, pw=pw, stamps=stamps, bands=bands,
                shifts=np.array(shifts, dtype=np.float64),
                fft_shape=list(fftconv.fft_shape((h0, w0), (h0, w0), padding=10, axes=(-2, -1))),
                data=rng.normal(0.0, 1.0, (nb, C, H, W)).astype(np.float32),
                weights=np.ones((nb, C, H, W), dtype=np.float32), blends=blends)


def embed(stamp, ph, pw):
    """(bands, h0, w0) stamps centred in zeros (bands, ph, pw): corner (ph//2 - h0//2, ...)."""
    bands, h0, w0 = stamp.shape
    out = np.zeros((bands, ph, pw), dtype=stamp.dtype)
    oy, ox = ph // 2 - h0 // 2, pw // 2 - w0 // 2
    out[:, oy:oy + h0, ox:ox + w0] = stamp
    return out


def kernel_scene(kc, b, free=True):
    """float64 oracle scene of blend ``b`` of a kernel case.  ``free``: the scene's kernel is the
    unshifted stamp with ``psf_shift`` (the stamp must fill the batch kernel); else the kernel
    is the shifted stamp embedded in the batch kernel's zeros, held fixed."""
    from oracle import fftconv, pgm

    stamp = kc["stamps"][b].astype(np.float64)
    shift = kc["shifts"][b]
    if free:
        assert stamp.shape[1:] == (kc["ph"], kc["pw"])
        kernel, psf_shift = stamp, shift.copy()
    else:
        kernel, psf_shift = embed(fftconv.fourier_shift(stamp, shift), kc["ph"], kc["pw"]), None
    comps = []
    for c in kc["blends"][b]:
        oc = pgm.Component(c["sed"].astype(np.float64), c["morph"].astype(np.float64), c["origin"])
        oc.morph_prox = lambda x, step: x
        comps.append(oc)
    return pgm.Scene((kc["C"], kc["H"], kc["W"]), kc["data"][b].astype(np.float64),
                     kc["weights"][b].astype(np.float64), kernel, comps, dtype=np.float64,
                     psf_shift=psf_shift)


def kernel_gradient_image(sc, ph, pw):
    """``G_K[c, u] = d(-logL)/dK_c[u] = sum_x r_c[x] model_c[x - (u - p//2)]`` over the whole
    (ph, pw) stamp of a scene with a per-band kernel, by direct sums (zero outside the frame)."""
    model = sc.get_model()
    r = sc.weights * (sc.render(model) - sc.data)
    C, H, W = model.shape
    pad = np.zeros((C, H + 2 * ph, W + 2 * pw))
    pad[:, ph:ph + H, pw:pw + W] = model
    out = np.zeros((C, ph, pw))
    for uy in range(ph):
        for ux in range(pw):
            dy, dx = uy - ph // 2, ux - pw // 2
            out[:, uy, ux] = (r * pad[:, ph - dy:ph - dy + H, pw - dx:pw - dx + W]).sum(axis=(1, 2))
    return out


def stamp_shift_gradient(stamp, shift, G_K):
    """d(-logL)/d(shift) of a kernel ``embed(fourier_shift(stamp, shift))``: ShiftOperator of the
    stamp's shape applied to the central crop of ``G_K`` (C, ph, pw).  One stamp band shared by
    all C bands collects their ``G_K``."""
    from oracle import fftconv

    bands, h0, w0 = stamp.shape
    C, ph, pw = G_K.shape
    oy, ox = ph // 2 - h0 // 2, pw // 2 - w0 // 2
    crop = G_K[:, oy:oy + h0, ox:ox + w0]
    if bands == 1:
        crop = crop.sum(axis=0, keepdims=True)
    op = fftconv.ShiftOperator((h0, w0), shift)
    return sum(op.shift_gradient(stamp[j].astype(np.float64), crop[j]) for j in range(bands))
