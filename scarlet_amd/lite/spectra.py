"""``fit_spectra_blends``: ``LiteBlend.fit_spectra`` for a catalogue of blends, one device
batch (two launches of csrc/lite_spectra.hip) per group of blends that share dtype, bands and
stamp shape.

The device forms the float64 normal equations of ``multifit_seds`` -- per blend and band the
Gram matrix of the convolved morphologies on the union box and their products with the image
-- and the host solves them (``_solve_spectra``: minimum norm, as ``lstsq``).  Grouping,
chunking and packing follow ``lite/measure.py::weight_blends``."""

import numpy as np

from .._catalog import call_args, chunks, defaults

# lite_spectra.hip: side of a tile of the union box (one workgroup, one thread per pixel);
# stamp sides; components of a blend; components whose box grown by the stamp's half meets one
# tile (their columns share the LDS of a CU); sides of a union box.  A blend beyond them takes
# LiteBlend.fit_spectra.
TILE = 16
MAX_STAMP = 63
MAX_COMPONENTS = 64
MAX_PRESENT = 32
MAX_EXTENT = 4096

_BLEND_DESC = np.dtype([("h", "i4"), ("w", "i4"), ("y0", "i4"), ("x0", "i4"), ("fh", "i4"),
                        ("fw", "i4"), ("comp0", "i4"), ("n_comp", "i4"), ("image_off", "i8"),
                        ("stamp_off", "i8"), ("out_off", "i8")], align=True)
_COMP_DESC = np.dtype([("y0", "i4"), ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("morph_off", "i8")],
                      align=True)
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _solve_spectra(gram, rhs, dtype):
    """Spectra ``(..., K)`` of ``dtype`` from the normal equations ``gram (..., K, K)`` and
    ``rhs (..., K)``: the minimum-norm solution ``pinv(G) r`` of every system -- what ``lstsq``
    gives for the design, a zero or duplicated column included -- then the ``< 0`` clip of
    ``multifit_seds``."""
    gram, rhs = np.asarray(gram, np.float64), np.asarray(rhs, np.float64)
    # (lstsq drops singular values of the design below eps * pixels of the largest; their
    # squares are the eigenvalues here, which float64 sums resolve to about 1e-12)
    sol = np.einsum("...ij,...j->...i", np.linalg.pinv(gram, rcond=1e-12, hermitian=True), rhs)
    seds = sol.astype(dtype)
    seds[seds < 0] = 0
    return seds


def _stamp_of(blend):
    """The (Ck, kh, kw) stamp the design is convolved with, in float64 (no difference kernel:
    the 1 x 1 stamp of ones); None for what is not a cube."""
    kernel = blend.observation.diff_kernel
    if kernel is None:
        return np.ones((1, 1, 1))
    image = np.asarray(kernel.image)
    if image.ndim != 3 or image.dtype.kind != "f":
        return None
    return image.astype(np.float64)


def _geometry(blend):
    """``(boxes, union)`` relative to the corner of the frame: ``(y0, x0, h, w)`` of every
    component of ``blend.components`` and of the union of them all (not clipped to the frame)."""
    _, fy, fx = blend.observation.bbox.origin
    boxes = []
    for c in blend.components:
        h, w = c.morph.shape
        boxes.append((int(c.bbox.origin[1] - fy), int(c.bbox.origin[2] - fx), int(h), int(w)))
    y0, x0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    y1, x1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
    return boxes, (y0, x0, y1 - y0, x1 - x0)


def _tile_plan(boxes, union, kh, kw):
    """The tiles of a union box as lite_spectra.hip walks them, row-major: ``(y0, x0, h, w,
    present)`` in union-box coordinates, ``present`` the components (in order) whose box grown
    by the stamp's half meets the tile."""
    uy, ux, fh, fw = union
    tiles = []
    for ty in range(0, fh, TILE):
        for tx in range(0, fw, TILE):
            th, tw = min(TILE, fh - ty), min(TILE, fw - tx)
            present = []
            for k, (y0, x0, h, w) in enumerate(boxes):
                cy, cx = y0 - uy, x0 - ux
                if (h > 0 and w > 0 and cy - kh // 2 < ty + th and cy + h + kh // 2 > ty
                        and cx - kw // 2 < tx + tw and cx + w + kw // 2 > tx):
                    present.append(k)
            tiles.append((ty, tx, th, tw, present))
    return tiles


def _max_present(boxes, union, kh, kw):
    """The largest number of components present on one tile (vectorised ``_tile_plan``)."""
    uy, ux, fh, fw = union
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    ty = np.arange(0, fh, TILE)[:, None]
    tx = np.arange(0, fw, TILE)[:, None]
    cy, cx = b[:, 0] - uy, b[:, 1] - ux
    full = (b[:, 2] > 0) & (b[:, 3] > 0)
    rows = (cy - kh // 2 < np.minimum(ty + TILE, fh)) & (cy + b[:, 2] + kh // 2 > ty) & full
    cols = (cx - kw // 2 < np.minimum(tx + TILE, fw)) & (cx + b[:, 3] + kw // 2 > tx)
    return int((rows.astype(np.int64) @ cols.astype(np.int64).T).max())


def _out_of_reach(boxes, frame, kh, kw):
    """Components the data do not reach: the box, grown by the stamp's half, meets neither the
    frame nor the grown box of another component.  Their convolved morphology multiplies zeros
    only, so their least-squares spectrum is an exact 0."""
    H, W = frame
    grown = [(y0 - kh // 2, x0 - kw // 2, y0 + h + kh // 2, x0 + w + kw // 2)
             for y0, x0, h, w in boxes]

    def meet(a, b):
        return a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]

    return [k for k, g in enumerate(grown)
            if boxes[k][2] > 0 and boxes[k][3] > 0 and not meet(g, (0, 0, H, W))
            and not any(meet(g, o) for j, o in enumerate(grown)
                        if j != k and boxes[j][2] > 0 and boxes[j][3] > 0)]


def _plan_blend(blend, clip=False):
    """``(key, plan)`` of a blend the device batch takes -- its group ``(dtype, C, kh, kw)``, and
    the blend with the geometry and the float64 stamp ``_pack`` needs -- or ``(None, reason)``
    for one that goes through ``LiteBlend.fit_spectra``."""
    obs = blend.observation
    images = obs.images
    if not isinstance(images, np.ndarray) or images.ndim != 3:
        return None, "images.ndim != 3"
    dtype = images.dtype
    if dtype not in _FLOATS:
        return None, "images are neither float32 nor float64"
    C = images.shape[0]
    if min(images.shape) < 1 or tuple(obs.bbox.shape) != tuple(images.shape):
        return None, "the observation's box is not its image"
    stamp = _stamp_of(blend)
    if stamp is None or stamp.shape[0] not in (1, C):
        return None, "difference kernel is not a stamp per band"
    kh, kw = stamp.shape[1:]
    if kh % 2 == 0 or kw % 2 == 0:
        return None, "even difference-kernel stamp"
    if max(kh, kw) > MAX_STAMP:
        return None, "stamp beyond the kernel's limits"
    comps = list(blend.components)
    if not comps:
        return None, "no components"
    for c in list(comps) + [c for s in blend.sources for c in s.components]:
        sed, morph = getattr(c, "sed", None), getattr(c, "morph", None)
        if not (isinstance(sed, np.ndarray) and isinstance(morph, np.ndarray)):
            return None, "a component is not spectrum x morphology arrays"
        if sed.dtype != dtype or morph.dtype != dtype:
            return None, "mixed dtypes"
        if (sed.shape != (C,) or morph.ndim != 2 or c.bbox.D != 3
                or tuple(c.bbox.shape) != (C,) + morph.shape):
            return None, "a component does not cover all bands of its box"
    if len(comps) > MAX_COMPONENTS:
        return None, "more than {} components".format(MAX_COMPONENTS)
    boxes, union = _geometry(blend)
    if (max(union[2:]) > MAX_EXTENT or max(images.shape[1:]) > (1 << 24)
            or max(abs(v) for v in union[:2]) > (1 << 24)):
        return None, "union box beyond the kernel's limits"
    if _max_present(boxes, union, kh, kw) > MAX_PRESENT:
        return None, "more than {} components on one {} x {} tile".format(MAX_PRESENT, TILE, TILE)
    if clip and _out_of_reach(boxes, images.shape[1:], kh, kw):
        # (exact spectrum 0: the batch would return it and the tail drop the component, where
        # the loop keeps or drops it on the sign of its convolution's round-off)
        return None, ("clip=True with a component the data do not reach: the loop's round-off "
                      "decides whether it stays")
    return (dtype, int(C), int(kh), int(kw)), dict(blend=blend, boxes=boxes, union=union,
                                                   stamp=stamp)


def _spectra_key(blend, clip=False):
    """``(key, reason)``: the group of a blend, or None and why it takes the loop."""
    key, plan = _plan_blend(blend, clip)
    return (key, None) if key is not None else (None, plan)


def _plan_groups(blends, clip=False):
    """``(groups, fallback)``: per key the ``(position, plan)`` of its blends, and
    ``(position, reason)`` of the others."""
    groups, fallback = {}, []
    for i, b in enumerate(blends):
        key, plan = _plan_blend(b, clip)
        if key is None:
            fallback.append((i, plan))
        else:
            groups.setdefault(key, []).append((i, plan))
    return groups, fallback


def plan_fit_spectra_blends(blends, clip=False):
    """``(groups, fallback)`` of ``fit_spectra_blends(blends, clip)``, without touching the
    GPU: the positions of the blends of every device group, keyed by ``(dtype, C, kh, kw)`` in
    order of first appearance and in input order inside a group, and ``(position, reason)`` of
    the blends that go through ``LiteBlend.fit_spectra``."""
    groups, fallback = _plan_groups(blends, clip)
    return {key: [i for i, _ in items] for key, items in groups.items()}, fallback


def _plan_bytes(plan, key):
    """Bytes of the device working set of a planned blend: image, stamp and morphologies, the
    sums of every tile and the output."""
    dtype, C, kh, kw = key
    _, h, w = plan["blend"].observation.images.shape
    K = len(plan["boxes"])
    tiles = -(-plan["union"][2] // TILE) * -(-plan["union"][3] // TILE)
    morphs = sum(b[2] * b[3] for b in plan["boxes"])
    return ((C * h * w + morphs) * dtype.itemsize
            + (C * kh * kw + (tiles + 1) * C * (K * K + K)) * 8)


def _pack(plans, key):
    """Descriptor tables and packed buffers of one chunk (the arguments of
    smi_lite_spectra_*)."""
    dtype, C, kh, kw = key
    blends = np.zeros(len(plans), _BLEND_DESC)
    comps = np.zeros(sum(len(p["boxes"]) for p in plans), _COMP_DESC)
    images, stamps, morphs = [], [], []
    image_off = morph_off = out_off = k = 0
    for b, p in enumerate(plans):
        blend = p["blend"]
        _, h, w = blend.observation.images.shape
        images.append(np.ascontiguousarray(blend.observation.images, dtype).reshape(-1))
        stamps.append(np.ascontiguousarray(np.broadcast_to(p["stamp"], (C, kh, kw)))
                      .reshape(-1))
        K = len(p["boxes"])
        blends[b] = (h, w) + tuple(p["union"]) + (k, K, image_off, b * C * kh * kw, out_off)
        image_off += C * h * w
        out_off += C * (K * K + K)
        for c, box in zip(blend.components, p["boxes"]):
            comps[k] = tuple(box) + (morph_off,)
            morphs.append(np.ascontiguousarray(c.morph, dtype).reshape(-1))
            morph_off += c.morph.size
            k += 1
    return dict(blends=blends, comps=comps, images=np.concatenate(images),
                stamps=np.concatenate(stamps), morphs=np.concatenate(morphs), n_out=out_off)


def _run_chunk(packed, key, device):
    """One smi_lite_spectra_* call: the packed sums of a chunk, float64."""
    import ctypes

    from .. import _lib

    dtype, C, kh, kw = key
    lib = _lib.load()
    ct, fn = ((ctypes.c_double, lib.smi_lite_spectra_f64) if dtype == np.float64
              else (ctypes.c_float, lib.smi_lite_spectra_f32))
    out = np.empty(packed["n_out"], np.float64)
    args = call_args([packed["blends"], packed["comps"]],
                     [(packed["images"], ct), (packed["stamps"], ctypes.c_double),
                      (packed["morphs"], ct)], [(out, ctypes.c_double)])
    _lib.check(fn(device, C, kh, kw, *args))
    return out


def _normal_equations(packed, out, C):
    """Per blend of a chunk ``(gram (C, K, K), rhs (C, K))``, views of ``out``."""
    result = []
    for bl in packed["blends"]:
        K, at = int(bl["n_comp"]), int(bl["out_off"])
        sums = out[at:at + C * (K * K + K)].reshape(C, K * K + K)
        result.append((sums[:, :K * K].reshape(C, K, K), sums[:, K * K:]))
    return result


def fit_spectra_blends(blends, clip=False, device=None, _working_set_bytes=None):
    """``LiteBlend.fit_spectra`` for many blends: what ``[b.fit_spectra(clip) for b in
    blends]`` leaves -- spectra written in place into every component's array, then the
    components without spectrum or morphology dropped (``clip``) or ``prox_sed`` -- with the
    spectra from float64 normal equations, all components of a blend jointly, instead of a
    float32 FFT convolution and ``lstsq`` (the contract of ``init_blends`` for its joint fits).
    One device batch, two launches of csrc/lite_spectra.hip, per group of blends that share
    dtype, bands and stamp shape; frames, boxes and component counts may differ.  The device
    path convolves with the stamp in float64 for either ``convolution_mode``.

    Blends the device path does not take (``plan_fit_spectra_blends`` names them: an even
    stamp, other or mixed dtypes, no components, a stamp or a number of components beyond the
    kernel's limits; with ``clip=True`` also a blend with a component whose convolved
    morphology meets neither the frame nor another component -- its exact spectrum is 0, and
    whether the loop drops it hangs on the sign of round-off only the loop reproduces) go
    through ``fit_spectra`` after the device groups.  ``device``: GPU index
    of the batches (default 0).  Returns the list of the blends."""
    blends = list(blends)
    budget, device = defaults(_working_set_bytes, device)
    groups, fallback = _plan_groups(blends, clip)
    for key, items in groups.items():
        dtype, C = key[:2]
        for chunk in chunks([(plan, _plan_bytes(plan, key)) for _, plan in items], budget):
            packed = _pack(chunk, key)
            out = _run_chunk(packed, key, device)
            equations = _normal_equations(packed, out, C)
            # one solve for all blends of the chunk with the same number of components
            same = {}
            for b, (gram, _) in enumerate(equations):
                same.setdefault(gram.shape[-1], []).append(b)
            for rows in same.values():
                seds = _solve_spectra(np.stack([equations[b][0] for b in rows]),
                                      np.stack([equations[b][1] for b in rows]), dtype)
                for b, sed in zip(rows, seds):
                    chunk[b]["blend"]._set_spectra(sed.T, clip)
    for i, _ in fallback:
        blends[i].fit_spectra(clip)
    return blends
