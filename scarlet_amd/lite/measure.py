"""Measurements of ``scarlet.lite`` (reference scarlet/lite/measure.py)."""

import numpy as np

from .._catalog import call_args, cat, chunks, defaults
from ..bbox import Box, overlapped_slices
from .utils import insert_image


def calculate_snr(images, variance, psfs, center):
    """PSF-weighted signal-to-noise at ``center``: ``sum(I P) / sqrt(sum(P^2 var))`` over
    the PSF stamp placed on the centre."""
    py, px = psfs.shape[1] // 2, psfs.shape[2] // 2
    bbox = Box(psfs.shape, origin=(0, center[0] - py, center[1] - px))
    noise = bbox.extract_from(variance)
    img = bbox.extract_from(images)
    return np.sum(img * psfs) / np.sqrt(np.sum(psfs * noise * psfs))


def weight_sources(blend, mask_footprint=True):
    """Redistribute the observed flux among the sources in proportion to their convolved
    models (the classical deblending template trick): sets ``src.flux`` and
    ``src.flux_box`` on every source (lite/measure.py:39-91)."""
    obs = blend.observation
    py, px = obs.psfs.shape[-2] // 2, obs.psfs.shape[-1] // 2
    images = obs.images.copy()
    if mask_footprint:
        images = images * (obs.weights > 0)
    total = obs.convolve(blend.get_model(), mode="real")
    total[total < 0] = 0
    for src in blend.sources:
        if len(src.components) == 0:
            src.flux = 0
            src.flux_box = Box((0, 0, 0))
            continue
        bbox = src.bbox.grow((0, py, px))
        model = obs.convolve(insert_image(bbox, src.bbox, src.get_model()), mode="real")
        model[model < 0] = 0
        in_obs, in_box = overlapped_slices(obs.bbox, bbox)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = model[in_box] / total[in_obs]
        ratio[total[in_obs] == 0] = 0
        ratio[ratio > 1] = 1  # round-off can lift a hot pixel slightly above 1
        src.flux = ratio * images[in_obs]
        src.flux_box = obs.bbox & bbox


# ---------------------------------------------------------------------------
# weight_blends: weight_sources for a catalogue, one device batch per group
# ---------------------------------------------------------------------------
# reweight.hip: a workgroup computes a 32 x 32 tile and keeps its halo (odd row pitch) and
# the band's stamp in at most 64 KiB of LDS; larger stamps take weight_sources
_TILE = 32
_LDS_BYTES = 64 * 1024

_BLEND_DESC = np.dtype([("h", "i4"), ("w", "i4"), ("comp0", "i4"), ("n_comp", "i4"),
                        ("image_off", "i8"), ("stamp_off", "i8")], align=True)
_SOURCE_DESC = np.dtype([("blend", "i4"), ("comp0", "i4"), ("n_comp", "i4"), ("y0", "i4"),
                         ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("reserved", "i4"),
                         ("out_off", "i8")], align=True)
_COMP_DESC = np.dtype([("y0", "i4"), ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("stride", "i4"),
                       ("reserved", "i4"), ("sed_off", "i8"), ("morph_off", "i8")], align=True)


def _stamp_fits(kh, kw, itemsize):
    """The halo of a tile plus the stamp fit the LDS of reweight.hip."""
    pitch = (_TILE + kw - 1) | 1
    return ((_TILE + kh - 1) * pitch + kh * kw) * itemsize <= _LDS_BYTES


def _stamp_of(blend):
    """The (Ck, kh, kw) stamp ``obs.convolve(mode="real")`` uses (None: no convolution).
    Raises the ``ValueError`` of ``_filter_bounds`` for an even stamp."""
    from .models import _filter_bounds

    kernel = blend.observation.diff_kernel
    if kernel is None:
        return None
    image = np.asarray(kernel.image)
    _filter_bounds(image.shape[1:])
    return image


def _group_key(blend):
    """``(dtype, C, kh, kw)`` of a blend the device batch takes, None for one that goes
    through ``weight_sources``: mixed dtypes, components that are not spectrum x morphology
    over all bands, or a stamp beyond the LDS tile."""
    obs = blend.observation
    stamp = _stamp_of(blend)
    images = obs.images
    dtype = images.dtype
    if dtype not in (np.float32, np.float64) or images.ndim != 3:
        return None
    C = images.shape[0]
    if tuple(obs.bbox.shape) != tuple(images.shape) or np.shape(obs.weights) != images.shape:
        return None
    comps = list(blend.components) + [c for s in blend.sources for c in s.components]
    for c in comps:
        sed, morph = getattr(c, "sed", None), getattr(c, "morph", None)
        if not (isinstance(sed, np.ndarray) and isinstance(morph, np.ndarray)):
            return None
        if sed.dtype != dtype or morph.dtype != dtype or sed.shape != (C,):
            return None
        if (c.bbox.D != 3 or c.bbox.origin[0] != obs.bbox.origin[0]
                or tuple(c.bbox.shape) != (C,) + morph.shape):
            return None
    if any(np.dtype(s.dtype) != dtype for s in blend.sources):
        return None
    kh, kw = (1, 1) if stamp is None else stamp.shape[1:]
    if stamp is not None and stamp.shape[0] not in (1, C):
        return None
    if not _stamp_fits(kh, kw, dtype.itemsize):
        return None
    return (dtype, C, int(kh), int(kw))


def _rect(sl):
    return sl[0].start, sl[1].start, sl[0].stop - sl[0].start, sl[1].stop - sl[1].start


def _plan_blend(blend):
    """Geometry of one batched blend, relative to the corner of its frame.

    ``comps``: ``(component, y0, x0, h, w, my, mx)`` -- the rectangle a component covers and
    the morphology pixel at its corner: first the blend's components clipped to the frame as
    ``c.slices`` has them (the scene), then every source's, unclipped (its model on
    ``src.bbox``).  ``scene``: the number of the former.  ``sources``: ``(source, comp0,
    n_comp, y0, x0, shape)`` with the range of its components in ``comps`` and the part of
    its grown box inside the frame -- ``shape`` is the (C, h, w) of its flux, empty when the
    box misses the frame; null sources have ``comp0 = None``."""
    obs = blend.observation
    _, fy, fx = obs.bbox.origin
    py, px = obs.psfs.shape[-2] // 2, obs.psfs.shape[-1] // 2
    comps = []
    for c in blend.components:
        y0, x0, h, w = _rect(c.slices[0][1:])
        comps.append((c, y0, x0, max(h, 0), max(w, 0), c.slices[1][1].start, c.slices[1][2].start))
    scene = len(comps)
    sources = []
    for src in blend.sources:
        if len(src.components) == 0:
            sources.append((src, None, 0, 0, 0, None))
            continue
        comp0 = len(comps)
        for c in src.components:
            _, oy, ox = c.bbox.origin
            h, w = c.morph.shape
            comps.append((c, oy - fy, ox - fx, h, w, 0, 0))
        box = obs.bbox & src.bbox.grow((0, py, px))
        sources.append((src, comp0, len(src.components), box.origin[1] - fy, box.origin[2] - fx,
                        tuple(box.shape)))
    return dict(blend=blend, comps=comps, scene=scene, sources=sources)


def _plan_elements(plan):
    """Elements of the device working set of a planned blend: inputs, total and fluxes."""
    C, h, w = plan["blend"].observation.images.shape
    morphs = {id(c[0]): c[0].morph.size for c in plan["comps"]}
    fluxes = sum(int(np.prod(s[5])) for s in plan["sources"] if s[1] is not None)
    return 2 * C * h * w + sum(morphs.values()) + C * len(morphs) + fluxes


def _plan_bytes(plan, key):
    """Bytes of the device working set of a planned blend of group ``key`` (packed inputs,
    ``total`` and fluxes, the stamp)."""
    dtype, C, kh, kw = key
    return (_plan_elements(plan) + C * kh * kw) * dtype.itemsize


def _pack(plans, key, mask_footprint):
    """Descriptor tables and packed buffers of one chunk (the arguments of smi_reweight_*),
    and ``results``: per source with a flux on the device ``(source, out_off, shape)``."""
    dtype, C, kh, kw = key
    blends = np.zeros(len(plans), _BLEND_DESC)
    n_src = sum(1 for p in plans for s in p["sources"] if s[1] is not None and np.prod(s[5]) > 0)
    sources = np.zeros(n_src, _SOURCE_DESC)
    comps = np.zeros(sum(len(p["comps"]) for p in plans), _COMP_DESC)
    images, stamps, seds, morphs, results = [], [], [], [], []
    image_off = sed_off = morph_off = out_off = 0
    k = s_at = 0
    for b, p in enumerate(plans):
        obs = p["blend"].observation
        img = obs.images * (obs.weights > 0) if mask_footprint else obs.images
        images.append(np.ascontiguousarray(img, dtype).reshape(-1))
        stamp = _stamp_of(p["blend"])
        stamp = np.ones((1, 1, 1), dtype) if stamp is None else np.asarray(stamp, dtype)
        stamps.append(np.ascontiguousarray(np.broadcast_to(stamp, (C, kh, kw))).reshape(-1))
        _, h, w = obs.images.shape
        blends[b] = (h, w, k, p["scene"], image_off, b * C * kh * kw)
        image_off += C * h * w
        placed = {}
        for c, y0, x0, ch, cw, my, mx in p["comps"]:
            if id(c) not in placed:
                placed[id(c)] = (sed_off, morph_off)
                seds.append(np.ascontiguousarray(c.sed, dtype))
                morphs.append(np.ascontiguousarray(c.morph, dtype).reshape(-1))
                sed_off += C
                morph_off += c.morph.size
            so, mo = placed[id(c)]
            stride = c.morph.shape[1]
            comps[k] = (y0, x0, ch, cw, stride, 0, so, mo + my * stride + mx)
            k += 1
        first = int(blends[b]["comp0"])
        for src, comp0, n, y0, x0, shape in p["sources"]:
            if comp0 is None or np.prod(shape) == 0:
                continue
            sources[s_at] = (b, first + comp0, n, y0, x0, shape[1], shape[2], 0, out_off)
            results.append((src, out_off, shape))
            out_off += int(np.prod(shape))
            s_at += 1
    return dict(blends=blends, sources=sources, comps=comps, images=cat(images, dtype),
                stamps=cat(stamps, dtype), seds=cat(seds, dtype), morphs=cat(morphs, dtype),
                n_out=out_off, results=results)


def _run_chunk(packed, key, device):
    """One smi_reweight_* call: the packed fluxes of a chunk."""
    import ctypes

    from .. import _lib

    dtype, C, kh, kw = key
    lib = _lib.load()
    ct, fn = ((ctypes.c_double, lib.smi_reweight_f64) if dtype == np.float64
              else (ctypes.c_float, lib.smi_reweight_f32))
    out = np.empty(packed["n_out"], dtype)
    args = call_args([packed[name] for name in ("blends", "sources", "comps")],
                     [(packed[name], ct) for name in ("images", "stamps", "seds", "morphs")],
                     [(out, ct)])
    _lib.check(fn(device, C, kh, kw, *args))
    return out


def _assign(plans, packed, out):
    """Hand the results of a chunk to its sources, as arrays of their own."""
    dtype = out.dtype
    for p in plans:
        obs = p["blend"].observation
        for src, comp0, _, y0, x0, shape in p["sources"]:
            if comp0 is None:
                src.flux, src.flux_box = 0, Box((0, 0, 0))
                continue
            _, fy, fx = obs.bbox.origin
            src.flux_box = Box(shape, origin=(obs.bbox.origin[0], y0 + fy, x0 + fx))
            if np.prod(shape) == 0:
                src.flux = np.zeros(shape, dtype)
    for src, off, shape in packed["results"]:
        src.flux = out[off:off + int(np.prod(shape))].reshape(shape).copy()


def plan_blends(blends):
    """``(groups, fallback)``: the positions of the blends of every device group, keyed by
    ``(dtype, C, kh, kw)`` in order of first appearance and in input order inside a group,
    and the positions of the blends that go through ``weight_sources``.  Raises the
    ``ValueError`` of an even stamp before any GPU work."""
    groups, fallback = {}, []
    for i, b in enumerate(blends):
        key = _group_key(b)
        if key is None:
            fallback.append(i)
        else:
            groups.setdefault(key, []).append(i)
    return groups, fallback


def weight_blends(blends, mask_footprint=True, device=None, _working_set_bytes=None):
    """``weight_sources`` for many blends: sets ``src.flux`` and ``src.flux_box`` on every
    source of every blend, bit for bit what ``[weight_sources(b, mask_footprint) for b in
    blends]`` sets, with one device batch (two launches of reweight.hip) per group of
    blends that share dtype, bands and stamp shape; frames, boxes and source counts may
    differ.  Blends with mixed dtypes, or a stamp beyond the kernel's LDS tile, take
    ``weight_sources`` (on the current device).  ``device``: GPU index of the batches
    (default 0).  Returns None."""
    blends = list(blends)
    budget, device = defaults(_working_set_bytes, device)
    groups, fallback = plan_blends(blends)
    for key, idx in groups.items():
        plans = [_plan_blend(blends[i]) for i in idx]
        for chunk in chunks([(p, _plan_bytes(p, key)) for p in plans], budget):
            packed = _pack(chunk, key, mask_footprint)
            out = _run_chunk(packed, key, device)
            _assign(chunk, packed, out)
    for i in fallback:
        weight_sources(blends[i], mask_footprint)
