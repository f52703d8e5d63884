"""The images of a fitted catalogue: ``render_blends`` forms, for many ``Blend``s at once, the
scene as every observation sees it, the residual, chi^2 and log-likelihood, every source's own
rendering and the flux of the data shared out among the sources (reference
scarlet/lite/measure.py:65-90, applied to a ``Blend``) with three launches of
csrc/render_sources.hip per chunk.  Nothing here is on the fitting path."""

import numpy as np

from ._catalog import call_args, cat, chunks, defaults
from .measure import _BAND_DESC, _COMP_DESC, _rect, _refusal, _Tables, region_of
from .measure import plan_blend as _measure_plan_blend

_TILE = 16
SOURCES, REWEIGHT, MASK = 1, 2, 4  # SMI_RENDER_*

_BLEND_DESC = np.dtype([("fh", "i4"), ("fw", "i4"), ("comp0", "i4"), ("n_comp", "i4"),
                        ("band0", "i4"), ("n_band", "i4"), ("out_off", "i8")], align=True)
_SOURCE_DESC = np.dtype([("y0", "i4"), ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("blend", "i4"),
                         ("comp0", "i4"), ("n_comp", "i4"), ("reserved", "i4"),
                         ("out_off", "i8")], align=True)


def plan_render_blends(blends):
    """``(groups, fallback)`` of ``render_blends``, without touching the GPU or the library: the
    positions of the blends of every device group, keyed by ``(C, kh, kw)`` -- model bands and
    stamp shape, (1, 1) without a convolution -- in order of first appearance and in list order
    inside a group, and ``{position: reason}`` of the blends that go through the host loop."""
    groups, fallback = {}, {}
    for i, blend in enumerate(blends):
        reason, key = _refusal(blend, zero_weights=True, null_subset=True, plain_data=True)
        if reason is None:
            groups.setdefault(key, []).append(i)
        else:
            fallback[i] = reason
    return groups, fallback


def plan_blend(blend, key):
    """``measure.plan_blend`` of one blend of group ``key`` -- ``sources``, ``bands`` and the
    frame's ``shape`` -- with ``data``: per observed band, observations in a row, its float32
    image, and ``regions``: per source its region, ``(0, 0, 0, 0)`` for a null source.  Raises
    ``ValueError`` for what only the values show."""
    _, kh, kw = key
    plan = _measure_plan_blend(blend, key)
    for _, comps in plan["sources"]:
        for _, sed, image in comps:
            if not (np.isfinite(sed).all() and np.isfinite(image).all()):
                raise ValueError("a model value that is not finite")
    for _, stamp, _ in plan["bands"]:
        if not np.isfinite(stamp).all():
            raise ValueError("a difference kernel that is not finite")
    plan["data"] = [obs.data[b] for obs in blend.observations for b in range(obs.shape[0])]
    plan["regions"] = [region_of(rect, plan["shape"][1:], kh, kw) if comps else (0, 0, 0, 0)
                       for rect, comps in plan["sources"]]
    return plan


def _tiles(h, w):
    return -(-h // _TILE) * -(-w // _TILE) if h > 0 and w > 0 else 0


def _plan_bytes(plan, key, flags=0):
    """Bytes of the device working set of a planned blend: inputs, tables, work lists, the
    outputs and, with ``REWEIGHT``, the float64 scene."""
    _, kh, kw = key
    _, H, W = plan["shape"]
    n_band = len(plan["bands"])
    want_flux = bool(flags & REWEIGHT)
    want_sources = want_flux or bool(flags & SOURCES)
    # data and weights in, rendered and residual out, (the float64 total), stamp, descriptor,
    # the chi2 partials and work items of the scene's tiles, the row and chi2 of the band
    need = _BLEND_DESC.itemsize + n_band * (
        (16 + 8 * want_flux) * H * W + 4 * kh * kw + _BAND_DESC.itemsize
        + _tiles(H, W) * (12 + 8) + 16 + 8)
    for (rect, comps), (_, _, gh, gw) in zip(plan["sources"], plan["regions"]):
        need += sum(8 * (c[2].size + c[1].size) + _COMP_DESC.itemsize for c in comps)
        if comps and want_sources:
            need += _SOURCE_DESC.itemsize + n_band * (
                (4 + 4 * want_flux) * gh * gw + 12 * _tiles(gh, gw))
    return need


def pack(plans, key, flags=0):
    """Descriptor tables and packed buffers of one chunk (the arguments of
    smi_render_sources_f32), one array per kind; the sizes ``n_out`` of the scene cubes and
    ``n_source_out`` of the per-source cubes; and ``layout``: per blend ``(out_off, regions,
    offsets)`` -- where its cubes start, per source its region and where its cubes start (None
    for a source without components, or when the sources are not rendered)."""
    want_sources = bool(flags & (SOURCES | REWEIGHT))
    blends = np.zeros(len(plans), _BLEND_DESC)
    live = [s for p in plans for s in p["sources"] if s[1]]
    sources = np.zeros(len(live) if want_sources else 0, _SOURCE_DESC)
    t = _Tables(plans, key, sum(len(s[1]) for s in live))
    data, layout = [], []
    out_off = source_off = s_at = 0
    for i, p in enumerate(plans):
        _, H, W = p["shape"]
        band0, comp0 = t.b_at, t.k
        t.add_bands(p)
        data += [np.ascontiguousarray(image, np.float32).reshape(-1) for image in p["data"]]
        n_band = t.b_at - band0
        offsets = []
        for (rect, parts), region in zip(p["sources"], p["regions"]):
            if not parts:
                offsets.append(None)
                continue
            if want_sources:
                sources[s_at] = rect + (i, t.k, len(parts), 0, source_off)
                offsets.append(source_off)
                source_off += n_band * region[2] * region[3]
                s_at += 1
            else:
                offsets.append(None)
            t.add_components(parts)
        blends[i] = (H, W, comp0, t.k - comp0, band0, n_band, out_off)
        layout.append((out_off, list(p["regions"]), offsets))
        out_off += n_band * H * W
    return dict(t.packed(), blends=blends, sources=sources, data=cat(data, np.float32),
                layout=layout, n_out=out_off, n_source_out=source_off)


def _run_chunk(packed, key, flags, device):
    """One smi_render_sources_f32 call: ``rendered``, ``residual`` (``n_out``), ``chi2`` (bands),
    ``source_rendered`` and ``flux`` (``n_source_out``; ``flux`` None without ``REWEIGHT``) and
    ``launch_ms``: the milliseconds of the scene, sources and reduce launches."""
    import ctypes

    from . import _lib

    C, kh, kw = key
    lib = _lib.load()
    out = dict(rendered=np.empty(packed["n_out"], np.float32),
               residual=np.empty(packed["n_out"], np.float32),
               chi2=np.empty(len(packed["bands"]), np.float64),
               source_rendered=np.empty(packed["n_source_out"], np.float32),
               flux=np.empty(packed["n_source_out"], np.float32) if flags & REWEIGHT else None)
    f32, f64 = ctypes.c_float, ctypes.c_double
    args = call_args(
        [packed[name] for name in ("blends", "sources", "comps", "bands")],
        [(packed["seds"], f64), (packed["morphs"], f64), (packed["stamps"], f32),
         (packed["data"], f32), (packed["weights"], f32)],
        [(out["rendered"], f32), (out["residual"], f32), (out["chi2"], f64),
         (out["source_rendered"], f32), (out["flux"], f32)])
    ms = (ctypes.c_double * 3)()
    _lib.check(lib.smi_render_sources_f32(device, C, kh, kw, flags, *args, ms))
    out["launch_ms"] = tuple(ms)
    return out


def _split(flat, off, counts, h, w):
    """The cubes ``(n, h, w)`` of consecutive observations that start at ``flat[off]``."""
    out = []
    for n in counts:
        out.append(flat[off:off + n * h * w].reshape(n, h, w))
        off += n * h * w
    return out


def _log_likelihood(observations, chi2):
    return float(sum(-(obs.log_norm + np.sum(c) / 2) for obs, c in zip(observations, chi2)))


def _results(blends, packed, out, flags):
    """The result dicts of one chunk from the device's buffers (views of them)."""
    results = []
    b_at = 0
    for blend, (out_off, regions, offsets) in zip(blends, packed["layout"]):
        _, H, W = blend.frame.shape
        counts = [obs.shape[0] for obs in blend.observations]
        chi2 = []
        for n in counts:
            chi2.append(out["chi2"][b_at:b_at + n].copy())
            b_at += n
        res = dict(rendered=_split(out["rendered"], out_off, counts, H, W),
                   residual=_split(out["residual"], out_off, counts, H, W), chi2=chi2,
                   log_likelihood=_log_likelihood(blend.observations, chi2))
        if flags & (SOURCES | REWEIGHT):
            res["sources"] = []
            for src, region, off in zip(blend.sources, regions, offsets):
                if off is None:  # a NullSource
                    region, off = (0, 0, 0, 0), 0
                entry = dict(region=tuple(int(v) for v in region),
                             rendered=_split(out["source_rendered"], off, counts, *region[2:]))
                if flags & REWEIGHT:
                    entry["flux"] = _split(out["flux"], off, counts, *region[2:])
                res["sources"].append(entry)
        results.append(res)
    return results


def share_flux(R_k, R_tot, image):
    """The ratio rules of the reference's ``weight_sources`` in float64:
    ``max(R_k, 0) / max(R_tot, 0)``, 0 where the denominator is 0, 1 where the ratio exceeds 1,
    times ``image``; float32."""
    num = np.array(R_k, np.float64)
    den = np.array(R_tot, np.float64)
    num[num < 0] = 0
    den[den < 0] = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = num / den
        ratio[den == 0] = 0
        ratio[ratio > 1] = 1
        return (ratio * image).astype(np.float32)


def _host_render(obs, model):
    """``obs.render(model)`` on the observation's bands (a ``NullRenderer`` hands the model back
    as it is: its channel map is applied here)."""
    R = np.asarray(obs.render(model))
    if R.shape[0] != obs.shape[0]:
        R = np.asarray(obs.renderer.map_channels(R))
    return R


def _host_region(blend, src, obs):
    """Region of a source in an observation of the host loop: the box grown by half the stamp of
    the blend's ``ConvolutionRenderer``s (the largest) and clipped, on an observation that
    covers the frame pixel by pixel; the whole image of any other observation."""
    from .renderer import ConvolutionRenderer

    frame = blend.frame
    if tuple(obs.shape[1:]) != tuple(frame.shape[1:]):
        return (0, 0) + tuple(int(v) for v in obs.shape[1:])
    kh = kw = 1
    for o in blend.observations:
        if isinstance(getattr(o, "renderer", None), ConvolutionRenderer):
            shape = np.shape(o.renderer.diff_kernel.image)
            kh, kw = max(kh, 2 * (shape[-2] // 2) + 1), max(kw, 2 * (shape[-1] // 2) + 1)
    fy, fx = frame.bbox.origin[1:]
    y0, x0, h, w = _rect(src.bbox)
    return region_of((y0 - fy, x0 - fx, h, w), frame.shape[1:], kh, kw)


def render_blend_host(blend, sources=False, reweight=False, mask_footprint=True):
    """The result of one blend through the host loop -- ``obs.render(blend.get_model())``, one
    ``obs.render(src.get_model(frame=frame))`` per source and observation cropped to its region,
    the ratio rules in NumPy float64 --: what ``render_blends`` returns for a blend the device
    does not take.  An observation that is not on the frame's pixels (``ResolutionRenderer``, a
    user's renderer of another shape) keeps its whole image as every source's region there;
    ``region`` is that of the first observation."""
    from .source import NullSource

    frame = blend.frame
    observations = list(blend.observations)
    model = blend.get_model()
    res = dict(rendered=[], residual=[], chi2=[])
    for obs in observations:
        R = _host_render(obs, model)
        res["rendered"].append(R)
        res["residual"].append(obs.data - R)
        d = np.asarray(obs.data, np.float64)
        w = np.asarray(np.ma.filled(obs.weights, 0), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            res["chi2"].append((w * (np.asarray(R, np.float64) - d) ** 2).sum(axis=(1, 2)))
    res["log_likelihood"] = _log_likelihood(observations, res["chi2"])
    if not (sources or reweight):
        return res
    res["sources"] = []
    for src in blend.sources:
        null = isinstance(src, NullSource)
        entry = dict(region=(0, 0, 0, 0), rendered=[])
        if reweight:
            entry["flux"] = []
        full = None if null else src.get_model(frame=frame)
        for at, (obs, R_tot) in enumerate(zip(observations, res["rendered"])):
            if null:
                empty = np.zeros((obs.shape[0], 0, 0), R_tot.dtype)
                entry["rendered"].append(empty)
                if reweight:
                    entry["flux"].append(empty.astype(np.float32))
                continue
            y0, x0, h, w = _host_region(blend, src, obs)
            if at == 0:
                entry["region"] = (y0, x0, h, w)
            crop = (slice(None), slice(y0, y0 + h), slice(x0, x0 + w))
            R_k = _host_render(obs, full)[crop]
            entry["rendered"].append(R_k)
            if reweight:
                image = np.asarray(obs.data)
                if mask_footprint:
                    image = image * (np.asarray(np.ma.filled(obs.weights, 0)) > 0)
                entry["flux"].append(share_flux(R_k, R_tot[crop], image[crop]))
        res["sources"].append(entry)
    return res


def render_blends(blends, sources=False, reweight=False, mask_footprint=True, device=None,
                  _working_set_bytes=None, _report=None):
    """The images of a catalogue: one dict per blend, every list in it with one entry per
    observation in the order of ``blend.observations`` --

    ``rendered``  float32 (C_obs, H, W): the scene, what ``obs.render(blend.get_model())``
                  stands for
    ``residual``  float32: ``data - rendered``, bit for bit
    ``chi2``      float64 (C_obs,): ``sum w (R - d)^2`` per band, from the float64 rendering R
    ``log_likelihood``  the sum over the observations of ``-(obs.log_norm + chi2.sum() / 2)``
    ``sources``   (``sources=True``; ``reweight=True`` implies it) per entry of ``blend.sources``
                  a dict of ``region`` -- ``(y0, x0, h, w)`` relative to the frame's corner: the
                  source's box grown by half the stamp and clipped to the frame --, ``rendered``
                  float32 (C_obs, h, w), that source alone, and with ``reweight=True`` ``flux``:
                  the data shared out by the rules of the reference's
                  ``lite.measure.weight_sources``,
                  ``float32(min(max(R_k, 0) / max(R, 0), 1) * image)``, 0 where ``max(R, 0)`` is 0,
                  ``image = data * (weights > 0)`` if ``mask_footprint`` else ``data``.  A
                  ``NullSource`` has the region (0, 0, 0, 0) and empty arrays.

    -- with three launches of csrc/render_sources.hip per chunk of blends that share the number
    of bands and the stamp shape; frames, boxes, source and observation counts may differ.

    The model is evaluated in float64 from spectrum and morphology image and rendered by a
    float64 tap loop over the renderer's float32 stamp; a source's rendering has the bits
    ``measure_blends`` sums, and ``R`` in the ratio is the scene itself, not the sum of the
    sources.  Every sum has an order fixed by the frame, the boxes and the stamp shape: a blend's
    outputs have the same bits alone, in any list and in any chunk.  ``Observation.render`` and
    the host loop below render in float32 through the FFT; their images differ from these in the
    last float32 digits.

    Blends the device does not take (``plan_render_blends`` says why) and blends with a model
    value that is not finite go through ``render_blend_host``, after the device groups and in
    list order.  ``device``: GPU index (default 0).  ``_working_set_bytes``: device working set of
    a chunk (default 1 GiB).  ``_report``: a dict that receives ``groups``, ``fallback`` --
    ``(position, reason)`` --, the number of ``chunks``, ``launches`` per chunk, ``launch_ms``
    summed over the chunks and the seconds by step in ``times``."""
    import time

    blends = list(blends)
    budget, device = defaults(_working_set_bytes, device)
    flags = ((SOURCES if sources or reweight else 0) | (REWEIGHT if reweight else 0)
             | (MASK if mask_footprint else 0))
    times = dict(plan=0.0, pack=0.0, device=0.0, results=0.0, loop=0.0)
    t0 = time.perf_counter()
    groups, refused = plan_render_blends(blends)
    fallback = sorted(refused.items())
    results = [None] * len(blends)
    launch_ms = np.zeros(3)
    n_chunks = 0
    times["plan"] = time.perf_counter() - t0
    for key, idx in groups.items():
        t0 = time.perf_counter()
        plans = {}
        for i in idx:
            try:
                plans[i] = plan_blend(blends[i], key)
            except ValueError as why:
                fallback.append((i, "at run time: {}".format(why)))
        items = [(i, _plan_bytes(plans[i], key, flags)) for i in idx if i in plans]
        times["plan"] += time.perf_counter() - t0
        for chunk in chunks(items, budget):
            t0 = time.perf_counter()
            packed = pack([plans[i] for i in chunk], key, flags)
            t1 = time.perf_counter()
            out = _run_chunk(packed, key, flags, device)
            launch_ms += out["launch_ms"]
            n_chunks += 1
            t2 = time.perf_counter()
            made = _results([blends[i] for i in chunk], packed, out, flags)
            for i, res in zip(chunk, made):
                if all(np.isfinite(r).all() for r in res["rendered"]):
                    results[i] = res
                else:
                    fallback.append((i, "at run time: a model value that is not finite"))
            t3 = time.perf_counter()
            times["pack"] += t1 - t0
            times["device"] += t2 - t1
            times["results"] += t3 - t2
    t0 = time.perf_counter()
    for i, res in enumerate(results):
        if res is None:
            results[i] = render_blend_host(blends[i], sources=sources, reweight=reweight,
                                           mask_footprint=mask_footprint)
    times["loop"] = time.perf_counter() - t0
    if _report is not None:
        _report["groups"] = groups
        _report["fallback"] = sorted(fallback)
        _report["chunks"] = n_chunks
        _report["launches"] = 3
        _report["launch_ms"] = tuple(float(v) for v in launch_ms)
        _report["times"] = times
    return results
