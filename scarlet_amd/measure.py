"""Post-fit measurements on components or model cubes (reference
scarlet/measure.py:6-149).  The per-source functions are host NumPy on downloaded models;
``measure_blends`` forms the same quantities for a catalogue of blends on the device
(csrc/measure_sources.hip).  Nothing here is on the fitting path."""

import numpy as np

from ._catalog import call_args, cat, chunks, defaults


def _model_and_origin(component):
    if hasattr(component, "get_model"):
        return component.get_model(), np.array(component.bbox.origin)
    return np.asarray(component), 0


def max_pixel(component):
    """Index (channel, y, x) of the brightest model pixel, in frame coordinates for
    a component."""
    model, origin = _model_and_origin(component)
    return tuple(np.array(np.unravel_index(np.argmax(model), model.shape)) + origin)


def flux(component):
    """Total flux per channel."""
    model, _ = _model_and_origin(component)
    return model.sum(axis=(1, 2))


def centroid(component):
    """Flux-weighted mean index along every axis (channel, y, x)."""
    model, origin = _model_and_origin(component)
    total = model.sum()
    grids = np.indices(model.shape)
    return np.array([(g * model).sum() for g in grids]) / total + origin


def snr(component, observations):
    """Matched-filter signal-to-noise with the rendered, flux-normalised model as
    the weight function: ``sum(M W) / sqrt(sum(var W^2))`` over all observations."""
    if not hasattr(observations, "__iter__"):
        observations = (observations,)
    if hasattr(component, "get_model"):
        model = component.get_model(frame=observations[0].model_frame)
    else:
        model = np.asarray(component)
    signal, weight, var = [], [], []
    for obs in observations:
        rendered = obs.render(model)
        signal.append(rendered.reshape(-1))
        weight.append((rendered / rendered.sum(axis=(-2, -1))[:, None, None]).reshape(-1))
        var.append((np.asarray(obs.noise_rms) ** 2).reshape(-1))
    signal, weight, var = map(np.concatenate, (signal, weight, var))
    return (signal * weight).sum() / np.sqrt((var * weight * weight).sum())


def moments(component, N=2, centroid=None, weight=None):
    """Image moments ``M[p, q] = sum (a0 - c0)^p (a1 - c1)^q model weight`` for all
    ``p + q <= N``, where a0 / a1 are the indices along the first / second spatial
    axis and ``centroid = (c1, c0)`` (the reference's convention, measure.py:132-139);
    per channel for a cube."""
    model, _ = _model_and_origin(component)
    if weight is None:
        weight = 1
    else:
        assert model.shape == np.shape(weight)
    if centroid is None:
        centroid = np.array(model.shape) // 2
    a0, a1 = np.indices(model.shape[-2:], dtype=np.float64)
    a1 = a1 - centroid[0]
    a0 = a0 - centroid[1]
    if model.ndim == 3:
        a0, a1 = a0[None], a1[None]
    return {
        (p, n - p): (a1**p * a0 ** (n - p) * model * weight).sum(axis=(-2, -1))
        for n in range(N + 1)
        for p in range(n + 1)
    }


# ---------------------------------------------------------------------------
# measure_blends: the functions above for a catalogue of Blends, one device batch per group
# ---------------------------------------------------------------------------
# csrc/measure_sources.hip: 16 x 16 tiles, the window of a tile's taps in LDS
_TILE = 16
MAX_STAMP = 63
MAX_BOX_SIDE = 1 << 14
_RECORD = 8    # SMI_MEASURE_SOURCES_RECORD
_RENDERED = 3  # sum R, sum R^2, sum R^2 / w

_SOURCE_DESC = np.dtype([("y0", "i4"), ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("fh", "i4"),
                         ("fw", "i4"), ("comp0", "i4"), ("n_comp", "i4"), ("band0", "i4"),
                         ("n_band", "i4")], align=True)
_COMP_DESC = np.dtype([("y0", "i4"), ("x0", "i4"), ("h", "i4"), ("w", "i4"), ("sed_off", "i8"),
                       ("morph_off", "i8")], align=True)
_BAND_DESC = np.dtype([("channel", "i4"), ("reserved", "i4"), ("stamp_off", "i8"),
                       ("weight_off", "i8")], align=True)


def table_dtype(C, C_obs):
    """The row of ``measure_blends`` for a model frame of ``C`` bands and observations of
    ``C_obs`` bands in all."""
    C, C_obs = int(C), int(C_obs)
    return np.dtype([
        ("n_components", "i4"), ("box", "i4", (4,)),
        ("flux", "f8", (C,)), ("sums", "f8", (C, 5)),
        ("peak", "i8", (3,)), ("peak_value", "f8"),
        ("centroid", "f8", (3,)), ("moments", "f8", (C, 3)),
        ("rendered_flux", "f8", (C_obs,)), ("rendered_sq", "f8", (C_obs,)),
        ("rendered_var", "f8", (C_obs,)), ("snr", "f8"),
    ])


class _Refused(Exception):
    pass


def _leaves(src, inside=()):
    """The ``FactorizedComponent``s a source is the sum of, in the order they are added, each
    checked against the boxes ``inside`` of the containers above it."""
    from .component import CombinedComponent, FactorizedComponent
    from .source import NullSource

    if isinstance(src, NullSource):
        return []
    if isinstance(src, CombinedComponent):
        if src.operation != "add":
            raise _Refused("CombinedComponent('{}')".format(src.operation))
        return [leaf for child in src.children for leaf in _leaves(child, inside + (src.bbox,))]
    if not isinstance(src, FactorizedComponent):
        raise _Refused("{} is not a sum of factorized components".format(type(src).__name__))
    box, frame = src.bbox, src.frame
    if box.D != 3 or box.origin[0] != frame.bbox.origin[0] or box.shape[0] != frame.C:
        raise _Refused("a component whose channel box is not the frame's")
    mbox = src.children[1].bbox
    if not (mbox.D == 2 or (mbox.D == 3 and mbox.shape[0] == 1)):
        raise _Refused("a morphology with an image per band")
    if tuple(mbox.shape[-2:]) != tuple(box.shape[1:]) or min(box.shape) < 1:
        raise _Refused("a morphology that does not fill its component's box")
    if max(box.shape[1:]) > MAX_BOX_SIDE:
        raise _Refused("a box beyond {} pixels a side".format(MAX_BOX_SIDE))
    for outer in inside:
        if (outer & box) != box:
            raise _Refused("a component's box leaves its source's box")
    return [src]


def _covers(slices, shape):
    return all(isinstance(s, slice) and range(*s.indices(n)) == range(n)
               for s, n in zip(slices, shape))


def _channels(renderer, C_obs):
    """The model band every observed band renders: ``channel_map`` spelled out."""
    cmap = renderer.channel_map
    if cmap is None:
        return list(range(C_obs))
    if isinstance(cmap, slice):
        return list(range(*cmap.indices(renderer.model_frame.C)))
    return [int(c) for c in cmap]


def _refusal(blend, zero_weights=False, null_subset=False, plain_data=False):
    """``(reason, None)`` why the device path of ``measure_blends`` does not take a blend, or
    ``(None, (C, kh, kw))``: its group.  ``render_blends`` asks with all three switches on:
    ``zero_weights`` lets weights be zero (finite and not negative: they enter chi^2 and the
    mask only), ``null_subset`` takes a ``NullRenderer`` of a subset of the frame's bands, and
    ``plain_data`` wants the data to be a plain float32 array as well.  Host only."""
    from .renderer import ConvolutionRenderer, NullRenderer

    frame = blend.frame
    if np.dtype(frame.dtype) != np.float32:
        return "frame dtype {} is not float32".format(np.dtype(frame.dtype).name), None
    try:
        for src in blend.sources:
            if getattr(src, "frame", None) is not frame:
                raise _Refused("a source of another frame")
            _leaves(src)
    except _Refused as why:
        return str(why), None
    shape, stamp = tuple(frame.shape), None
    for obs in blend.observations:
        renderer = getattr(obs, "renderer", None)
        if renderer is None or getattr(obs, "model_frame", None) is not frame:
            return "an observation that is not matched to the frame", None
        if type(renderer) not in (NullRenderer, ConvolutionRenderer):
            return "renderer {} is neither ConvolutionRenderer nor NullRenderer".format(
                type(renderer).__name__), None
        if (tuple(obs.shape[1:]) != shape[1:]
                or not all(_covers(sl[1:], shape[1:]) for sl in renderer.slices)):
            return "an observation that does not cover exactly the model frame", None
        channels = _channels(renderer, obs.shape[0])
        if len(channels) != obs.shape[0] or not all(0 <= c < shape[0] for c in channels):
            return "an observation whose bands are not bands of the frame", None
        if not null_subset and type(renderer) is NullRenderer and renderer.channel_map is not None:
            # (its rendering is the whole model: measure.snr has no value for it)
            return "a NullRenderer of a subset of the frame's bands", None
        if type(renderer) is ConvolutionRenderer:
            kshape = tuple(np.shape(renderer.diff_kernel.image))
            if len(kshape) != 3 or kshape[0] not in (1, obs.shape[0]):
                return "a difference kernel that is not one stamp per band", None
            if kshape[1] % 2 == 0 or kshape[2] % 2 == 0:
                return "even difference-kernel stamp", None
            if max(kshape[1:]) > MAX_STAMP:
                return "difference-kernel stamp beyond {0} x {0}".format(MAX_STAMP), None
            if stamp is not None and stamp != kshape[1:]:
                return "ConvolutionRenderers with different stamp shapes", None
            stamp = kshape[1:]
        weights = obs.weights
        for name, image in (("weights", weights),) + ((("data", obs.data),) if plain_data else ()):
            if (type(image) is not np.ndarray or image.dtype != np.float32
                    or image.shape != tuple(obs.shape)):
                return "{} that are not a plain float32 array".format(name), None
        low = weights.min()
        if not ((low >= 0 if zero_weights else low > 0) and np.isfinite(weights.max())):
            return "a weight that is {}negative or not finite".format(
                "" if zero_weights else "zero, "), None
    kh, kw = (1, 1) if stamp is None else stamp
    return None, (int(shape[0]), int(kh), int(kw))


def plan_measure_blends(blends):
    """``(groups, fallback)`` of ``measure_blends``, without touching the GPU or the library:
    the positions of the blends of every device group, keyed by ``(C, kh, kw)`` -- model bands
    and stamp shape, (1, 1) without a convolution -- in order of first appearance and in list
    order inside a group, and ``{position: reason}`` of the blends that go through the
    per-source functions."""
    groups, fallback = {}, {}
    for i, blend in enumerate(blends):
        reason, key = _refusal(blend)
        if reason is None:
            groups.setdefault(key, []).append(i)
        else:
            fallback[i] = reason
    return groups, fallback


def _rect(box):
    """(y0, x0, h, w) of the spatial part of a box."""
    return (int(box.origin[-2]), int(box.origin[-1]), int(box.shape[-2]), int(box.shape[-1]))


def plan_blend(blend, key):
    """What the device needs of one blend of group ``key``, coordinates relative to the frame's
    corner: ``sources`` -- per source ``(rect, components)``, a component ``(rect, spectrum,
    image)`` in float64, no components for a null source --, ``bands`` -- per observed band,
    observations in a row, ``(model band, stamp, weights)`` in float32 -- and the frame's
    ``shape``.  Raises ``ValueError`` for what only the values show."""
    from .renderer import ConvolutionRenderer

    C, kh, kw = key
    frame = blend.frame
    fy, fx = frame.bbox.origin[1:]
    sources = []
    for src in blend.sources:
        comps = []
        for leaf in _leaves(src):
            spectrum, morphology = leaf.children
            sed = np.asarray(spectrum.get_model(), dtype=np.float64).reshape(-1)
            image = np.asarray(morphology.get_model(), dtype=np.float64)
            y0, x0, h, w = _rect(leaf.bbox)
            if sed.shape != (C,) or image.size != h * w:
                raise ValueError("a spectrum or morphology that does not fill its box")
            comps.append(((y0 - fy, x0 - fx, h, w), sed, image.reshape(h, w)))
        y0, x0, h, w = _rect(src.bbox)
        sources.append(((y0 - fy, x0 - fx, h, w), comps))
    bands = []
    delta = np.zeros((kh, kw), np.float32)
    delta[kh // 2, kw // 2] = 1
    for obs in blend.observations:
        renderer = obs.renderer
        n = obs.shape[0]
        if type(renderer) is ConvolutionRenderer:
            stamps = np.broadcast_to(np.asarray(renderer.kernel_image(), np.float32), (n, kh, kw))
        else:
            stamps = [delta] * n  # the identity: the single tap 1
        for b, channel in enumerate(_channels(renderer, n)):
            bands.append((channel, stamps[b], obs.weights[b]))
    return dict(sources=sources, bands=bands, shape=tuple(frame.shape))


def region_of(rect, frame_hw, kh, kw):
    """``(y0, x0, h, w)`` of the frame pixels a source's rendered model reaches: its box grown by
    the stamp's half and clipped to the frame (``region_of`` of csrc/measure_sources.hip)."""
    y0, x0, h, w = rect
    gy0, gx0 = max(y0 - kh // 2, 0), max(x0 - kw // 2, 0)
    gh = max(min(y0 + h + kh // 2, frame_hw[0]) - gy0, 0)
    gw = max(min(x0 + w + kw // 2, frame_hw[1]) - gx0, 0)
    return gy0, gx0, gh, gw


def _region_tiles(rect, frame_hw, kh, kw):
    """Tiles of the region of a source."""
    _, _, gh, gw = region_of(rect, frame_hw, kh, kw)
    return -(-gh // _TILE) * -(-gw // _TILE)


def _plan_bytes(plan, key):
    """Bytes of the device working set of a planned blend."""
    _, kh, kw = key
    _, H, W = plan["shape"]
    n_band = len(plan["bands"])
    need = n_band * (4 * H * W + 4 * kh * kw + _BAND_DESC.itemsize)
    for rect, comps in plan["sources"]:
        if not comps:
            continue
        tiles = _region_tiles(rect, (H, W), kh, kw)
        need += _SOURCE_DESC.itemsize + n_band * (tiles * (12 + 8 * _RENDERED) + 16 + 8 * _RENDERED)
        need += 8 * _RECORD * key[0]
        need += sum(8 * (c[2].size + c[1].size) + _COMP_DESC.itemsize for c in comps)
    return need


class _Tables:
    """The band and component tables of a chunk with their packed buffers, filled blend by
    blend: what ``pack`` here and ``rendering.pack`` share."""

    def __init__(self, plans, key, n_comps):
        self.C, self.kh, self.kw = key
        self.comps = np.zeros(n_comps, _COMP_DESC)
        self.bands = np.zeros(sum(len(p["bands"]) for p in plans), _BAND_DESC)
        self.seds, self.morphs, self.stamps, self.weights = [], [], [], []
        self.sed_off = self.morph_off = self.weight_off = 0
        self.k = self.b_at = 0

    def add_bands(self, plan):
        """The rows of a blend's observed bands."""
        _, H, W = plan["shape"]
        for channel, stamp, weight in plan["bands"]:
            self.bands[self.b_at] = (channel, 0, self.b_at * self.kh * self.kw, self.weight_off)
            self.stamps.append(np.ascontiguousarray(stamp, np.float32).reshape(-1))
            self.weights.append(np.ascontiguousarray(weight, np.float32).reshape(-1))
            self.weight_off += H * W
            self.b_at += 1

    def add_components(self, parts):
        """The rows of a source's components."""
        for crect, sed, image in parts:
            self.comps[self.k] = crect + (self.sed_off, self.morph_off)
            self.seds.append(sed)
            self.morphs.append(image.reshape(-1))
            self.sed_off += self.C
            self.morph_off += image.size
            self.k += 1

    def packed(self):
        return dict(comps=self.comps, bands=self.bands, seds=cat(self.seds, np.float64),
                    morphs=cat(self.morphs, np.float64), stamps=cat(self.stamps, np.float32),
                    weights=cat(self.weights, np.float32))


def pack(plans, key):
    """Descriptor tables and packed buffers of one chunk (the arguments of
    smi_measure_sources_f32), one array per kind, and ``layout``: per blend ``(rows, live,
    C_obs)`` -- its number of sources, the rows of those with components (the device's sources,
    in order) and its observed bands."""
    C = key[0]
    live = [(p, s) for p in plans for s in p["sources"] if s[1]]
    sources = np.zeros(len(live), _SOURCE_DESC)
    t = _Tables(plans, key, sum(len(s[1]) for _, s in live))
    layout = []
    s_at = 0
    for p in plans:
        _, H, W = p["shape"]
        band0 = t.b_at
        t.add_bands(p)
        rows = []
        for row, (rect, parts) in enumerate(p["sources"]):
            if not parts:
                continue
            rows.append(row)
            sources[s_at] = rect + (H, W, t.k, len(parts), band0, t.b_at - band0)
            s_at += 1
            t.add_components(parts)
        layout.append((len(p["sources"]), np.array(rows, np.int64), t.b_at - band0))
    return dict(t.packed(), sources=sources, layout=layout, n_record=len(live) * C * _RECORD,
                n_rendered=int(sources["n_band"].sum()) * _RENDERED)


def _run_chunk(packed, key, device):
    """One smi_measure_sources_f32 call: ``records`` (sources, C, 8) and ``rendered``
    (observed bands of all sources in a row, 3)."""
    import ctypes

    from . import _lib

    C, kh, kw = key
    lib = _lib.load()
    records = np.empty(packed["n_record"], np.float64)
    rendered = np.empty(packed["n_rendered"], np.float64)
    f32, f64 = ctypes.c_float, ctypes.c_double
    args = call_args([packed[name] for name in ("sources", "comps", "bands")],
                     [(packed["seds"], f64), (packed["morphs"], f64), (packed["stamps"], f32),
                      (packed["weights"], f32)], [(records, f64), (rendered, f64)])
    _lib.check(lib.smi_measure_sources_f32(device, C, kh, kw, *args))
    return records.reshape(-1, C, _RECORD), rendered.reshape(-1, _RENDERED)


def last_launch_ms():
    """Milliseconds the model, render and reduce launches of this thread's last device call
    took (events around them)."""
    import ctypes

    from . import _lib

    ms = (ctypes.c_double * 3)()
    _lib.check(_lib.load().smi_measure_sources_last_launch_ms(ms))
    return tuple(ms)


def snr_of_sums(S, Q, V):
    """``measure.snr`` from the per-band sums of the rendered model R: S = sum R, Q = sum R^2,
    V = sum R^2 var.  With the weight function R / S of every band,
    ``sum_b Q_b / S_b / sqrt(sum_b V_b / S_b^2)``."""
    S, Q, V = (np.asarray(a, np.float64) for a in (S, Q, V))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (Q / S).sum(axis=-1) / np.sqrt((V / (S * S)).sum(axis=-1))


def fill_table(layout, sources, records, rendered):
    """The tables of one chunk from the device's sums, all its sources at once.

    ``layout``: per blend ``(rows, live, C_obs)`` as ``pack`` returns it; ``sources``: the
    source descriptors (box, components, bands); ``records`` (sources, C, 8) and ``rendered``
    (bands of all sources in a row, 3): the outputs of smi_measure_sources_f32.  Returns one
    structured array per blend; rows that are not ``live`` stay zero."""
    S, C = records.shape[:2]
    y0, x0, w = (sources[f].astype(np.int64) for f in ("y0", "x0", "w"))
    flux, sums = records[:, :, 0], records[:, :, 1:6]
    band = np.argmax(records[:, :, 6], axis=1)  # (the first of equal bands, as np.argmax)
    each = np.arange(S)
    peak_value = records[each, band, 6]
    at = records[each, band, 7].astype(np.int64)
    peak = np.stack([band, y0 + at // np.maximum(w, 1), x0 + at % np.maximum(w, 1)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        total = flux.sum(axis=1)
        centroid = np.stack([(np.arange(C) * flux).sum(axis=1) / total,
                             sums[:, :, 0].sum(axis=1) / total + y0,
                             sums[:, :, 1].sum(axis=1) / total + x0], axis=1)
        # central moments about every band's own centroid (Sy / F, Sx / F)
        Sy, Sx = sums[:, :, 0], sums[:, :, 1]
        moments = np.stack([sums[:, :, 2] - Sy * Sy / flux, sums[:, :, 3] - Sy * Sx / flux,
                            sums[:, :, 4] - Sx * Sx / flux], axis=2)
    tables, s_at, r_at = [], 0, 0
    for rows, live, C_obs in layout:
        table = np.zeros(rows, table_dtype(C, C_obs))
        n = len(live)
        sl = slice(s_at, s_at + n)
        table["n_components"][live] = sources["n_comp"][sl]
        table["box"][live] = np.stack([sources[f][sl] for f in ("y0", "x0", "h", "w")], axis=1)
        table["flux"][live], table["sums"][live] = flux[sl], sums[sl]
        table["peak"][live], table["peak_value"][live] = peak[sl], peak_value[sl]
        table["centroid"][live], table["moments"][live] = centroid[sl], moments[sl]
        r = rendered[r_at:r_at + n * C_obs].reshape(n, C_obs, _RENDERED)
        table["rendered_flux"][live] = r[:, :, 0]
        table["rendered_sq"][live] = r[:, :, 1]
        table["rendered_var"][live] = r[:, :, 2]
        table["snr"][live] = snr_of_sums(r[:, :, 0], r[:, :, 1], r[:, :, 2])
        tables.append(table)
        s_at += n
        r_at += n * C_obs
    return tables


def measure_sources(blend):
    """The table of one blend through the per-source functions above, on the host and with one
    rendering per source and observation: what ``measure_blends`` returns for a blend the device
    does not take.  The box is relative to the frame's corner."""
    from .component import CombinedComponent, FactorizedComponent
    from .source import NullSource

    def count(c):
        if isinstance(c, CombinedComponent):
            return sum(count(child) for child in c.children)
        return int(isinstance(c, FactorizedComponent))

    frame = blend.frame
    observations = tuple(blend.observations)
    C = frame.C
    table = np.zeros(len(blend.sources), table_dtype(C, sum(o.shape[0] for o in observations)))
    for row, src in zip(table, blend.sources):
        if isinstance(src, NullSource):
            continue
        model = np.asarray(src.get_model())
        fy, fx = frame.bbox.origin[1:]
        y0, x0, h, w = _rect(src.bbox)
        row["n_components"] = count(src)
        row["box"] = (y0 - fy, x0 - fx, h, w)
        row["flux"] = flux(src)
        y, x = np.indices((h, w), dtype=np.float64)
        terms = (y, x, y * y, y * x, x * x)
        row["sums"] = np.stack([(t * model).sum(axis=(1, 2)) for t in terms], axis=1)
        at = max_pixel(src)
        row["peak"] = at
        row["peak_value"] = model[tuple(np.array(at) - np.array(src.bbox.origin))]
        with np.errstate(divide="ignore", invalid="ignore"):
            row["centroid"] = centroid(src)
            for c in range(C):
                F = model[c].sum()
                m = moments(model[c], N=2, centroid=((x * model[c]).sum() / F,
                                                     (y * model[c]).sum() / F))
                row["moments"][c] = (m[0, 2], m[1, 1], m[2, 0])
            full = src.get_model(frame=frame)
            R = np.concatenate([np.asarray(o.render(full), np.float64) for o in observations])
            var = np.concatenate([np.asarray(o.noise_rms, np.float64) ** 2 for o in observations])
            row["rendered_flux"] = R.sum(axis=(1, 2))
            row["rendered_sq"] = (R * R).sum(axis=(1, 2))
            row["rendered_var"] = (R * R * var).sum(axis=(1, 2))
            row["snr"] = snr(src, observations)
    return table


def measure_blends(blends, device=None, _working_set_bytes=None, _report=None):
    """``scarlet.measure`` for a catalogue: one structured array (``table_dtype``) per blend
    with a row per entry of ``blend.sources`` -- components and box, ``flux``, the first- and
    second-moment ``sums`` per band, ``peak`` (``max_pixel``) and its value, ``centroid``,
    central ``moments`` per band, per observed band the sums of the source's model alone
    rendered into it, and ``snr`` -- with three launches of csrc/measure_sources.hip per chunk
    of blends that share the number of bands and the stamp shape; frames, boxes, source and
    observation counts may differ.

    The model is evaluated in float64 from spectrum and morphology image (``peak`` is exactly
    ``max_pixel``'s), rendered by a float64 tap loop over the renderer's float32 stamp on the
    pixels it can reach, and every sum has an order fixed by the source's box, its frame and the
    stamp shape: a blend's table has the same bits alone, in any list and in any chunk.
    ``measure.snr`` renders in float32 through the FFT; its value differs in the last float32
    digits.  A nested ``CombinedComponent`` is added component by component.

    Blends the device does not take (``plan_measure_blends`` says why) and blends whose sums
    are not finite go through ``measure_sources``, after the device groups and in list order.
    ``device``: GPU index (default 0).  ``_report``: a dict that receives ``fallback`` --
    ``(position, reason)`` --, the number of ``launches`` and ``launch_ms`` of the last chunk
    and the seconds by step in ``times``."""
    import time

    blends = list(blends)
    budget, device = defaults(_working_set_bytes, device)
    times = dict(plan=0.0, pack=0.0, device=0.0, table=0.0, loop=0.0)
    t0 = time.perf_counter()
    groups, refused = plan_measure_blends(blends)
    fallback = sorted(refused.items())
    tables = [None] * len(blends)
    times["plan"] = time.perf_counter() - t0
    for key, idx in groups.items():
        t0 = time.perf_counter()
        plans = {}
        for i in idx:
            try:
                plans[i] = plan_blend(blends[i], key)
            except ValueError as why:
                fallback.append((i, "at run time: {}".format(why)))
        items = [(i, _plan_bytes(plans[i], key)) for i in idx if i in plans]
        times["plan"] += time.perf_counter() - t0
        for chunk in chunks(items, budget):
            t0 = time.perf_counter()
            packed = pack([plans[i] for i in chunk], key)
            t1 = time.perf_counter()
            if len(packed["sources"]):
                records, rendered = _run_chunk(packed, key, device)
                if _report is not None:
                    _report["launches"], _report["launch_ms"] = 3, last_launch_ms()
            else:
                records = np.zeros((0, key[0], _RECORD))
                rendered = np.zeros((0, _RENDERED))
            t2 = time.perf_counter()
            made = fill_table(packed["layout"], packed["sources"], records, rendered)
            s_at = r_at = 0
            for i, table, (_, live, C_obs) in zip(chunk, made, packed["layout"]):
                n = len(live)
                if (np.isfinite(records[s_at:s_at + n]).all()
                        and np.isfinite(rendered[r_at:r_at + n * C_obs]).all()):
                    tables[i] = table
                else:
                    fallback.append((i, "at run time: a model value that is not finite"))
                s_at, r_at = s_at + n, r_at + n * C_obs
            t3 = time.perf_counter()
            times["pack"] += t1 - t0
            times["device"] += t2 - t1
            times["table"] += t3 - t2
    t0 = time.perf_counter()
    for i, table in enumerate(tables):
        if table is None:
            tables[i] = measure_sources(blends[i])
    times["loop"] = time.perf_counter() - t0
    if _report is not None:
        _report["times"] = times
        _report["fallback"] = sorted(fallback)
    return tables
