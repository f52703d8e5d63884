"""A catalogue row per source: fluxes, centroid, second moments, brightest pixel and
signal-to-noise of the reweighted fluxes of ``weight_blends``, without the flux cubes leaving
the device.

The device (csrc/lite_measure.hip) forms every source's flux cube as ``weight_blends`` does
and returns, per source and band, eight float64 sums over it and its brightest pixel; the row
is derived from those on the host.  Blends are grouped, chunked, planned and packed by
``lite/measure.py``, so a measured catalogue is batched exactly like a reweighted one, and the
blends it sends to ``weight_sources`` are measured here in NumPy (``records_of``)."""

import numpy as np

from .._catalog import call_args, chunks, defaults
from ..bbox import overlapped_slices
from . import measure
from .utils import insert_image

# per (source, band), as smi_lite_measure_* writes them (SMI_LITE_MEASURE_RECORD): sum M,
# sum M^2, sum f, sum y f, sum x f, sum y^2 f, sum y x f, sum x^2 f, the largest f, and
# y * w + x of the first pixel that holds it; y, x count from the corner of the flux box
RECORD = 10


def table_dtype(C):
    """The structured dtype of a blend's table for ``C`` bands."""
    C = int(C)
    return np.dtype([
        ("n_components", "i4"), ("box", "i4", (4,)), ("flux", "f8", (C,)), ("sums", "f8", (C, 5)),
        ("model_flux", "f8", (C,)), ("model_sq", "f8", (C,)), ("peak", "i4", (3,)),
        ("peak_value", "f8"), ("centroid", "f8", (2,)), ("moments", "f8", (C, 3)), ("snr", "f8")])


def records_of(flux, model):
    """The ``(C, RECORD)`` float64 records of a source in NumPy: ``flux`` its reweighted
    ``(C, h, w)`` cube and ``model`` its convolved model clipped at 0 on the same box.  The
    host measurement of the blends the device does not take."""
    f = np.asarray(flux, np.float64)
    m = np.asarray(model, np.float64)
    C, h, w = f.shape
    assert m.shape == f.shape and h * w > 0
    y, x = np.indices((h, w), dtype=np.float64)
    out = np.empty((C, RECORD), np.float64)
    terms = (m, m * m, f, y * f, x * f, (y * y) * f, (y * x) * f, (x * x) * f)
    for k, t in enumerate(terms):
        out[:, k] = t.sum(axis=(1, 2))
    at = f.reshape(C, -1).argmax(axis=1)  # the first maximum of every band
    out[:, 8] = f.reshape(C, -1)[np.arange(C), at]
    out[:, 9] = at
    return out


def snr_of(model_flux, model_sq, noise_rms):
    """Erben (2001), eq. 16 over bands, with the flux-normalised rendered model as the weight
    function (reference scarlet/measure.py:89-102): with S = sum M and Q = sum M^2 of a band
    and n its noise, ``sum(Q / S) / sqrt(sum(n^2 Q / S^2))`` over the bands with S != 0; 0
    when there is none.  The bands are the last axis."""
    S, Q = np.asarray(model_flux, np.float64), np.asarray(model_sq, np.float64)
    n = np.asarray(noise_rms, np.float64)
    keep = S != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        signal = np.where(keep, Q / S, 0).sum(axis=-1)
        noise = np.sqrt(np.where(keep, n * n * Q / (S * S), 0).sum(axis=-1))
        return np.where(keep.any(axis=-1), signal / noise, 0.0)


def fill_table(table, n_components, boxes, index, records, noise_rms, band0):
    """Fill the rows of a table at once.  Per row: ``n_components`` (0: a null source, the
    row stays all zeros), ``boxes`` ``(y0, x0, h, w)`` of the flux box, ``index`` of its
    ``(C, RECORD)`` entry in ``records`` (-1: an empty box, no sums), ``noise_rms`` per band,
    ``band0`` the first band of the flux box (``observation.bbox.origin[0]``)."""
    n = len(table)
    if n == 0:
        return
    live = np.asarray(n_components, np.int64).reshape(n) > 0
    boxes = np.asarray(boxes, np.int64).reshape(n, 4)
    index = np.asarray(index, np.int64).reshape(n)
    has = live & (index >= 0)
    rec = np.zeros((n,) + table["flux"].shape[1:] + (RECORD,), np.float64)
    rec[..., 9] = -1
    if has.any():
        rec[has] = np.asarray(records, np.float64)[index[has]]
    table["n_components"] = np.where(live, n_components, 0)
    table["box"] = np.where(live[:, None], boxes, 0)
    table["model_flux"], table["model_sq"] = rec[..., 0], rec[..., 1]
    table["flux"], table["sums"] = rec[..., 2], rec[..., 3:8]
    # the brightest pixel over the bands: argmax takes the first, so the lower band wins ties
    seen = rec[..., 9] >= 0
    best = np.where(seen, rec[..., 8], -np.inf).argmax(axis=1)
    rows = np.arange(n)
    found = seen[rows, best]
    at = np.where(found, rec[rows, best, 9], 0).astype(np.int64)
    width = np.maximum(boxes[:, 3], 1)
    peak = np.stack([np.asarray(band0, np.int64).reshape(n) + best, boxes[:, 0] + at // width,
                     boxes[:, 1] + at % width], axis=1)
    table["peak"] = np.where(found[:, None], peak, 0)
    table["peak_value"] = np.where(found, rec[rows, best, 8], 0)
    flux, sums = rec[..., 2], rec[..., 3:8]
    with np.errstate(divide="ignore", invalid="ignore"):
        total = flux.sum(axis=1)
        cy, cx = sums[..., 0].sum(axis=1) / total, sums[..., 1].sum(axis=1) / total
        centroid = np.stack([cy + boxes[:, 0], cx + boxes[:, 1]], axis=1)
        cy, cx = cy[:, None], cx[:, None]
        moments = np.stack([sums[..., 2] - 2 * cy * sums[..., 0] + cy * cy * flux,
                            sums[..., 3] - cy * sums[..., 1] - cx * sums[..., 0] + cy * cx * flux,
                            sums[..., 4] - 2 * cx * sums[..., 1] + cx * cx * flux], axis=2)
    table["centroid"] = np.where(live[:, None], centroid, 0)
    table["moments"] = np.where(live[:, None, None], moments, 0)
    table["snr"] = np.where(live, snr_of(rec[..., 0], rec[..., 1], noise_rms), 0)


def fill_row(row, n_components, box, records, noise_rms, band0=0):
    """``fill_table`` for one row: ``records`` ``(C, RECORD)``, None for an empty box."""
    table = np.zeros(1, row.dtype)
    C = table["flux"].shape[1]
    fill_table(table, [n_components], [box], [-1 if records is None else 0],
               None if records is None else np.asarray(records, np.float64).reshape(1, C, RECORD),
               np.asarray(noise_rms, np.float64).reshape(1, C), [band0])
    for name in row.dtype.names:
        row[name] = table[0][name]


def _noise(obs):
    C = obs.images.shape[0]
    return np.broadcast_to(np.asarray(obs.noise_rms, np.float64), (C,))


def _source_model(blend, src):
    """The ``model[in_box]`` of ``weight_sources``: the source's convolved model clipped at
    0, on its flux box."""
    obs = blend.observation
    py, px = obs.psfs.shape[-2] // 2, obs.psfs.shape[-1] // 2
    bbox = src.bbox.grow((0, py, px))
    model = obs.convolve(insert_image(bbox, src.bbox, src.get_model()), mode="real")
    model[model < 0] = 0
    return model[overlapped_slices(obs.bbox, bbox)[1]]


def _measure_fallback(blend, table, mask_footprint, keep_flux):
    """``weight_sources`` and the NumPy measurement, for a blend the device does not take."""
    obs = blend.observation
    before = [(src.flux, src.flux_box) for src in blend.sources]
    measure.weight_sources(blend, mask_footprint)
    noise = _noise(obs)
    n_components, boxes, index, records = [], [], [], []
    for src in blend.sources:
        n_components.append(len(src.components))
        _, y0, x0 = src.flux_box.origin
        _, h, w = src.flux_box.shape
        boxes.append((y0, x0, h, w))
        index.append(len(records) if len(src.components) and h * w > 0 else -1)
        if index[-1] >= 0:
            records.append(records_of(src.flux, _source_model(blend, src)))
    fill_table(table, n_components, boxes, index, records, noise[None].repeat(len(table), 0),
               [obs.bbox.origin[0]] * len(table))
    if not keep_flux:
        for src, (flux, flux_box) in zip(blend.sources, before):
            src.flux, src.flux_box = flux, flux_box


def _run_chunk(packed, key, device, keep_flux):
    """One smi_lite_measure_* call: ``(records, cubes)`` of a chunk -- ``(n_sources, C,
    RECORD)`` in the order of ``packed["results"]``, and the packed fluxes or None."""
    import ctypes

    from .. import _lib

    dtype, C, kh, kw = key
    lib = _lib.load()
    ct, fn = ((ctypes.c_double, lib.smi_lite_measure_f64) if dtype == np.float64
              else (ctypes.c_float, lib.smi_lite_measure_f32))
    out = np.empty(packed["n_out"], dtype) if keep_flux else None
    records = np.zeros((len(packed["sources"]), C, RECORD), np.float64)
    args = call_args([packed[name] for name in ("blends", "sources", "comps")],
                     [(packed[name], ct) for name in ("images", "stamps", "seds", "morphs")],
                     [(out, ct), (records, ctypes.c_double)])
    _lib.check(fn(device, C, kh, kw, *args))
    return records, out


def _fill_chunk(plans, tables, packed, records):
    """Rows of the sources of a chunk, derived for the whole chunk at once; ``tables``: the
    table of every plan's blend."""
    at = {id(src): k for k, (src, _, _) in enumerate(packed["results"])}
    n_components, boxes, index, noise, band0 = [], [], [], [], []
    for p in plans:
        obs = p["blend"].observation
        b0, fy, fx = obs.bbox.origin
        rms = _noise(obs)
        for src, comp0, n, y0, x0, shape in p["sources"]:
            null = comp0 is None
            n_components.append(0 if null else n)
            boxes.append((0, 0, 0, 0) if null else (y0 + fy, x0 + fx, shape[1], shape[2]))
            index.append(at.get(id(src), -1))
            noise.append(rms)
            band0.append(b0)
    if not index:
        return
    rows = np.zeros(len(index), tables[0].dtype)
    fill_table(rows, n_components, boxes, index, records, np.array(noise), band0)
    start = 0
    for table in tables:
        table[:] = rows[start:start + len(table)]
        start += len(table)


def plan_measure_blends(blends):
    """``(groups, fallback)`` as ``measure.plan_blends``: the device groups of
    ``measure_blends`` and the blends it measures on the host."""
    return measure.plan_blends(blends)


def measure_blends(blends, mask_footprint=True, keep_flux=False, device=None,
                   _working_set_bytes=None):
    """The catalogue of many blends: a list with one structured array (``table_dtype``) per
    blend, one row per entry of ``blend.sources``, in order.

    Per source the sums of its reweighted flux ``f`` -- the ``src.flux`` of ``weight_blends``
    -- and of its convolved model ``M``, clipped at 0, over its flux box: ``flux`` (per band),
    ``sums`` (per band: y f, x f, y^2 f, y x f, x^2 f with integer y, x from the box's corner),
    ``model_flux`` and ``model_sq``; ``box`` = (y0, x0, h, w) of the flux box; ``peak`` and
    ``peak_value``: the first brightest pixel in (band, y, x) order; and derived from the sums:
    ``centroid`` (y, x), the central second ``moments`` (yy, yx, xx) per band about it, and
    ``snr`` (``snr_of``) with ``observation.noise_rms``.  A null source has ``n_components =
    0`` and an all-zero row.  Finite data are assumed.

    One device batch (three launches of lite_measure.hip) per chunk of a group of blends that
    share dtype, bands and stamp shape, as ``weight_blends``; only the sums come back.  With
    ``keep_flux`` the cubes come back too and ``src.flux`` / ``src.flux_box`` are set bit for
    bit as ``weight_blends`` sets them; without, no cube exists and the sources are left as
    they were.  Blends ``plan_measure_blends`` lists as fallback take ``weight_sources`` and
    NumPy.  ``device``: GPU index of the batches (default 0)."""
    blends = list(blends)
    budget, device = defaults(_working_set_bytes, device)
    groups, fallback = plan_measure_blends(blends)
    tables = [np.zeros(len(b.sources), table_dtype(b.observation.images.shape[0])) for b in blends]
    for key, idx in groups.items():
        plans = [measure._plan_blend(blends[i]) for i in idx]
        table_of = {id(p): tables[i] for p, i in zip(plans, idx)}
        for chunk in chunks([(p, measure._plan_bytes(p, key)) for p in plans], budget):
            packed = measure._pack(chunk, key, mask_footprint)
            records, out = _run_chunk(packed, key, device, keep_flux)
            _fill_chunk(chunk, [table_of[id(p)] for p in chunk], packed, records)
            if keep_flux:
                measure._assign(chunk, packed, out)
    for i in fallback:
        _measure_fallback(blends[i], tables[i], mask_footprint, keep_flux)
    return tables
