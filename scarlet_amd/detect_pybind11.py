"""Footprints and peaks: drop-in for the reference's compiled ``scarlet.detect_pybind11``.

``get_footprints`` runs in the library (``csrc/detect.cpp``, host code: a labelling pass
with a branch at every pixel); ``get_footprints_device`` gives the same answer for planes
that are on the GPU already (``csrc/footprints.hip``: union-find labelling, records, masks
and peaks as kernels, only the footprints' records cross to the host);
``get_footprints_batch`` does so for a list of device planes of different shapes in one chain
of launches (``csrc/footprints_batch.hip``); ``get_connected_pixels`` and ``get_peaks`` are
the single-footprint helpers of the same module, here in NumPy.

Where the reference's behaviour is undefined, this module defines it: equal-flux peaks keep
raster order (a stable sort), ``min_separation > 0`` keeps peaks brightest first and drops
every later one closer than that to a kept peak, a footprint without a strict maximum keeps an
empty peak list (the reference asserts), and large footprints do not overflow a stack (the
reference's fill is recursive).
"""

import ctypes

import numpy as np

from . import _lib


class Peak:
    """A local maximum of a footprint: pixel ``(y, x)`` in the full image and its flux."""

    def __init__(self, y, x, flux):
        self._y, self._x, self._flux = int(y), int(x), float(flux)

    @property
    def y(self):
        return self._y

    @property
    def x(self):
        return self._x

    @property
    def flux(self):
        return self._flux

    def __repr__(self):
        return "Peak(y={}, x={}, flux={!r})".format(self._y, self._x, self._flux)


class Footprint:
    """A connected set of pixels: ``footprint`` (bool mask of its bounding box), ``peaks``
    (brightest first) and ``bounds`` = ``(y0, y1, x0, x1)``, inclusive."""

    def __init__(self, footprint, peaks, bounds):
        self._footprint = np.asarray(footprint, dtype=bool)
        self.peaks = list(peaks)
        self._bounds = np.asarray(bounds, dtype=np.int32)

    @property
    def footprint(self):
        return self._footprint

    @property
    def bounds(self):
        return self._bounds


def get_footprints(image, min_separation, min_area, thresh):
    """All footprints of the 2-D ``image``: 4-connected pixels ``> int(thresh)`` (the
    reference's threshold is an ``int``), seeds in raster order, kept when the bounding box
    has more than ``min_area`` pixels and the footprint at least ``min_area``; peaks as in
    :func:`get_peaks` on the box with the pixels outside the footprint set to 0."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("get_footprints: a 2-D image is needed, got shape %s" % (image.shape,))
    lib = _lib.load()
    if image.dtype == np.float32:
        img, fn, ct = np.ascontiguousarray(image), lib.smi_get_footprints_f32, ctypes.c_float
    else:
        img = np.ascontiguousarray(image, dtype=np.float64)
        fn, ct = lib.smi_get_footprints_f64, ctypes.c_double
    counts = np.zeros(3, dtype=np.int32)
    _lib.check(fn(_lib.ptr(img, ct), img.shape[0], img.shape[1], float(min_separation),
                  int(min_area), int(thresh), _lib.ptr(counts, ctypes.c_int32)))
    n, n_mask, n_peaks = (int(v) for v in counts)
    bounds = np.zeros((n, 4), dtype=np.int32)
    masks = np.zeros(n_mask, dtype=np.uint8)
    start = np.zeros(n + 1, dtype=np.int32)
    yx = np.zeros((n_peaks, 2), dtype=np.int32)
    flux = np.zeros(n_peaks, dtype=np.float64)
    _lib.check(lib.smi_footprints_fetch(
        _lib.ptr(bounds, ctypes.c_int32), _lib.ptr(masks, ctypes.c_uint8),
        _lib.ptr(start, ctypes.c_int32), _lib.ptr(yx, ctypes.c_int32),
        _lib.ptr(flux, ctypes.c_double)))
    return _footprint_objects(bounds, masks, start, yx, flux)


def _footprint_objects(bounds, masks, start, yx, flux):
    """``Footprint``s from the arrays of ``smi_footprints_fetch``"""
    footprints = []
    offset = 0
    for f in range(len(bounds)):
        y0, y1, x0, x1 = (int(v) for v in bounds[f])
        h, w = y1 - y0 + 1, x1 - x0 + 1
        mask = masks[offset:offset + h * w].reshape(h, w).astype(bool)
        offset += h * w
        peaks = [Peak(yx[k, 0], yx[k, 1], flux[k]) for k in range(start[f], start[f + 1])]
        footprints.append(Footprint(mask, peaks, bounds[f]))
    return footprints


def _is_device_tensor(x):
    """True for a torch tensor on a GPU, without importing torch for anything else"""
    mod = type(x).__module__
    return (mod == "torch" or mod.startswith("torch.")) and hasattr(x, "data_ptr") \
        and getattr(x, "is_cuda", False)


def label_device(d_image, min_area, thresh):
    """First step of :func:`get_footprints_device` on a contiguous ``(P, H, W)`` float32 /
    float64 device tensor: one labelling call for all planes.  Returns ``(counts, work)``:
    the ``(P, 3)`` int32 array (footprints, mask bytes, strict maxima) of every plane and the
    device buffer :func:`fetch_device` reads."""
    import torch

    lib = _lib.load()
    P, H, W = d_image.shape
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.smi_footprints_device_work_bytes(P, H, W, ctypes.byref(nbytes)))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=d_image.device)
    counts = np.zeros((P, 3), dtype=np.int32)
    fn = lib.smi_footprints_device_label_f32 if d_image.dtype == torch.float32 else \
        lib.smi_footprints_device_label_f64
    stream = ctypes.c_void_p(torch.cuda.current_stream(d_image.device).cuda_stream)
    with torch.cuda.device(d_image.device):
        _lib.check(fn(ctypes.c_void_p(d_image.data_ptr()), P, H, W, int(min_area), int(thresh),
                      ctypes.c_void_p(work.data_ptr()), nbytes.value,
                      _lib.ptr(counts, ctypes.c_int32), stream))
    return counts, work


def fetch_device(d_image, plane, min_separation, counts, work):
    """Second step: the arrays ``(bounds, masks, peak_start, peak_yx, peak_flux)`` of one plane,
    in the layout of ``smi_footprints_fetch``."""
    import torch

    lib = _lib.load()
    P, H, W = d_image.shape
    c = np.ascontiguousarray(counts[plane], dtype=np.int32)
    n, n_mask, n_peaks = (int(v) for v in c)
    bounds = np.zeros((n, 4), dtype=np.int32)
    masks = np.zeros(n_mask, dtype=np.uint8)
    start = np.zeros(n + 1, dtype=np.int32)
    yx = np.zeros((n_peaks, 2), dtype=np.int32)
    flux = np.zeros(n_peaks, dtype=np.float64)
    if n:
        nbytes = ctypes.c_int64(0)
        _lib.check(lib.smi_footprints_device_fetch_bytes(_lib.ptr(c, ctypes.c_int32),
                                                         ctypes.byref(nbytes)))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=d_image.device)
        fn = lib.smi_footprints_device_fetch_f32 if d_image.dtype == torch.float32 else \
            lib.smi_footprints_device_fetch_f64
        stream = ctypes.c_void_p(torch.cuda.current_stream(d_image.device).cuda_stream)
        with torch.cuda.device(d_image.device):
            _lib.check(fn(ctypes.c_void_p(d_image.data_ptr()), P, H, W, int(plane),
                          float(min_separation), _lib.ptr(c, ctypes.c_int32),
                          ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                          nbytes.value, _lib.ptr(bounds, ctypes.c_int32),
                          _lib.ptr(masks, ctypes.c_uint8), _lib.ptr(start, ctypes.c_int32),
                          _lib.ptr(yx, ctypes.c_int32), _lib.ptr(flux, ctypes.c_double), stream))
    kept = int(start[n])  # min_separation may have dropped some of the maxima counted
    return bounds, masks, start, yx[:kept], flux[:kept]


def get_footprints_device(d_image, min_separation, min_area, thresh):
    """:func:`get_footprints` of a 2-D image, or of every plane of a 3-D stack, that lives on
    the GPU: a float32 / float64 torch device tensor (made contiguous if it is not).  Labels,
    bounds, masks and peaks are found on the device (``csrc/footprints.hip``); only the records
    of the footprints come back.  Returns the list of ``Footprint``s of a 2-D image, a list of
    such lists for a 3-D stack; all planes go through one labelling call.  The results equal
    :func:`get_footprints` of the same pixels exactly.  Host arrays: :func:`get_footprints`."""
    if not _is_device_tensor(d_image):
        raise TypeError("get_footprints_device: a torch device tensor is needed, got %s "
                        "(host arrays go through get_footprints)" % type(d_image).__name__)
    if d_image.dim() not in (2, 3):
        raise ValueError("get_footprints_device: a 2-D image or a 3-D stack is needed, got "
                         "shape %s" % (tuple(d_image.shape),))
    import torch

    if d_image.dtype not in (torch.float32, torch.float64):
        raise TypeError("get_footprints_device: float32 or float64 is needed, got %s"
                        % d_image.dtype)
    planes = (d_image if d_image.dim() == 3 else d_image[None]).contiguous()
    if planes.numel() == 0:
        raise ValueError("get_footprints_device: empty image of shape %s"
                         % (tuple(d_image.shape),))
    counts, work = label_device(planes, min_area, thresh)
    found = [_footprint_objects(*fetch_device(planes, k, min_separation, counts, work))
             for k in range(planes.shape[0])]
    return found if d_image.dim() == 3 else found[0]


# ---------------------------------------------------------------------------
# get_footprints_device for a ragged list of planes: one device chain per chunk
# ---------------------------------------------------------------------------
# Bytes of one chunk's work buffer (labels, records, scan sums: 32 bytes per pixel and a little
# more): a group whose planes need more is cut into chunks.
FOOTPRINT_BATCH_BYTES = 1 << 30
_TILE, _CHUNK = 64, 2048  # kTile and kChunk of csrc/footprints_device.h

# one plane of smi_footprints_batch_*: ``smi_footprint_plane`` of include/scarlet_amd.h
FOOTPRINT_PLANE = np.dtype([("address", np.uint64), ("h", np.int32), ("w", np.int32),
                            ("pixel_off", np.int64), ("tile0", np.int64), ("chunk0", np.int64)])


def footprint_plane_table(shapes, addresses):
    """The plane table of ``smi_footprints_batch_*`` for planes of ``shapes`` = ``(h, w)`` at
    the device ``addresses``: the exclusive prefixes over the planes of their pixels, 64 x 64
    tiles and scan chunks of 2048 pixels."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    table = np.zeros(len(shapes), dtype=FOOTPRINT_PLANE)
    table["address"] = np.asarray(list(addresses), dtype=np.uint64)
    pixels = tiles = chunks = 0
    for k, (h, w) in enumerate(shapes):
        table[k]["h"], table[k]["w"] = h, w
        table[k]["pixel_off"], table[k]["tile0"], table[k]["chunk0"] = pixels, tiles, chunks
        pixels += h * w
        tiles += -(-h // _TILE) * -(-w // _TILE)
        chunks += -(-h * w // _CHUNK)
    return table


def _plane_work_bytes(h, w):
    """bytes one plane adds to the work buffer: eight int32 per pixel, its chunk sums, its table
    record, border prefix and totals"""
    return 32 * h * w + 16 * -(-h * w // _CHUNK) + 80


_CHUNK_BYTES = 80  # of a chunk whatever it holds: roundings to 16 bytes, the prefix's last entry


def _plane_dtype(plane):
    name = str(plane.dtype).replace("torch.", "")
    if name not in ("float32", "float64"):
        raise TypeError("footprints: float32 or float64 planes are needed, got %s" % plane.dtype)
    return np.dtype(name)


def plan_footprints_batch(planes, _max_bytes=None):
    """``groups`` of ``get_footprints_batch``, without touching the GPU: per dtype of the planes
    (float32, float64), in order of first appearance, the chunks of one device chain each --
    lists of input positions in input order whose work buffer stays within
    ``FOOTPRINT_BATCH_BYTES`` (a plane beyond the budget is a chunk of its own).  ``planes``:
    anything with ``.shape``, ``.dtype`` and ``.device``.  Raises ``TypeError`` for host arrays
    and other dtypes, ``ValueError`` for planes that are not 2-D, empty planes and planes on
    different devices."""
    max_bytes = FOOTPRINT_BATCH_BYTES if _max_bytes is None else _max_bytes
    groups, used, device = {}, {}, None
    for i, p in enumerate(planes):
        if isinstance(p, np.ndarray) or not all(hasattr(p, a) for a in ("shape", "dtype", "device")) \
                or str(p.device).startswith("cpu"):
            raise TypeError("footprints: plane %d is no device tensor but %s (host arrays go "
                            "through get_footprints)" % (i, type(p).__name__))
        dtype = _plane_dtype(p)
        shape = tuple(int(v) for v in p.shape)
        if len(shape) != 2:
            raise ValueError("footprints: plane %d is not 2-D, its shape is %s" % (i, shape))
        if shape[0] == 0 or shape[1] == 0:
            raise ValueError("footprints: plane %d is empty, its shape is %s" % (i, shape))
        if device is None:
            device = str(p.device)
        elif str(p.device) != device:
            raise ValueError("footprints: plane %d is on %s, the planes before it on %s"
                             % (i, p.device, device))
        need = _plane_work_bytes(*shape)
        chunks = groups.setdefault(dtype, [[]])
        if chunks[-1] and used[dtype] + need > max_bytes:
            chunks.append([])
            used[dtype] = _CHUNK_BYTES
        chunks[-1].append(i)
        used[dtype] = used.get(dtype, _CHUNK_BYTES) + need
    return groups


def label_batch_device(planes, min_area, thresh):
    """First step of :func:`get_footprints_batch` for the contiguous 2-D device tensors
    ``planes`` of one dtype: one labelling chain for all of them.  Returns ``(table, counts,
    work, stats)``: the plane table, the ``(len(planes), 3)`` int32 array (footprints, mask
    bytes, strict maxima), the device buffer :func:`fetch_batch_device` reads and ``(kernel
    launches, stream synchronisations)`` of the call."""
    import torch

    lib = _lib.load()
    table = footprint_plane_table([p.shape for p in planes], [p.data_ptr() for p in planes])
    n, device = len(planes), planes[0].device
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.smi_footprints_batch_work_bytes(n, ctypes.c_void_p(table.ctypes.data),
                                                   ctypes.byref(nbytes)))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    counts = np.zeros((n, 3), dtype=np.int32)
    stats = np.zeros(2, dtype=np.int32)
    fn = lib.smi_footprints_batch_label_f32 if planes[0].dtype == torch.float32 else \
        lib.smi_footprints_batch_label_f64
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _lib.check(fn(ctypes.c_void_p(table.ctypes.data), n, int(min_area), int(thresh),
                      ctypes.c_void_p(work.data_ptr()), nbytes.value,
                      _lib.ptr(counts, ctypes.c_int32), _lib.ptr(stats, ctypes.c_int32), stream))
    return table, counts, work, (int(stats[0]), int(stats[1]))


def fetch_batch_device(planes, table, min_separation, counts, work):
    """Second step: ``(per_plane, stats)`` -- for every plane the arrays ``(bounds, masks,
    peak_start, peak_yx, peak_flux)`` in the layout of ``smi_footprints_fetch`` (``peak_start``
    indexes the arrays all planes share) -- from one fetch chain for all planes."""
    import torch

    lib = _lib.load()
    n, device = len(planes), planes[0].device
    n_fp, n_mask, n_peaks = (int(v) for v in counts.sum(axis=0, dtype=np.int64))
    bounds = np.zeros((n_fp, 4), dtype=np.int32)
    masks = np.zeros(n_mask, dtype=np.uint8)
    fp_start = np.zeros(n + 1, dtype=np.int32)
    start = np.zeros(n_fp + 1, dtype=np.int32)
    yx = np.zeros((n_peaks, 2), dtype=np.int32)
    flux = np.zeros(n_peaks, dtype=np.float64)
    stats = np.zeros(2, dtype=np.int32)
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.smi_footprints_batch_fetch_bytes(n, _lib.ptr(counts, ctypes.c_int32),
                                                    ctypes.byref(nbytes)))
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    fn = lib.smi_footprints_batch_fetch_f32 if planes[0].dtype == torch.float32 else \
        lib.smi_footprints_batch_fetch_f64
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _lib.check(fn(ctypes.c_void_p(table.ctypes.data), n, float(min_separation),
                      _lib.ptr(counts, ctypes.c_int32), ctypes.c_void_p(work.data_ptr()),
                      ctypes.c_void_p(scratch.data_ptr()), nbytes.value,
                      _lib.ptr(bounds, ctypes.c_int32), _lib.ptr(masks, ctypes.c_uint8),
                      _lib.ptr(fp_start, ctypes.c_int32), _lib.ptr(start, ctypes.c_int32),
                      _lib.ptr(yx, ctypes.c_int32), _lib.ptr(flux, ctypes.c_double),
                      _lib.ptr(stats, ctypes.c_int32), stream))
    mask_start = np.concatenate([[0], np.cumsum(counts[:, 1], dtype=np.int64)])
    per_plane = [(bounds[fp_start[k]:fp_start[k + 1]], masks[mask_start[k]:mask_start[k + 1]],
                  start[fp_start[k]:fp_start[k + 1] + 1], yx, flux) for k in range(n)]
    return per_plane, (int(stats[0]), int(stats[1]))


def get_footprints_batch(planes, min_separation, min_area, thresh, _max_bytes=None, _stats=None):
    """``[get_footprints_device(p, min_separation, min_area, thresh) for p in planes]`` for a
    list of 2-D float32 / float64 device tensors whose shapes and dtypes may differ, equal in
    every bound, mask byte, peak position and peak flux: per chunk of
    ``plan_footprints_batch`` one labelling and one fetch call (``csrc/footprints_batch.hip``)
    whose numbers of launches and of waits do not depend on the number of planes.  Views into
    other tensors are read where they lie; planes that are not contiguous are copied first, as
    ``get_footprints_device`` does.  ``_stats``: a list that receives, per chunk, the
    ``(launches, synchronisations)`` pairs of the two calls."""
    planes = list(planes)
    for i, p in enumerate(planes):
        if not _is_device_tensor(p):
            raise TypeError("get_footprints_batch: plane %d is no torch device tensor but %s "
                            "(host arrays go through get_footprints)" % (i, type(p).__name__))
    groups = plan_footprints_batch(planes, _max_bytes)
    out = [None] * len(planes)
    for chunks in groups.values():
        for chunk in chunks:
            held = [planes[i].contiguous() for i in chunk]
            table, counts, work, label_stats = label_batch_device(held, min_area, thresh)
            per_plane, fetch_stats = fetch_batch_device(held, table, min_separation, counts, work)
            for i, arrays in zip(chunk, per_plane):
                out[i] = _footprint_objects(*arrays)
            if _stats is not None:
                _stats.append((label_stats, fetch_stats))
    return out


def get_connected_pixels(i, j, image, unchecked, footprint, bounds, thresh=0):
    """Mark in ``footprint`` the pixels 4-connected to ``(i, j)`` with ``image > thresh`` and
    grow ``bounds`` = ``[y0, y1, x0, x1]`` over them.  ``unchecked`` (bool) is cleared for
    every pixel visited, as in the reference; all three arrays are updated in place."""
    height, width = image.shape
    stack = [(i, j)]
    while stack:
        y, x = stack.pop()
        if not unchecked[y, x]:
            continue
        unchecked[y, x] = False
        if not image[y, x] > thresh:
            continue
        footprint[y, x] = True
        bounds[0] = min(bounds[0], y)
        bounds[1] = max(bounds[1], y)
        bounds[2] = min(bounds[2], x)
        bounds[3] = max(bounds[3], x)
        for a, b in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= a < height and 0 <= b < width and unchecked[a, b]:
                stack.append((a, b))


def get_peaks(image, min_separation, y0, x0):
    """Strict local maxima of ``image`` over their existing 8 neighbours, as ``Peak``s at
    ``(y + y0, x + x0)``, brightest first (ties in raster order); with
    ``min_separation > 0`` a peak closer than that to a brighter kept peak is dropped."""
    image = np.asarray(image)
    h, w = image.shape
    pad = np.full((h + 2, w + 2), -np.inf)
    pad[1:-1, 1:-1] = image
    is_peak = np.ones((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                is_peak &= image > pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(is_peak)
    flux = image[ys, xs].astype(np.float64)
    order = np.argsort(-flux, kind="stable")
    kept = []
    min2 = float(min_separation) ** 2
    for k in order:
        y, x = int(ys[k]) + y0, int(xs[k]) + x0
        if min_separation > 0 and any((p.y - y) ** 2 + (p.x - x) ** 2 < min2 for p in kept):
            continue
        kept.append(Peak(y, x, flux[k]))
    return kept
