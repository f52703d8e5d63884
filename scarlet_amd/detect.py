"""Source detection on starlet coefficients (reference scarlet/detect.py).

The wavelet stages -- the coadd of the bands, the starlet transform and the multiresolution
support -- run on the GPU in one device-resident chain; ``get_detect_wavelets_batch`` runs
them for a catalogue of blends of different frames in one chain per dtype
(``csrc/detect_batch.hip``).  Footprints and peaks of coefficients
that stay on the device (``get_detect_wavelets(..., device=True)``) are found there too
(``detect_pybind11.get_footprints_device``), and ``get_peaks_batch`` /
``get_blend_structures_batch`` find them for a whole catalogue in one chain
(``get_footprints_batch``, ``csrc/footprints_batch.hip``); host arrays take the host code
(``get_footprints``).  The structures that connect the footprints across scales are plain
Python over ``Box``es, as in the reference.  ``QuadTreeRegion.query`` returns a ``set`` as the
reference does, so the order in which ``get_peaks`` lists the peaks is the reference's.
Display helpers (``draw_*``, matplotlib) are not part of this package.
"""

import numpy as np

from .bbox import Box, overlapped_slices
from .detect_pybind11 import (get_footprints, get_footprints_device, get_footprints_batch,
                              _is_device_tensor)
from . import wavelet


def bounds_to_bbox(bounds):
    """Box of the inclusive bounds ``(bottom, top, left, right)`` of a footprint."""
    return Box((bounds[1] + 1 - bounds[0], bounds[3] + 1 - bounds[2]),
               origin=(bounds[0], bounds[2]))


def box_intersect(box1, box2):
    """True when the two boxes overlap."""
    overlap = box1 & box2
    return overlap.shape[0] != 0 and overlap.shape[1] != 0


def footprint_intersect(footprint1, box1, footprint2, box2):
    """True when the two footprint masks (in boxes ``box1``, ``box2``) share a pixel."""
    if not box_intersect(box1, box2):
        return False
    s1, s2 = overlapped_slices(box1, box2)
    return np.sum(footprint1[s1] * footprint2[s2]) > 0


class QuadTreeRegion:
    """A quad tree of boxes: a region holds up to ``capacity - 1`` boxes, then splits into
    four sub-regions, each receiving every box that overlaps it."""

    def __init__(self, bbox, capacity=5, sub_regions=None, boxes=None, depth=0, detect=None):
        self.bbox = bbox
        self.sub_regions = sub_regions
        self.boxes = [] if boxes is None else boxes
        self.capacity = capacity
        self.depth = depth
        self.detect = detect

    def footprint_image(self, bbox=None):
        """Sum of the masks of all footprints in the tree, in ``bbox`` (default: the union of
        their boxes)."""
        boxes = self.query(self.bbox)
        if bbox is None:
            bbox = Box((0, 0))
            for box in boxes:
                bbox = bbox | box
        image = np.zeros(bbox.shape)
        for box in boxes:
            full, local = overlapped_slices(bbox, box)
            image[full] += box.footprint.footprint[local]
        return image

    @property
    def peaks(self):
        """All peaks of the footprints in the tree."""
        for box in self.query(self.bbox):
            yield from box.footprint.peaks

    def add(self, other_box):
        """Insert a box (it goes to every sub-region it overlaps)."""
        if not box_intersect(self.bbox, other_box):
            return
        if self.sub_regions is not None:
            self._add_to_sub_regions(other_box)
            return
        if self.boxes is None:
            self.boxes = []
        if len(self.boxes) < self.capacity - 1:
            self.boxes.append(other_box)
        else:
            self.split()
            self.boxes = None
            self._add_to_sub_regions(other_box)

    def add_footprints(self, footprints):
        """Insert the bounding box of each footprint (the box carries it as ``.footprint``)."""
        for fp in footprints:
            box = bounds_to_bbox(fp.bounds)
            box.footprint = fp
            self.add(box)
        return self

    def split(self):
        """Divide the region into four: top-left, bottom-left, top-right, bottom-right."""
        height, width = self.bbox.shape
        h2, w2 = height // 2, width // 2
        y, x = self.bbox.origin
        quads = (((h2, w2), (y, x)), ((height - h2, w2), (y + h2, x)),
                 ((h2, width - w2), (y, x + w2)), ((height - h2, width - w2), (y + h2, x + w2)))
        self.sub_regions = [QuadTreeRegion(Box(shape, origin), capacity=self.capacity,
                                           depth=self.depth + 1) for shape, origin in quads]
        for box in self.boxes:
            self._add_to_sub_regions(box)

    def _add_to_sub_regions(self, other_box):
        for region in self.sub_regions:
            region.add(other_box)

    def query(self, other_box=None):
        """The ``set`` of boxes in the tree that overlap ``other_box`` (default: the region)."""
        if other_box is None:
            other_box = self.bbox
        if self.boxes is not None:
            return set(box for box in self.boxes if box_intersect(box, other_box))
        found = set()
        if self.sub_regions is not None:
            for region in self.sub_regions:
                if box_intersect(region.bbox, other_box):
                    found |= region.query(other_box)
        return found


class SingleScaleStructure:
    """A footprint at one wavelet scale and the peaks, per scale, of the footprints at other
    scales that overlap its box."""

    def __init__(self, scale, footprint):
        self.scale = scale
        self.footprint = footprint
        self.bbox = bounds_to_bbox(footprint.bounds)
        self.peaks = {scale: footprint.peaks}
        self._all_peaks = None

    def add_footprint(self, scale, footprint):
        """Add the peaks of ``footprint`` at ``scale``."""
        self.peaks[scale] = self.peaks.get(scale, []) + list(footprint.peaks)
        self._all_peaks = None

    def add_scale_tree(self, scale, tree):
        """Add every footprint of ``tree`` (at ``scale``) whose box overlaps this one."""
        for box in tree.query(self.bbox):
            self.add_footprint(scale, box.footprint)
        return self

    @property
    def all_peaks(self):
        """``set`` of ``(x, y)`` of the peaks at all scales."""
        if self._all_peaks is None:
            self._all_peaks = set((p.x, p.y) for peaks in self.peaks.values() for p in peaks)
        return self._all_peaks


def get_wavelets(images, variance, scales=3):
    """Significant starlet coefficients ``M * w`` of every band, shape
    ``(bands, scales+1, Ny, Nx)`` (as the reference's code returns them; its docstring names
    the axes the other way round).  Band ``b`` uses ``sigma = median(sqrt(variance[b]))``.
    All bands are transformed in one batch and their supports found together on the
    device."""
    images = np.asarray(images)
    sigma = np.median(np.sqrt(variance), axis=(1, 2))
    scales = wavelet._checked_scales(images.shape, scales)
    d_coeffs = wavelet.transform_device(wavelet._upload(images), scales)
    P = scales + 1
    s0, t0 = zip(*(wavelet.initial_sigma(images[b].dtype, P, sigma[b], 3)
                   for b in range(len(images))))
    _, Mw, _ = wavelet.support_device(d_coeffs, np.stack(s0), np.stack(t0), 3, 1e-1, 20)
    return Mw.transpose(0, 1).contiguous().cpu().numpy()


def get_detect_wavelets(images, variance, scales=3, device=False):
    """Significant starlet coefficients ``(scales+1, Ny, Nx)`` of the coadd
    ``np.sum(images, axis=0)``, with ``sigma = median(sqrt(variance))``: coadd, transform and
    support on the device, one copy of the result to the host.  ``device=True`` returns the
    float64 device tensor instead, without the copy (``get_blend_trees``,
    ``get_blend_structures`` and ``get_peaks`` accept it)."""
    images = np.asarray(images)
    sigma = np.median(np.sqrt(variance))
    scales = wavelet._checked_scales(images.shape, scales)
    detect = wavelet.coadd_device(wavelet._upload(images))
    d_coeffs = wavelet.transform_device(detect[None], scales)
    dtype = np.float32 if images.dtype == np.float32 else np.float64
    s0, t0 = wavelet.initial_sigma(dtype, scales + 1, sigma, 3)
    _, Mw, _ = wavelet.support_device(d_coeffs, s0[None], t0[None], 3, 1e-1, 20)
    return Mw[:, 0] if device else Mw[:, 0].cpu().numpy()


# ---------------------------------------------------------------------------
# get_detect_wavelets for a catalogue: one device chain per group of blends
# ---------------------------------------------------------------------------
# Device bytes of one chunk (images, coefficients, M * w, work planes): a group whose blends
# need more is cut into chunks.
BATCH_BYTES = 1 << 30


def _batch_dtype(images):
    """dtype of the device copy ``wavelet._upload`` makes of ``images``."""
    return np.dtype(np.float32 if images.dtype == np.float32 else np.float64)


def plan_detect_wavelets_batch(images, variance, scales=3, _max_tasks=None, _max_bytes=None):
    """``(groups, fallback)`` of ``get_detect_wavelets_batch``, without touching the GPU.
    ``groups``: per image dtype on the device (float32, or float64 for everything else, as
    ``wavelet._upload`` converts), in order of first appearance, the chunks of one device
    call each -- lists of input positions in input order, at most 65535 blends and
    ``BATCH_BYTES`` of device buffers (a blend beyond the budget is a chunk of its own).
    ``fallback``: ``(position, reason)`` of the blends that go through
    ``get_detect_wavelets``: a frame of more than ``wavelet.DETECT_BATCH_MAX_PIXELS`` =
    65536 pixels -- one workgroup runs all support iterations of a blend, and beyond 32 blocks
    of pixels per plane the per-blend call's many workgroups are the better shape -- or images
    that are not a ``(bands, Ny, Nx)`` cube with a band.  Raises ``ValueError`` for lists of
    different lengths and for a frame one pixel high or wide."""
    images, variance = list(images), list(variance)
    if len(images) != len(variance):
        raise ValueError("images and variance must have one entry per blend, got {} and {}"
                         .format(len(images), len(variance)))
    max_tasks = wavelet.DETECT_BATCH_MAX_TASKS if _max_tasks is None else _max_tasks
    max_bytes = BATCH_BYTES if _max_bytes is None else _max_bytes
    groups, fallback, used = {}, [], {}
    for i, im in enumerate(images):
        im = np.asarray(im)
        if im.ndim != 3 or im.shape[0] < 1:
            fallback.append((i, "images are not a (bands, Ny, Nx) cube"))
            continue
        planes = wavelet._checked_scales(im.shape, scales) + 1
        bands, h, w = im.shape
        if h * w > wavelet.DETECT_BATCH_MAX_PIXELS:
            fallback.append((i, "frame of more than %d pixels" % wavelet.DETECT_BATCH_MAX_PIXELS))
            continue
        dtype = _batch_dtype(im)
        need = h * w * (bands * dtype.itemsize + (2 * planes + 1) * 8)
        chunks = groups.setdefault(dtype, [[]])
        if chunks[-1] and (len(chunks[-1]) >= max_tasks or used[dtype] + need > max_bytes):
            chunks.append([])
            used[dtype] = 0
        chunks[-1].append(i)
        used[dtype] = used.get(dtype, 0) + need
    return groups, fallback


def _batch_sigmas(variance):
    """``median(sqrt(variance))`` of every blend, on the host as ``get_detect_wavelets``."""
    return [np.median(np.sqrt(var)) for var in variance]


def _batch_table(images, sigmas, scales):
    """Task table of the blends of one chunk (``images``: arrays of one device dtype)."""
    dtype = _batch_dtype(images[0]).type
    first = [wavelet.initial_sigma(dtype, 1, sigma, 3) for sigma in sigmas]
    return wavelet.detect_task_table(
        [im.shape for im in images], [wavelet._checked_scales(im.shape, scales) for im in images],
        [s0[0] for s0, _ in first], [t0[0] for _, t0 in first])


def _batch_upload(images):
    """The images of one chunk, packed one after another, in one copy to the device."""
    torch = wavelet._torch()
    dtype = _batch_dtype(images[0])
    packed = np.empty(sum(im.size for im in images), dtype)
    at = 0
    for im in images:
        packed[at:at + im.size] = im.reshape(-1)
        at += im.size
    return torch.from_numpy(packed).to("cuda")


def _batch_views(flat, table):
    """Blend by blend ``(planes, H, W)`` views of the flat coefficient buffer."""
    out = []
    for t in table:
        planes, h, w = int(t["scales"]) + 1, int(t["h"]), int(t["w"])
        at = int(t["coeff_off"])
        out.append(flat[at:at + planes * h * w].reshape(planes, h, w))
    return out


def get_detect_wavelets_batch(images, variance, scales=3, device=False):
    """``[get_detect_wavelets(im, var, scales, device) for im, var in zip(images, variance)]``
    for a catalogue of blends whose frames, band counts and dtypes may differ, bit for bit:
    per group of ``plan_detect_wavelets_batch`` one packed upload and one device chain
    (csrc/detect_batch.hip) whose number of launches does not depend on the number of blends,
    the convergence test of every blend's support included.  ``sigma = median(sqrt(variance))``
    of every blend stays on the host.  Returns the list of ``(scales_i + 1, Ny_i, Nx_i)``
    float64 arrays -- with ``device=True`` float64 device tensors, views into their group's
    buffer, without the copy to the host."""
    images = [np.asarray(im) for im in images]
    variance = list(variance)
    groups, fallback = plan_detect_wavelets_batch(images, variance, scales)
    out = [None] * len(images)
    for chunks in groups.values():
        for chunk in chunks:
            ims = [images[i] for i in chunk]
            table = _batch_table(ims, _batch_sigmas([variance[i] for i in chunk]), scales)
            masked, _, _ = wavelet.detect_wavelets_batch_device(_batch_upload(ims), table)
            flat = masked if device else masked.cpu().numpy()
            for i, view in zip(chunk, _batch_views(flat, table)):
                out[i] = view
    for i, _ in fallback:
        out[i] = get_detect_wavelets(images[i], variance[i], scales, device)
    return out


def _scale_footprints(detect):
    if _is_device_tensor(detect):  # every scale but the last in one labelling call
        return get_footprints_device(detect[:-1], min_separation=0, min_area=4, thresh=0)
    return [get_footprints(plane, min_separation=0, min_area=4, thresh=0) for plane in detect[:-1]]


def get_blend_trees(detect):
    """Quad tree and footprints of every wavelet scale but the last of ``detect``
    ``(scales+1, Ny, Nx)``.  Returns ``(trees, all_footprints)``."""
    all_footprints = _scale_footprints(detect)
    trees = [QuadTreeRegion(Box(detect.shape[-2:]), capacity=10).add_footprints(fps)
             for fps in all_footprints]
    return trees, all_footprints


def _structures(all_footprints, frame):
    """``get_blend_structures`` from the footprints of the first three scales of a ``frame``"""
    low, middle = all_footprints[:2]
    low_tree = QuadTreeRegion(Box(frame), capacity=10).add_footprints(low)
    middle_tree = QuadTreeRegion(Box(frame), capacity=10).add_footprints(middle)
    structures = [SingleScaleStructure(2, fp).add_scale_tree(0, low_tree)
                  .add_scale_tree(1, middle_tree) for fp in all_footprints[2]]
    return structures, middle_tree


def get_blend_structures(detect):
    """Structures of the third wavelet scale, each with the overlapping footprints of the first
    two scales, and the quad tree of the second scale.  Returns
    ``(high_structures, middle_tree)`` (the reference's effective definition)."""
    return _structures(_scale_footprints(detect), detect.shape[-2:])


def _checked_blends(detects, name):
    """The list of a catalogue's detection coefficients, refused before any device work when
    one is no device tensor or has fewer than the four planes the structures need."""
    detects = list(detects)
    for i, d in enumerate(detects):
        if not _is_device_tensor(d):
            raise TypeError("%s: the blend at position %d is no torch device tensor but %s "
                            "(host arrays go through get_peaks, blend by blend)"
                            % (name, i, type(d).__name__))
    for i, d in enumerate(detects):
        shape = tuple(d.shape)
        if len(shape) != 3 or shape[0] < 4:
            raise ValueError("%s: the blend at position %d has shape %s; (planes, Ny, Nx) with "
                             "at least four planes is needed (scales=3 of a frame that allows "
                             "them)" % (name, i, shape))
    return detects


def get_blend_structures_batch(detects):
    """``[get_blend_structures(d) for d in detects]`` for a catalogue of device tensors
    ``(planes, Ny, Nx)`` whose frames may differ: the footprints of scales 0 .. 2 of every
    blend come from one ``get_footprints_batch``; the quad trees and structures are built on
    the host from the same footprints in the same order, so every structure, peak and query
    order is the per-blend call's.  Raises ``TypeError`` for host arrays and ``ValueError``,
    naming the position, for a blend with fewer than four planes."""
    detects = _checked_blends(detects, "get_blend_structures_batch")
    found = get_footprints_batch([d[s] for d in detects for s in range(3)],
                                 min_separation=0, min_area=4, thresh=0)
    return [_structures(found[3 * k:3 * k + 3], tuple(d.shape[-2:]))
            for k, d in enumerate(detects)]


def get_peaks_batch(detects, bboxes=None):
    """``[get_peaks(d, bbox=b) for d, b in zip(detects, bboxes)]`` for a catalogue of device
    tensors ``(planes, Ny, Nx)`` whose frames may differ (``bboxes``: one entry per blend, or
    ``None`` for every blend's whole frame).  ``get_peaks`` reads the middle tree only, so one
    ``get_footprints_batch`` labels scale 1 of every blend and nothing else.  Raises as
    ``get_blend_structures_batch``."""
    detects = _checked_blends(detects, "get_peaks_batch")
    bboxes = [None] * len(detects) if bboxes is None else list(bboxes)
    if len(bboxes) != len(detects):
        raise ValueError("get_peaks_batch: {} blends and {} boxes".format(len(detects),
                                                                          len(bboxes)))
    found = get_footprints_batch([d[1] for d in detects], min_separation=0, min_area=4, thresh=0)
    out = []
    for d, bbox, middle in zip(detects, bboxes, found):
        frame = tuple(d.shape[1:])
        tree = QuadTreeRegion(Box(frame), capacity=10).add_footprints(middle)
        bbox = Box(frame) if bbox is None else bbox[1:]
        out.append([(peak.y, peak.x) for box in tree.query(bbox) for peak in box.footprint.peaks])
    return out


def get_peaks(detect=None, images=None, variance=None, bbox=None, scales=3):
    """``(y, x)`` of the peaks of the second wavelet scale, in the order of the middle tree's
    query.  Without ``detect``, ``images``, ``variance`` and ``bbox`` are needed and the
    detection coefficients come from ``get_detect_wavelets(images, variance, scales=3)`` and
    stay on the device, footprints and peaks included.  ``detect`` may be a host array or a
    device tensor."""
    if detect is None:
        if images is None or variance is None or bbox is None:
            raise ValueError("Must pass either 'detect' or 'images' and 'variance' and 'bbox'")
        detect = get_detect_wavelets(images, variance, scales=3, device=True)
    bbox = Box(tuple(detect.shape[1:])) if bbox is None else bbox[1:]
    _, tree = get_blend_structures(detect)
    return [(peak.y, peak.x) for box in tree.query(bbox) for peak in box.footprint.peaks]
