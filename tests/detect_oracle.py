"""Pure-Python restatement of the footprint / peak finder of scarlet.detect_pybind11, written
from its documented behaviour.  Slow (a Python loop over pixels) and meant for small images:
it checks the library's footprints in the host tests, and it stands in for the compiled
module when the golden vectors are generated from the reference.

Behaviour: 4-connected pixels > int(thresh), seeds in raster order, kept when the bounding
box has more than min_area pixels and the footprint at least min_area; peaks = strict maxima
over the existing 8 neighbours in the box with non-footprint pixels zeroed, brightest first
(equal fluxes in raster order); min_separation > 0 drops peaks near a brighter kept one."""

import numpy as np


class Peak:
    def __init__(self, y, x, flux):
        self.y, self.x, self.flux = int(y), int(x), float(flux)


class Footprint:
    def __init__(self, footprint, peaks, bounds):
        self.footprint = np.asarray(footprint, dtype=bool)
        self.peaks = list(peaks)
        self.bounds = np.asarray(bounds, dtype=np.int32)


def peaks_of(patch, min_separation, y0, x0):
    h, w = patch.shape
    found = []
    for i in range(h):
        for j in range(w):
            v = patch[i, j]
            neighbours = [patch[a, b] for a in range(max(i - 1, 0), min(i + 2, h))
                          for b in range(max(j - 1, 0), min(j + 2, w)) if (a, b) != (i, j)]
            if all(v > n for n in neighbours):
                found.append(Peak(i + y0, j + x0, v))
    found.sort(key=lambda p: -p.flux)  # list.sort is stable
    if min_separation > 0:
        kept = []
        for p in found:
            if all((p.y - k.y) ** 2 + (p.x - k.x) ** 2 >= min_separation ** 2 for k in kept):
                kept.append(p)
        found = kept
    return found


def get_footprints(image, min_separation, min_area, thresh):
    image = np.asarray(image)
    thresh = int(thresh)
    height, width = image.shape
    label = np.zeros(image.shape, dtype=np.int64)
    footprints = []
    n = 0
    for i in range(height):
        for j in range(width):
            if label[i, j] or not image[i, j] > thresh:
                continue
            n += 1
            label[i, j] = n
            todo, members = [(i, j)], []
            while todo:
                y, x = todo.pop()
                members.append((y, x))
                for a, b in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= a < height and 0 <= b < width and not label[a, b] \
                            and image[a, b] > thresh:
                        label[a, b] = n
                        todo.append((a, b))
            ys = [m[0] for m in members]
            xs = [m[1] for m in members]
            y0, y1, x0, x1 = min(ys), max(ys), min(xs), max(xs)
            h, w = y1 - y0 + 1, x1 - x0 + 1
            if not (h * w > min_area and len(members) >= min_area):
                continue
            mask = label[y0:y1 + 1, x0:x1 + 1] == n
            patch = np.where(mask, image[y0:y1 + 1, x0:x1 + 1], 0).astype(image.dtype)
            footprints.append(Footprint(mask, peaks_of(patch, min_separation, y0, x0),
                                        (y0, y1, x0, x1)))
    return footprints


def as_module():
    """A module object with the names of scarlet.detect_pybind11."""
    import types

    mod = types.ModuleType("scarlet.detect_pybind11")
    mod.get_footprints = get_footprints
    mod.Footprint = Footprint
    mod.Peak = Peak
    mod.get_peaks = lambda image, min_separation, y0, x0: peaks_of(
        np.asarray(image), min_separation, y0, x0)
    return mod
