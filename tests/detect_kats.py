"""Known-answer cases of get_footprints, worked out by hand from the footprint rules:
4-connected pixels > int(thresh), seeds in raster order, kept when the box has more than
min_area pixels and the footprint at least min_area; peaks = strict maxima over the existing
8 neighbours with the pixels outside the footprint at 0, brightest first, ties in raster
order; min_separation > 0 keeps peaks greedily, brightest first.

Each case: (name, image, min_separation, min_area, thresh,
            [((y0, y1, x0, x1), [(y, x, flux), ...]), ...])"""

import numpy as np


def _a(rows):
    return np.array(rows, dtype=np.float64)


KATS = [
    # touching at a corner only: two footprints, found in raster order of their seeds
    ("diagonal_contact",
     _a([[1, 2, 0, 0],
         [3, 4, 0, 0],
         [0, 0, 5, 6],
         [0, 0, 7, 9]]), 0, 3, 0,
     [((0, 1, 0, 1), [(1, 1, 4.0)]),
      ((2, 3, 2, 3), [(3, 3, 9.0)])]),
    # a 1 x 3 line: h*w == min_area is dropped; the 3-pixel L in a 2 x 2 box is kept, and the
    # pixel of its box outside the footprint counts as 0
    ("area_boundary",
     _a([[1, 2, 1, 0, 0, 0, 0],
         [0, 0, 0, 0, 2, 0, 0],
         [0, 0, 0, 0, 7, 3, 0],
         [0, 0, 0, 0, 0, 0, 0]]), 0, 3, 0,
     [((1, 2, 4, 5), [(2, 4, 7.0)])]),
    # box 2 x 3 = 6 > 5 but only 4 pixels < 5: dropped
    ("count_below_min_area",
     _a([[1, 0, 0],
         [2, 3, 4],
         [0, 0, 0]]), 0, 5, 0, []),
    # thresh 0.7 is truncated to 0: the whole plus is one footprint (with 0.7 itself only
    # the centre would pass and be dropped as too small)
    ("thresh_truncated",
     _a([[0, 0.5, 0],
         [0.5, 0.75, 0.5],
         [0, 0.5, 0]]), 0, 4, 0.7,
     [((0, 2, 0, 2), [(1, 1, 0.75)])]),
    # maxima in two corners and on an edge
    ("edges_and_corners",
     _a([[9, 1, 1, 5],
         [1, 1, 1, 1],
         [1, 6, 1, 1]]), 0, 4, 0,
     [((0, 2, 0, 3), [(0, 0, 9.0), (2, 1, 6.0), (0, 3, 5.0)])]),
    # a plateau of two equal pixels has no strict maximum: kept, without peaks
    ("plateau",
     _a([[0, 0, 0, 0],
         [0, 5, 5, 0],
         [0, 0, 0, 0]]), 0, 1, 0,
     [((1, 1, 1, 2), [])]),
    # equal fluxes stay in raster order behind the brighter peak
    ("equal_flux",
     _a([[4, 1, 1, 1, 4],
         [1, 1, 1, 1, 1],
         [1, 1, 4, 1, 7]]), 0, 4, 0,
     [((0, 2, 0, 4), [(2, 4, 7.0), (0, 0, 4.0), (0, 4, 4.0), (2, 2, 4.0)])]),
    # min_separation 2.5: the 8 two pixels from the 9 goes, the 7 five pixels away stays
    ("min_separation",
     _a([[1, 1, 1, 1, 1, 1, 1],
         [9, 1, 8, 1, 1, 7, 1],
         [1, 1, 1, 1, 1, 1, 1]]), 2.5, 4, 0,
     [((0, 2, 0, 6), [(1, 0, 9.0), (1, 5, 7.0)])]),
]
