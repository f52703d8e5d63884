"""Detection on the host (no GPU): footprints and peaks of the library against hand-worked
cases and the pure-Python restatement, the box / quad-tree helpers of scarlet_amd.detect, and
the footprint and structure stages of the reference's run (tests/golden/detect.npz) computed
from its recorded coefficients."""

import ctypes

import numpy as np
import pytest

from conftest import golden
from detect_kats import KATS
import detect_oracle


def as_lists(footprints):
    return [(tuple(int(v) for v in fp.bounds), [(p.y, p.x, p.flux) for p in fp.peaks])
            for fp in footprints]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kat", KATS, ids=[k[0] for k in KATS])
def test_footprint_kats(kat, dtype):
    from scarlet_amd import detect_pybind11

    name, image, min_sep, min_area, thresh, want = kat
    image = image.astype(dtype)
    for impl in (detect_pybind11, detect_oracle):
        fps = impl.get_footprints(image, min_sep, min_area, thresh)
        assert as_lists(fps) == want, (name, impl.__name__)
        for fp in fps:
            y0, y1, x0, x1 = fp.bounds
            assert fp.footprint.shape == (y1 - y0 + 1, x1 - x0 + 1)
            assert fp.footprint.dtype == bool


def test_footprint_masks_and_random_images():
    """masks and peaks equal the restatement's on random images (both dtypes)"""
    from scarlet_amd import detect_pybind11

    rng = np.random.default_rng(5)
    for k in range(6):
        image = rng.normal(size=(23 + k, 31 - k)) * 2
        for dtype in (np.float32, np.float64):
            img = image.astype(dtype)
            a = detect_pybind11.get_footprints(img, 0 if k % 2 else 1.5, 2 + k % 3, k % 2)
            b = detect_oracle.get_footprints(img, 0 if k % 2 else 1.5, 2 + k % 3, k % 2)
            assert as_lists(a) == as_lists(b)
            for fa, fb in zip(a, b):
                assert np.array_equal(fa.footprint, fb.footprint)


def test_single_footprint_of_four_million_pixels():
    """a 2000 x 2000 footprint (a recursive fill would overflow the stack)"""
    from scarlet_amd import detect_pybind11

    yy, xx = np.mgrid[:2000, :2000]
    image = (1 + 100.0 / (1 + (yy - 700) ** 2 + (xx - 1300) ** 2)).astype(np.float32)
    fps = detect_pybind11.get_footprints(image, 0, 4, 0)
    assert len(fps) == 1
    assert tuple(fps[0].bounds) == (0, 1999, 0, 1999)
    assert fps[0].footprint.all()
    assert [(p.y, p.x) for p in fps[0].peaks] == [(700, 1300)]


def test_connected_pixels_and_peaks_helpers():
    from scarlet_amd import detect_pybind11

    image = KATS[0][1]
    unchecked = np.ones(image.shape, bool)
    footprint = np.zeros(image.shape, bool)
    bounds = np.array([3, 3, 3, 3])
    detect_pybind11.get_connected_pixels(3, 3, image, unchecked, footprint, bounds, 0)
    assert list(bounds) == [2, 3, 2, 3]
    assert footprint.sum() == 4 and footprint[2:, 2:].all()
    peaks = detect_pybind11.get_peaks(KATS[6][1], 0, 10, 20)
    assert [(p.y, p.x, p.flux) for p in peaks] == [(12, 24, 7.0), (10, 20, 4.0), (10, 24, 4.0),
                                                   (12, 22, 4.0)]


def test_box_helpers():
    from scarlet_amd import Box
    from scarlet_amd.detect import bounds_to_bbox, box_intersect, footprint_intersect

    b = bounds_to_bbox((2, 5, 3, 9))
    assert b == Box((4, 7), origin=(2, 3))
    assert box_intersect(b, Box((2, 2), origin=(5, 9)))
    assert not box_intersect(b, Box((2, 2), origin=(6, 3)))
    assert not box_intersect(b, Box((3, 3), origin=(0, 0)))
    f1 = np.array([[1, 0], [0, 0]], bool)
    f2 = np.array([[0, 0], [0, 1]], bool)
    b1, b2 = Box((2, 2), origin=(0, 0)), Box((2, 2), origin=(-1, -1))
    assert footprint_intersect(f1, b1, f2, b2)  # pixel (0, 0) in both
    assert not footprint_intersect(f1, b1, f2, Box((2, 2), origin=(0, 0)))
    assert not footprint_intersect(f1, b1, f2, Box((2, 2), origin=(5, 5)))


def test_quad_tree_split_and_query():
    from scarlet_amd import Box
    from scarlet_amd.detect import QuadTreeRegion

    tree = QuadTreeRegion(Box((16, 16)), capacity=3)
    boxes = [Box((2, 2), origin=(1, 1)), Box((2, 2), origin=(12, 1)),
             Box((4, 4), origin=(6, 6)), Box((2, 2), origin=(1, 12))]
    for b in boxes[:2]:
        tree.add(b)
    assert tree.sub_regions is None and tree.boxes == boxes[:2]
    tree.add(boxes[2])  # third box: capacity - 1 reached, the region splits
    assert tree.boxes is None and len(tree.sub_regions) == 4
    quads = [(r.bbox.origin, r.bbox.shape) for r in tree.sub_regions]
    assert quads == [((0, 0), (8, 8)), ((8, 0), (8, 8)), ((0, 8), (8, 8)), ((8, 8), (8, 8))]
    # the central box overlaps all four quadrants and is listed in each, returned once
    assert all(boxes[2] in r.boxes for r in tree.sub_regions)
    tree.add(boxes[3])
    assert tree.query() == set(boxes)
    assert tree.query(Box((3, 3), origin=(0, 0))) == {boxes[0]}
    assert tree.query(Box((1, 1), origin=(15, 0))) == set()


def _golden_footprints(g, s):
    starts = g["fp%d_peak_start" % s]
    return [(tuple(int(v) for v in g["fp%d_bounds" % s][f]),
             [tuple(int(v) for v in yx) + (float(fl),)
              for yx, fl in zip(g["fp%d_peak_yx" % s][starts[f]:starts[f + 1]],
                                g["fp%d_peak_flux" % s][starts[f]:starts[f + 1]])])
            for f in range(len(starts) - 1)]


def test_footprints_and_structures_of_the_reference_run():
    """get_footprints on the recorded detection coefficients of hsc_cosmos_35 and
    get_blend_structures on top: footprints, masks, peaks, structures and the order of the
    middle tree's query equal the reference's"""
    from scarlet_amd import Box, detect
    from scarlet_amd.detect_pybind11 import get_footprints

    g = golden("detect")
    det = g["detect_s3"]
    for s in range(3):
        fps = get_footprints(det[s], min_separation=0, min_area=4, thresh=0)
        assert as_lists(fps) == _golden_footprints(g, s), s
        masks = np.concatenate([fp.footprint.ravel() for fp in fps])
        assert np.array_equal(np.packbits(masks), g["fp%d_masks" % s])
    structures, middle = detect.get_blend_structures(det)
    assert len(structures) == int(g["n_structures"])
    for k, st in enumerate(structures):
        for scale in (0, 1, 2):
            got = [(p.y, p.x) for p in st.peaks.get(scale, [])]
            assert got == [tuple(v) for v in g["struct%d_peaks%d" % (k, scale)].tolist()], (k, scale)
    order = [(b.origin[0], b.origin[1], b.shape[0], b.shape[1]) for b in middle.query()]
    assert order == [tuple(v) for v in g["middle_query_bounds"].tolist()]
    peaks = detect.get_peaks(det, bbox=Box((5,) + det.shape[1:]))
    assert peaks == [tuple(v) for v in g["lite_centers"].tolist()]
    trees, all_fps = detect.get_blend_trees(det)
    assert len(trees) == len(all_fps) == 3
    assert as_lists(all_fps[1]) == _golden_footprints(g, 1)


def test_device_entry_points_report_no_device():
    """without a GPU the wavelet entry points fail loudly (there is no CPU fallback)"""
    from scarlet_amd import _lib

    lib = _lib.load()
    if lib.smi_device_count() > 0:
        pytest.skip("a GPU is present")
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.smi_starlet_transform_f64(p, 1, 8, 8, 1, 2, p, p, None) == -3
    assert lib.smi_starlet_transform_f32(p, 1, 8, 8, 1, 2, p, p, None) == -3
    assert lib.smi_starlet_reconstruction_f64(p, 1, 8, 8, 1, 2, p, p, None) == -3
    sig = np.ones(2)
    assert lib.smi_multiresolution_support_f64(
        p, 1, 2, 4, 4, 16, 16, _lib.ptr(sig, ctypes.c_double), _lib.ptr(sig, ctypes.c_double),
        3.0, 0.1, 20, p, p, None, None) == -3
    assert lib.smi_coadd_f32(p, 2, 4, 4, p, None) == -3
    assert "no HIP device" in lib.smi_last_error().decode()
