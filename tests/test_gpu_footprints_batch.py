"""Footprints and peaks of a ragged list of device planes (csrc/footprints_batch.hip) against
the host library's get_footprints and the per-plane get_footprints_device, plane by plane;
get_peaks_batch and get_blend_structures_batch against the per-blend calls and the reference's
recorded run.  Everything compared is integers, booleans and copied pixel values: every
comparison is exact.  The planes are those of tests/footprints_batch_cases.py."""

import numpy as np
import pytest

import footprints_batch_cases as cases
from conftest import golden
from detect_kats import KATS
from test_gpu_footprints import _golden_footprints, as_lists, assert_same, dev

pytestmark = pytest.mark.gpu

DTYPES = {"float32": np.float32, "float64": np.float64, "mixed": cases.MIXED}
_device, _single = {}, {}


def device_planes(dtype_key):
    """the case planes on the device, one tensor each, made once per dtype"""
    if dtype_key not in _device:
        _device[dtype_key] = [dev(image) for image in cases.images(DTYPES[dtype_key])]
    return _device[dtype_key]


def single(plane, image, params):
    """get_footprints_device of one plane, once per image and parameters"""
    from scarlet_amd import detect_pybind11

    key = (id(image), params)
    if key not in _single:
        _single[key] = (image, detect_pybind11.get_footprints_device(plane, *params))
    return _single[key][1]


def batch(planes, params, **kw):
    from scarlet_amd import detect_pybind11

    return detect_pybind11.get_footprints_batch(planes, *params, **kw)


def assert_all_same(got, want, what=""):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert_same(a, b, (what, k))


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_key", list(DTYPES))
def test_all_case_planes_in_one_call(dtype_key):
    images, planes = cases.images(DTYPES[dtype_key]), device_planes(dtype_key)
    for params in cases.PARAMS:
        got = batch(planes, params)
        assert len(got) == len(planes)
        for name, image, plane, fps in zip(cases.NAMES, images, planes, got):
            assert_same(fps, cases.host_footprints(image, params), (name, params, "host"))
            assert_same(fps, single(plane, image, params), (name, params, "per plane"))
    # the planes are not empty-handed: what the host library finds in them
    found = [len(fps) for fps in batch(planes, cases.PARAMS[0])]
    by_name = dict(zip(cases.NAMES, found))
    assert by_name["serpentine_67x129"] == 1 and by_name["combs_67x129"] == 2
    assert by_name["all_zero_37x41"] == by_name["all_nan_5x9"] == by_name["1x1"] == 0
    assert by_name["noise_65x63"] > 20 and by_name["noise_40x50_a"] > 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_negative_combs_with_a_negative_threshold(dtype):
    from scarlet_amd import detect_pybind11

    image = cases.NEGATIVE.astype(dtype)
    plane = dev(image)
    for params in ((0, 4, -1), (3, 1, -1)):
        got = batch([plane], params)
        assert len(got) == 1
        assert_same(got[0], detect_pybind11.get_footprints(image, *params), params)
        assert_same(got[0], detect_pybind11.get_footprints_device(plane, *params), params)
        assert [(tuple(fp.bounds), fp.peaks) for fp in got[0]] == \
            [((0, 64, 0, 128), []), ((2, 66, 0, 128), [])]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kats_equal_their_recorded_answers(dtype):
    """the hand-worked cases, each set of parameters in one call of all cases that use it"""
    by_params = {}
    for name, image, min_sep, min_area, thresh, want in KATS:
        by_params.setdefault((min_sep, min_area, thresh), []).append((name, image, want))
    assert len(by_params) > 3
    for params, group in by_params.items():
        got = batch([dev(image.astype(dtype)) for _, image, _ in group], params)
        for (name, _, want), fps in zip(group, got):
            assert as_lists(fps) == want, name


# ---------------------------------------------------------------------------------------
# the same planes, handed over differently: the per-plane results do not change
# ---------------------------------------------------------------------------------------
PARAMS_V = cases.PARAMS[1]


@pytest.fixture(scope="module")
def base():
    return batch(device_planes("mixed"), PARAMS_V)


def test_reversed(base):
    got = batch(device_planes("mixed")[::-1], PARAMS_V)
    assert_all_same(got[::-1], base, "reversed")


def test_views_into_one_buffer(base):
    """per dtype one flat buffer that holds the planes one after another, as
    get_detect_wavelets_batch(device=True) returns them"""
    import torch

    planes = device_planes("mixed")
    views = [None] * len(planes)
    for dtype in (torch.float32, torch.float64):
        mine = [k for k, p in enumerate(planes) if p.dtype == dtype]
        flat = torch.cat([planes[k].reshape(-1) for k in mine])
        at = 0
        for k in mine:
            views[k] = flat[at:at + planes[k].numel()].reshape(planes[k].shape)
            at += planes[k].numel()
            assert views[k].is_contiguous() and views[k].data_ptr() != planes[k].data_ptr()
    assert_all_same(batch(views, PARAMS_V), base, "views")


def test_a_non_contiguous_slice(base):
    import torch

    planes = list(device_planes("mixed"))
    k = cases.NAMES.index("combs_67x129")
    wide = torch.zeros((69, 140), dtype=planes[k].dtype, device="cuda")
    wide[1:68, 5:134] = planes[k]
    planes[k] = wide[1:68, 5:134]
    j = cases.NAMES.index("noise_40x50_a")
    planes[j] = planes[j].T.contiguous().T
    assert not planes[k].is_contiguous() and not planes[j].is_contiguous()
    assert_all_same(batch(planes, PARAMS_V), base, "slices")


def test_cut_into_chunks(base):
    from scarlet_amd import detect_pybind11

    planes = device_planes("mixed")
    groups = detect_pybind11.plan_footprints_batch(planes, _max_bytes=150000)
    # a 67 x 129 plane needs 276 KB: beyond the budget and alone in its chunk; the small
    # planes before it share one, and the planes of the other dtype take two
    chunks64, chunks32 = groups[np.dtype(np.float64)], groups[np.dtype(np.float32)]
    serpentine, combs = cases.NAMES.index("serpentine_67x129"), cases.NAMES.index("combs_67x129")
    assert [serpentine] in chunks32 and [combs] in chunks32 and len(chunks32[0]) > 3
    assert len(chunks64) == 2 and min(len(c) for c in chunks64) > 2
    stats = []
    got = batch(planes, PARAMS_V, _max_bytes=150000, _stats=stats)
    assert len(stats) == len(chunks64) + len(chunks32)
    assert_all_same(got, base, "chunks")


# ---------------------------------------------------------------------------------------
def test_launches_and_waits_do_not_depend_on_the_number_of_planes():
    planes = device_planes("float32")
    combs = planes[cases.NAMES.index("combs_67x129")]
    params = cases.PARAMS[0]
    one, many, tiles = [], [], []
    batch([combs], params, _stats=one)
    batch(planes, params, _stats=many)
    assert len(one) == len(many) == 1
    # label: eight launches and the wait for the totals; fetch: three launches, one wait
    assert one[0] == many[0] == ((8, 1), (3, 1))
    # planes of a single tile have no border to merge: one launch fewer
    single_tile = [planes[k] for k in cases.SINGLE_TILE]
    assert len(single_tile) > 10
    batch(single_tile, params, _stats=tiles)
    assert tiles == [((7, 1), (3, 1))]


# ---------------------------------------------------------------------------------------
def same_structures(got, want, what=""):
    (g_structs, g_middle), (w_structs, w_middle) = got, want
    assert len(g_structs) == len(w_structs), what
    for a, b in zip(g_structs, w_structs):
        assert a.scale == b.scale and a.bbox == b.bbox, what
        assert sorted(a.peaks) == sorted(b.peaks), what
        for scale in a.peaks:
            assert [(p.y, p.x, p.flux) for p in a.peaks[scale]] == \
                [(p.y, p.x, p.flux) for p in b.peaks[scale]], (what, scale)
        assert a.all_peaks == b.all_peaks and list(a.all_peaks) == list(b.all_peaks), what
    g_query, w_query = list(g_middle.query()), list(w_middle.query())
    assert g_query == w_query, what
    assert_same([b.footprint for b in g_query], [b.footprint for b in w_query], what)


@pytest.mark.parametrize("dtype_key", ["float32", "mixed"])
def test_peaks_and_structures_of_a_catalogue(dtype_key):
    import detect_batch_cases as dbc
    from scarlet_amd import Box, detect

    dtypes = np.float32 if dtype_key == "float32" else dbc.MIXED
    images, variance = dbc.catalogue(dtypes)
    coeffs = detect.get_detect_wavelets_batch(images, variance, scales=3, device=True)
    assert [int(c.shape[0]) for c in coeffs] == [1, 1, 2, 4, 4, 4, 4, 4, 4]
    with pytest.raises(ValueError, match="position 0"):
        detect.get_peaks_batch(coeffs)
    with pytest.raises(ValueError, match="position 0"):
        detect.get_blend_structures_batch(coeffs)
    full = [c for c in coeffs if c.shape[0] == 4]
    peaks = detect.get_peaks_batch(full)
    assert peaks == [detect.get_peaks(c) for c in full]
    assert sum(len(p) for p in peaks) > 10
    # with boxes: a corner of every frame; None stands for the whole frame
    boxes = [None if k % 2 else Box((5, c.shape[1] // 2, c.shape[2] // 2), origin=(0, 1, 2))
             for k, c in enumerate(full)]
    assert detect.get_peaks_batch(full, bboxes=boxes) == \
        [detect.get_peaks(c, bbox=b) for c, b in zip(full, boxes)]
    structures = detect.get_blend_structures_batch(full)
    assert len(structures) == len(full)
    for k, c in enumerate(full):
        same_structures(structures[k], detect.get_blend_structures(c), k)


def test_the_reference_run_through_the_batch():
    """the planes of tests/golden/detect.npz give the footprints and structures that
    test_footprints_and_structures_of_the_reference_run checks for the per-blend path -- twice
    in one call, with a small blend between the two copies"""
    import torch
    from scarlet_amd import Box, detect

    g = golden("detect")
    det = g["detect_s3"]
    small = np.round(np.random.default_rng(7).normal(size=(4, 17, 19)) * 2)
    blends = [dev(det), dev(small), dev(det.copy())]
    fps = batch([b[s] for b in blends for s in range(3)], (0, 4, 0))
    for copy in (0, 2):
        for s in range(3):
            found = fps[3 * copy + s]
            assert as_lists(found) == _golden_footprints(g, s), (copy, s)
            masks = np.concatenate([fp.footprint.ravel() for fp in found])
            assert np.array_equal(np.packbits(masks), g["fp%d_masks" % s]), (copy, s)
    for s in range(3):
        assert_same(fps[3 + s], cases.host_footprints(small[s], (0, 4, 0)), ("small", s))
    structures = detect.get_blend_structures_batch(blends)
    want = [tuple(v) for v in g["lite_centers"].tolist()]
    bbox = Box((5,) + det.shape[1:])
    peaks = detect.get_peaks_batch(blends, bboxes=[bbox, None, bbox])
    for copy in (0, 2):
        structs, middle = structures[copy]
        assert len(structs) == int(g["n_structures"])
        for k, st in enumerate(structs):
            for scale in (0, 1, 2):
                got = [(p.y, p.x) for p in st.peaks.get(scale, [])]
                assert got == [tuple(v) for v in g["struct%d_peaks%d" % (k, scale)].tolist()], \
                    (copy, k, scale)
        order = [(b.origin[0], b.origin[1], b.shape[0], b.shape[1]) for b in middle.query()]
        assert order == [tuple(v) for v in g["middle_query_bounds"].tolist()], copy
        assert peaks[copy] == want, copy
    assert peaks[1] == detect.get_peaks(blends[1]) == detect.get_peaks(small)
    assert torch.equal(blends[0], blends[2])
