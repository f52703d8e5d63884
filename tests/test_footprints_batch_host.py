"""Footprints of a ragged list of planes without a GPU: the plane table and the two size
functions against arithmetic written out here, the planning of groups and chunks, the refusals
before any device call, and the C-ABI entry points, which refuse loudly without a device."""

import ctypes

import numpy as np
import pytest

import footprints_batch_cases as cases


def a16(v):
    return (v + 15) // 16 * 16


def ceil_div(a, b):
    return -(-a // b)


class FakePlane:
    """has what plan_footprints_batch reads, and is no tensor"""

    def __init__(self, shape, dtype="float32", device="cuda:0"):
        self.shape, self.dtype, self.device = shape, dtype, device


def work_bytes(table):
    from scarlet_amd import _lib

    n = ctypes.c_int64(-1)
    status = _lib.load().smi_footprints_batch_work_bytes(
        len(table), ctypes.c_void_p(table.ctypes.data), ctypes.byref(n))
    return status, n.value


def test_plane_record_is_the_c_struct():
    from scarlet_amd.detect_pybind11 import FOOTPRINT_PLANE

    assert FOOTPRINT_PLANE.itemsize == 40
    assert [FOOTPRINT_PLANE.fields[f][1] for f in FOOTPRINT_PLANE.names] == [0, 8, 12, 16, 24, 32]
    assert FOOTPRINT_PLANE.names == ("address", "h", "w", "pixel_off", "tile0", "chunk0")


def test_table_prefixes_of_the_case_list():
    from scarlet_amd.detect_pybind11 import footprint_plane_table

    addresses = [4096 + 8 * k for k in range(len(cases.SHAPES))]
    table = footprint_plane_table(cases.SHAPES, addresses)
    pixels = tiles = chunks = 0
    for k, (h, w) in enumerate(cases.SHAPES):
        row = table[k]
        assert (int(row["address"]), int(row["h"]), int(row["w"])) == (addresses[k], h, w)
        assert (int(row["pixel_off"]), int(row["tile0"]), int(row["chunk0"])) == \
            (pixels, tiles, chunks), cases.NAMES[k]
        pixels += h * w
        tiles += ceil_div(h, 64) * ceil_div(w, 64)
        chunks += ceil_div(h * w, 2048)
    # a few of them by hand: 67 x 129 is 2 x 3 tiles and 8643 pixels = five chunks of 2048,
    # 65 x 63 two tiles and two chunks, the checkerboard one tile and two chunks
    by_name = dict(zip(cases.NAMES, range(len(cases.NAMES))))
    s, c, n = by_name["serpentine_67x129"], by_name["checkerboard_64x64"], by_name["noise_65x63"]
    assert int(table[s + 1]["tile0"] - table[s]["tile0"]) == 6
    assert int(table[s + 1]["chunk0"] - table[s]["chunk0"]) == 5
    assert int(table[c + 1]["tile0"] - table[c]["tile0"]) == 1
    assert int(table[c + 1]["chunk0"] - table[c]["chunk0"]) == 2
    assert int(table[n + 1]["tile0"] - table[n]["tile0"]) == 2
    assert int(table[n + 1]["chunk0"] - table[n]["chunk0"]) == 2

    # the work buffer: the table, the prefix of border blocks (n + 1 int64), the labels, seven
    # int32 records per pixel, two int64 per chunk, four int64 of totals per plane
    status, got = work_bytes(table)
    n_planes = len(table)
    want = (a16(40 * n_planes) + a16(8 * (n_planes + 1)) + a16(4 * pixels) + a16(28 * pixels)
            + a16(16 * chunks) + 32 * n_planes)
    assert (status, got) == (0, want)
    one = footprint_plane_table([(1, 1)], [0])  # the address plays no part in the sizes
    assert work_bytes(one) == (0, 48 + 16 + 16 + 32 + 16 + 32)


def test_work_bytes_refuses_bad_tables():
    from scarlet_amd import _lib
    from scarlet_amd.detect_pybind11 import footprint_plane_table

    lib = _lib.load()
    n = ctypes.c_int64(0)
    assert lib.smi_footprints_batch_work_bytes(1, None, ctypes.byref(n)) == -1
    assert "null plane table" in lib.smi_last_error().decode()
    good = footprint_plane_table([(5, 7), (67, 129), (3, 3)], [64, 128, 256])
    assert work_bytes(good)[0] == 0
    assert lib.smi_footprints_batch_work_bytes(0, ctypes.c_void_p(good.ctypes.data),
                                               ctypes.byref(n)) == -1
    for field, value in (("h", 0), ("w", -1), ("pixel_off", 34), ("tile0", 2), ("chunk0", 0)):
        bad = good.copy()
        bad[1][field] = value
        assert work_bytes(bad)[0] == -1, field
    # 65536 x 32768 = 2^31 pixels is one too many; 65536 x 32767 is allowed
    assert work_bytes(footprint_plane_table([(65536, 32768)], [64]))[0] == -1
    assert "pixels in a plane" in lib.smi_last_error().decode()
    assert work_bytes(footprint_plane_table([(65536, 32767)], [64]))[0] == 0


def test_fetch_bytes_is_arithmetic():
    from scarlet_amd import _lib

    lib = _lib.load()
    n = ctypes.c_int64(0)
    counts = np.array([[2, 100, 5], [0, 0, 0], [1, 9, 0]], dtype=np.int32)
    assert lib.smi_footprints_batch_fetch_bytes(3, _lib.ptr(counts, ctypes.c_int32),
                                                ctypes.byref(n)) == 0
    fp, mask, peaks = 3, 109, 5
    # two int32 prefixes over the planes; first mask byte, root and plane of every footprint;
    # then the block that is downloaded whole: bounds, the counter, 24-byte peak records, masks
    want = 2 * a16(4 * 4) + 3 * a16(4 * fp) + 16 * fp + 16 + 24 * peaks + a16(mask)
    assert n.value == want
    assert lib.smi_footprints_batch_fetch_bytes(3, None, ctypes.byref(n)) == -1
    bad = counts.copy()
    bad[1, 1] = -1
    assert lib.smi_footprints_batch_fetch_bytes(3, _lib.ptr(bad, ctypes.c_int32),
                                                ctypes.byref(n)) == -1
    # totals beyond int32: each plane's mask bytes fit, their sum does not
    big = np.array([[1, 2 ** 30, 0], [1, 2 ** 30, 0]], dtype=np.int32)
    assert lib.smi_footprints_batch_fetch_bytes(2, _lib.ptr(big, ctypes.c_int32),
                                                ctypes.byref(n)) == -1
    assert "2^31" in lib.smi_last_error().decode()


def test_plan_groups_by_dtype_and_cuts_chunks():
    from scarlet_amd import detect_pybind11 as dp

    assert dp.FOOTPRINT_BATCH_BYTES == 1 << 30
    planes = [FakePlane((10, 10), "float32"), FakePlane((20, 5), "float64"),
              FakePlane((64, 64), "torch.float32"), FakePlane((3, 3), "torch.float64")]
    groups = dp.plan_footprints_batch(planes)
    assert list(groups) == [np.dtype(np.float32), np.dtype(np.float64)]
    assert groups[np.dtype(np.float32)] == [[0, 2]] and groups[np.dtype(np.float64)] == [[1, 3]]
    assert dp.plan_footprints_batch([]) == {}

    # 32 bytes per pixel and a little more: with a budget of 4000 bytes a 10 x 10 plane (3296)
    # fills a chunk, a 5 x 5 one (896) leaves room for three more, and the 64 x 64 plane
    # (131184) is beyond the budget and alone in its chunk
    shapes = [(10, 10), (5, 5), (5, 5), (5, 5), (5, 5), (5, 5), (64, 64), (5, 5), (10, 10)]
    need = [32 * h * w + 16 * ceil_div(h * w, 2048) + 80 for h, w in shapes]
    assert need[:2] == [3296, 896] and need[6] == 131184
    groups = dp.plan_footprints_batch([FakePlane(s) for s in shapes], _max_bytes=4000)
    chunks = groups[np.dtype(np.float32)]
    assert chunks == [[0], [1, 2, 3, 4], [5], [6], [7], [8]]
    # (80 bytes per chunk cover the roundings to 16 bytes and the last entry of a prefix)
    for chunk in chunks:
        assert len(chunk) == 1 or 80 + sum(need[i] for i in chunk) <= 4000
    # and the library's count of a chunk's buffer is within that sum
    for chunk in chunks:
        table = dp.footprint_plane_table([shapes[i] for i in chunk], [64] * len(chunk))
        status, got = work_bytes(table)
        assert status == 0 and got <= 80 + sum(need[i] for i in chunk)


def test_plan_refusals():
    torch = pytest.importorskip("torch")
    from scarlet_amd import detect_pybind11 as dp

    for bad in (np.zeros((4, 4), np.float32), [[1.0, 2.0]], None, torch.zeros((4, 4)),
                FakePlane((4, 4), device="cpu")):
        with pytest.raises(TypeError):
            dp.plan_footprints_batch([FakePlane((4, 4)), bad])
    for dtype in ("float16", "torch.bfloat16", "int32", "torch.complex64"):
        with pytest.raises(TypeError):
            dp.plan_footprints_batch([FakePlane((4, 4), dtype)])
    for shape in ((4,), (2, 4, 4), (0, 4), (4, 0), ()):
        with pytest.raises(ValueError):
            dp.plan_footprints_batch([FakePlane((4, 4)), FakePlane(shape)])
    with pytest.raises(ValueError, match="cuda:1"):
        dp.plan_footprints_batch([FakePlane((4, 4)), FakePlane((4, 4), device="cuda:1")])


def _no_library(monkeypatch):
    from scarlet_amd import _lib

    def boom():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", boom)


def test_batch_calls_refuse_host_arrays_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from scarlet_amd import detect, detect_pybind11

    _no_library(monkeypatch)
    for bad in (np.zeros((4, 4)), np.zeros((4, 4), np.float32), [[1.0, 2.0]], None,
                torch.zeros((4, 4)), FakePlane((4, 4))):
        with pytest.raises(TypeError):
            detect_pybind11.get_footprints_batch([bad], 0, 4, 0)
    for bad in (np.zeros((4, 8, 8)), torch.zeros((4, 8, 8)), None):
        with pytest.raises(TypeError):
            detect.get_peaks_batch([bad])
        with pytest.raises(TypeError):
            detect.get_blend_structures_batch([bad])
    assert detect_pybind11.get_footprints_batch([], 0, 4, 0) == []
    assert detect.get_peaks_batch([]) == [] and detect.get_blend_structures_batch([]) == []


def test_batch_calls_refuse_short_blends_before_any_device_call(monkeypatch):
    """a blend with fewer than four planes has no third scale: the position is named"""
    from scarlet_amd import detect

    _no_library(monkeypatch)
    monkeypatch.setattr(detect, "_is_device_tensor", lambda x: isinstance(x, FakePlane))
    full, short = FakePlane((4, 8, 8), "torch.float64"), FakePlane((3, 8, 8), "torch.float64")
    for fn in (detect.get_peaks_batch, detect.get_blend_structures_batch):
        with pytest.raises(ValueError, match="position 2"):
            fn([full, full, short, full])
        with pytest.raises(ValueError, match="position 0"):
            fn([FakePlane((1, 2, 2)), short])
        with pytest.raises(ValueError, match="position 1"):
            fn([full, FakePlane((8, 8))])
    with pytest.raises(ValueError, match="2 blends and 1 boxes"):
        detect.get_peaks_batch([full, full], bboxes=[None])


def test_batch_footprint_symbols_report_no_device():
    from scarlet_amd import _lib
    from scarlet_amd.detect_pybind11 import footprint_plane_table

    lib = _lib.load()
    for name in ("smi_footprints_batch_label_f32", "smi_footprints_batch_label_f64",
                 "smi_footprints_batch_fetch_f32", "smi_footprints_batch_fetch_f64",
                 "smi_footprints_batch_work_bytes", "smi_footprints_batch_fetch_bytes"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    if lib.smi_device_count() > 0:
        return  # (with a device the calls are the subject of tests/test_gpu_footprints_batch.py)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    table = footprint_plane_table([(4, 4)], [p.value])
    tp = ctypes.c_void_p(table.ctypes.data)
    counts = np.zeros((1, 3), dtype=np.int32)
    stats = np.zeros(2, dtype=np.int32)
    for fn in (lib.smi_footprints_batch_label_f32, lib.smi_footprints_batch_label_f64):
        assert fn(tp, 1, 4, 0, p, 1 << 20, _lib.ptr(counts, ctypes.c_int32),
                  _lib.ptr(stats, ctypes.c_int32), None) == -3
        assert "no HIP device" in lib.smi_last_error().decode()
        assert fn(None, 1, 4, 0, p, 1 << 20, _lib.ptr(counts, ctypes.c_int32), None, None) == -1
    one = np.array([[1, 4, 1]], dtype=np.int32)
    bounds, masks = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    fp_start, start = np.zeros(2, np.int32), np.zeros(2, np.int32)
    yx, flux = np.zeros(2, np.int32), np.zeros(1, np.float64)
    for fn in (lib.smi_footprints_batch_fetch_f32, lib.smi_footprints_batch_fetch_f64):
        assert fn(tp, 1, 0.0, _lib.ptr(one, ctypes.c_int32), p, p, 1 << 20,
                  _lib.ptr(bounds, ctypes.c_int32), _lib.ptr(masks, ctypes.c_uint8),
                  _lib.ptr(fp_start, ctypes.c_int32), _lib.ptr(start, ctypes.c_int32),
                  _lib.ptr(yx, ctypes.c_int32), _lib.ptr(flux, ctypes.c_double), None,
                  None) == -3
        assert "no HIP device" in lib.smi_last_error().decode()
