"""Device footprints without a GPU: the C-ABI entry points exist and refuse loudly when there is
no device, and the Python side checks rank and type before any device call."""

import ctypes
import inspect

import numpy as np
import pytest


class _NotATensor:
    """claims a shape, is no torch tensor"""
    shape = (4, 4)


def test_device_footprint_symbols_report_no_device():
    from scarlet_amd import _lib

    lib = _lib.load()
    for name in ("smi_footprints_device_label_f32", "smi_footprints_device_label_f64",
                 "smi_footprints_device_fetch_f32", "smi_footprints_device_fetch_f64",
                 "smi_footprints_device_work_bytes", "smi_footprints_device_fetch_bytes"):
        assert hasattr(lib, name), name
    if lib.smi_device_count() > 0:
        pytest.skip("a GPU is present")
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    counts = np.zeros(3, dtype=np.int32)
    cp = _lib.ptr(counts, ctypes.c_int32)
    for fn in (lib.smi_footprints_device_label_f32, lib.smi_footprints_device_label_f64):
        assert fn(p, 1, 4, 4, 4, 0, p, 1 << 20, cp, None) == -3
        assert "no HIP device" in lib.smi_last_error().decode()
    one = np.array([1, 4, 1], dtype=np.int32)
    bounds = np.zeros(4, np.int32)
    masks = np.zeros(4, np.uint8)
    start = np.zeros(2, np.int32)
    yx = np.zeros(2, np.int32)
    flux = np.zeros(1, np.float64)
    for fn in (lib.smi_footprints_device_fetch_f32, lib.smi_footprints_device_fetch_f64):
        assert fn(p, 1, 4, 4, 0, 0.0, _lib.ptr(one, ctypes.c_int32), p, p, 1 << 20,
                  _lib.ptr(bounds, ctypes.c_int32), _lib.ptr(masks, ctypes.c_uint8),
                  _lib.ptr(start, ctypes.c_int32), _lib.ptr(yx, ctypes.c_int32),
                  _lib.ptr(flux, ctypes.c_double), None) == -3
        assert "no HIP device" in lib.smi_last_error().decode()


def test_buffer_sizes_are_arithmetic():
    """the two size functions need no device; the work buffer holds eight int32 per pixel (the
    labels and seven record arrays) plus the scan's chunk sums"""
    from scarlet_amd import _lib

    lib = _lib.load()
    n = ctypes.c_int64(0)
    assert lib.smi_footprints_device_work_bytes(3, 67, 129, ctypes.byref(n)) == 0
    assert 32 * 3 * 67 * 129 <= n.value <= 33 * 3 * 67 * 129 + 4096
    assert lib.smi_footprints_device_work_bytes(1, 65536, 65536, ctypes.byref(n)) == -1
    assert lib.smi_footprints_device_work_bytes(0, 4, 4, ctypes.byref(n)) == -1
    counts = np.array([2, 100, 5], dtype=np.int32)
    assert lib.smi_footprints_device_fetch_bytes(_lib.ptr(counts, ctypes.c_int32),
                                                 ctypes.byref(n)) == 0
    # bounds, offsets and roots of 2 footprints, 5 peak records of 16 bytes, 100 mask bytes
    assert n.value >= 2 * 24 + 5 * 16 + 100


def test_get_footprints_device_refuses_host_arrays_before_any_device_call():
    from scarlet_amd import detect_pybind11

    assert callable(detect_pybind11.get_footprints_device)
    for bad in (np.zeros((4, 4)), np.zeros((4, 4), np.float32), [[1.0, 2.0]], _NotATensor(), None):
        with pytest.raises(TypeError):
            detect_pybind11.get_footprints_device(bad, 0, 4, 0)


def test_get_footprints_device_checks_host_tensors_and_rank():
    """a torch tensor in host memory is no device tensor either"""
    torch = pytest.importorskip("torch")
    from scarlet_amd import detect_pybind11

    with pytest.raises(TypeError):
        detect_pybind11.get_footprints_device(torch.zeros((4, 4)), 0, 4, 0)
    with pytest.raises(TypeError):
        detect_pybind11.get_footprints_device(torch.zeros((2, 2, 4, 4)), 0, 4, 0)


def test_get_detect_wavelets_has_the_device_keyword():
    from scarlet_amd import detect

    par = inspect.signature(detect.get_detect_wavelets).parameters
    assert "device" in par and par["device"].default is False
    assert list(par)[:3] == ["images", "variance", "scales"]


def test_host_arrays_keep_the_host_path(monkeypatch):
    """_scale_footprints of a NumPy array never calls the device route; something that is no
    NumPy array but claims to be a device tensor is handed to it whole, minus the last plane"""
    from scarlet_amd import detect

    calls = []

    def device_route(d_image, min_separation, min_area, thresh):
        calls.append((d_image, min_separation, min_area, thresh))
        return [[], [], []]

    monkeypatch.setattr(detect, "get_footprints_device", device_route)
    det = np.zeros((4, 12, 12))
    det[:3, 3:7, 3:8] = 1.0
    det[:3, 5, 5] = 2.0
    fps = detect._scale_footprints(det)
    assert calls == []
    assert [len(f) for f in fps] == [1, 1, 1]
    assert tuple(fps[0][0].bounds) == (3, 6, 3, 7)
    assert [(p.y, p.x) for p in fps[0][0].peaks] == [(5, 5)]
    structures, middle = detect.get_blend_structures(det)
    assert calls == [] and len(structures) == 1

    monkeypatch.setattr(detect, "_is_device_tensor", lambda x: not isinstance(x, np.ndarray))
    assert detect._scale_footprints(list(range(4))) == [[], [], []]
    assert calls == [([0, 1, 2], 0, 4, 0)]
