"""The planning of ``detect.get_detect_wavelets_batch`` and its task table, without a GPU:
groups by the dtype the device copy takes, input positions, chunks at a task limit and a byte
budget, oversize frames as fallbacks, the errors raised before any device call, and the new
entry points in the header and in the ctypes table.  The scenes are those of
tests/detect_batch_cases.py; their plane and iteration counts are pinned to the oracle here."""

import os
import re

import numpy as np
import pytest

import detect_batch_cases as dc
from conftest import ROOT


def test_catalogue_is_what_the_gpu_tests_assume():
    """plane counts, iteration counts and the rounding margin of all nine blends, float32 and
    float64, at scales 3 and 5"""
    from scarlet_amd import wavelet

    for dtype in (np.float32, np.float64):
        images, variance = dc.catalogue(dtype)
        for scales in (3, 5):
            chains = [dc.oracle_chain(im, var, scales) for im, var in zip(images, variance)]
            for (shape, _), (w, _, M, _, margin) in zip(dc.CATALOGUE, chains):
                assert margin == (True, True), (shape, dtype, scales)
                assert len(w) == wavelet.get_scales(shape, scales) + 1 and M.shape == w.shape
            if scales == 5:
                assert [len(c[0]) for c in chains] == dc.PLANES_5
                assert [c[3] for c in chains] == dc.ITERATIONS_5
    pixels = [h * w for (h, w), _ in dc.CATALOGUE]
    assert len(dc.SMALLEST) == 5
    assert max(pixels[k] for k in dc.SMALLEST) < min(
        p for k, p in enumerate(pixels) if k not in dc.SMALLEST)


def test_plan_groups_by_device_dtype_and_keeps_positions():
    from scarlet_amd import detect

    images, variance = dc.catalogue(dc.MIXED)
    images = images + [np.ones((2, 8, 9), np.int16), np.ones((1, 4, 4), np.float16)]
    variance = variance + [np.ones((2, 8, 9)), np.ones((1, 4, 4))]
    groups, fallback = detect.plan_detect_wavelets_batch(images, variance, scales=5)
    assert fallback == []
    assert list(groups) == [np.dtype(np.float32), np.dtype(np.float64)]  # first appearance
    assert groups[np.dtype(np.float32)] == [[0, 2, 4, 6, 8]]
    assert groups[np.dtype(np.float64)] == [[1, 3, 5, 7, 9, 10]]  # int16, float16 -> float64
    assert detect.plan_detect_wavelets_batch([], []) == ({}, [])


def test_plan_splits_chunks_at_task_limit_and_byte_budget():
    from scarlet_amd import detect, wavelet

    images, variance = dc.catalogue(np.float32)
    groups, _ = detect.plan_detect_wavelets_batch(images, variance, scales=5, _max_tasks=4)
    assert groups[np.dtype(np.float32)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]

    def need(k):
        (h, w), bands = dc.CATALOGUE[k]
        planes = wavelet.get_scales((h, w), 5) + 1
        return h * w * (bands * 4 + (2 * planes + 1) * 8)

    # room for the first six blends but not for the seventh as well; the last two are beyond
    # the budget alone, a chunk each
    budget = need(5) + need(6)
    assert sum(need(k) for k in range(6)) <= budget < sum(need(k) for k in range(7))
    assert need(6) + need(7) > budget and need(7) > budget and need(8) > budget
    groups, fallback = detect.plan_detect_wavelets_batch(images, variance, scales=5,
                                                         _max_bytes=budget)
    assert groups[np.dtype(np.float32)] == [[0, 1, 2, 3, 4, 5], [6], [7], [8]] and not fallback


def test_plan_reports_oversize_frames_as_fallbacks():
    from scarlet_amd import detect, wavelet

    assert wavelet.DETECT_BATCH_MAX_PIXELS == 256 * 256 and wavelet.DETECT_BATCH_MAX_TASKS == 65535
    shapes = [(1, 256, 256), (1, 256, 257), (1, 16, 16), (2, 2, 40000)]
    images = [np.zeros(s, np.float32) for s in shapes]
    groups, fallback = detect.plan_detect_wavelets_batch(images, images)
    assert groups == {np.dtype(np.float32): [[0, 2]]}
    assert [i for i, _ in fallback] == [1, 3]
    assert all("65536 pixels" in reason for _, reason in fallback)
    # what is no cube of bands is left to the per-blend function as well
    groups, fallback = detect.plan_detect_wavelets_batch([np.zeros((8, 8))], [np.zeros((8, 8))])
    assert groups == {} and fallback[0][0] == 0 and "cube" in fallback[0][1]


def test_plan_raises_before_any_device_call(monkeypatch):
    from scarlet_amd import detect, wavelet

    def no_device(*a, **k):
        raise AssertionError("device call")

    monkeypatch.setattr(wavelet, "_torch", no_device)
    monkeypatch.setattr(wavelet, "detect_wavelets_batch_device", no_device)
    images, variance = dc.catalogue(np.float32)
    with pytest.raises(ValueError, match="one entry per blend"):
        detect.plan_detect_wavelets_batch(images, variance[:-1])
    with pytest.raises(ValueError, match="one entry per blend"):
        detect.get_detect_wavelets_batch(images, variance[:-1])
    thin = np.zeros((3, 1, 40), np.float32)
    with pytest.raises(ValueError) as per_blend:
        wavelet._checked_scales(thin.shape, 3)
    for fn in (detect.plan_detect_wavelets_batch, detect.get_detect_wavelets_batch):
        with pytest.raises(ValueError) as batch:
            fn(images + [thin], variance + [thin])
        assert str(batch.value) == str(per_blend.value)
    assert detect.get_detect_wavelets_batch([], []) == []


def test_task_table_of_the_catalogue():
    from scarlet_amd import detect, wavelet

    for dtype in (np.float32, np.float64):
        images, variance = dc.catalogue(dtype)
        sigmas = detect._batch_sigmas(variance)
        table = detect._batch_table(images, sigmas, 5)
        assert table.dtype == wavelet.DETECT_TASK and table.dtype.itemsize == 56
        assert (table["scales"] + 1).tolist() == dc.PLANES_5
        image_off = coeff_off = work_off = 0
        for t, ((h, w), bands), var, planes in zip(table, dc.CATALOGUE, variance, dc.PLANES_5):
            assert (t["bands"], t["h"], t["w"]) == (bands, h, w)
            assert (t["image_off"], t["coeff_off"], t["work_off"]) == (image_off, coeff_off,
                                                                      work_off)
            image_off += bands * h * w
            coeff_off += planes * h * w
            work_off += h * w
            # what get_detect_wavelets passes to the support of this blend
            s0, t0 = wavelet.initial_sigma(dtype, planes, np.median(np.sqrt(var)), 3)
            assert np.all(s0 == t["sigma0"]) and np.all(t0 == t["thresh0"])
            assert s0.dtype == t0.dtype == np.float64
        assert wavelet.detect_table_sizes(table) == (image_off, coeff_off, work_off)
    # the float32 median of sqrt(1.1), ... is not the float64 one: the rounding is the dtype's
    t32 = detect._batch_table(*_with_sigmas(np.float32))
    t64 = detect._batch_table(*_with_sigmas(np.float64))
    assert not np.array_equal(t32["sigma0"], t64["sigma0"])
    assert np.array_equal(t32["sigma0"], t64["sigma0"].astype(np.float32).astype(np.float64))


def _with_sigmas(dtype):
    from scarlet_amd import detect

    images, variance = dc.catalogue(dtype)
    return images, detect._batch_sigmas(variance), 5


def test_entry_point_refuses_a_bad_table_before_any_launch():
    """SMI_ERR_INVALID (-1) for every table or buffer that would let a kernel leave its
    buffers; the checks come before the device is looked for, so nothing is launched (the
    device pointers below are never dereferenced)"""
    import ctypes

    from scarlet_amd import _lib, wavelet

    lib = _lib.load()
    good = wavelet.detect_task_table([(2, 9, 11), (1, 17, 19)], [2, 3], [1.0, 1.0], [3.0, 3.0])
    n_images, n_coeffs, n_work = wavelet.detect_table_sizes(good)
    assert (n_images, n_coeffs, n_work) == (2 * 99 + 323, 3 * 99 + 4 * 323, 99 + 323)
    nbytes = ctypes.c_int64(-1)
    assert lib.smi_detect_wavelets_scratch_bytes(2, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 2 * 32 * 8
    assert lib.smi_detect_wavelets_scratch_bytes(-1, ctypes.byref(nbytes)) == -1
    fake = ctypes.c_void_p(256)  # stands for device memory

    def status(table, sizes=(n_images, n_coeffs, n_work), max_iter=20, generation=2,
               scratch=nbytes.value, fn=lib.smi_detect_wavelets_f32):
        table = np.ascontiguousarray(table)
        return fn(len(table), table.ctypes.data, fake, 3.0, 0.1, max_iter, generation, fake,
                  sizes[0], fake, sizes[1], fake, sizes[2], fake, None, fake, fake, scratch, None)

    def edited(**fields):
        table = good.copy()
        for name, value in fields.items():
            table[name][1] = value
        return table

    bad = {
        "too many pixels": edited(h=256, w=257),
        "no band": edited(bands=0),
        "empty frame": edited(h=0),
        "scales": edited(scales=31),
        "negative scales": edited(scales=-1),
        "more planes than the buffer holds": edited(scales=4),
        "images outside": edited(image_off=n_images - 322),
        "negative offset": edited(image_off=-1),
        "coefficients shared": edited(coeff_off=3 * 99 - 1),
        "coefficients outside": edited(coeff_off=3 * 99 + 1),
        "work plane shared": edited(work_off=98),
        "work plane outside": edited(work_off=100),
    }
    for fn in (lib.smi_detect_wavelets_f32, lib.smi_detect_wavelets_f64):
        for name, table in bad.items():
            assert status(table, fn=fn) == -1, name
            assert lib.smi_last_error(), name
        assert status(good, max_iter=0, fn=fn) == -1
        assert status(good, generation=3, fn=fn) == -1
        assert status(good, scratch=nbytes.value - 1, fn=fn) == -1
        assert status(good, sizes=(n_images - 1, n_coeffs, n_work), fn=fn) == -1
        assert status(good, sizes=(n_images, n_coeffs - 1, n_work), fn=fn) == -1
        assert status(good, sizes=(n_images, n_coeffs, n_work - 1), fn=fn) == -1
    if lib.smi_device_count() == 0:  # a good table gets as far as the device
        assert status(good) == -3
    assert status(good[:0]) == 0  # an empty table is done


def test_new_symbols_are_declared_and_bound():
    from scarlet_amd import _lib

    header = open(os.path.join(ROOT, "include", "scarlet_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("smi_detect_wavelets_f32", "smi_detect_wavelets_f64",
                 "smi_detect_wavelets_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
    args = _lib.SYMBOLS["smi_detect_wavelets_f32"][1]
    assert args == _lib.SYMBOLS["smi_detect_wavelets_f64"][1] and len(args) == 19
    # the record of the table is the header's struct: four int32, three int64, two doubles
    from scarlet_amd import wavelet

    fields = re.search(r"typedef struct smi_detect_task \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == list(wavelet.DETECT_TASK.names)
