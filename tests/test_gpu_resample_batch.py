"""The pooled spectral chain of scarlet_amd/csrc/resample.hip (LowResPool: N resamplers of one
shape class in a fixed number of launches) against the single resampler, bit for bit, and
against float64 (resample_oracle.py) within the bound tests/test_gpu_resample.py uses for the
single resampler; the guard bands around the pooled outputs must come back untouched.  The
classes are those of the two-resolution blends of tests/multires_batch_cases.py."""

import ctypes
import functools

import numpy as np
import pytest

import multires_batch_cases as mc
import resample_cases as rc
import resample_oracle as ro
from scarlet_amd import _lib
from test_gpu_resample import TOL, Resampler, peak_dev

pytestmark = pytest.mark.gpu

F = ctypes.c_float
N_MAX = 7

# (C, n_a, n_b, Fy, Fx) of every low-resolution observation of the cases
SHAPES = sorted({(bands, side, side) + tuple(fft)
                 for _, lows, _, ffts in mc.CLASSES.values()
                 for (bands, side, _), fft in zip(lows, ffts)})


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@functools.lru_cache(maxsize=None)
def operands(shape):
    """N_MAX resamplers of one class: operands, the float64 results and what the single
    resampler gives for each of them (computed once, read-only)."""
    C, n_a, n_b, Fy, Fx = shape
    lib = _lib.load()
    members = []
    for m in range(N_MAX):
        A, s, model, resid = rc.spectral_operands("pool %d %r" % (m, shape), (Fy, Fx, n_a, n_b, C))
        Pt = ro.circulant(s)
        with Resampler(lib, A, Pt, C, Fy, Fx, n_a, n_b) as r:
            assert r.path == 1
            single = r.render(model), r.adjoint(resid)
        both64 = ro.render64(A, Pt, model), ro.adjoint64(A, Pt, resid)
        members.append((A, np.ascontiguousarray(Pt, np.float32), model, resid) + single + both64)
    for member in members:
        for arr in member:
            arr.setflags(write=False)
    return members


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-na%d-nb%d-F%dx%d" % s)
def test_pooled_chain_gives_every_member_the_bits_of_its_own_resampler(lib, shape, n):
    C, n_a, n_b, Fy, Fx = shape
    # (N = 2 takes the last two: a member's result may not depend on its place in the pool)
    members = operands(shape)[N_MAX - n:] if n == 2 else operands(shape)[:n]
    A, Pt, model, resid = (np.ascontiguousarray(np.stack([m[i] for m in members]))
                           for i in range(4))
    out = np.full((n, C, n_a, n_b), np.nan, np.float32)
    gpad = np.full((n, C, Fy, Fx), np.nan, np.float32)
    guard_ok = ctypes.c_int32(-1)
    _lib.check(lib.smi_lowres_pool_test(n, _lib.ptr(A, F), _lib.ptr(Pt, F), C, n_a, n_b, Fy, Fx,
                                        _lib.ptr(model, F), _lib.ptr(resid, F), _lib.ptr(out, F),
                                        _lib.ptr(gpad, F), ctypes.byref(guard_ok)))
    assert guard_ok.value == 1, "written outside the pooled outputs"
    assert np.isfinite(out).all() and np.isfinite(gpad).all()
    for m, (_, _, _, _, out1, grad1, out64, grad64) in enumerate(members):
        assert np.array_equal(out[m], out1), (m, (out[m] != out1).sum())
        assert np.array_equal(gpad[m], grad1), (m, (gpad[m] != grad1).sum())
        dev = peak_dev(out[m], out64), peak_dev(gpad[m], grad64)
        print("member %d: render %.2e adjoint %.2e" % ((m,) + dev))
        assert max(dev) <= TOL, (m, dev)
