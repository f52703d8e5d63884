"""The kernels of scarlet_amd/csrc/resample.hip one by one against float64 (resample_oracle.py):
the MFMA matrix product and its slice sum bit for bit on integer operands, every variant
and slicing named through smi_gemm_plan, with NaN-filled outputs and guard bands about them;
the dense resampler and its transposes bit for bit; the spectral resampler branch by branch
on Gaussian data, both paths, with impulses that pin where every tile lands."""

import ctypes
import functools

import numpy as np
import pytest

import resample_cases as rc
import resample_oracle as ro
from scarlet_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 2e-5  # of the float64 peak: the project's bound for these products (tools/fuzz_resampler.py)
F = ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------
# a. the product
# ---------------------------------------------------------------------------------------------

def run_product(lib, name, case):
    A, B = rc.product_operands(name, case)
    M, N, K, n_batch = case["M"], case["N"], case["K"], case["n_batch"]
    ref = ro.matmul64(A, B)
    # exact in float32 whatever the order of the sums: asserted on the reference alone
    assert ro.matmul64(np.abs(A), np.abs(B)).max() < 2 ** 24
    scratch = case["scratch"]
    if scratch == "ample":
        scratch = rc.ample_scratch(M, N, K, n_batch)
    C = np.zeros((n_batch, M, N), np.float32)
    plan, guard_ok = (ctypes.c_int32 * 5)(), ctypes.c_int32(-1)
    _lib.check(lib.smi_gemm_test(_lib.ptr(A, F), M * K, _lib.ptr(B, F),
                                 0 if case["shared_b"] else K * N, _lib.ptr(C, F), M * N, n_batch,
                                 M, N, K, scratch, plan, ctypes.byref(guard_ok)))
    plan = dict(zip(("tm", "tn", "bk", "kslice", "n_slices"), plan))
    code, host_plan = rc.gemm_plan(lib, M, N, K, n_batch, scratch)
    assert code == 0 and plan == host_plan  # the launch is the plan
    assert not np.isnan(C).any(), "%d outputs never written" % np.isnan(C).sum()
    assert guard_ok.value == 1, "written outside C or the scratch"
    assert np.array_equal(C, ref), "%d of %d outputs differ" % ((C != ref).sum(), C.size)
    return plan


@pytest.mark.parametrize("name", list(rc.PRODUCT_CASES))
def test_product_is_exact(lib, name):
    case = rc.PRODUCT_CASES[name]
    plan = run_product(lib, name, case)
    # these shapes are small: the 64 x 64 variant, sliced wherever K asks for it
    assert (plan["tm"], plan["tn"], plan["bk"]) == (1, 1, 32)
    assert plan["n_slices"] == rc.slices_wanted(case["K"])


@pytest.mark.parametrize("name", list(rc.VARIANT_CASES))
def test_product_variant_is_exact(lib, name):
    case = rc.VARIANT_CASES[name]
    plan = run_product(lib, name, case)
    for key, val in case["expect"].items():
        assert plan[key] == val, (key, plan)


@pytest.mark.parametrize("name", list(rc.SLICE_CASES))
def test_product_slicing_is_exact(lib, name):
    case = rc.SLICE_CASES[name]
    plan = run_product(lib, name, case)
    for key, val in case["expect"].items():
        assert plan[key] == val, (key, plan)


def test_product_leaves_the_gaps_of_a_strided_output_alone(lib):
    """strideC > M N: the floats between the matrices keep their NaNs (sliced and unsliced)"""
    for K in (17, 641):
        M, N, n_batch, gap = 33, 65, 3, 7
        case = dict(M=M, N=N, K=K, n_batch=n_batch, shared_b=True)
        A, B = rc.product_operands("gaps", case)
        C = np.zeros((n_batch, M * N + gap), np.float32)
        plan, guard_ok = (ctypes.c_int32 * 5)(), ctypes.c_int32(-1)
        _lib.check(lib.smi_gemm_test(_lib.ptr(A, F), M * K, _lib.ptr(B, F), 0, _lib.ptr(C, F),
                                     M * N + gap, n_batch, M, N, K,
                                     rc.ample_scratch(M, N, K, n_batch), plan,
                                     ctypes.byref(guard_ok)))
        assert guard_ok.value == 1
        # (the last matrix has no gap behind it: the buffer ends with it)
        assert np.isnan(C[:-1, M * N:]).all()
        assert np.array_equal(C[:, :M * N].reshape(n_batch, M, N), ro.matmul64(A, B))


# ---------------------------------------------------------------------------------------------
# the resampler through the C interface
# ---------------------------------------------------------------------------------------------

class Resampler:
    def __init__(self, lib, A, Pt, C, Fy, Fx, n_a, n_b):
        self.lib, self.shape = lib, (C, Fy, Fx, n_a, n_b)
        self.handle = ctypes.c_void_p()
        _lib.check(lib.smi_resampler_create(_lib.ptr(A, F), _lib.ptr(Pt, F), C, n_a, n_b, Fy, Fx,
                                            ctypes.byref(self.handle)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.smi_resampler_destroy(self.handle)

    @property
    def path(self):
        path = ctypes.c_int32(-1)
        _lib.check(self.lib.smi_resampler_get_path(self.handle, ctypes.byref(path)))
        return path.value

    def render(self, model):
        C, Fy, Fx, n_a, n_b = self.shape
        model = np.ascontiguousarray(model, np.float32)
        out = np.full((C, n_a, n_b), np.nan, np.float32)
        _lib.check(self.lib.smi_resampler_render(self.handle, _lib.ptr(model, F), _lib.ptr(out, F)))
        return out

    def adjoint(self, resid):
        C, Fy, Fx, n_a, n_b = self.shape
        resid = np.ascontiguousarray(resid, np.float32)
        gpad = np.full((C, Fy, Fx), np.nan, np.float32)
        _lib.check(self.lib.smi_resampler_adjoint(self.handle, _lib.ptr(resid, F),
                                                  _lib.ptr(gpad, F)))
        return gpad


# ---------------------------------------------------------------------------------------------
# b. the dense resampler
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.DENSE_CASES))
def test_dense_resampler_is_exact(lib, name):
    C, Fy, Fx, n_a, n_b = rc.DENSE_CASES[name]
    A, Pt, model, resid = rc.dense_operands(name)
    absA, absPt = np.abs(A), np.abs(Pt)
    # both chained products of either direction stay below 2^24 in absolute terms
    assert ro.matmul64(np.abs(model), absPt).max() < 2 ** 24
    assert ro.render64(absA, absPt, np.abs(model)).max() < 2 ** 24
    assert ro.matmul64(absA.transpose(0, 2, 1), np.abs(resid)).max() < 2 ** 24
    assert ro.adjoint64(absA, absPt, np.abs(resid)).max() < 2 ** 24
    with Resampler(lib, A, Pt, C, Fy, Fx, n_a, n_b) as r:
        assert r.path == 0
        assert lib.smi_resampler_set_path(r.handle, 1) != 0  # not circulant
        out, grad = r.render(model), r.adjoint(resid)
    assert np.array_equal(out, ro.render64(A, Pt, model))
    assert np.array_equal(grad, ro.adjoint64(A, Pt, resid))


# ---------------------------------------------------------------------------------------------
# c. the spectral resampler
# ---------------------------------------------------------------------------------------------

def peak_dev(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def spectral_reference(name):
    """Operands, float64 results and the emulation's own deviation of a row"""
    A, s, model, resid = rc.spectral_operands(name)
    Pt = ro.circulant(s)
    out64, grad64 = ro.render64(A, Pt, model), ro.adjoint64(A, Pt, resid)
    emu_out, emu_grad = ro.spectral_emulation(A, s, model, resid)
    for arr in (A, Pt, model, resid, out64, grad64):
        arr.setflags(write=False)
    return A, Pt, model, resid, out64, grad64, peak_dev(emu_out, out64), peak_dev(emu_grad, grad64)


@pytest.mark.parametrize("name", list(rc.SPECTRAL_CASES))
def test_spectral_resampler_branch(lib, name):
    Fy, Fx, n_a, n_b, C = rc.SPECTRAL_CASES[name]
    A, Pt, model, resid, out64, grad64, emu_out, emu_grad = spectral_reference(name)
    with Resampler(lib, A, Pt, C, Fy, Fx, n_a, n_b) as r:
        assert r.path == 1
        out1, grad1 = r.render(model), r.adjoint(resid)
        _lib.check(lib.smi_resampler_set_path(r.handle, 0))
        assert r.path == 0
        out0, grad0 = r.render(model), r.adjoint(resid)
        # and back: the spectral tables outlive the switch
        _lib.check(lib.smi_resampler_set_path(r.handle, 1))
        assert np.array_equal(r.render(model), out1)
    dev = dict(render1=peak_dev(out1, out64), adjoint1=peak_dev(grad1, grad64),
               render0=peak_dev(out0, out64), adjoint0=peak_dev(grad0, grad64))
    x64, y64 = model.astype(np.float64), resid.astype(np.float64)
    scale = np.sum(np.abs(x64) * np.abs(grad64))
    inner = {p: abs(np.sum(o.astype(np.float64) * y64) - np.sum(x64 * g.astype(np.float64))) / scale
             for p, (o, g) in enumerate(((out0, grad0), (out1, grad1)))}
    cross = dict(render=float(np.abs(out1.astype(np.float64) - out0).max() / np.abs(out64).max()),
                 adjoint=float(np.abs(grad1.astype(np.float64) - grad0).max() / np.abs(grad64).max()))
    print("%s: spectral render %.2e adjoint %.2e | emulation %.2e %.2e | dense %.2e %.2e | "
          "path against path %.2e %.2e | inner product %.2e (dense) %.2e (spectral)"
          % (name, dev["render1"], dev["adjoint1"], emu_out, emu_grad, dev["render0"],
             dev["adjoint0"], cross["render"], cross["adjoint"], inner[0], inner[1]))
    for arr in (out1, grad1, out0, grad0):
        assert np.isfinite(arr).all()
    for key, val in dev.items():
        assert val <= TOL, (key, val)
    for key, val in cross.items():  # two results, each within the bound
        assert val <= 2 * TOL, (key, val)
    for key, val in inner.items():
        assert val <= 2 * TOL, (key, val)


@functools.lru_cache(maxsize=None)
def impulse_reference():
    A, s, _, _ = rc.spectral_operands("impulse", rc.IMPULSE_CASE)
    Pt = ro.circulant(s)
    for arr in (A, Pt):
        arr.setflags(write=False)
    return A, Pt


@pytest.mark.parametrize("path", [1, 0])
def test_impulses_give_the_columns_of_the_operator(lib, path):
    """One model pixel renders to one column of the float64 operator, one low-resolution pixel
    pulls back to one row: a tile written to the wrong place cannot hide behind its size."""
    Fy, Fx, n_a, n_b, C = rc.IMPULSE_CASE
    A, Pt = impulse_reference()
    with Resampler(lib, A, Pt, C, Fy, Fx, n_a, n_b) as r:
        assert r.path == 1
        _lib.check(lib.smi_resampler_set_path(r.handle, path))
        for y, x in rc.IMPULSE_MODEL_PIXELS:
            model = np.zeros((C, Fy, Fx), np.float32)
            model[0, y, x] = 1.0
            ref = ro.render64(A, Pt, model)
            # the column itself, straight from the operands
            P = np.asarray(Pt, np.float64).reshape(Fx, Fx, n_b)[x]  # [x'', b]
            col = A.astype(np.float64).reshape(C, n_a, Fy, Fx)[0, :, y, :] @ P
            assert np.abs(ref[0] - col).max() <= 1e-12 * np.abs(col).max()
            dev = peak_dev(r.render(model), ref)
            print("path %d model pixel (%d, %d): %.2e" % (path, y, x, dev))
            assert dev <= TOL, (y, x, dev)
        for a, b in rc.IMPULSE_RESID_PIXELS:
            resid = np.zeros((C, n_a, n_b), np.float32)
            resid[0, a, b] = 1.0
            ref = ro.adjoint64(A, Pt, resid)
            Pb = np.asarray(Pt, np.float64).reshape(Fx, Fx, n_b)[:, :, b]  # [x', x'']
            row = A.astype(np.float64).reshape(C, n_a, Fy, Fx)[0, a] @ Pb.T
            assert np.abs(ref[0] - row).max() <= 1e-12 * np.abs(row).max()
            dev = peak_dev(r.adjoint(resid), ref)
            print("path %d residual pixel (%d, %d): %.2e" % (path, a, b, dev))
            assert dev <= TOL, (a, b, dev)


def test_circulant_operator_wider_than_2048_keeps_the_dense_products(lib):
    Fy, Fx, n_a, n_b, C = rc.FALLBACK_CASE
    A, s, model, resid = rc.spectral_operands("fallback", rc.FALLBACK_CASE)
    Pt = ro.circulant(s)
    with Resampler(lib, A, Pt, C, Fy, Fx, n_a, n_b) as r:
        assert r.path == 0
        assert lib.smi_resampler_set_path(r.handle, 1) != 0
        assert r.path == 0
        out, grad = r.render(model), r.adjoint(resid)
    dev = peak_dev(out, ro.render64(A, Pt, model)), peak_dev(grad, ro.adjoint64(A, Pt, resid))
    print("Fx = 2049 on the dense products: render %.2e adjoint %.2e" % dev)
    assert max(dev) <= TOL
