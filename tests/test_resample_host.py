"""The host side of the multi-resolution products: the launch plan of the matrix product
(smi_gemm_plan, no GPU needed) over a sweep of shapes, and the identities of the float64
oracle the GPU tests compare against (tests/resample_oracle.py)."""

import itertools

import numpy as np
import pytest

import resample_cases as rc
import resample_oracle as ro
from scarlet_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _scratches(M, N, K, n_batch):
    ample = rc.ample_scratch(M, N, K, n_batch)
    return {"ample": ample, "tight": max(0, ample // 2 - 1), "zero": 0}


def test_plan_properties_over_the_sweep(lib):
    n = 0
    for M, N, K, n_batch in itertools.product(rc.PLAN_MN, rc.PLAN_MN, rc.PLAN_K, rc.PLAN_BATCH):
        for kind, scratch in _scratches(M, N, K, n_batch).items():
            code, p = rc.gemm_plan(lib, M, N, K, n_batch, scratch)
            what = (M, N, K, n_batch, kind, p)
            assert code == 0, what
            assert p["kslice"] > 0 and p["kslice"] % 16 == 0, what
            # every slice holds terms, and together they cover K
            assert p["n_slices"] * p["kslice"] >= K > (p["n_slices"] - 1) * p["kslice"], what
            assert p["n_slices"] == 1 or p["n_slices"] * n_batch * M * N <= scratch, what
            assert p["n_slices"] * n_batch <= 65535, what
            few = rc.few_rule(M, N, K, n_batch)
            assert ((p["tm"], p["tn"], p["bk"]) == (1, 1, 32)) == few, what
            if not few:
                assert (p["tm"], p["tn"], p["bk"]) == (1 if M <= 96 else 2, 1 if N <= 96 else 2, 16), what
            if kind == "zero":
                assert p["n_slices"] == 1, what
            if kind == "ample":  # never more slices than K / 320 asks for
                assert p["n_slices"] <= rc.slices_wanted(K), what
            n += 1
    assert n == 11 * 11 * 12 * 3 * 3


def test_plan_refuses_a_grid_beyond_the_z_limit(lib):
    # 1563 slices of 320 terms x 50 matrices = 78150 > 65535
    code, p = rc.gemm_plan(lib, 1, 1, 500000, 50, rc.ample_scratch(1, 1, 500000, 50))
    assert code != 0 and "z limit" in lib.smi_last_error().decode()
    assert p["n_slices"] * 50 > 65535
    # the same product without scratch runs unsliced: 50 <= 65535
    code, p = rc.gemm_plan(lib, 1, 1, 500000, 50, 0)
    assert code == 0 and p["n_slices"] == 1
    # the batch alone
    assert rc.gemm_plan(lib, 1, 1, 16, 65535, 0)[0] == 0
    assert rc.gemm_plan(lib, 1, 1, 16, 65536, 0)[0] != 0
    # just inside: 1311 slices x 50 = 65550 > 65535, 1310 x 50 = 65500
    K = 1310 * 320
    assert rc.gemm_plan(lib, 1, 1, K, 50, rc.ample_scratch(1, 1, K, 50))[0] == 0
    assert rc.gemm_plan(lib, 1, 1, K + 1, 50, rc.ample_scratch(1, 1, K + 1, 50))[0] != 0


def test_plan_refuses_empty_products(lib):
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1)):
        assert rc.gemm_plan(lib, *shape, 0)[0] != 0, shape


def test_plan_of_the_named_cases(lib):
    """The cases of test_gpu_resample.py run the variant and the slicing they are named for."""
    for name, case in {**rc.VARIANT_CASES, **rc.SLICE_CASES}.items():
        scratch = case["scratch"]
        if scratch == "ample":
            scratch = rc.ample_scratch(case["M"], case["N"], case["K"], case["n_batch"])
        code, p = rc.gemm_plan(lib, case["M"], case["N"], case["K"], case["n_batch"], scratch)
        assert code == 0, name
        for key, val in case["expect"].items():
            assert p[key] == val, (name, key, p)
    # the tile rule counts tiles of the variant that runs: 32 products of 512 x 512 are 512
    # tiles of 128 x 128, fewer than 2048, and K = 321 stays cut in two
    code, p = rc.gemm_plan(lib, 512, 512, 321, 32, rc.ample_scratch(512, 512, 321, 32))
    assert code == 0 and (p["tm"], p["tn"], p["n_slices"]) == (2, 2, 2)
    # 2048 tiles of 128 x 128: unsliced
    code, p = rc.gemm_plan(lib, 1024, 1024, 321, 32, rc.ample_scratch(1024, 1024, 321, 32))
    assert code == 0 and (p["tm"], p["tn"], p["n_slices"]) == (2, 2, 1)
    # ... up to K = 1280 only
    code, p = rc.gemm_plan(lib, 1024, 1024, 1281, 32, rc.ample_scratch(1024, 1024, 1281, 32))
    assert code == 0 and p["n_slices"] == 5


def test_case_tables_cover_what_they_claim():
    axis = {1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 161}
    ks = {1, 2, 15, 16, 17, 31, 32, 33, 319, 320, 321, 336, 337, 641}
    cases = rc.PRODUCT_CASES.values()
    assert 50 <= len(rc.PRODUCT_CASES) <= 70
    assert {c["M"] for c in cases if c["N"] == 70} >= axis
    assert {c["N"] for c in cases if c["M"] == 70} >= axis
    assert {c["M"] for c in cases if c["M"] == c["N"]} >= axis
    assert {c["K"] for c in cases} >= ks
    assert {(c["n_batch"], c["shared_b"]) for c in cases} >= {(1, True), (3, True), (3, False)}
    rows = list(rc.SPECTRAL_CASES.values())
    assert {r[0] for r in rows} >= {1, 5, 17, 64, 65, 113, 130}
    assert {r[1] for r in rows} >= {126, 127, 128, 129, 258, 322}
    assert {r[2] for r in rows} >= {1, 3, 13, 16, 17, 29}
    assert {r[3] for r in rows} >= {1, 63, 64, 65, 130}
    assert {r[4] for r in rows} == {1, 3}


SMALL = {"odd": (7, 15, 3, 5, 2), "even": (6, 16, 4, 3, 1), "Fy1": (1, 9, 1, 1, 1)}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_spectral_emulation_in_float64_is_the_dense_map(name):
    A, s, model, resid = rc.spectral_operands(name, SMALL[name])
    Pt = ro.circulant(s)
    out, grad = ro.spectral_emulation(A, s, model, resid, table_dtype=np.float64)
    ref_out, ref_grad = ro.render64(A, Pt, model), ro.adjoint64(A, Pt, resid)
    assert np.abs(out - ref_out).max() <= 1e-12 * np.abs(ref_out).max()
    assert np.abs(grad - ref_grad).max() <= 1e-12 * np.abs(ref_grad).max()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_spectral_emulation_in_float32_is_close_and_not_equal(name):
    """The float32 tables cost 1e-8 .. 1e-6 of the peak: far inside the 2e-5 the device is
    held to, and not zero (the emulation does round)."""
    A, s, model, resid = rc.spectral_operands(name, SMALL[name])
    Pt = ro.circulant(s)
    out, grad = ro.spectral_emulation(A, s, model, resid)
    for got, ref in ((out, ro.render64(A, Pt, model)), (grad, ro.adjoint64(A, Pt, resid))):
        dev = np.abs(got - ref).max() / np.abs(ref).max()
        assert 0 < dev < 2e-6, dev


@pytest.mark.parametrize("circ", [False, True])
def test_adjoint64_is_the_transpose_of_render64(circ):
    C, Fy, Fx, n_a, n_b = 2, 7, 12, 5, 4
    rng = np.random.RandomState(5)
    A = rng.normal(0, 1, (C, n_a, Fy * Fx))
    Pt = ro.circulant(rng.normal(0, 1, (n_b, Fx))) if circ else rng.normal(0, 1, (Fx, Fx * n_b))
    x, y = rng.normal(0, 1, (C, Fy, Fx)), rng.normal(0, 1, (C, n_a, n_b))
    lhs, rhs = np.sum(ro.render64(A, Pt, x) * y), np.sum(x * ro.adjoint64(A, Pt, y))
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(x) * np.abs(ro.adjoint64(A, Pt, y)))


def test_circulant_matches_its_definition():
    kern = np.arange(12, dtype=np.float64).reshape(2, 6)
    Pt = ro.circulant(kern).reshape(6, 6, 2)  # [x', x, b]
    for xp, x, b in itertools.product(range(6), range(6), range(2)):
        assert Pt[xp, x, b] == kern[b, (x - xp) % 6]
    # render64 with it is a circular convolution along x
    model = np.zeros((1, 1, 6))
    model[0, 0, 2] = 1.0
    A = np.eye(6).reshape(1, 6, 6)  # n_a = Fx, Fy = 1: picks column x
    assert np.array_equal(ro.render64(A, ro.circulant(kern), model)[0, :, 1], np.roll(kern[1], 2))


def test_integer_operands_are_exact_in_float32():
    """What the bit-for-bit GPU tests rest on: sum |a||b| < 2^24 for every case of the tables"""
    for name, case in {**rc.PRODUCT_CASES, **rc.VARIANT_CASES, **rc.SLICE_CASES}.items():
        assert 2 * 2 * case["K"] < 2 ** 24, name
    for name, (C, Fy, Fx, n_a, n_b) in rc.DENSE_CASES.items():
        # |model . Pt| <= Fx, |A . B| <= Fy Fx Fx; the adjoint: n_a, then Fx n_b n_a
        assert Fy * Fx * Fx < 2 ** 24 and Fx * n_b * n_a < 2 ** 24, name
