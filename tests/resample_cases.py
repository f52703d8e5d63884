"""Case tables of the resampling tests (test_resample_host.py, test_gpu_resample.py) and the
deterministic operands that go with them."""

import ctypes

import numpy as np

SLICE_TERMS = 320  # kSliceTerms of resample.hip: float32 accumulation length inside a slice

# --- smi_gemm_plan sweep (host) -----------------------------------------------------------
PLAN_MN = (1, 32, 33, 64, 65, 96, 97, 128, 129, 300, 15000)
PLAN_K = (1, 15, 16, 17, 319, 320, 321, 336, 337, 1280, 1281, 90000)
PLAN_BATCH = (1, 3, 50)


def slices_wanted(K):
    return max(1, -(-K // SLICE_TERMS))


def ample_scratch(M, N, K, n_batch):
    return slices_wanted(K) * n_batch * M * N


def few_rule(M, N, K, n_batch):
    """The rule of gemm_plan's comment: 64 x 64 tiles and k tiles of twice the depth where the
    tiles of the default variant times the slices wanted are fewer than 200."""
    tm, tn = (1 if M <= 96 else 2), (1 if N <= 96 else 2)
    tiles = -(-M // (64 * tm)) * -(-N // (64 * tn)) * n_batch
    return tiles * slices_wanted(K) < 200


def gemm_plan(lib, M, N, K, n_batch, scratch_elems):
    """(return code, dict of the plan) of smi_gemm_plan"""
    plan = (ctypes.c_int32 * 5)()
    rc = lib.smi_gemm_plan(M, N, K, n_batch, scratch_elems, plan)
    return rc, dict(zip(("tm", "tn", "bk", "kslice", "n_slices"), plan))


# --- a. the product ------------------------------------------------------------------------
_AXIS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 161)
_K = (1, 2, 15, 16, 17, 31, 32, 33, 319, 320, 321, 336, 337, 641)


def _product(M, N, K, n_batch=1, shared_b=True, scratch="ample", **expect):
    return dict(M=M, N=N, K=K, n_batch=n_batch, shared_b=shared_b, scratch=scratch, expect=expect)


def _product_table():
    cases = {}
    # either axis against a partner of 70, and the diagonal; K walks through its list
    for i, m in enumerate(_AXIS):
        cases["M%d-x70-K%d" % (m, _K[i % len(_K)])] = _product(m, 70, _K[i % len(_K)])
        cases["70xN%d-K%d" % (m, _K[(i + 5) % len(_K)])] = _product(70, m, _K[(i + 5) % len(_K)])
        cases["diag%d-K%d" % (m, _K[(i + 9) % len(_K)])] = _product(m, m, _K[(i + 9) % len(_K)])
    # every K on one shape off the tiles
    for k in _K:
        cases["65x33-K%d" % k] = _product(65, 33, k)
    # batches: the right operand shared (stride 0, as Pt and Wx are) or one per matrix
    for m, n, k in ((65, 97, 33), (129, 70, 321), (33, 129, 641), (97, 161, 17)):
        for shared in (True, False):
            cases["batch3-%dx%dx%d-%s" % (m, n, k, "shared" if shared else "strided")] = _product(
                m, n, k, n_batch=3, shared_b=shared)
    return cases


PRODUCT_CASES = _product_table()

# one case per kernel variant gemm_mfma_kernel<tm, tn, bk>
VARIANT_CASES = {
    "variant<1,1,32>": _product(33, 65, 17, tm=1, tn=1, bk=32),
    "variant<1,1,16>": _product(70, 70, 16001, tm=1, tn=1, bk=16),
    "variant<1,2>": _product(90, 129, 33, n_batch=50, tm=1, tn=2, bk=16),
    "variant<2,1>": _product(129, 90, 33, n_batch=50, tm=2, tn=1, bk=16),
    "variant<2,2>": _product(129, 161, 321, n_batch=50, tm=2, tn=2, bk=16),
}

# slicing of K = 641 under ample, tight and no scratch; and the rule that a product of 2048
# tiles or more with K <= 1280 runs unsliced however much scratch there is.  (512 matrices of
# 65 x 65: four 64 x 64 tiles each.  A batch of 32 products 512 x 512 x 321 is 16 tiles of
# 128 x 128 each, 512 in all, and stays sliced in two: test_resample_host.py pins that.)
SLICE_CASES = {
    "K641-ample-3-slices": _product(97, 70, 641, n_slices=3),
    "K641-scratch-for-2": _product(97, 70, 641, scratch=2 * 97 * 70, n_slices=2),
    "K641-scratch-for-2-less-one": _product(97, 70, 641, scratch=2 * 97 * 70 - 1, n_slices=1),
    "K641-no-scratch": _product(97, 70, 641, scratch=0, n_slices=1),
    "2048-tiles-K321-unsliced": _product(65, 65, 321, n_batch=512, n_slices=1, tm=1, tn=1, bk=16),
}


def product_operands(name, case):
    """Integer operands in {-2 .. 2}, about a third of them zero: (A[n][M][K], B[n or 1][K][N])"""
    rng = np.random.RandomState(sum(map(ord, name)) % (2 ** 31))
    p = (1 / 6., 1 / 6., 1 / 3., 1 / 6., 1 / 6.)
    nB = 1 if case["shared_b"] else case["n_batch"]
    A = rng.choice(np.arange(-2, 3), (case["n_batch"], case["M"], case["K"]), p=p)
    B = rng.choice(np.arange(-2, 3), (nB, case["K"], case["N"]), p=p)
    return A.astype(np.float32), B.astype(np.float32)


# --- b. the dense resampler: (C, Fy, Fx, n_a, n_b) -------------------------------------------
DENSE_CASES = {
    "C1-5x33-na1-nb1": (1, 5, 33, 1, 1),
    "C3-17x40-na13-nb7": (3, 17, 40, 13, 7),
    "C2-130x100-na33-nb70": (2, 130, 100, 33, 70),
    "C1-97x129-na29-nb65": (1, 97, 129, 29, 65),
}


def dense_operands(name):
    """Integer A, Pt (not circulant), model and residual in {-1, 0, 1}"""
    C, Fy, Fx, n_a, n_b = DENSE_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    draw = lambda *shape: rng.randint(-1, 2, shape).astype(np.float32)  # noqa: E731
    return (draw(C, n_a, Fy * Fx), draw(Fx, Fx * n_b), draw(C, Fy, Fx), draw(C, n_a, n_b))


# --- c. the spectral resampler: one row per branch, (Fy, Fx, n_a, n_b, C) -----------------
SPECTRAL_CASES = {
    # Kx = Fx / 2 + 1 either side of the 64-lane chunk of k, Fx even (Nyquist weight 1) and odd
    "Kx64-Fx126-even-nyquist-in-last-lane": (5, 126, 13, 63, 1),
    "Kx64-Fx127-odd-no-nyquist": (17, 127, 3, 64, 1),
    "Kx65-Fx128-even-nyquist-alone-in-chunk-2": (64, 128, 16, 65, 1),
    "Kx65-Fx129-odd-C3": (65, 129, 17, 65, 3),
    "Kx130-Fx258-three-k-chunks": (113, 258, 16, 70, 1),
    "Fx322-both-transforms-sliced": (130, 322, 29, 130, 1),
    # rows y per wavefront: idle wavefronts, tail only, unrolled body + tail
    "Fy1-idle-wavefronts-na1-nb1": (1, 40, 1, 1, 1),
    "Fy5-tail-only-C3": (5, 66, 3, 1, 3),
    "Fy130-body-and-tail-na13-nb64": (130, 70, 13, 64, 1),
    "Fy17-Kx66-na29-nb63-C3": (17, 130, 29, 63, 3),
    "Fy64-Kx33-na17-nb130": (64, 65, 17, 130, 1),
    "Fy113-Kx17-na16-nb65": (113, 33, 16, 65, 1),
}

IMPULSE_CASE = (65, 129, 17, 65, 1)  # Kx = 65, n_b = 65: one past the chunks of k and of b
IMPULSE_MODEL_PIXELS = ((0, 0), (64, 128), (16, 64))  # corners; second pass of y / second x tile
IMPULSE_RESID_PIXELS = ((0, 0), (16, 64), (4, 63))  # corners (a = 16: tail after the body)

FALLBACK_CASE = (2, 2049, 2, 1, 1)  # Fx > 2048: a circulant operator keeps the dense products


def spectral_operands(name, shape=None):
    """Gaussian A, shift kernels s[n_b][Fx], model and residual (float32)"""
    Fy, Fx, n_a, n_b, C = shape or SPECTRAL_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    draw = lambda *s: rng.normal(0, 1, s).astype(np.float32)  # noqa: E731
    return draw(C, n_a, Fy * Fx), draw(n_b, Fx), draw(C, Fy, Fx), draw(C, n_a, n_b)
