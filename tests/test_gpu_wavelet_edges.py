"""The starlet, coadd and multiresolution-support kernels against the float64 restatement
tests/wavelet_oracle.py (itself pinned to the reference's run by tests/test_wavelet_host.py),
bit for bit, at the shapes, options and batches where such kernels go wrong: thin images,
widths around the block edge, spacings past the extent (up to 2^30), more image rows than
the grid has blocks, NaN / huge images beside zero images, every tap guard's boundary,
unconverged and unevenly converging supports, the image-major layout of the C ABI.

The supports are compared exactly as well.  The device's standard deviations differ from
NumPy's in summation order only, so each case first shows on the CPU
(``wavelet_oracle.rounding_margin_ok``) that neither the iteration count nor any
coefficient's side of a threshold hinges on a relative change of ``npix * 2**-52`` in the
``sigma_j``; the seeds below were picked so that this holds, and the assertion stays."""

import ctypes

import numpy as np
import pytest

import wavelet_oracle as wo
from wavelet_oracle import same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 64), (64, 1), (2, 2), (3, 200), (200, 3), (5, 255), (5, 256), (5, 257),
          (9, 513), (37, 63), (64, 64)]


def ids(values):
    return ["x".join(str(v) for v in value) for value in values]


def noise(shape, seed, dtype=np.float64):
    """normal values with a few exact zeros, negative zeros and large entries"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=shape)
    flat = a.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, k)] = 0.0
    flat[rng.integers(0, flat.size, k)] = -0.0
    flat[rng.integers(0, flat.size, k)] *= 1e6
    return a.astype(dtype)


def device_transform(batch, scales, generation):
    """(scales+1, n, H, W) coefficients of a (n, H, W) batch through transform_device"""
    from scarlet_amd import wavelet

    return wavelet.transform_device(wavelet._upload(batch), scales, generation)


def check_batch(batch, scales, generation):
    """transform and reconstruction of every image of the batch against the restatement"""
    from scarlet_amd import wavelet

    d_w = device_transform(batch, scales, generation)
    w = d_w.cpu().numpy()
    assert w.dtype == np.float64 and w.shape == (scales + 1,) + batch.shape
    rec = wavelet.reconstruction_device(d_w, generation).cpu().numpy()
    for b, img in enumerate(batch):
        want = wo.transform(img, scales, generation)
        assert same_bits(w[:, b], want), (b, scales, generation)
        assert same_bits(rec[b], wo.reconstruction(want, generation)), (b, scales, generation)
    return w


# ---------------------------------------------------------------------------
# transform and reconstruction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_edge_shapes_clamped_and_forced_scales(shape, generation, dtype):
    """the clamped number of scales, then scales forced through transform_device up to and
    past the extent (spacings 2^j >= H or W leave the centre tap), and the single plane"""
    from scarlet_amd import wavelet

    img = noise(shape, 100 + shape[0] * 7 + shape[1], dtype)
    clamped = wavelet.get_scales(shape)
    past = max(shape).bit_length()  # 2^past > max extent
    forced = {0, 1, 2, past - 1, past, past + 1, 12}
    if clamped >= 0:
        forced.add(clamped)
    for scales in sorted(forced):
        check_batch(img[None], scales, generation)
    if clamped >= 0:  # the public functions, which clamp
        w = wavelet.starlet_transform(img, 12, generation)
        assert same_bits(w, wo.transform(img, clamped, generation))
        assert same_bits(wavelet.starlet_reconstruction(w, generation),
                         wo.reconstruction(w, generation))
    # coefficient stacks deeper than the clamp through the public reconstruction
    deep = wo.transform(img, past + 1, generation)
    assert same_bits(wavelet.starlet_reconstruction(deep, generation),
                     wo.reconstruction(deep, generation))
    assert same_bits(wavelet.starlet_reconstruction(deep[:1], generation),
                     np.asarray(deep[0], dtype=np.float64))


def test_inputs_the_uploader_converts():
    from scarlet_amd import wavelet

    rng = np.random.default_rng(21)
    base = rng.normal(size=(40, 66)) * 100
    cases = {
        "int16": base.astype(np.int16),
        "uint8": np.abs(base).astype(np.uint8),
        "bool": base > 0,
        "fortran": np.asfortranarray(base),
        "fortran32": np.asfortranarray(base.astype(np.float32)),
        "strided": base[::2, 1::3],
        "strided32": base.astype(np.float32)[::2, 1::3],
        "big-endian": base.astype(">f8"),
        "big-endian32": base.astype(">f4"),
    }
    for name, img in cases.items():
        before = img.copy()
        for generation in (1, 2):
            scales = wavelet.get_scales(img.shape)
            w = wavelet.starlet_transform(img, generation=generation)
            assert same_bits(w, wo.transform(img, scales, generation)), name
            cube = np.stack([img, img[::-1]])
            if name.startswith("strided"):
                cube = np.stack([base, base[::-1]]).astype(img.dtype)[:, ::2, 1::3]
                assert not cube.flags.c_contiguous
            multi = wavelet.multiband_starlet_transform(cube, generation=generation)
            assert multi.dtype == cube.dtype, name
            for b in range(2):
                want = wo.transform(cube[b], scales, generation).astype(cube.dtype)
                assert same_bits(multi[:, b], want), name
        assert np.array_equal(img, before) and img.dtype == before.dtype, name
    # coefficient stacks that are not float64 / not contiguous
    w = wo.transform(base, 3)
    for stack in (w.astype(np.float32), np.asfortranarray(w), w[:, ::2, ::-1], w.astype(">f8")):
        assert same_bits(wavelet.starlet_reconstruction(stack), wo.reconstruction(stack))


@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("n,H,W", [(3, 30000, 8), (2100, 32, 40)], ids=["3x30000x8", "2100x32x40"])
def test_more_image_rows_than_grid_rows(n, H, W, generation):
    """n * H > 65535: every block of the pass kernel walks several rows, across the seams
    between the images of the batch"""
    assert n * H > 65535
    rng = np.random.default_rng(n + generation)
    batch = rng.normal(size=(n, H, W)).astype(np.float32)
    check_batch(batch, 4, generation)


@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("shape", [(11, 13), (16, 70)], ids=ids([(11, 13), (16, 70)]))
def test_no_leak_across_image_seams(shape, generation):
    """zero images between a NaN image and a 1e300 image stay exactly +0.0 at every spacing
    from 1 to past the height"""
    from scarlet_amd import wavelet

    zeros = np.zeros(shape)
    for dtype, huge in ((np.float64, 1e300), (np.float32, 1e38)):
        cube = np.stack([zeros, np.full(shape, np.nan), zeros, np.full(shape, huge),
                         zeros]).astype(dtype)
        for scales in (1, 3, 6):  # spacings 1 .. 32 >= H
            w = check_batch(cube, scales, generation)
            for b in (0, 2, 4):
                assert not w[:, b].any() and not np.signbit(w[:, b]).any(), (b, scales)
            assert np.isnan(w[:, 1]).all()
            assert np.isfinite(w[:, 3]).all() and w[-1, 3].all()
            rec = wavelet.reconstruction_device(wavelet._upload(w), generation).cpu().numpy()
            for b in (0, 2, 4):
                assert not rec[b].any() and not np.signbit(rec[b]).any(), (b, scales)


@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("axis", [0, 1])
def test_unit_impulse_at_every_position(axis, generation):
    """one image per position of a unit impulse along an extent of 11: with spacings 1, 2, 4
    and 8 every tap guard is met at u == d, 2d, L - d, L - 2d and on both sides of them"""
    L, other = 11, 7
    shape = (L, other) if axis == 0 else (other, L)
    batch = np.zeros((L * 2,) + shape)
    for u in range(L):
        for k, v in enumerate((0, other - 1)):
            batch[2 * u + k][(u, v) if axis == 0 else (v, u)] = 1.0
    w = check_batch(batch, 4, generation)
    # the four spacings reach their neighbours: an impulse at 0 shows at d and 2d
    for j, d in enumerate((1, 2, 4)):
        line = w[j + 1, 0, :, 0] if axis == 0 else w[j + 1, 0, 0, :]
        assert line[d] != 0 and line[2 * d] != 0
    check_batch(batch.astype(np.float32), 4, generation)


@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("shape", [(8, 8), (1, 1)], ids=ids([(8, 8), (1, 1)]))
def test_thirty_scales(shape, generation):
    """the admitted maximum: spacings up to 2^29 in the transform and the reconstruction of
    31 planes"""
    from scarlet_amd import wavelet

    batch = np.stack([noise(shape, 7), noise(shape, 8)])
    check_batch(batch, 30, generation)
    w = wo.transform(batch[0], 30, generation)
    assert same_bits(wavelet.starlet_reconstruction(w, generation),
                     wo.reconstruction(w, generation))


# ---------------------------------------------------------------------------
# coadd
# ---------------------------------------------------------------------------
COADD_SHAPES = [(1, 1), (7, 300), (128, 128)]


def coadd_case(bands, shape, dtype, seed):
    rng = np.random.default_rng(seed)
    size = (bands,) + shape
    x = rng.choice([-1.0, 1.0], size=size) * 10 ** rng.uniform(-8, 8, size=size)
    return x.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", COADD_SHAPES, ids=ids(COADD_SHAPES))
@pytest.mark.parametrize("bands", [1, 2, 5, 37])
def test_coadd_is_the_sum_in_band_order(bands, shape, dtype):
    from scarlet_amd import wavelet

    x = coadd_case(bands, shape, dtype, 3)
    want = wo.coadd(x)
    assert want.dtype == dtype
    # another order gives other bits, and so does a wider accumulator (five bands of a single
    # pixel are too few values for that to be certain)
    if bands == 37 or (bands == 5 and shape != (1, 1)):
        assert not np.array_equal(wo.coadd(x[::-1]), want)
        if dtype == np.float32:
            assert not np.array_equal(wo.coadd(x.astype(np.float64)).astype(np.float32), want)
    got = wavelet.coadd_device(wavelet._upload(x)).cpu().numpy()
    assert same_bits(got, want)


# ---------------------------------------------------------------------------
# multiresolution support
# ---------------------------------------------------------------------------
SUPPORT_SHAPES = [(17, 19), (45, 70), (33, 257), (128, 128), (200, 150), (1024, 768)]
SUPPORT_OPTIONS = [(3, 0.1, 20), (2, 1e-3, 20), (5, 0.0, 4), (3, 0.1, 1), (3, 0.1, 2)]
# seed of the synthetic image per (shape, options) where the first seed did not meet the
# rounding margin (wavelet_oracle.rounding_margin_ok); every other case uses seed 0
SUPPORT_SEEDS = {}


def blob_image(shape, seed, blobs=4, noise_sigma=1.0):
    """unit normal noise plus a few Gaussian blobs, float32"""
    rng = np.random.default_rng(seed)
    H, W = shape
    img = rng.normal(size=shape) * noise_sigma
    yy, xx = np.mgrid[:H, :W]
    for _ in range(blobs):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        amp, s = rng.uniform(5, 40), rng.uniform(1, 3)
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return img.astype(np.float32)


def run_support(image_dtype, coeffs, sigma, K, epsilon, max_iter):
    """support of one (planes, H, W) stack on the device: M (int32), M * w, iterations"""
    from scarlet_amd import wavelet

    P = len(coeffs)
    s0, t0 = wavelet.initial_sigma(image_dtype, P, sigma, K)
    d = wavelet._upload(np.asarray(coeffs, dtype=np.float64))
    M, Mw, iters = wavelet.support_device(d[:, None], s0[None], t0[None], K, epsilon, max_iter)
    assert M.dtype.is_floating_point is False and iters.shape == (1,)
    return M[:, 0].cpu().numpy(), Mw[:, 0].cpu().numpy(), int(iters[0])


def check_support(image, coeffs, sigma, K, epsilon, max_iter):
    """margin on the CPU, then device == restatement exactly; returns the restatement's"""
    from scarlet_amd import wavelet

    image = np.asarray(image)
    a, b = wo.rounding_margin_ok(image.dtype, coeffs, sigma, K, epsilon, max_iter)
    assert a, "the iteration count hinges on the rounding of sigma_j: pick another seed"
    assert b, "a coefficient lies within rounding of a threshold: pick another seed"
    M_ref, it_ref, used = wo.support(image.dtype, coeffs, sigma, K, epsilon, max_iter)
    M, Mw, iters = run_support(image.dtype, coeffs, sigma, K, epsilon, max_iter)
    print("support", coeffs.shape, (K, epsilon, max_iter), "iterations", it_ref, iters,
          "mask differences", int((M != M_ref).sum()))
    assert iters == it_ref
    assert M.dtype == np.int32 and np.array_equal(M, M_ref)
    assert set(np.unique(M)) <= {0, 1}
    assert same_bits(Mw, M_ref * np.asarray(coeffs, dtype=np.float64))
    M_public = wavelet.get_multiresolution_support(image, coeffs, sigma, K, epsilon, max_iter)
    assert M_public.dtype == M_ref.dtype == np.dtype(int)
    assert np.array_equal(M_public, M_ref)
    return M_ref, it_ref, used


@pytest.mark.parametrize("K,epsilon,max_iter", SUPPORT_OPTIONS,
                         ids=["K%g-eps%g-it%d" % o for o in SUPPORT_OPTIONS])
@pytest.mark.parametrize("shape", SUPPORT_SHAPES, ids=ids(SUPPORT_SHAPES))
def test_support_at_shapes_and_options(shape, K, epsilon, max_iter):
    """one block per plane (H * W < 2048) up to many partial sums per plane; options other
    than the defaults; epsilon 0 never converges, so the mask is the one of iteration
    max_iter's thresholds"""
    seed = SUPPORT_SEEDS.get((shape, (K, epsilon, max_iter)), 0)
    image = blob_image(shape, seed)
    coeffs = wo.transform(image, 3)
    M, iterations, used = check_support(image, coeffs, np.float32(1.0), K, epsilon, max_iter)
    assert len(used) == iterations <= max_iter
    if epsilon == 0.0 or max_iter == 1:
        assert iterations == max_iter
    if (K, epsilon, max_iter) == (3, 0.1, 20):
        # negative coefficients outside the support: M * w holds -0.0 there
        assert ((M == 0) & (coeffs < 0)).any() and ((M == 1) & (coeffs < 0)).any()


def special_planes(seed=0):
    rng = np.random.default_rng(seed)
    shape = (45, 70)
    big = rng.normal(size=shape) * 1e6       # every coefficient significant at sigma 1
    plain = rng.normal(size=shape) * 3       # not converged after one iteration at sigma 1
    plain[10:14, 20:24] += 90
    zero = np.zeros(shape)
    holed = rng.normal(size=shape)
    holed[7, 9] = np.nan
    return np.stack([big, plain, zero, holed])


def test_support_of_degenerate_planes():
    """a plane that is all significant (its sigma_j becomes 0 and leaves the convergence
    test), an all-zero plane, a plane holding one NaN (its sigma_j is NaN: it leaves the
    convergence test too, its later thresholds are NaN and nothing of it is significant);
    a sigma so small that everything is significant and so large that nothing is"""
    coeffs = special_planes()
    image = np.zeros(coeffs.shape[1:], dtype=np.float32)
    M, iterations, used = check_support(image, coeffs, np.float32(1.0), 3, 0.1, 20)
    assert iterations >= 2
    assert M[0].all() and used[1][0] == 0.0          # all significant, sigma_0 == 0
    assert not M[2].any() and used[1][2] == 0.0      # all zero
    assert not M[3].any() and np.isnan(used[1][3])   # NaN
    assert 0 < M[1].sum() < M[1].size
    # one iteration only: the NaN plane is thresholded with K * sigma like any other
    M1, it1, _ = check_support(image, coeffs, np.float32(1.0), 3, 0.1, 1)
    assert it1 == 1 and M1[3].any() and not M1[3, 7, 9]
    finite = coeffs[:2]
    for image_dtype in (np.float32, np.float64):
        image = np.zeros(finite.shape[1:], dtype=image_dtype)
        M, iterations, used = check_support(image, finite, 1e-30, 3, 0.1, 20)
        assert M.all() and iterations == 1           # no sigma_j left to compare
        M, iterations, used = check_support(image, finite, 1e30, 3, 0.1, 20)
        assert iterations >= 2 and not (np.abs(finite) > used[0][:, None, None]).any()


def uneven_batch():
    """four images of four planes and their initial sigmas, whose supports take different
    numbers of iterations"""
    shape = (45, 70)
    images = [blob_image(shape, 1, blobs=0), blob_image(shape, 2, blobs=12),
              blob_image(shape, 3, blobs=4), blob_image(shape, 4, blobs=4, noise_sigma=3.0)]
    sigmas = [np.float32(1.0), np.float32(1.0), np.float32(20.0), np.float32(0.05)]
    return images, [wo.transform(img, 3) for img in images], sigmas


@pytest.mark.parametrize("K,epsilon,max_iter", [(3, 0.1, 20), (3, 0.02, 6)],
                         ids=["defaults", "eps0.02-it6"])
def test_images_of_one_call_converge_separately(K, epsilon, max_iter):
    """an image that has converged keeps its thresholds and its count while the others go
    on; every image's result is the one of a call of its own"""
    from scarlet_amd import wavelet

    images, stacks, sigmas = uneven_batch()
    want = []
    for img, w, sigma in zip(images, stacks, sigmas):
        a, b = wo.rounding_margin_ok(img.dtype, w, sigma, K, epsilon, max_iter)
        assert a and b
        want.append(wo.support(img.dtype, w, sigma, K, epsilon, max_iter))
    counts = [it for _, it, _ in want]
    print("iterations of the four images", counts)
    assert len(set(counts)) >= (3 if max_iter == 20 else 2) and counts[0] < max(counts)
    if max_iter == 6:  # some images stop at max_iter while the first has long converged
        assert max(counts) == 6 and min(counts) < 6
    d = wavelet._upload(np.stack(stacks, axis=1))  # (planes, n, H, W)
    s0, t0 = zip(*(wavelet.initial_sigma(np.float32, 4, sigma, K) for sigma in sigmas))
    M, Mw, iters = wavelet.support_device(d, np.stack(s0), np.stack(t0), K, epsilon, max_iter)
    M, Mw = M.cpu().numpy(), Mw.cpu().numpy()
    assert iters.tolist() == counts
    for b in range(4):
        assert np.array_equal(M[:, b], want[b][0]), b
        assert same_bits(Mw[:, b], want[b][0] * stacks[b]), b
        alone = run_support(np.float32, stacks[b], sigmas[b], K, epsilon, max_iter)
        assert np.array_equal(M[:, b], alone[0]) and same_bits(Mw[:, b], alone[1])
        assert alone[2] == counts[b]


def test_support_image_major_layout_and_optional_outputs():
    """the C ABI with plane_stride = H*W, image_stride = planes*H*W (Python passes the
    plane-major layout only), and each output left out in turn"""
    import torch
    from scarlet_amd import _lib, wavelet

    lib = _lib.load()
    images, stacks, sigmas = uneven_batch()
    K, epsilon, max_iter = 3, 0.1, 20
    n, P, (H, W) = 4, 4, stacks[0].shape[1:]
    want = [wo.support(np.float32, w, s, K, epsilon, max_iter) for w, s in zip(stacks, sigmas)]
    s0, t0 = zip(*(wavelet.initial_sigma(np.float32, P, sigma, K) for sigma in sigmas))
    s0, t0 = np.ascontiguousarray(np.stack(s0)), np.ascontiguousarray(np.stack(t0))
    d = wavelet._upload(np.stack(stacks, axis=0))  # (n, planes, H, W): image-major
    stream = wavelet._stream(torch)

    def call(with_M, with_Mw):
        M = torch.full((n, P, H, W), -7, dtype=torch.int32, device="cuda") if with_M else None
        Mw = torch.full((n, P, H, W), -7.0, dtype=torch.float64, device="cuda") if with_Mw else None
        iters = np.zeros(n, dtype=np.int32)
        _lib.check(lib.smi_multiresolution_support_f64(
            wavelet._vp(d), n, P, H, W, H * W, P * H * W, _lib.ptr(s0, ctypes.c_double),
            _lib.ptr(t0, ctypes.c_double), float(K), float(epsilon), max_iter,
            wavelet._vp(M) if with_M else None, wavelet._vp(Mw) if with_Mw else None,
            _lib.ptr(iters, ctypes.c_int32), stream))
        torch.cuda.synchronize()
        return (M.cpu().numpy() if with_M else None, Mw.cpu().numpy() if with_Mw else None,
                iters.tolist())

    for with_M, with_Mw in ((True, True), (True, False), (False, True), (False, False)):
        M, Mw, iters = call(with_M, with_Mw)
        assert iters == [it for _, it, _ in want], (with_M, with_Mw)
        for b in range(n):
            if with_M:
                assert np.array_equal(M[b], want[b][0]), b
            if with_Mw:
                assert same_bits(Mw[b], want[b][0] * stacks[b]), b
    # the plane-major call of the Python layer gives the same
    pm = wavelet.support_device(d.transpose(0, 1).contiguous(), s0, t0, K, epsilon, max_iter)
    M, Mw, _ = call(True, True)
    assert np.array_equal(pm[0].cpu().numpy().transpose(1, 0, 2, 3), M)
    assert same_bits(pm[1].cpu().numpy().transpose(1, 0, 2, 3), Mw)
    assert pm[2].tolist() == [it for _, it, _ in want]


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("seed", [1234, 77])
def test_detection_chain_on_synthetic_scenes(seed, dtype):
    """get_detect_wavelets, get_wavelets and get_peaks on synthetic blends against the
    restatement's coadd -> transform -> support -> M * w"""
    from scarlet_amd import Box, detect, synthetic, wavelet

    s = synthetic.make_blend(seed)
    images = s["data"].astype(dtype)
    variance = (1 / s["weights"]).astype(dtype)
    for scales in (3, 9):  # 9 is clamped
        used_scales = wavelet.get_scales(images.shape, scales)
        coadd = wo.coadd(images)
        assert coadd.dtype == dtype
        w = wo.transform(coadd, used_scales)
        sigma = np.median(np.sqrt(variance))
        a, b = wo.rounding_margin_ok(coadd.dtype, w, sigma, 3, 0.1, 20)
        assert a and b
        want = wo.support(coadd.dtype, w, sigma)[0] * w
        got = detect.get_detect_wavelets(images, variance, scales=scales)
        assert same_bits(got, want), scales
        assert 0 < (want != 0).sum() < want.size
        sigmas = np.median(np.sqrt(variance), axis=(1, 2))
        bands = []
        for band, sigma_b in zip(images, sigmas):
            wb = wo.transform(band, used_scales)
            a, b = wo.rounding_margin_ok(band.dtype, wb, sigma_b, 3, 0.1, 20)
            assert a and b
            bands.append(wo.support(band.dtype, wb, sigma_b)[0] * wb)
        assert same_bits(detect.get_wavelets(images, variance, scales=scales), np.array(bands))
        if scales == 3:
            peaks = detect.get_peaks(images=images, variance=variance, bbox=Box(images.shape))
            assert peaks == detect.get_peaks(want) and len(peaks) > 0
