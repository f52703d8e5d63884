"""``detect.get_detect_wavelets_batch`` and its plumbing ``wavelet.detect_wavelets_batch_device``
(csrc/detect_batch.hip) against the per-blend calls, bit for bit and without a margin
condition -- the batch reproduces the per-blend summation tree -- and, where
``wavelet_oracle.rounding_margin_ok`` holds, against the CPU restatement
tests/wavelet_oracle.py.  The scenes are those of tests/detect_batch_cases.py."""

import numpy as np
import pytest

import detect_batch_cases as dc
import init_cases as ic
from wavelet_oracle import same_bits

pytestmark = pytest.mark.gpu

_references = {}


def reference(images, variance, scales):
    """``get_detect_wavelets`` of one blend, computed once per blend and ``scales``"""
    from scarlet_amd import detect

    key = (id(images), id(variance), scales)
    if key not in _references:  # (the arrays are kept, so that their ids stay theirs)
        _references[key] = (images, variance,
                            detect.get_detect_wavelets(images, variance, scales=scales))
        _references[key][2].setflags(write=False)
    return _references[key][2]


def host(result):
    return result.cpu().numpy() if hasattr(result, "cpu") else result


def assert_equal_per_blend(got, images, variance, scales):
    assert len(got) == len(images)
    for k, (g, im, var) in enumerate(zip(got, images, variance)):
        want = reference(im, var, scales)
        assert same_bits(host(g), want), (k, im.shape, im.dtype, scales)


# ---------------------------------------------------------------------------
# 1. the whole catalogue, float32 and float64 blends mixed in one call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scales", [3, 5])
def test_mixed_catalogue_equals_per_blend_calls_and_oracle(scales, device):
    from scarlet_amd import detect, wavelet

    images, variance = dc.catalogue(dc.MIXED)
    got = detect.get_detect_wavelets_batch(images, variance, scales=scales, device=device)
    if device:
        import torch

        assert all(isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64
                   for g in got)
        # views into the buffer of their dtype group
        for dtype in (np.float32, np.float64):
            ptrs = {g.untyped_storage().data_ptr() for g, dt in zip(got, dc.MIXED) if dt == dtype}
            assert len(ptrs) == 1
    else:
        assert all(isinstance(g, np.ndarray) for g in got)
    for k, (g, im, var) in enumerate(zip(got, images, variance)):  # in input order
        planes = wavelet.get_scales(im.shape, scales) + 1
        assert tuple(g.shape) == (planes,) + im.shape[1:], k
        g = host(g)
        assert g.dtype == np.float64
        assert same_bits(g, reference(im, var, scales)), (k, im.shape, im.dtype)
        w, _, M, _, margin = dc.oracle_chain(im, var, scales)
        assert margin == (True, True), k
        assert same_bits(g, M * w), (k, im.shape, im.dtype)
    if scales == 5:
        assert [len(g) for g in got] == dc.PLANES_5
        assert (host(got[-1]) != 0).any() and (host(got[-1]) == 0).any()


# ---------------------------------------------------------------------------
# 2. options the detection step fixes, through the plumbing function
# ---------------------------------------------------------------------------
OPTIONS = [(3, 0.1, 20), (3, 0.02, 6), (5, 0.0, 4), (3, 0.1, 1)]


def per_blend_support(images, sigma, scales, K, epsilon, max_iter, generation):
    """coadd -> transform -> support of one blend through the per-blend device functions"""
    from scarlet_amd import wavelet

    coadd = wavelet.coadd_device(wavelet._upload(images))
    d_coeffs = wavelet.transform_device(coadd[None], scales, generation)
    s0, t0 = wavelet.initial_sigma(images.dtype.type, scales + 1, sigma, K)
    M, Mw, iters = wavelet.support_device(d_coeffs, s0[None], t0[None], K, epsilon, max_iter)
    return M[:, 0].cpu().numpy(), Mw[:, 0].cpu().numpy(), int(iters[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("generation", [1, 2])
@pytest.mark.parametrize("K,epsilon,max_iter", OPTIONS, ids=["K%g-eps%g-it%d" % o for o in OPTIONS])
def test_plumbing_equals_support_device_per_blend(K, epsilon, max_iter, generation, dtype):
    from scarlet_amd import detect, wavelet

    images, variance = dc.catalogue(dtype)
    images = [images[k] for k in dc.SMALLEST]
    variance = [variance[k] for k in dc.SMALLEST]
    oracle = [dc.oracle_chain(im, var, 5, K, epsilon, max_iter, generation)
              for im, var in zip(images, variance)]
    counts = [o[3] for o in oracle]
    print("oracle iterations", counts)
    if (K, epsilon, max_iter) == (3, 0.02, 6):  # some blends stop early, others reach max_iter
        assert min(counts) < 6 and max(counts) == 6 and counts.count(6) < len(counts)
    if epsilon == 0.0:
        # never converged: max_iter, except where no sigma_j is left to compare -- the single
        # plane of the 2 x 2 blend is all significant, its sigma_0 is 0
        assert counts == [1] + [max_iter] * 4 and oracle[0][2].all()
    sigmas = detect._batch_sigmas(variance)
    scales = [wavelet.get_scales(im.shape, 5) for im in images]
    first = [wavelet.initial_sigma(dtype, 1, sigma, K) for sigma in sigmas]
    table = wavelet.detect_task_table([im.shape for im in images], scales,
                                      [s0[0] for s0, _ in first], [t0[0] for _, t0 in first])
    masked, M, iters = wavelet.detect_wavelets_batch_device(
        detect._batch_upload(images), table, K, epsilon, max_iter, generation, support=True)
    import torch

    assert M.dtype == torch.int32 and iters.dtype == torch.int32 and masked.is_cuda
    iters = iters.cpu().numpy().tolist()
    masked = detect._batch_views(masked.cpu().numpy(), table)
    M = detect._batch_views(M.cpu().numpy(), table)
    for k, (im, sigma, s) in enumerate(zip(images, sigmas, scales)):
        M_one, Mw_one, it_one = per_blend_support(im, sigma, s, K, epsilon, max_iter, generation)
        assert iters[k] == it_one, (k, iters, it_one)
        assert M[k].dtype == np.int32 and np.array_equal(M[k], M_one), k
        assert set(np.unique(M[k])) <= {0, 1}
        assert same_bits(masked[k], Mw_one), k
        if oracle[k][4] == (True, True):
            assert iters[k] == counts[k], (k, iters, counts)
            assert np.array_equal(M[k], oracle[k][2]) and same_bits(masked[k],
                                                                  oracle[k][2] * oracle[k][0])
    if epsilon == 0.0:
        assert iters[1:] == [max_iter] * 4


# ---------------------------------------------------------------------------
# 3. independence of the blends of one call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [3, 5])
def test_reversed_and_alone_give_the_same_bits(scales):
    from scarlet_amd import detect

    images, variance = dc.catalogue(dc.MIXED)
    got = detect.get_detect_wavelets_batch(images[::-1], variance[::-1], scales=scales)
    assert_equal_per_blend(got, images[::-1], variance[::-1], scales)
    for im, var in zip(images, variance):
        assert_equal_per_blend(detect.get_detect_wavelets_batch([im], [var], scales=scales),
                               [im], [var], scales)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_an_impulse_next_to_a_seam_stays_in_its_blend(dtype):
    """a unit impulse in the first pixel of a blend leaves the all-zero blend in front of it
    all zero, one in the last pixel the all-zero blend behind it; the variance is small
    enough for a leaked tap (at least 2^-24) to be significant"""
    from scarlet_amd import detect

    first = np.zeros((1, 17, 19), dtype)
    first[0, 0, 0] = 1.0
    last = np.zeros((2, 17, 19), dtype)
    last[1, -1, -1] = 1.0
    images = [np.zeros((2, 9, 11), dtype), first, last, np.zeros((1, 12, 7), dtype)]
    variance = [np.full(im.shape, 1e-20, dtype) for im in images]
    for device in (False, True):
        got = [host(g) for g in detect.get_detect_wavelets_batch(images, variance, scales=5,
                                                                 device=device)]
        for k in (0, 3):
            assert not got[k].any() and not np.signbit(got[k]).any(), k
        for k in (1, 2):
            want = detect.get_detect_wavelets(images[k], variance[k], scales=5)
            assert same_bits(got[k], want) and (want != 0).sum() > 100, k


# ---------------------------------------------------------------------------
# 4. degenerate blends beside ordinary ones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_degenerate_blends_in_one_call(dtype):
    from scarlet_amd import detect

    plain, plain_var = dc.blend((45, 70), 5, dtype)
    small, small_var = dc.blend((17, 19), 1, dtype)
    holed = plain.copy()
    holed[2, 7, 9] = np.nan
    cases = {
        "ordinary": (small, small_var),
        "zero": (np.zeros_like(plain), plain_var),
        "nan": (holed, plain_var),
        "all significant": (plain, np.full(plain.shape, 1e-30, dtype)),
        "nothing significant": (plain, np.full(plain.shape, 1e30, dtype)),
        "ordinary too": (plain, plain_var),
    }
    images = [c[0] for c in cases.values()]
    variance = [c[1] for c in cases.values()]
    got = dict(zip(cases, detect.get_detect_wavelets_batch(images, variance, scales=5)))
    for name, (im, var) in cases.items():
        want = detect.get_detect_wavelets(im, var, scales=5)
        assert same_bits(got[name], want), name
    assert not got["zero"].any() and not np.signbit(got["zero"]).any()
    assert np.isnan(got["nan"]).any() and np.isfinite(got["nan"]).any()
    assert got["all significant"].all()
    # the supports' own numbers, through the plumbing: every sigma_j of the zero image is 0
    # (one iteration), and so is the all-significant one's; where nothing is significant at
    # first, the second iteration's sigma_j is the plane's own and the loop goes on from it
    from scarlet_amd import wavelet

    table = detect._batch_table(images, detect._batch_sigmas(variance), 5)
    _, _, iters = wavelet.detect_wavelets_batch_device(detect._batch_upload(images), table)
    iters = iters.cpu().numpy().tolist()
    _, _, _, huge_count, margin = dc.oracle_chain(images[4], variance[4], 5)
    assert margin == (True, True) and huge_count >= 2
    assert iters[1] == 1 and iters[3] == 1 and iters[4] == huge_count
    assert iters[5] == dc.ITERATIONS_5[4]


# ---------------------------------------------------------------------------
# 5. the route: no per-blend call, one entry-point call per dtype group
# ---------------------------------------------------------------------------
def test_catalogue_takes_one_device_call_per_dtype_group(monkeypatch):
    from scarlet_amd import _lib, detect

    images, variance = dc.catalogue(dc.MIXED)
    for im, var in zip(images, variance):
        reference(im, var, 5)  # (before the per-blend function is taken away)
    lib = _lib.load()
    calls = []

    def counted(name):
        fn = getattr(lib, name)

        def call(*args):
            calls.append((name, args[0]))
            return fn(*args)
        return call

    def refuse(*a, **k):
        raise AssertionError("the batch went through get_detect_wavelets")

    for name in ("smi_detect_wavelets_f32", "smi_detect_wavelets_f64"):
        monkeypatch.setattr(lib, name, counted(name))
    monkeypatch.setattr(detect, "get_detect_wavelets", refuse)
    got = detect.get_detect_wavelets_batch(images, variance, scales=5)
    groups, fallback = detect.plan_detect_wavelets_batch(images, variance, scales=5)
    assert not fallback and len(groups) == 2
    assert sorted(calls) == [("smi_detect_wavelets_f32", 5), ("smi_detect_wavelets_f64", 4)]
    assert_equal_per_blend(got, images, variance, 5)


# ---------------------------------------------------------------------------
# 6. lite.init_blends computes its coefficients with the batch
# ---------------------------------------------------------------------------
def test_init_blends_without_the_per_blend_function(monkeypatch):
    from scarlet_amd import detect, lite
    from scarlet_amd.lite import initialization

    cases = [ic.make_case(name) for name in ic.MIXED] + [ic.make_blob(name) for name in ic.BLOBS]
    observations = [c.obs for c in cases]
    centers = [c.centers for c in cases]
    groups, fallback = lite.plan_init_blends(observations, centers, scales=5)
    assert not fallback and len(groups) >= 2
    wavelets = [detect.get_detect_wavelets(o.images, o.variance, scales=5) for o in observations]
    want = lite.init_blends(observations, centers, scales=5, wavelets=wavelets,
                            **ic.MIXED_OPTIONS)

    def refuse(*a, **k):
        raise AssertionError("init_blends went through get_detect_wavelets")

    monkeypatch.setattr(initialization, "get_detect_wavelets", refuse)
    got = lite.init_blends(observations, centers, scales=5, wavelets=None, **ic.MIXED_OPTIONS)
    assert sum(len(s) for s in got) == sum(len(c) for c in centers) > 0
    assert sum(len(s.components) for ss in got for s in ss if s is not None) > len(cases)
    for a, b in zip(got, want):  # every spectrum too: both came from the same device fits
        ic.assert_matches_loop(a, b, joint=[False] * len(a))
