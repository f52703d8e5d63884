"""The fused convolution's mirror-block exchange (fused_conv.hip, blocks_forward /
blocks_inverse): the lanes l and l ^ 32 of a radix-16 pass hand each other the values of a
block and its mirror block through v_permlane32_swap.

Only wavefronts of kind 0 exchange; block 0 and block FX1 / 2 (kinds 1, 2) have no partner, and
the lanes without a work item of their own -- pairs beyond the last one in the last group of
32, the pad slot of an odd FX1 -- sit next to them and repeat a neighbour's item.  The shapes
are the smallest in which all of that occurs:

  * every x-length 64, 80, 96, 128, 160 (FX1 = 4, 5, 6, 8, 10: odd and even, with and without a
    middle block), in the 512-thread build and, where the launcher picks it, the 1024-thread one;
  * 19, 35, 49 and 64 row pairs: below and above 32, a multiple of 32 and not, an odd height;
  * 66 row pairs under 160 x 80 and 160 x 96: three groups of 32 pairs where a 512-thread workgroup
    takes two per trip, i.e. a second trip whose only group has two pairs of its own (the four
    frames up to 128 rows never need a second trip, so these two come on top).

One blend, two bands, two small components (one overhangs the frame), a kernel per band.
Tolerances: those of tests/test_gpu_parity.py for the same quantities.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # test_gpu_parity.RTOL

# H, W, kernel size, fft_shape given to BlendBatch (None: its own choice), the shape it must report
CASES = [
    (37, 50, 15, None, (64, 64)),
    (37, 50, 41, None, (64, 80)),
    (37, 50, 15, (64, 160), (64, 160)),
    (70, 48, 15, None, (80, 64)),
    (70, 48, 15, (80, 96), (80, 96)),
    (70, 48, 15, (80, 160), (80, 160)),      # 1024 threads
    (97, 100, 15, None, (128, 128)),
    (97, 100, 15, (128, 160), (128, 160)),   # 1024 threads
    (128, 128, 15, None, (160, 160)),        # 1024 threads, the benchmark's instance
    (131, 50, 15, (160, 80), (160, 80)),     # second trip, odd FX1
    (131, 50, 15, (160, 96), (160, 96)),     # second trip, even FX1
]
IDS = ["%dx%d-k%d-F%dx%d" % (c[0], c[1], c[2], c[4][0], c[4][1]) for c in CASES]
N_IT = 3


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd
    from scarlet_amd import _lib

    assert _lib.load().smi_device_count() >= 1
    return scarlet_amd


@functools.lru_cache(maxsize=None)
def scene(H, W, P):
    """(specs, kernel (2, P, P), data, weights) of the frame; computed once, never written to"""
    from oracle import pgm
    from scarlet_amd import fft
    from scarlet_amd.psf import GaussianPSF

    C = 2
    rng = np.random.default_rng(1000 * H + W + P)
    specs = []
    for (h, w), (oy, ox) in (((15, 15), (H // 2 - 4, W // 2 - 9)), ((11, 17), (H - 8, 3))):
        yy, xx = np.mgrid[:h, :w]
        morph = np.exp(-0.5 * (((yy - h // 2) / (0.2 * h)) ** 2 + ((xx - w // 2) / (0.25 * w)) ** 2))
        morph = (morph * rng.uniform(0.7, 1.3, morph.shape)).astype(np.float32)
        specs.append((rng.uniform(0.5, 3, C).astype(np.float32), morph / morph.max(), (oy, ox)))
    obs = np.concatenate([GaussianPSF(s, boxsize=P).get_model() for s in (1.5, 2.1)]).astype(np.float32)
    mod = GaussianPSF(0.8).get_model().astype(np.float32)
    kernel = fft.match_psf(fft.Fourier(obs), fft.Fourier(mod), padding=10).image.astype(np.float32)
    assert kernel.shape == (C, P, P)
    truth = pgm.Scene((C, H, W), None, None, kernel,
                      [pgm.Component(s.copy(), m.copy(), o) for s, m, o in specs])
    data = (truth.render(truth.get_model()) + rng.normal(0, 0.05, (C, H, W))).astype(np.float32)
    weights = rng.uniform(200.0, 600.0, (C, H, W)).astype(np.float32)
    for a in (kernel, data, weights):
        a.setflags(write=False)
    return specs, kernel, data, weights


def oracle_scene(H, W, P):
    """a fresh oracle scene at the start values of the fit (seds 20 % low)"""
    from oracle import pgm

    specs, kernel, data, weights = scene(H, W, P)
    return pgm.Scene(data.shape, data, weights, kernel,
                     [pgm.Component((s * 0.8).astype(np.float32), m.copy(), o, sed_min_step=0.05)
                      for s, m, o in specs])


def batch_of(amd, H, W, P, **kw):
    specs, kernel, data, weights = scene(H, W, P)
    comps = [amd.ComponentSpec(s * 0.8, m, o, sed_min_step=0.05) for s, m, o in specs]
    return amd.BlendBatch(data[None], weights[None], [comps], kernel=kernel, max_iter=N_IT + 1, **kw)


@functools.lru_cache(maxsize=None)
def float64_forward(H, W, P):
    """model, rendered (float64 FFT convolution) and chi^2 / 2 at the start values"""
    from oracle import fftconv

    _, kernel, data, weights = scene(H, W, P)
    model = oracle_scene(H, W, P).get_model()
    rendered = fftconv.convolve(model.astype(np.float64), kernel.astype(np.float64), axes=(1, 2))
    assert rendered.dtype == np.float64
    half_chi2 = np.sum(weights.astype(np.float64) * (rendered - data) ** 2) / 2
    return model, rendered, half_chi2


@functools.lru_cache(maxsize=None)
def oracle_fit(H, W, P):
    sc = oracle_scene(H, W, P)
    for it in range(N_IT):
        sc.step(it, 1e-3)
    return sc


_rocfft = {}


def rocfft_gradient(amd, H, W, P):
    """the same batch through the rocFFT pipeline (one per frame, shared by its FFT shapes)"""
    if (H, W, P) not in _rocfft:
        b = batch_of(amd, H, W, P, conv_path="rocfft")
        g_sed, g_morph = b.gradient()
        b.close()
        _rocfft[H, W, P] = g_sed, np.concatenate([g.ravel() for g in g_morph])
    return _rocfft[H, W, P]


@pytest.mark.parametrize("H,W,P,fft_shape,F", CASES, ids=IDS)
def test_forward_against_float64(amd, H, W, P, fft_shape, F):
    batch = batch_of(amd, H, W, P, conv_path="fused", fft_shape=fft_shape)
    assert tuple(batch.fft_shape) == F
    model, rendered, logL = batch.forward()
    ref_model, ref_rendered, ref_half_chi2 = float64_forward(H, W, P)
    err_model, err_rendered = rel_err(model[0], ref_model), rel_err(rendered[0], ref_rendered)
    half_chi2 = -(logL[0] + oracle_scene(H, W, P).log_norm)
    print("model %.3g rendered %.3g chi2 %.3g" % (err_model, err_rendered,
                                                  abs(half_chi2 - ref_half_chi2) / ref_half_chi2))
    assert err_model < RTOL
    assert err_rendered < RTOL
    assert abs(half_chi2 - ref_half_chi2) < RTOL * abs(ref_half_chi2)


@pytest.mark.parametrize("H,W,P,fft_shape,F", CASES, ids=IDS)
def test_gradient_against_rocfft(amd, H, W, P, fft_shape, F):
    batch = batch_of(amd, H, W, P, conv_path="fused", fft_shape=fft_shape)
    assert tuple(batch.fft_shape) == F
    g_sed, g_morph = batch.gradient()
    got = g_sed, np.concatenate([g.ravel() for g in g_morph])
    for a, f in zip(rocfft_gradient(amd, H, W, P), got):
        assert np.abs(a).max() > 0
        print("gradient %.3g" % (np.abs(a - f).max() / max(np.abs(a).max(), 1e-3)))
        assert np.abs(a - f).max() < 1e-4 * max(np.abs(a).max(), 1e-3)


@pytest.mark.parametrize("H,W,P,fft_shape,F", CASES, ids=IDS)
def test_three_iterations_against_the_oracle(amd, H, W, P, fft_shape, F):
    batch = batch_of(amd, H, W, P, conv_path="fused", fft_shape=fft_shape)
    assert tuple(batch.fft_shape) == F
    batch.step(0, N_IT, e_rel=1e-3)
    sed, morphs = batch.parameters()
    sc = oracle_fit(H, W, P)
    chi = np.asarray(batch.loss_history()[0], dtype=np.float64) - sc.log_norm
    ref = np.asarray(sc.loss, dtype=np.float64) - sc.log_norm
    assert chi.shape == ref.shape == (N_IT,)
    print("loss", np.abs(chi - ref) / np.abs(ref))
    assert np.all(np.abs(chi - ref) <= 3e-5 * np.abs(ref)), (chi, ref)
    for k, c in enumerate(sc.components):
        assert rel_err(sed[k], c.sed) < 2e-4, k
        assert np.abs(morphs[k] - c.morph).max() < 2e-4, k
