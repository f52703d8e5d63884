"""ResolutionRenderer between rotated pixel grids, the part that needs no GPU: the renderer's
set-up against the reference's (tests/golden/resolution_rotated.npz, made by
tools/make_golden_resolution_rot.py), the float64 restatement (resolution_rot_oracle.py) against
the reference's rendering, its Fourier-space form -- what the device evaluates -- against the
restatement, with and without the edge-column projection, the adjoint identity, the refusals,
and where ``plan_fit_blends`` puts such blends."""

import functools

import numpy as np
import pytest

import multires_batch_cases as mc
import resolution_rot_cases as cases
from conftest import golden
from oracle import resample
from resolution_rot_oracle import RotatedLowResObservation

TOL = 2e-5  # the project's bound for these products on the device (tests/test_gpu_resample.py)


@functools.lru_cache(maxsize=None)
def scene(name, angle=None):
    return cases.scene(name, angle)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The restatement built from the REFERENCE's set-up quantities."""
    g = golden("resolution_rotated")
    case = cases.CASES[name]
    frame = case["frame"]
    idx = list(range(1, 1 + case["bands"]))  # the frame's channels: "hr", then the LR bands
    _, _, im_lr, _ = cases.arrays(name)
    return RotatedLowResObservation(
        g[name + "_kernel"], g[name + "_shifts"], g[name + "_other_shifts"], float(g[name + "_h"]),
        idx, frame[1:], im_lr, np.full(im_lr.shape, 400.0))


def padded_model(name):
    o = oracle(name)
    return o._pad(golden("resolution_rotated")[name + "_model"].astype(np.float64)[o.channels])


def test_the_cases_cover_what_the_kernels_can_get_wrong():
    g = golden("resolution_rotated")
    assert sorted(cases.CASES) == [str(n) for n in g["cases"]]
    C = cases.CASES
    angles = [c["angle"] for c in C.values()]
    assert any(0.2 <= a <= 0.7 for a in angles) and any(-0.7 <= a <= -0.2 for a in angles)
    assert any(a == 1e-6 for a in angles) and np.sin(1e-6) ** 2 > np.finfo(float).eps
    assert any(c["fft"][0] != c["fft"][1] for c in C.values())
    assert any(c["fft"][0] % 2 == 1 or c["fft"][1] % 2 == 1 for c in C.values())
    assert any(c["fft"][1] // 2 + 1 > 64 for c in C.values())
    assert any(c["side"] < 16 for c in C.values())
    assert {1, 3} <= {c["bands"] for c in C.values()}
    assert all(c["bands"] < c["frame"][0] for c in C.values())  # a strict subset of the channels
    assert any(c["offset"] != (0.0, 0.0) for c in C.values())
    for name, case in C.items():
        assert tuple(g[name + "_frame_shape"]) == case["frame"], name
        assert tuple(g[name + "_fft_shape"]) == case["fft"], name
        # power at both Nyquist frequencies
        spectrum = np.abs(np.fft.rfftn(padded_model(name), axes=(-2, -1)))
        Fy, Fx = case["fft"]
        if Fy % 2 == 0:
            assert spectrum[:, Fy // 2].max() > 1e-3 * spectrum.max(), name
        if Fx % 2 == 0:
            assert spectrum[:, :, Fx // 2].max() > 1e-3 * spectrum.max(), name


def rotated_plan(n_a, n_b, Fy, Fx):
    import ctypes

    from scarlet_amd import _lib

    plan = (ctypes.c_int32 * 7)()
    _lib.check(_lib.load().smi_resampler_rotated_plan(n_a, n_b, Fy, Fx, plan))
    return dict(zip(("ti", "tj", "tiles_a", "tiles_b", "kslice", "n_slices", "b_chunks"), plan))


def test_the_cases_reach_every_path_of_the_launch_plan():
    """What the device launches follows the shapes alone (smi_resampler_rotated_plan, no GPU):
    the scenes all take the 16 x 16 tile, so the resampler-level cases bring the other tile
    sizes along a and along b, several tiles each way, several 64-column chunks of the transpose
    and slices of more than 64 terms."""
    plans = {}
    for name, case in cases.CASES.items():
        Fy, Fx = case["fft"]
        plans[name] = rotated_plan(case["side"], case["side"], Fy, Fx)
        assert (plans[name]["ti"], plans[name]["tj"]) == (1, 1), name
    for name, case in cases.KERNEL_CASES.items():
        plans[name] = rotated_plan(case["n_a"], case["n_b"], case["Fy"], case["Fx"])
    assert {p["ti"] for p in plans.values()} == {1, 2, 3, 4}
    assert {p["tj"] for p in plans.values()} == {1, 2, 3, 4}
    assert any(p["ti"] != p["tj"] for p in plans.values())
    assert (plans["three"]["ti"], plans["three"]["tj"]) == (3, 3)  # the tutorial's 36 x 36 variant
    assert rotated_plan(36, 36, 120, 120)["ti"] == 3
    assert max(p["tiles_a"] for p in plans.values()) > 1
    assert max(p["tiles_b"] for p in plans.values()) > 2
    assert max(p["b_chunks"] for p in plans.values()) > 2
    assert any(p["n_slices"] > 1 for p in plans.values())
    assert plans["long"]["kslice"] == 96 and plans["long"]["n_slices"] == 175  # 130 x 129 terms
    assert all(p["kslice"] == 64 for n, p in plans.items() if n != "long")
    # sides that are no multiple of 16, and of the tile
    assert any(c["n_a"] % 16 and c["n_b"] % 16 for c in cases.KERNEL_CASES.values())
    # the tutorial's size: 115 slices of 64 terms per band
    assert rotated_plan(36, 36, 120, 120) == dict(ti=3, tj=3, tiles_a=1, tiles_b=1, kslice=64,
                                                  n_slices=115, b_chunks=1)


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_restatement_of_the_resampler_level_cases(name):
    """n_a != n_b: the restatement's Fourier form and its adjoint hold there too."""
    kernel, h, shifts, other, model, resid = cases.kernel_case(name)
    C, Fy, Fx = kernel.shape
    o = RotatedLowResObservation(kernel, shifts, other, h, range(C), (Fy, Fx), np.zeros(1),
                                 np.ones(1))
    out = o.render_padded(model)
    assert out.shape == resid.shape
    assert np.abs(o.render_fourier(model) - out).max() < 1e-12 * np.abs(out).max()
    lhs = np.sum(out * resid)
    assert abs(lhs - np.sum(model * o.adjoint_padded(resid))) < 1e-12 * np.abs(out * resid).sum()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_set_up_matches_the_reference(name):
    """(a) angle, h, FFT shape; the shift tables to 1e-8 pixel (LinearWCS against astropy's TAN
    with a common crval); the difference kernel at the bound of tests/test_oracle_golden.py."""
    g = golden("resolution_rotated")
    frame, obs_hr, obs_lr = scene(name)
    r = obs_lr.renderer
    assert type(r).__name__ == "ResolutionRenderer" and r.isrot
    assert type(obs_hr.renderer).__name__ == "ConvolutionRenderer"
    assert tuple(frame.shape) == tuple(g[name + "_frame_shape"])
    np.testing.assert_allclose(frame.wcs.wcs.crpix, g[name + "_frame_crpix"], atol=1e-12)
    assert tuple(r._fft_shape) == tuple(g[name + "_fft_shape"])
    np.testing.assert_allclose([float(r.angle[0]), float(r.angle[1])], g[name + "_angle"],
                               rtol=0, atol=1e-14)
    assert abs(r.h - float(g[name + "_h"])) < 1e-13
    assert r.shifts.shape == g[name + "_shifts"].shape == (2, cases.CASES[name]["side"])
    assert np.abs(r.shifts - g[name + "_shifts"]).max() < 1e-8
    assert np.abs(r.other_shifts - g[name + "_other_shifts"]).max() < 1e-8
    np.testing.assert_allclose(r.diff_kernel.image, g[name + "_kernel"], rtol=0, atol=1e-7)
    # what the device is handed
    kernel, scale, shifts, other, fft_shape = r._operators()
    assert kernel.dtype == np.float32 and kernel.shape == (cases.CASES[name]["bands"],) + fft_shape
    assert scale == r.h ** 2 and shifts.dtype == other.dtype == np.float64
    assert r.shape_class() == (kernel.shape[0], shifts.shape[1], other.shape[1]) + fft_shape
    assert not r.on_spectral_path() and not hasattr(r, "_resconv_op")
    C, n_a, _, Fy, Fx = r.shape_class()
    assert r.operator_bytes() == C * n_a * Fy * (Fx // 2 + 1) * 8
    assert r.channel_map == slice(1, 1 + C)  # a strict subset of the frame's channels


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_matches_the_reference_rendering(name):
    """(b) within float32 rounding of the peak, 5e-7.  Measured: odd 4.9e-8, skew 5.1e-8,
    tiny 5.7e-8, turn 4.6e-8, wide 4.1e-8."""
    g = golden("resolution_rotated")
    ref = g[name + "_rendered"]
    out = oracle(name).render(g[name + "_model"])
    dev = np.abs(out - ref).max() / np.abs(out).max()
    print("%s: restatement against the reference %.2e of the peak" % (name, dev))
    assert dev < 5e-7


def test_fourier_form_is_the_restatement_and_needs_the_projection():
    """(c) the Fourier-space evaluation, to 1e-12 of the peak; with pure phases on the
    self-conjugate columns it is another map, beyond the device bound on at least one case.
    Measured without the projection: turn 6.0e-6, skew 3.4e-5, odd 3.9e-5, wide 4.9e-5,
    tiny 5.8e-11."""
    without = {}
    for name in cases.CASES:
        o, pad = oracle(name), padded_model(name)
        out = o.render_padded(pad)
        peak = np.abs(out).max()
        assert np.abs(o.render_fourier(pad) - out).max() < 1e-12 * peak, name
        without[name] = np.abs(o.render_fourier(pad, project=False) - out).max() / peak
    print("without the projection:", {k: "%.1e" % v for k, v in without.items()})
    assert max(without.values()) > TOL


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_adjoint_identity(name):
    """(d) <R m, r> = <m, R^T r> to 1e-12: ``render`` shifts the model, ``adjoint`` goes through
    the dense operator built with the opposite shifts."""
    o = oracle(name)
    rng = np.random.RandomState(3)
    model = rng.normal(0, 1, cases.CASES[name]["frame"])
    out = o.render(model)
    upstream = rng.normal(0, 1, out.shape)
    lhs = np.sum(out * upstream)
    rhs = np.sum(model * o.adjoint(upstream, model.shape[0]))
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)
    # the padded pair as well (what the device's transpose is compared with)
    pad = rng.normal(0, 1, (o.C, o.Fy, o.Fx))
    lhs = np.sum(o.render_padded(pad) * upstream)
    assert abs(lhs - np.sum(pad * o.adjoint_padded(upstream))) < 1e-12 * abs(lhs)
    # a channel that is not observed gets no gradient
    assert not o.adjoint(upstream, model.shape[0])[0].any()


def test_refusals_and_unrotated_renderers_are_what_they_were():
    """(e)"""
    import scarlet_amd as scarlet

    # a rotated grid with an observation that is not square
    case = cases.CASES["turn"]
    obs_hr, _ = cases.observations("turn", scarlet, cases.linear_wcs)
    frame = scarlet.Frame.from_observations([obs_hr], model_psf=scarlet.GaussianPSF(sigma=0.8))
    data = np.zeros((1, 9, 7), np.float32)
    obs = scarlet.Observation(
        data, wcs=cases.linear_wcs(*cases.wcs_params((9, 7), cases.LR_SCALE, case["angle"]), (9, 7)),
        psf=scarlet.ImagePSF(cases.gaussian_psf(9, 1.3, 1)), channels=["hr"])
    with pytest.raises(NotImplementedError, match="needs a square observation.*9 x 7"):
        scarlet.ResolutionRenderer(obs, frame)
    # rows beyond the device's transform tables: refused at construction, with the number
    hr = (12, 2100)
    wide_hr = scarlet.Observation(
        np.zeros((1,) + hr, np.float32), wcs=cases.linear_wcs(*cases.wcs_params(hr, cases.HR_SCALE), hr),
        psf=scarlet.ImagePSF(cases.gaussian_psf(11, 1.6, 1)), channels=["hr"])
    wide = scarlet.Frame.from_observations([wide_hr], model_psf=scarlet.GaussianPSF(sigma=0.8))
    square = scarlet.Observation(
        np.zeros((1, 5, 5), np.float32),
        wcs=cases.linear_wcs(*cases.wcs_params((5, 5), cases.LR_SCALE, 0.3), (5, 5)),
        psf=scarlet.ImagePSF(cases.gaussian_psf(9, 1.3, 1)), channels=["hr"])
    assert scarlet.ResolutionRenderer.MAX_ROW == 2048
    with pytest.raises(NotImplementedError, match=r"rows of up to 2048 pixels.*has 2\d\d\d"):
        scarlet.ResolutionRenderer(square, wide)
    # an unrotated renderer: class, bytes, path and operators as before
    blend = mc.make_blend("first", 100)
    r = blend.observations[1].renderer
    assert not r.isrot and r.on_spectral_path()
    assert r.shape_class() == (2, 11, 11, 54, 60)
    assert r.operator_bytes() == 2 * 11 * 54 * 31 * 8
    A, Pt, fft_shape = r._operators()
    assert A.shape == (2, 11, 54 * 60) and Pt.shape == (60, 60 * 11) and fft_shape == (54, 60)
    assert A.dtype == Pt.dtype == np.float32
    # the unrotated refusal of interpolate_observation and the non-square one stay
    with pytest.raises(ValueError):
        scarlet.ResolutionRenderer(
            scarlet.Observation(
                data, wcs=cases.linear_wcs(*cases.wcs_params((9, 7), cases.LR_SCALE), (9, 7)),
                psf=scarlet.ImagePSF(cases.gaussian_psf(9, 1.3, 1)), channels=["hr"]), frame)


def test_tiny_angle_is_continuous_with_the_unrotated_branch():
    """(f) the restatement at 1e-6 rad against oracle.resample.LowResObservation for the same
    scene at angle 0: under a tenth of the device bound, which the GPU continuity test needs.
    Measured 1.3e-6 of the peak."""
    g = golden("resolution_rotated")
    model = g["tiny_model"]
    out = oracle("tiny").render(model)
    frame0, _, obs0 = scene("tiny", 0.0)
    r0 = obs0.renderer
    assert not r0.isrot and tuple(frame0.shape) == cases.CASES["tiny"]["frame"]
    assert tuple(r0._fft_shape) == cases.CASES["tiny"]["fft"]
    flat = resample.LowResObservation(r0.diff_kernel.image, r0.shifts[0], r0.other_shifts[1], r0.h,
                                      oracle("tiny").channels, frame0.shape[1:], obs0.data,
                                      obs0.weights)
    dev = np.abs(flat.render(model) - out).max() / np.abs(out).max()
    print("1e-6 rad against 0: %.2e of the peak" % dev)
    assert dev < TOL / 10


def test_plan_fit_blends_fits_a_rotated_blend_by_itself():
    """(g) unrotated two-resolution blends keep their groups and keys, the rotated one gets the
    new reason."""
    from scarlet_amd.fitting import plan_fit_blends

    before, alone = plan_fit_blends(mc.LISTS["first"](), 25, e_rel=1e-4)
    assert alone == {}
    blends = mc.first_five()
    blends.insert(2, cases.make_blend("turn"))
    groups, alone = plan_fit_blends(blends, 25, e_rel=1e-4)
    assert alone == {2: "a low-resolution observation on a rotated grid"}
    assert [idx for _, idx in groups] == [[0, 1, 3, 4, 5]]
    assert [key for key, _ in groups] == [key for key, _ in before]
