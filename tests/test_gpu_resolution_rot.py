"""ResolutionRenderer between rotated pixel grids on the device (scarlet_amd/csrc/resample_rot.hip,
path 2 of a resampler): rendering and transpose of every case of resolution_rot_cases.py against
the float64 restatement (resolution_rot_oracle.py, built from the reference's set-up quantities)
with NaN-filled outputs between guard bands; the adjoint identity; continuity with the
unrotated spectral path at 1e-6 rad; the facade against the reference's rendering; the term in a
device batch against the oracle's loss, gradients and trajectory; ``Blend.fit`` and
``fit_blends``."""

import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose

import multires_batch_cases as mc
import resolution_rot_cases as cases
from conftest import golden
from resolution_rot_oracle import RotatedLowResObservation, build_scene
from scarlet_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 2e-5   # of the float64 peak: the bound of tests/test_gpu_resample.py
RTOL = 1e-5  # gradients, as in tests/test_gpu_facade.py
F, D = ctypes.c_float, ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@functools.lru_cache(maxsize=None)
def oracle(name):
    g = golden("resolution_rotated")
    case = cases.CASES[name]
    idx = list(range(1, 1 + case["bands"]))
    _, _, im_lr, _ = cases.arrays(name)
    return RotatedLowResObservation(
        g[name + "_kernel"], g[name + "_shifts"], g[name + "_other_shifts"], float(g[name + "_h"]),
        idx, case["frame"][1:], im_lr, np.full(im_lr.shape, 400.0))


class Rotated:
    """A rotated resampler made from the REFERENCE's set-up quantities (the golden)."""

    def __init__(self, lib, name, operators=None):
        if operators is None:
            g = golden("resolution_rotated")
            operators = (g[name + "_kernel"], float(g[name + "_h"]), g[name + "_shifts"],
                         g[name + "_other_shifts"])
        kernel = np.ascontiguousarray(operators[0], np.float32)
        shifts = np.ascontiguousarray(operators[2], np.float64)
        other = np.ascontiguousarray(operators[3], np.float64)
        C, Fy, Fx = kernel.shape
        self.lib, self.shape = lib, (C, Fy, Fx, shifts.shape[1], other.shape[1])
        self.handle = ctypes.c_void_p()
        _lib.check(lib.smi_resampler_create_rotated(
            _lib.ptr(kernel, F), float(operators[1]) ** 2, _lib.ptr(shifts, D),
            _lib.ptr(other, D), C, shifts.shape[1], other.shape[1], Fy, Fx,
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

    def guarded(self, model, resid):
        """(out, gpad) through smi_resampler_rotated_test: NaN fill and guard bands."""
        C, Fy, Fx, n_a, n_b = self.shape
        model = np.ascontiguousarray(model, np.float32)
        resid = np.ascontiguousarray(resid, np.float32)
        out = np.zeros((C, n_a, n_b), np.float32)
        gpad = np.zeros((C, Fy, Fx), np.float32)
        ok = ctypes.c_int32(-1)
        _lib.check(self.lib.smi_resampler_rotated_test(
            self.handle, _lib.ptr(model, F), _lib.ptr(resid, F), _lib.ptr(out, F),
            _lib.ptr(gpad, F), ctypes.byref(ok)))
        assert ok.value == 1, "written outside an output or a work array"
        assert not np.isnan(out).any(), "%d outputs never written" % np.isnan(out).sum()
        assert not np.isnan(gpad).any(), "%d gradient pixels never written" % np.isnan(gpad).sum()
        return out, gpad


def padded_model(name):
    o = oracle(name)
    model = golden("resolution_rotated")[name + "_model"]
    return o._pad(model.astype(np.float64)[o.channels]).astype(np.float32)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_render_and_transpose_match_the_restatement(lib, name):
    o = oracle(name)
    pad = padded_model(name)
    rng = np.random.RandomState(7)
    with Rotated(lib, name) as r:
        assert r.path == 2
        # a rotated resampler has no other path
        assert lib.smi_resampler_set_path(r.handle, 0) != 0
        assert lib.smi_resampler_set_path(r.handle, 1) != 0
        _lib.check(lib.smi_resampler_set_path(r.handle, 2))
        C, Fy, Fx, n_a, n_b = r.shape
        resid = rng.normal(0, 1, (C, n_a, n_b)).astype(np.float32)
        out, gpad = r.guarded(pad, resid)
        ref = o.render_padded(pad.astype(np.float64))
        dev = np.abs(out - ref).max() / np.abs(ref).max()
        ref_g = o.adjoint_padded(resid.astype(np.float64))
        dev_g = np.abs(gpad - ref_g).max() / np.abs(ref_g).max()
        print("%s: rendering %.2e, transpose %.2e of the peak" % (name, dev, dev_g))
        assert dev < TOL
        assert dev_g < TOL
        # the rendering interface gives those bits, every time
        first = r.render(pad)
        assert np.array_equal(first, out)
        assert np.array_equal(r.render(pad), first)
        assert np.array_equal(r.adjoint(resid), gpad)
        # <R m, r> = <m, R^T r> on the device
        lhs = np.sum(out.astype(np.float64) * resid)
        rhs = np.sum(pad.astype(np.float64) * gpad)
        assert abs(lhs - rhs) < 1e-5 * abs(lhs)
        # an impulse response is not translation invariant here: a second model
        other = rng.normal(0, 1, pad.shape).astype(np.float32)
        ref2 = o.render_padded(other.astype(np.float64))
        assert np.abs(r.render(other) - ref2).max() < TOL * np.abs(ref2).max()


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_every_tile_variant_chunk_and_slicing_matches_the_restatement(lib, name):
    """The resampler-level cases (resolution_rot_cases.KERNEL_CASES): contraction tiles of 32, 48
    and 64 outputs a side, several tiles along a and b, three 64-column chunks of the transpose,
    slices of 96 terms -- test_resolution_rot_host.py asserts that the launch plan of these
    shapes is that.  The guarded call runs twice, the second time on work arrays that the first
    has used: they are refilled with NaNs, so an element that is never written shows either
    time."""
    kernel, h, shifts, other, model, resid = cases.kernel_case(name)
    C, Fy, Fx = kernel.shape
    o = RotatedLowResObservation(kernel, shifts, other, h, range(C), (Fy, Fx), np.zeros(1),
                                 np.ones(1))
    ref = o.render_padded(model.astype(np.float64))
    ref_g = o.adjoint_padded(resid.astype(np.float64))
    with Rotated(lib, name, (kernel, h, shifts, other)) as r:
        assert r.path == 2
        out, gpad = r.guarded(model, resid)
        dev = np.abs(out - ref).max() / np.abs(ref).max()
        dev_g = np.abs(gpad - ref_g).max() / np.abs(ref_g).max()
        print("%s: rendering %.2e, transpose %.2e of the peak" % (name, dev, dev_g))
        assert dev < TOL
        assert dev_g < TOL
        again = r.guarded(model, resid)
        assert np.array_equal(again[0], out) and np.array_equal(again[1], gpad)
        assert np.array_equal(r.render(model), out) and np.array_equal(r.adjoint(resid), gpad)
        lhs = np.sum(out.astype(np.float64) * resid)
        rhs = np.sum(model.astype(np.float64) * gpad)
        assert abs(lhs - rhs) < 1e-5 * np.abs(out.astype(np.float64) * resid).sum()
        # every output answers to its own row a and column b: impulses in the residual
        for a, b in ((0, 0), (r.shape[3] - 1, r.shape[4] - 1), (r.shape[3] // 2, r.shape[4] - 1)):
            one = np.zeros_like(resid)
            one[-1, a, b] = 1.0
            ref_1 = o.adjoint_padded(one.astype(np.float64))
            assert np.abs(r.adjoint(one) - ref_1).max() < TOL * np.abs(ref_1).max(), (a, b)


def test_tiny_angle_is_continuous_with_the_spectral_path(lib):
    """The rotated path at 1e-6 rad against the unrotated spectral path of the same scene at
    angle 0, both on the device; no restatement involved."""
    model = golden("resolution_rotated")["tiny_model"]
    _, _, obs_rot = cases.scene("tiny")
    _, _, obs_flat = cases.scene("tiny", 0.0)
    assert obs_rot.renderer.isrot and not obs_flat.renderer.isrot
    assert obs_rot.renderer.device_path() == 2 and obs_flat.renderer.device_path() == 1
    # an unrotated resampler cannot be moved to path 2
    lib_, handle, _ = obs_flat.renderer._resampler()
    assert lib_.smi_resampler_set_path(handle, 2) != 0
    assert obs_flat.renderer.device_path() == 1
    a, b = obs_rot.render(model), obs_flat.render(model)
    dev = np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()
    print("1e-6 rad against the spectral path at 0: %.2e of the peak" % dev)
    assert dev < TOL


@pytest.mark.parametrize("name", list(cases.CASES))
def test_facade_rendering_matches_the_reference(name):
    g = golden("resolution_rotated")
    _, _, obs_lr = cases.scene(name)
    assert obs_lr.renderer.device_path() == 2
    ref = g[name + "_rendered"]
    out = obs_lr.render(g[name + "_model"])
    assert out.shape == ref.shape and out.dtype == ref.dtype
    assert np.abs(out.astype(np.float64) - ref).max() < TOL * np.abs(ref).max()
    assert np.array_equal(obs_lr.render(g[name + "_model"]), out)
    assert obs_lr.renderer.device_path(2) == 2
    with pytest.raises(Exception):
        obs_lr.renderer.device_path(0)


def test_rotated_term_in_a_device_batch_matches_the_oracle(lib):
    """Patterned on test_lowres_term_on_the_device_matches_the_oracle (tests/test_gpu_facade.py),
    with its bounds: loss, low-resolution rendering and gradients of a blend with a rotated
    low-resolution observation, then 25 iterations against the oracle's trajectory."""
    from scarlet_amd.batch import BlendBatch, ComponentSpec

    g = golden("resolution_rotated")
    name = "skew"
    with Rotated(lib, name) as r:
        scene, lowres = build_scene(name, g)
        specs = [ComponentSpec(c.sed, c.morph, c.origin, sed_min_step=0.0)
                 for c in scene.components]
        batch = BlendBatch(scene.data[None], scene.weights[None], [specs], kernel=scene.kernel,
                           max_iter=30)
        batch.attach_lowres(r.handle, lowres.channels, lowres.data, lowres.weights,
                            lowres.log_norm)
        try:
            model, rendered, logL = batch.forward()
            loss, grads = scene.loss_and_gradients()
            assert abs(-logL[0] - loss) < 2e-6 * abs(loss)
            ref_lr = lowres.render(scene.get_model())
            assert np.abs(batch.lowres_rendered() - ref_lr).max() < 1e-5 * np.abs(ref_lr).max()
            g_sed, g_morph = batch.gradient()
            for k, (r_sed, r_morph) in enumerate(grads):
                assert np.abs(g_sed[k] - r_sed).max() < RTOL * np.abs(r_sed).max(), k
                assert np.abs(g_morph[k] - r_morph).max() < 2 * RTOL * np.abs(r_morph).max(), k
            # the term matters: the low-resolution bands are observed through it alone
            scene.extra_observations = []
            _, without = scene.loss_and_gradients()
            assert not np.any(without[0][0][lowres.channels])
            assert np.abs(grads[0][0][lowres.channels]).min() > 0
            scene.extra_observations = [lowres]
            scene.loss = []
            batch.fit(max_iter=25, e_rel=1e-9)
            n_ref, _ = scene.fit(25, e_rel=1e-9)
            hist = batch.loss_history()[0]
            assert len(hist) == n_ref == 25
            shift = lowres.log_norm + scene.log_norm
            assert_allclose(hist - shift, np.array(scene.loss) - shift, rtol=5e-4)
            assert hist[-1] < hist[0]
        finally:
            batch.close()
        # a batch of two blends does not take a rotated resampler
        two = BlendBatch(np.stack([scene.data] * 2), np.stack([scene.weights] * 2), [specs, specs],
                         kernel=scene.kernel, max_iter=4)
        try:
            with pytest.raises(Exception, match="on a rotated grid needs a batch of one blend"):
                two.attach_lowres(r.handle, lowres.channels, lowres.data, lowres.weights,
                                  lowres.log_norm)
        finally:
            two.close()


def test_blend_fit_with_a_rotated_observation():
    """Frame.from_observations, sources, Blend.fit(20, e_rel=1e-9) against the oracle's
    trajectory, at the bounds of test_blend_fit_with_two_resolutions (tests/test_gpu_facade.py);
    the oracle's low-resolution operator comes from the reference's set-up quantities."""
    g = golden("resolution_rotated")
    name = "turn"
    blend = cases.make_blend(name, resizing=False)
    assert blend.observations[1].renderer.isrot
    n, logL = blend.fit(20, e_rel=1e-9)
    scene, lowres = build_scene(name, g)
    n_ref, logL_ref = scene.fit(20, e_rel=1e-9)
    assert n == n_ref == 20
    shift = lowres.log_norm + scene.log_norm
    assert_allclose(np.array(blend.loss) - shift, np.array(scene.loss) - shift, rtol=1e-3)
    assert abs(logL - logL_ref) < 1e-4 * abs(logL_ref)
    assert blend.loss[-1] < blend.loss[0]
    for src, c in zip(blend.sources, scene.components):
        sed = np.asarray(src.children[0].parameters[0])
        assert np.abs(sed - c.sed).max() < 2e-3 * np.abs(c.sed).max()
        assert src.children[1].parameters[0].m is not None


def test_fit_blends_gives_a_rotated_blend_the_bits_of_its_own_fit():
    import scarlet_amd as scarlet
    from test_gpu_fit_blends_multires import assert_same, snapshot

    def make():
        return [mc.make_blend("first", 100), cases.make_blend("turn"),
                mc.make_blend("first", 101, offset=mc.OFFSETS[1])]

    ref = [snapshot(b, b.fit(15, e_rel=1e-4)) for b in make()]
    blends, report = make(), {}
    results = scarlet.fit_blends(blends, 15, e_rel=1e-4, _report=report)
    assert scarlet.fit_blends.errors == []
    assert report["alone"] == {1: "a low-resolution observation on a rotated grid"}
    assert [idx for _, idx in report["groups"]] == [[0, 2]]
    for i, (b, res) in enumerate(zip(blends, results)):
        assert ref[i]["n"] > 1 and np.isfinite(ref[i]["loss"]).all()
        assert_same(snapshot(b, res), ref[i], i)
