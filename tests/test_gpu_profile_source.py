"""Profile sources on the GPU: the device profiles through the probe entry, the profile kernels
(csrc/profile_source.hip) through the C ABI and Blend.fit / fit_blends through the facade, all
against the oracle (tests/profile_oracle.py), which tests/test_profile_source_host.py pins to the
reference's recorded results.

Tolerances of the steps and fits are those of tests/test_gpu_parity.py: 1e-5 after the first
step (lines 356-366), 1e-4 after five steps (lines 337-352), and for a whole fit the same
stopping iteration with chi^2 within 2e-5 over the first twelve iterations, 5e-4 throughout
and 1e-5 at the end (``_whole_fit_against_oracle``, lines 1672-1681)."""

import numpy as np
import pytest

from conftest import golden

import profile_oracle as po

pytestmark = pytest.mark.gpu

RTOL = 1e-5
PATHS = ["fused", "rocfft"]
FILTERS = list("grizy")


@pytest.fixture(scope="module")
def g():
    return golden("profile_source")


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd

    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# -- the probe entry ----------------------------------------------------------------------------
def probe(kind, params, h, w, oy, ox):
    import ctypes

    from scarlet_amd import _lib

    lib = _lib.load()
    params = np.ascontiguousarray(params, dtype=np.float64)
    out = np.zeros((7, h, w), dtype=np.float64)
    _lib.check(lib.smi_profile_probe(0, kind, _lib.ptr(params, ctypes.c_double), h, w, oy, ox,
                                     _lib.ptr(out, ctypes.c_double)))
    return out[0], out[1:]


NUS = [-0.85, -0.5, 0.0, 0.5, 1.3, 4.0]
# (centre, radius, e1, e2): round and centred on a pixel -- u runs from c_nu 1e-2 under the
# centre to the corner of the 101^2 box at radius 1 -- and sheared off-centre
SHAPES = [((50.0, 50.0), 1.0, 0.0, 0.0), ((49.3, 50.6), 1.0, 0.2, -0.1)]
TINY = np.finfo(np.float64).tiny
# |d ln f / d p| of exp(-R2/2) is at most R2 (1 + |e|) / (1 - |e|^2) for every parameter p at
# radius 1; R2 stays below 2 51^2 (1 + |e|)^2 / (1 - |e|^2) on the box, |e| <= 0.23 here
LOG_DERIVATIVE = 2e4


@pytest.mark.parametrize("center,radius,e1,e2", SHAPES)
def test_device_profiles_and_partials_against_the_oracle(center, radius, e1, e2):
    """Relative error at most 1e-10 of the value and of every partial, each relative to the
    oracle's own value of it: |device - oracle| <= 1e-10 |oracle|, pixel by pixel.

    The only exemption is where the oracle's number is zero or below the smallest normal
    float64, so that no relative error of 1e-10 exists in the format.  That happens in two
    places.  The Gaussian at radius 1 underflows inside this box, and the device has to underflow
    with the oracle: the value within that smallest normal number, a partial within it times
    the largest logarithmic derivative of the grid.  And a partial is exactly zero in the oracle
    on a line of symmetry of the round, pixel-centred shape (the centre partials on the axes,
    the ellipticity partials on the diagonals or axes; the Gaussian's nu partial everywhere):
    the same absolute floor holds there, which in practice asks the device for zero too."""
    side = 101
    Y = X = np.arange(side, dtype=np.float64)
    worst = {}
    for kind, nus in ((po.GAUSSIAN, [0.0]), (po.SPERGEL, NUS)):
        for nu in nus:
            params = [center[0], center[1], radius, e1, e2, nu]
            f, d = probe(kind, params, side, side, 0, 0)
            ref_f, ref_d = po.evaluate(kind, params, Y, X)
            if kind == po.SPERGEL and e1 == 0:
                u = po.cnu(nu) * np.sqrt(((Y[:, None] - 50) ** 2 + (X[None, :] - 50) ** 2) + 1e-4)
                assert np.isclose(u.min(), po.cnu(nu) * 1e-2) and u.max() > 70 * po.cnu(nu)
            assert np.all(np.isfinite(ref_f)) and np.all(np.isfinite(ref_d))
            assert np.all(np.isfinite(f)) and np.all(np.isfinite(d))
            normal = ref_f >= TINY
            if kind == po.SPERGEL:
                assert normal.all()
            else:
                # exp(-R2/2) leaves float64 beyond R2 ~ 1416, inside this box
                assert normal[50, 50] and not normal[0, 0]
                assert not d[5].any()
            normal_d = np.abs(ref_d) >= TINY
            err_f = np.abs(f - ref_f)
            err_d = np.abs(d - ref_d)
            floor_f = err_f[~normal].max(initial=0.0)
            floor_d = err_d[~normal_d].max(initial=0.0)
            rel_f = (err_f[normal] / ref_f[normal]).max()
            rel_d = np.array([(err_d[i][normal_d[i]] / np.abs(ref_d[i][normal_d[i]])).max(initial=0.0)
                              for i in range(6)])
            worst[(kind, nu)] = (rel_f, rel_d, floor_f, floor_d)
            print("kind %d nu %5.2f: value %.3g, partials %s; where the oracle is zero or "
                  "subnormal (%d values, %d partials): absolute %.3g, %.3g" % (
                      kind, nu, rel_f, " ".join("%.3g" % e for e in rel_d),
                      (~normal).sum(), (~normal_d).sum(), floor_f, floor_d))
    for key, (ef, ed, ff, fd) in worst.items():
        assert ef <= 1e-10 and np.all(ed <= 1e-10), (key, ef, ed)
        assert ff <= TINY and fd <= LOG_DERIVATIVE * TINY, (key, ff, fd)


# -- builders -----------------------------------------------------------------------------------
def profile_of(comp):
    """``profile=`` of a ComponentSpec from an oracle ProfileComponent"""
    return dict(kind=comp.kind, params=comp.params, step=comp.steps, rel_step=comp.rel_steps,
                fixed=comp.fixed_groups)


def spec_of(amd, comp):
    if isinstance(comp, po.ProfileComponent):
        return amd.ComponentSpec(comp.sed, np.zeros((comp.size, comp.size)), comp.origin,
                                 sed_min_step=comp.sed_min_step, sed_rel_step=comp.sed_rel_step,
                                 prox_flags=0, profile=profile_of(comp))
    return amd.ComponentSpec(comp.sed, comp.morph, comp.origin, sed_min_step=comp.sed_min_step)


def scene_batch(amd, sc, **kw):
    specs = [spec_of(amd, c) for c in sc.components]
    return amd.BlendBatch(sc.data[None], sc.weights[None], [specs], kernel=sc.kernel, **kw)


def check_gradients(batch, sc, what):
    """1e-5 relative for every profile-parameter and spectrum gradient.  The gradient of a
    Parameter is one array and its error is taken relative to the largest entry of the oracle's
    array, as ``rel_err`` does for every array in these tests: centre (2), radius (1),
    ellipticity (2), nu (1) and spectrum (bands) are the Parameters of a profile source."""
    g_sed, _ = batch.gradient()
    state = batch.profile_state()
    grads = sc.profile_gradients()
    assert state["components"] == sorted(grads)
    for k, (ref_sed, ref_par) in grads.items():
        comp = sc.components[k]
        errors = {"spectrum": rel_err(g_sed[k], ref_sed)}
        for name, sl in zip(po.GROUPS, po.SLOTS):
            if name == "nu" and comp.kind != po.SPERGEL:
                continue
            errors[name] = rel_err(state["gradient"][k][sl], ref_par[sl])
        print(what, "component", k, "gradient errors relative to the oracle's",
              " ".join("%s %.3g" % e for e in errors.items()),
              "| entry by entry:", np.abs(state["gradient"][k] - ref_par) /
              np.maximum(np.abs(ref_par), 1e-300), np.abs(g_sed[k] - ref_sed) / np.abs(ref_sed))
        for name, err in errors.items():
            assert err <= RTOL, (what, k, name, err)
        if comp.kind == po.GAUSSIAN:
            assert state["gradient"][k][5] == 0
        np.testing.assert_array_equal(state["params"][k], comp.params)


def check_state(batch, sc, tol, what):
    """parameters of every component against the oracle's within ``tol`` -- spectra relative to
    their peak, images absolute (unit peak), profile parameters absolute: centres are in pixels,
    the others of order one"""
    sed, morphs = batch.parameters()
    state = batch.profile_state()
    for k, c in enumerate(sc.components):
        assert rel_err(sed[k], c.sed) < tol, (what, k)
        if isinstance(c, po.ProfileComponent):
            err = np.abs(state["params"][k] - c.params)
            print(what, "component", k, "parameter error", err)
            assert err.max() < tol, (what, k, err)
            assert np.abs(morphs[k] - c.morph).max() < tol * max(c.morph.max(), 1.0), (what, k)
        else:
            assert np.abs(morphs[k] - c.morph).max() < tol, (what, k)


def assert_loss_close(loss, ref, log_norm, rtol):
    chi, chi_ref = np.asarray(loss) - log_norm, np.asarray(ref) - log_norm
    assert len(chi) == len(chi_ref)
    rel = np.abs(chi - chi_ref) / np.abs(chi_ref)
    assert rel.max() < rtol, rel


# -- the fixture scene through the C ABI ----------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_fixture_scene_forward_and_gradients(amd, g, hsc, path):
    sc = po.fixture_scene(g, hsc)
    batch = scene_batch(amd, sc, conv_path=path)
    assert batch.conv_path == path
    model, rendered, logL = batch.forward()
    assert rel_err(model[0], g["model"]) < RTOL
    assert rel_err(rendered[0], g["rendered"]) < RTOL
    assert abs(logL[0] - float(g["logL"])) < RTOL * abs(float(g["logL"]))
    check_gradients(batch, sc, "fixture/" + path)
    batch.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n_it,tol", [(1, RTOL), (5, 1e-4)])
def test_fixture_scene_steps(amd, g, hsc, path, n_it, tol):
    sc = po.fixture_scene(g, hsc)
    batch = scene_batch(amd, sc, conv_path=path, max_iter=8)
    batch.step(0, n_it, e_rel=1e-3)
    for it in range(n_it):
        sc.step(it, 1e-3)
    assert_loss_close(batch.loss_history()[0], sc.loss, sc.log_norm, tol)
    check_state(batch, sc, tol, "%d steps/%s" % (n_it, path))
    state = batch.profile_state()
    for k in state["components"]:
        c = sc.components[k]
        # m is linear in the gradients, v quadratic: the tolerance of the state and twice it,
        # Parameter by Parameter like the gradients (the six entries span orders of magnitude)
        for name, sl in zip(po.GROUPS, po.SLOTS):
            err_m, err_v = rel_err(state["m"][k][sl], c.m_p[sl]), rel_err(state["v"][k][sl], c.v_p[sl])
            print("%d steps/%s component %d %s: m %.3g v %.3g" % (n_it, path, k, name, err_m, err_v))
            assert err_m <= tol and err_v <= 2 * tol, (k, name)
    batch.close()


# -- box sizes ------------------------------------------------------------------------------------
# side, centre, frame (H, W): an even side; 21; beyond 63; the whole frame; overhanging two edges
BOXES = [(60, (33.3, 35.8), (70, 72)), (21, (20.4, 17.7), (40, 48)), (81, (45.2, 50.1), (96, 100)),
         (64, (31.6, 32.3), (64, 64)), (41, (4.7, 59.4), (64, 64))]


def single_scene(kind, side, center, frame, seed=0):
    rng = np.random.default_rng(seed)
    C = 3
    radius = side / 14.0
    params = [center[0], center[1], radius, 0.15, -0.1, 0.7]
    origin = None
    if side == frame[0] == frame[1]:
        origin = (0, 0)  # the box is the frame
    k1 = np.exp(-0.5 * (np.arange(-3, 4) / 1.2) ** 2)
    kernel = (k1[:, None] * k1[None, :] / k1.sum() ** 2)[None].astype(np.float32)
    comp = po.ProfileComponent(np.array([1.0, 2.0, 1.5]), kind, params, side, origin=origin,
                               rel_step=(0.0, 0.1 if kind == po.GAUSSIAN else 0.01, 0.0, 0.0),
                               sed_min_step=np.full(C, 1e-3))
    data = np.zeros((C,) + frame, dtype=np.float32)
    weights = (0.5 + rng.random((C,) + frame)).astype(np.float32)
    sc = po.ProfileScene((C,) + frame, data, weights, kernel, [comp])
    # the truth is another profile: every parameter has something to move to
    truth = po.ProfileComponent(np.array([1.3, 2.4, 1.9]), kind,
                                [center[0] + 0.4, center[1] - 0.3, 1.2 * radius, 0.05, 0.1, 0.4],
                                side, origin=comp.origin)
    sc.components = [truth]
    target = sc.render(sc.get_model())
    sc.components = [comp]
    sc.data = (target + 0.02 * rng.standard_normal(target.shape)).astype(np.float32)
    return sc


@pytest.mark.parametrize("kind", [po.GAUSSIAN, po.SPERGEL])
@pytest.mark.parametrize("side,center,frame", BOXES)
def test_box_sizes(amd, kind, side, center, frame):
    sc = single_scene(kind, side, center, frame)
    comp = sc.components[0]
    fs, _ = sc.box_slices(comp)
    covered = (fs[1].stop - fs[1].start) * (fs[2].stop - fs[2].start)
    assert (covered < side * side) == (side == 41), "only the 41 box overhangs (two edges)"
    batch = scene_batch(amd, sc, max_iter=8)
    what = "kind %d side %d" % (kind, side)
    model, _, _ = batch.forward()
    assert rel_err(model[0], sc.get_model()) < RTOL, what
    check_gradients(batch, sc, what)
    batch.step(0, 3, e_rel=1e-3)
    for it in range(3):
        sc.step(it, 1e-3)
    assert_loss_close(batch.loss_history()[0], sc.loss, sc.log_norm, 1e-4)
    check_state(batch, sc, 1e-4, what)
    batch.close()


# -- the facade -----------------------------------------------------------------------------------
def extended(scarlet, frame, g, k, scale=1.0):
    image = g["morph_%d" % k]
    h, w = image.shape
    oy, ox = (int(v) for v in g["origin_%d" % k])
    box = scarlet.Box((5, h, w), origin=(0, oy, ox))
    spectrum = scarlet.TabulatedSpectrum(frame, g["sed_%d" % k].copy() * scale, bbox=box[0],
                                         min_step=g["sed_step_minimum_%d" % k])
    morphology = scarlet.ExtendedSourceMorphology(
        frame, (oy + h // 2, ox + w // 2), image.copy(), bbox=box[1:], monotonic="angle",
        resizing=False)
    return scarlet.FactorizedComponent(frame, spectrum, morphology)


def fixture_blend(g, hsc, scale=1.0, extra=()):
    """The fixture scene through the mirror classes (the extended sources from their recorded
    images, without resizing); ``extra``: names of further sources, "point" and "starlet"."""
    import scarlet_amd as scarlet

    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=FILTERS)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=FILTERS).match(frame)
    sources = []
    for k in range(int(g["n_sources"])):
        kind, p = str(g["kinds"][k]), g["params_%d" % k] if "params_%d" % k in g.files else None
        sky = tuple(g["sky_coords"][k])
        if kind == "extended":
            src = extended(scarlet, frame, g, k, scale)
            if "starlet" in extra and k == 2:
                src = scarlet.StarletSource.from_source(src)
            sources.append(src)
            continue
        if kind == "gaussian":
            src = scarlet.GaussianSource(frame, sky, float(p[2]), p[3:5].copy(), obs)
        else:
            src = scarlet.SpergelSource(frame, sky, float(p[5]), float(p[2]), p[3:5].copy(), obs)
        src.children[0].parameters[0][...] *= scale
        sources.append(src)
    if "point" in extra:
        sources.append(scarlet.PointSource(frame, tuple(g["sky_coords"][5]), obs))
    return scarlet.Blend(sources, obs), obs


def oracle_for_blend(g, hsc):
    sc = po.fixture_scene(g, hsc)
    for c in sc.components:
        if not isinstance(c, po.ProfileComponent):
            c.resizing = False
    return sc


def boxes_of(blend):
    return [tuple(int(o) for o in s.children[1].bbox.origin[-2:]) +
            tuple(int(n) for n in s.children[1].bbox.shape[-2:]) for s in blend.sources]


@pytest.mark.parametrize("e_rel,converges", [(1e-4, False), (1e-3, True)])
def test_whole_fit_with_the_hook_follows_the_oracle(g, hsc, monkeypatch, e_rel, converges):
    """e_rel = 1e-4: the issue's fit; the oracle needs 190 iterations for it, so both sides
    run to ``max_iter``.  e_rel = 1e-3: the oracle's stopping rule fires at iteration 52, after
    two restarts, and the device has to stop at that iteration too."""
    import scarlet_amd as scarlet
    from scarlet_amd import blend as blend_module

    blend, _ = fixture_blend(g, hsc)
    sc = oracle_for_blend(g, hsc)
    history = [boxes_of(blend)]
    stock = blend_module._update_sources

    def recording(sources):
        restart = stock(sources)
        if restart:
            history.append(boxes_of(blend))
        return restart

    monkeypatch.setattr(blend_module, "_update_sources", recording)
    n_iter, logL = blend.fit(100, e_rel=e_rel)
    n_ref, logL_ref = sc.fit(max_iter=100, e_rel=e_rel, resizing=True)
    print("iterations", n_iter, n_ref, "boxes", history, sc.box_history)
    assert (n_ref < 100) == converges
    assert n_iter == n_ref and len(blend.loss) == n_ref
    assert history == sc.box_history and len(history) > 1
    chi, ref = np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("chi^2: first twelve %.3g, whole %.3g, final %.3g" % (rel[:12].max(), rel.max(), rel[-1]))
    assert rel[:12].max() < 2e-5 and rel.max() < 5e-4 and rel[-1] < RTOL
    for k, c in enumerate(sc.components):
        if isinstance(c, po.ProfileComponent):
            morphology = blend.sources[k].children[1]
            for name, sl in zip(po.GROUPS, po.SLOTS):
                p = morphology.get_parameter(name)
                if p is not None:
                    assert np.abs(np.asarray(p) - c.params[sl]).max() < 5e-4, (k, name)
                    assert p.m is not None and p.m.shape == p.shape and p.m.dtype == np.float64
    assert isinstance(blend.sources[0], scarlet.GaussianSource)


def test_fixed_parameters_come_back_bit_identical(g, hsc):
    import scarlet_amd as scarlet

    blend, obs = fixture_blend(g, hsc)
    frame = blend.sources[0].frame
    # one source with only its radius free, and the all-fixed morphology from plain numbers
    partly = blend.sources[1].children[1]
    for name in ("center", "ellipticity"):
        partly.get_parameter(name).fixed = True
    fixed = scarlet.GaussianMorphology(frame, (30.25, 20.5), 2.0)
    spectrum = scarlet.TabulatedSpectrum(frame, np.full(5, 3.0, dtype=np.float32),
                                         min_step=np.full(5, 1e-3))
    sources = list(blend.sources) + [scarlet.FactorizedComponent(frame, spectrum, fixed)]
    before = {id(p): np.array(p) for s in sources for p in s.children[1].parameters}
    blend = scarlet.Blend(sources, obs)
    blend.fit(25, e_rel=1e-6)
    moved = 0
    for s in sources:
        if not isinstance(s.children[1], scarlet.ProfileMorphology):
            continue
        for p in s.children[1].parameters:
            if p.fixed:
                np.testing.assert_array_equal(np.asarray(p), before[id(p)])
            else:
                moved += int(np.any(np.asarray(p) != before[id(p)]))
    assert moved >= 8 and np.any(np.asarray(partly.get_parameter("radius")) != 2.3)
    assert np.any(np.asarray(spectrum.parameters[0]) != 3.0)


def mixed_oracle_scene():
    """Extended, point, starlet, Gaussian and Spergel components in one oracle scene"""
    import starlet_oracle as so
    from oracle import pgm

    class MixedScene(po.ProfileScene, so.StarletScene):
        pass

    rng = np.random.default_rng(7)
    C, frame = 3, (56, 60)
    k1 = np.exp(-0.5 * (np.arange(-3, 4) / 1.2) ** 2)
    kernel = (k1[:, None] * k1[None, :] / k1.sum() ** 2)[None].astype(np.float32)
    step = np.full(C, 1e-3)
    yy, xx = np.mgrid[:21, :21]
    blob = np.exp(-((yy - 10) ** 2 + (xx - 10) ** 2) / (2 * 3.0 ** 2))
    shape = (24, 24)
    yy, xx = np.mgrid[:24, :24]
    fuzzy = np.exp(-((yy - 11) ** 2 + (xx - 13) ** 2) / (2 * 4.0 ** 2)) + 0.05 * rng.random(shape)
    comps = [
        pgm.Component(np.array([1.0, 1.5, 0.8]), blob / blob.max(), (4, 6), sed_min_step=step),
        pgm.PointComponent(np.array([2.0, 1.0, 0.5]), (40.3, 12.6), 0.8, sed_min_step=step),
        so.StarletComponent(np.array([0.6, 0.9, 1.1]), so.transform(fuzzy, so.get_scales(shape)),
                            (28, 30), so.thresholds(shape, 5e-3), sed_min_step=step),
        po.ProfileComponent(np.array([1.0, 2.0, 1.5]), po.GAUSSIAN, [15.4, 42.7, 2.3, 0.2, -0.1, 0],
                            23, sed_min_step=step),
        po.ProfileComponent(np.array([0.7, 0.9, 1.4]), po.SPERGEL, [44.2, 40.4, 2.0, 0.1, 0.05, 0.5],
                            20, rel_step=(0.0, 0.01, 0.0, 0.0), sed_min_step=step),
    ]
    data = np.zeros((C,) + frame, dtype=np.float32)
    weights = (0.5 + rng.random((C,) + frame)).astype(np.float32)
    sc = MixedScene((C,) + frame, data, weights, kernel, comps)
    truth = sc.render(sc.get_model())
    sc.data = (1.2 * truth + 0.02 * rng.standard_normal(truth.shape)).astype(np.float32)
    return sc


def test_mixed_scene_follows_the_oracle(amd):
    import starlet_oracle as so
    from oracle import pgm

    sc = mixed_oracle_scene()
    specs = []
    for c in sc.components:
        if isinstance(c, pgm.PointComponent):
            specs.append(amd.PointSourceSpec(c.sed, c.center, c.sigma, sed_min_step=c.sed_min_step,
                                             center_step=c.center_step))
        elif isinstance(c, so.StarletComponent):
            specs.append(amd.ComponentSpec(c.sed, np.zeros(c.morph.shape[1:]), c.origin,
                                           sed_min_step=c.sed_min_step, morph_step=1e-2,
                                           prox_flags=0, starlet=(c.morph, c.thresh)))
        else:
            specs.append(spec_of(amd, c))
    batch = amd.BlendBatch(sc.data[None], sc.weights[None], [specs], kernel=sc.kernel, max_iter=8)
    model, _, _ = batch.forward()
    assert rel_err(model[0], sc.get_model()) < RTOL
    n_it = 5
    batch.step(0, n_it, e_rel=1e-3)
    for it in range(n_it):
        sc.step(it, 1e-3)
    assert_loss_close(batch.loss_history()[0], sc.loss, sc.log_norm, 1e-4)
    sed, _ = batch.parameters()
    state = batch.profile_state()
    assert state["components"] == [3, 4]
    for k, c in enumerate(sc.components):
        assert rel_err(sed[k], c.sed) < 1e-4, k
        if isinstance(c, po.ProfileComponent):
            assert np.abs(state["params"][k] - c.params).max() < 1e-4, k
    # frame coordinates on both sides, as at tests/test_gpu_parity.py:1892-1895
    assert np.abs(batch.centers()["center"][1] - sc.components[1].center).max() < 1e-4
    batch.close()


def parameters_of(blend):
    out = []
    for p in blend.parameters:
        out.extend([np.array(p)] + [np.array(getattr(p, n)) for n in ("m", "v", "vhat")
                                    if getattr(p, n) is not None])
    return out


def test_fit_blends_equals_one_by_one_fits_bit_for_bit(g, hsc):
    import scarlet_amd as scarlet

    extra = ("point", "starlet")
    scales = [1.0, 0.7, 1.0, 1.4, 1.0]  # the same blend at positions 0, 2 and 4 of the batch
    alone = []
    for s in scales:
        blend, _ = fixture_blend(g, hsc, scale=s, extra=extra)
        alone.append((blend, blend.fit(35, e_rel=1e-6)))
    kinds = {type(s).__name__ for s in alone[0][0].sources}
    assert {"GaussianSource", "SpergelSource", "StarletSource", "PointSource",
            "FactorizedComponent"} <= kinds
    batch = [fixture_blend(g, hsc, scale=s, extra=extra)[0] for s in scales]
    results = scarlet.fit_blends(batch, 35, e_rel=1e-6)
    for (one, res_one), many, res_many in zip(alone, batch, results):
        assert tuple(res_one) == tuple(res_many)
        assert one.loss == many.loss
        assert boxes_of(one) == boxes_of(many)
        for a, b in zip(parameters_of(one), parameters_of(many)):
            np.testing.assert_array_equal(a, b)
    for i in (2, 4):  # repeats of blend 0
        assert batch[i].loss == batch[0].loss
    assert batch[1].loss != batch[0].loss and len(batch[0].loss) == 35


def test_a_second_fit_continues_from_the_stored_moments(g, hsc):
    blend, _ = fixture_blend(g, hsc)
    sc = oracle_for_blend(g, hsc)
    blend.fit(8, e_rel=1e-9)
    sc.fit(max_iter=8, e_rel=1e-9, resizing=True)
    radius = blend.sources[0].children[1].get_parameter("radius")
    assert radius.m is not None and radius.v.any()
    blend.fit(6, e_rel=1e-9)
    sc.fit(max_iter=6, e_rel=1e-9, resizing=True)
    assert len(blend.loss) == 14
    assert_loss_close(blend.loss, sc.loss, sc.log_norm, 1e-4)
    # a cold start from the same parameters is another trajectory
    cold = oracle_for_blend(g, hsc)
    cold.fit(max_iter=8, e_rel=1e-9, resizing=True)
    for c in cold.components:
        for name in ("m_sed", "v_sed", "vhat_sed", "m_morph", "v_morph", "vhat_morph"):
            getattr(c, name)[...] = 0
        if isinstance(c, po.ProfileComponent):
            c.m_p[...] = c.v_p[...] = c.vhat_p[...] = 0
    cold.fit(max_iter=6, e_rel=1e-9, resizing=True)
    chi, chi_cold = np.array(blend.loss) - sc.log_norm, np.array(cold.loss) - sc.log_norm
    assert np.abs(chi[-1] - chi_cold[-1]) > 1e-3 * abs(chi_cold[-1])
