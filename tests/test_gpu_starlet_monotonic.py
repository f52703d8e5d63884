"""Monotonic starlet sources on the GPU: the mask operator of csrc/mask_device.h alone (through
``smi_starlet_monotonic_mask_f32``) and inside the step kernel of csrc/starlet_source.hip, against
the oracle (tests/starlet_monotonic_oracle.py), and ``Blend.fit`` / ``fit_blends`` through the
facade.

The operator itself is compared bit for bit (``np.array_equal``) with the oracle in float32:
it copies, clears or interpolates with three float32 operations that both sides do alike.
Whole steps are compared with the float64 oracle at the tolerances of
tests/test_gpu_starlet_source.py; a monotonic plane has no thresholds a coefficient could be
"near" to, instead a rounding difference can flip one comparison of the fill and with it the
pixels behind it, so a share of the coefficients -- at most the 1 % ``assert_coefficients``
allows there -- may differ (the float32-state oracle against the float64-state one: 0.022 % at
the most over the 12 steps of the fixture scene, loss within 5.4e-6)."""

import numpy as np
import pytest

from conftest import golden

import starlet_monotonic_oracle as smo

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # of tests/test_gpu_starlet_source.py
LDS_PIXELS = 20000  # kStarLdsPixels of csrc/common.h


@pytest.fixture(scope="module")
def g():
    return golden("starlet_source")


@pytest.fixture(scope="module")
def gm():
    return golden("starlet_monotonic")


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd

    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# -- the operator alone -----------------------------------------------------------------------
def blob(planes, h, w, seed, noise=0.05, bumps=None):
    """A blob about a point near the middle per plane, plus seeded noise everywhere -- or, with
    ``bumps``, on that many pixels only (a smooth image whose passes stay short)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    out = np.empty((planes, h, w), dtype=np.float32)
    for p in range(planes):
        cy, cx = h / 2 + 0.3 * p, w / 2 - 0.4 * p
        s = max(min(h, w) / (3.0 + p), 0.7)
        image = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        if bumps is None:
            image += noise * rng.standard_normal((h, w))
        else:
            at = rng.choice(h * w, size=bumps, replace=False)
            image.reshape(-1)[at] *= 1 + 0.5 * rng.random(bumps)
        out[p] = image
    return out


def check_operator(amd, stack, rule, what):
    want, interpolated = smo.mask_planes(stack, *rule)
    got = amd.monotonic_planes_prox(stack, amd.MonotonicPlanes(*rule))
    print(what, stack.shape, rule, "kept %d of %d, interpolated %d"
          % ((want != 0).sum(), want.size, interpolated))
    assert got.dtype == np.float32 and np.array_equal(got, want), what
    return interpolated


RULES = [(1, 0.0, 3), (0, 0.0, 3), (1, 0.02, 3), (1, 0.0, 0), (0, 0.02, 1)]
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 3), (2, 7), (7, 2), (33, 33), (41, 41), (58, 48)]


@pytest.mark.parametrize("shape", SHAPES)
def test_operator_against_the_oracle(amd, shape):
    h, w = shape
    total = 0
    for planes in (1, 2, 3):
        for n, rule in enumerate(RULES):
            stack = blob(planes, h, w, seed=100 * planes + n)
            n_int = check_operator(amd, stack, rule, "blob")
            total += n_int if rule[2] > 0 else 0
    if h * w > 1024:  # the noisy inputs go through the interpolation passes
        assert total > 0


def test_operator_with_the_work_planes_in_global_memory(amd):
    h, w = 142, 141
    assert (h * w > LDS_PIXELS) and (h - 1) * w <= LDS_PIXELS
    stack = blob(2, h, w, seed=7, bumps=60)
    assert check_operator(amd, stack, (1, 0.0, 3), "beyond the LDS") > 0
    check_operator(amd, stack[:1], (0, 0.01, 1), "beyond the LDS")
    # ... and the largest box whose work planes are still in the LDS
    stack = blob(1, 125, 160, seed=8, bumps=60)
    assert stack[0].size == LDS_PIXELS
    assert check_operator(amd, stack, (1, 0.0, 3), "the last LDS box") > 0


def test_operator_special_cases(amd):
    # a plateau in the window of the centre: the first maximum in row-major order starts the fill
    stack = blob(2, 9, 9, seed=1, noise=0.0)
    stack[:, 3:6, 3:6] = 2.0
    stack[0, 3, 3] = 1.5  # the first of the maxima is then (3, 4)
    for rule in RULES:
        check_operator(amd, stack, rule, "plateau")
    # the maximum in each corner of the window in turn, also a window cut by the plane's edge
    for dy in (-1, 1):
        for dx in (-1, 1):
            stack = blob(1, 11, 7, seed=2, noise=0.01)
            stack[0, 5 + dy, 3 + dx] = 3.0
            check_operator(amd, stack, (1, 0.0, 3), "corner")
            small = blob(1, 2, 2, seed=3, noise=0.01)
            small[0, max(dy, 0), max(dx, 0)] = 3.0
            check_operator(amd, small, (1, 0.0, 3), "cut window")
    # nothing positive: only the start pixel survives, and that as it is
    stack = -1 - blob(3, 12, 10, seed=4) ** 2
    for rule in RULES:
        want, _ = smo.mask_planes(stack, *rule)
        assert np.count_nonzero(want) == 3
        check_operator(amd, stack, rule, "all negative")
    # a radius wider than the plane: the window is the plane
    check_operator(amd, blob(2, 6, 5, seed=5), (9, 0.0, 3), "wide window")


# -- the fixture scene through the C ABI ------------------------------------------------------
def fixture_specs(amd, g, gm, monotonic=None):
    """the fixture scene's components; ``monotonic``: which starlet sources are (all of them)"""
    starlet = [int(k) for k in gm["starlet_of"]]
    monotonic = starlet if monotonic is None else monotonic
    specs = []
    for k in range(int(g["n_sources"])):
        kw = dict(sed_min_step=g["sed_step_minimum_%d" % k],
                  sed_rel_step=float(g["sed_step_factor_%d" % k]))
        if float(g["sed_zero_%d" % k]) != 1e-20:
            kw["sed_floor"] = float(g["sed_zero_%d" % k])
        if k in starlet:
            coeffs = gm["coeffs_%d" % k]
            rule = amd.MonotonicPlanes(int(gm["center_radius_%d" % k]), float(gm["variance_%d" % k]),
                                       int(gm["max_iter_%d" % k]))
            specs.append(amd.ComponentSpec(
                gm["sed_%d" % k], np.zeros(coeffs.shape[1:]), gm["origin_%d" % k],
                morph_step=float(gm["step_%d" % k]), prox_flags=0,
                starlet=(coeffs, rule if k in monotonic else g["thresh_%d" % k]), **kw))
        else:
            specs.append(amd.ComponentSpec(g["sed_%d" % k], g["morph_%d" % k],
                                           g["origin_%d" % k], **kw))
    return specs


def fixture_batch(amd, g, gm, hsc, **kw):
    return amd.BlendBatch(hsc["images"][None], hsc["weights"][None], [fixture_specs(amd, g, gm)],
                          kernel=hsc["diff_kernel"], **kw)


def test_fixture_scene_forward(amd, g, gm, hsc):
    batch = fixture_batch(amd, g, gm, hsc)
    model, rendered, logL = batch.forward()
    assert rel_err(model[0], gm["model"]) < RTOL
    assert rel_err(rendered[0], gm["rendered"]) < RTOL
    assert abs(logL[0] - float(gm["logL"])) < RTOL * abs(float(gm["logL"]))
    batch.close()


def one_step(amd, g, gm, hsc, prox_max_iter):
    batch = fixture_batch(amd, g, gm, hsc, max_iter=4)
    batch.step(0, 1, e_rel=1e-3, prox_max_iter=prox_max_iter)
    state, sed = batch.starlet_state(), batch.parameters()[0]
    batch.close()
    return state, sed


@pytest.fixture(scope="module")
def first_step(amd, g, gm, hsc):
    """the device's first step without (prox_max_iter=0) and with one proximal evaluation, and
    the float64 oracle's without"""
    sc = smo.fixture_scene(g, gm, hsc)
    sc.step(0, 1e-3, prox_max_iter=0)
    return one_step(amd, g, gm, hsc, 0), one_step(amd, g, gm, hsc, 1), sc


def test_one_step_exact(gm, first_step):
    """prox_max_iter=0 leaves the device's own pre-prox coefficients; with prox_max_iter=1 the
    coefficients are the float32 operator of exactly those.  The pre-prox coefficients, the
    first moment and the spectrum against the float64 oracle's step."""
    (pre, sed), (post, _), sc = first_step
    assert list(pre["components"]) == [int(k) for k in gm["starlet_of"]]
    total = 0
    for j, k in enumerate(pre["components"]):
        comp = sc.components[k]
        x = pre["coeffs"][j]
        assert x.dtype == np.float32
        want, interpolated = smo.mask_planes(x, comp.center_radius, comp.variance, comp.max_iter)
        print("component", k, "interpolated", interpolated, "kept", (want != 0).mean(),
              "pre-prox", rel_err(x, comp.morph), "m", rel_err(pre["m"][j], comp.m_morph),
              "spectrum", rel_err(sed[k], comp.sed))
        total += interpolated
        assert np.array_equal(post["coeffs"][j], want), k
        assert rel_err(x, comp.morph) < RTOL, k
        assert rel_err(pre["m"][j], comp.m_morph) < RTOL, k
        for name in ("m", "v", "vhat"):
            np.testing.assert_array_equal(pre[name][j], post[name][j])
        assert rel_err(sed[k], comp.sed) < RTOL, k
    # (the spectra of the two runs differ by their own proximal step, which prox_max_iter=0 skips)
    assert total > 0  # the step went through the interpolation passes


def test_one_step_second_moments(gm, first_step):
    """v and vhat (= v at the first step) of the same step against the float64 oracle at RTOL.

    The moments of a monotonic component are taken with b1 and b2 in double
    (``smi_batch_set_optimizer_f64``): with the batch's float32 constants, which the other
    kernels keep, 1 - float32(0.999) alone puts 1.3e-5 on v = (1 - b2) g^2."""
    (pre, _), _, sc = first_step
    worst = {}
    for j, k in enumerate(pre["components"]):
        comp = sc.components[k]
        for name, ref in (("v", comp.v_morph), ("vhat", comp.vhat_morph)):
            worst[(int(k), name)] = rel_err(pre[name][j], ref)
    print("second moments against the float64 oracle:", worst)
    assert max(worst.values()) < RTOL, worst


def assert_coefficients(dev, comp, tol, what):
    """Equal supports and values within ``tol`` of the stack's peak (the scale
    ``assert_coefficients`` of tests/test_gpu_starlet_source.py argues for), but for at most
    1 % of the coefficients: those behind a comparison of the fill that rounding flipped."""
    ref = comp.morph
    peak = np.abs(ref).max()
    differs = ((dev != 0) != (ref != 0)) | (np.abs(dev - ref) > tol * peak)
    print(what, "differing %d of %d (%.4f%%), worst elsewhere %.3g of the peak"
          % (differs.sum(), differs.size, 100 * differs.mean(),
             (np.abs(dev - ref) / peak)[~differs].max()))
    assert dev.shape == ref.shape and differs.mean() <= 0.01, (what, differs.mean())


@pytest.mark.parametrize("n_it", [1, 2, 12])
def test_fixture_scene_steps(amd, g, gm, hsc, n_it):
    batch = fixture_batch(amd, g, gm, hsc, max_iter=16)
    batch.step(0, n_it, e_rel=1e-3)
    sc = smo.fixture_scene(g, gm, hsc)
    for it in range(n_it):
        sc.step(it, 1e-3)
    loss = batch.loss_history()[0]
    chi, ref = loss - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("steps", n_it, "loss", rel.max(), "interpolated by the oracle",
          [sc.components[int(k)].interpolated for k in gm["starlet_of"]])
    assert len(loss) == n_it and rel.max() < 2e-5
    sed, morphs = batch.parameters()
    state = batch.starlet_state()
    tol = RTOL if n_it == 1 else 1e-4
    for j, k in enumerate(state["components"]):
        comp = sc.components[k]
        assert comp.interpolated > 0
        assert_coefficients(state["coeffs"][j], comp, tol, "steps %d component %d" % (n_it, k))
        assert rel_err(sed[k], comp.sed) < tol, k
    for k, comp in enumerate(sc.components):
        if k not in state["components"]:
            assert np.abs(morphs[k] - comp.morph).max() < tol, k
            assert rel_err(sed[k], comp.sed) < tol, k
    batch.close()


def test_a_blend_that_has_converged_keeps_its_coefficients(amd, g, gm, hsc):
    """two blends in one batch; the second one's weights are so small that its loss is its
    normalisation term, which does not move: it stops at the first chance and its monotonic
    coefficients stay as they were while the first blend goes on"""
    specs = [fixture_specs(amd, g, gm) for _ in range(2)]
    batch = amd.BlendBatch(np.stack([hsc["images"]] * 2),
                           np.stack([hsc["weights"], hsc["weights"] * 1e-12]), specs,
                           kernel=hsc["diff_kernel"], max_iter=16)
    batch.step(0, 4, e_rel=1e-6, check_convergence=True)
    states = batch.states()
    assert states[0] == 0 and states[1] == 2
    n_star = len(gm["starlet_of"])
    before = [c.copy() for c in batch.starlet_state()["coeffs"][n_star:]]
    first = [c.copy() for c in batch.starlet_state()["coeffs"][:n_star]]
    batch.step(4, 3, e_rel=1e-6, check_convergence=True)
    after = batch.starlet_state()["coeffs"]
    for a, b in zip(before, after[n_star:]):
        np.testing.assert_array_equal(a, b)
    assert any(np.any(a != b) for a, b in zip(first, after[:n_star]))
    batch.close()


# -- the facade -------------------------------------------------------------------------------
def fixture_blend(g, hsc, monotonic=(0, 2, 7), drop=0, scale=1.0):
    """The fixture scene through the facade (``fixture_blend`` of
    tests/test_gpu_starlet_source.py): sources 0 and 2 by ``from_source``, the full-frame
    ``StarletSource(frame)`` under seed 0 last; those listed in ``monotonic`` with
    ``monotonic=True``."""
    import scarlet_amd as scarlet

    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    n = int(g["n_sources"])
    sources = []
    for k in range(n - 1):
        image = g["image_%d" % k] if k in (0, 2) else g["morph_%d" % k]
        h, w = image.shape
        oy, ox = (int(v) for v in g["origin_%d" % k])
        box = scarlet.Box((5, h, w), origin=(0, oy, ox))
        spectrum = scarlet.TabulatedSpectrum(frame, g["sed_%d" % k].copy() * scale, bbox=box[0],
                                             min_step=g["sed_step_minimum_%d" % k])
        morphology = scarlet.ExtendedSourceMorphology(
            frame, (oy + h // 2, ox + w // 2), image.copy(), bbox=box[1:], monotonic="angle",
            resizing=False)
        src = scarlet.FactorizedComponent(frame, spectrum, morphology)
        if k in (0, 2):
            src = scarlet.StarletSource.from_source(src, monotonic=k in monotonic)
        sources.append(src)
    np.random.seed(0)
    diffuse = scarlet.StarletSource(frame, monotonic=(n - 1) in monotonic)
    diffuse.children[0]._parameters[0][...] *= scale
    plain = [s for k, s in enumerate(sources) if k not in (0, 2)]
    keep = [s for s in sources if s not in plain[len(plain) - drop:]] if drop else sources
    return scarlet.Blend(keep + [diffuse], obs), obs


def test_mirror_classes_against_the_fixture(g, gm, hsc):
    import scarlet_amd as scarlet

    blend, _ = fixture_blend(g, hsc)
    for k in gm["starlet_of"]:
        morphology = blend.sources[int(k)].children[1]
        coeffs = morphology.parameters[0]
        assert morphology.monotonic is True and coeffs.step == float(gm["step_%d" % k])
        np.testing.assert_array_equal(np.asarray(coeffs), gm["coeffs_%d" % k])  # bit for bit
        c = coeffs.constraint
        assert type(c) is scarlet.MonotonicMaskConstraint
        assert tuple(c.center) == tuple(gm["center_%d" % k])
        assert (c.center_radius, c.variance, c.max_iter) == (
            int(gm["center_radius_%d" % k]), float(gm["variance_%d" % k]), int(gm["max_iter_%d" % k]))
        assert tuple(morphology.bbox.origin) == tuple(gm["origin_%d" % k])
        assert tuple(morphology.bbox.shape) == tuple(gm["shape_%d" % k])
    assert rel_err(blend.get_model(), gm["model"]) < RTOL


def test_blend_fit_follows_the_oracle_through_a_shrink(g, gm, hsc):
    """``Blend.fit(30, e_rel=1e-4)`` against ``StarletScene.fit`` with the re-centring shrink
    hook at every 10th iteration: iteration count, boxes, coefficients and loss"""
    blend, _ = fixture_blend(g, hsc)
    n, logL = blend.fit(30, e_rel=1e-4)
    sc = smo.fixture_scene(g, gm, hsc)
    starlet = [int(k) for k in gm["starlet_of"]]
    for k, comp in enumerate(sc.components):
        comp.resizing = k in starlet  # (the plain sources were built with resizing=False)
    n_ref, _ = sc.fit(30, e_rel=1e-4, resizing=True)
    assert n == len(blend.loss) == n_ref, (n, n_ref)
    chi, ref = np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("fit:", n, "iterations, loss", rel.max(), "boxes",
          [sc.components[k].morph.shape for k in starlet])
    assert rel.max() < 2e-5
    assert logL == -blend.loss[-1]
    for k in starlet:
        morphology = blend.sources[k].children[1]
        coeffs = morphology.parameters[0]
        comp = sc.components[k]
        assert coeffs.shape == comp.morph.shape, k
        assert tuple(morphology.bbox.origin) == tuple(comp.origin), k
        assert tuple(coeffs.constraint.center) == comp.center, k
        assert coeffs.m.shape == coeffs.v.shape == coeffs.vhat.shape == coeffs.shape
        assert coeffs.std.shape == coeffs.shape and coeffs.dtype == np.float64
        assert_coefficients(np.asarray(coeffs), comp, 1e-4, "fit component %d" % k)


def test_refusals_through_the_facade(g, hsc):
    import scarlet_amd as scarlet
    from scarlet_amd import _lib

    uploads = _lib.load().smi_observation_uploads()

    def blend_with(change):
        blend, _ = fixture_blend(g, hsc)
        change(blend.sources[0].children[1])
        return blend

    def unflagged(morphology):
        morphology.monotonic = False

    def foreign_centre(morphology):
        morphology.parameters[0].constraint = scarlet.MonotonicMaskConstraint((19, 20))

    def with_callable(morphology):
        morphology.parameters[0].step = lambda x, it=0: 1e-2

    for change in (unflagged, foreign_centre, with_callable):
        with pytest.raises(NotImplementedError):
            blend_with(change).fit(5)
    assert _lib.load().smi_observation_uploads() == uploads  # refused before any device work


def test_fit_blends_equals_the_single_fits(g, hsc):
    """monotonic, thresholded and mixed blends of different sizes in one batch"""
    import scarlet_amd as scarlet

    def make(k):
        return fixture_blend(g, hsc, monotonic=[(0, 2, 7), (), (2,)][k], drop=k,
                             scale=1 + 0.1 * k)[0]

    single = [make(k) for k in range(3)]
    want = [b.fit(25, e_rel=1e-5) for b in single]
    many = [make(k) for k in range(3)]
    got = scarlet.fit_blends(many, 25, e_rel=1e-5)
    for a, b, r1, r2 in zip(single, many, want, got):
        assert r1 == r2
        np.testing.assert_array_equal(a.loss, b.loss)
        for s, t in zip(a.sources, b.sources):
            assert s.bbox == t.bbox
        for p, q in zip(a.parameters, b.parameters):
            assert p.shape == q.shape
            np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
            if p.m is not None:
                np.testing.assert_array_equal(p.m, q.m)
                np.testing.assert_array_equal(p.v, q.v)


def test_a_monotonic_child_of_a_combined_component(g, hsc):
    """CombinedComponent("add") of a monotonic starlet source and a plain one fits as the two
    sources side by side do"""
    import scarlet_amd as scarlet

    apart, _ = fixture_blend(g, hsc)
    want = apart.fit(9, e_rel=1e-9)
    blend, obs = fixture_blend(g, hsc)
    sources = list(blend.sources)
    pair = scarlet.CombinedComponent(sources[:2], operation="add")
    joint = scarlet.Blend([pair] + sources[2:], obs)
    got = joint.fit(9, e_rel=1e-9)
    assert got == want
    np.testing.assert_array_equal(joint.loss, apart.loss)
    for p, q in zip(apart.parameters, joint.parameters):
        np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
