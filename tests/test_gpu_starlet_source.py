"""Starlet sources on the GPU: the mirror classes against the reference's recorded results, the
starlet kernels (csrc/starlet_source.hip) through the C ABI against the oracle
(tests/starlet_oracle.py), and Blend.fit / fit_blends through the facade.

Tolerances are those of tests/test_gpu_parity.py: RTOL = 1e-5 of the compared array's peak for
forward and gradient; for losses the early 2e-5 / whole 5e-4 / final 1e-5 of
``_whole_fit_against_oracle``."""

import numpy as np
import pytest

from conftest import golden

import starlet_oracle as so

pytestmark = pytest.mark.gpu

RTOL = 1e-5
PATHS = ["fused", "rocfft"]
STARLET_OF = (0, 2)  # made by from_source; the last source is the full-frame random one


@pytest.fixture(scope="module")
def g():
    return golden("starlet_source")


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd

    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# -- builders ---------------------------------------------------------------------------------
def fixture_specs(amd, g):
    starlet = set(int(k) for k in g["starlet_of"])
    specs = []
    for k in range(int(g["n_sources"])):
        kw = dict(sed_min_step=g["sed_step_minimum_%d" % k],
                  sed_rel_step=float(g["sed_step_factor_%d" % k]))
        if float(g["sed_zero_%d" % k]) != 1e-20:
            kw["sed_floor"] = float(g["sed_zero_%d" % k])
        if k in starlet:
            coeffs = g["coeffs_%d" % k]
            specs.append(amd.ComponentSpec(
                g["sed_%d" % k], np.zeros(coeffs.shape[1:]), g["origin_%d" % k], morph_step=1e-2,
                prox_flags=0, starlet=(coeffs, g["thresh_%d" % k]), **kw))
        else:
            specs.append(amd.ComponentSpec(g["sed_%d" % k], g["morph_%d" % k],
                                           g["origin_%d" % k], **kw))
    return specs


def fixture_batch(amd, g, hsc, n_blends=1, **kw):
    specs = [fixture_specs(amd, g) for _ in range(n_blends)]
    return amd.BlendBatch(np.stack([hsc["images"]] * n_blends),
                          np.stack([hsc["weights"]] * n_blends), specs,
                          kernel=hsc["diff_kernel"], **kw)


def fixture_blend(g, hsc, drop=0, scale=1.0):
    """The fixture scene through the facade: sources 0 and 2 by ``from_source``, the
    full-frame ``StarletSource(frame)`` under seed 0 last (``drop``: without that many of the
    plain sources in front of it; ``scale``: all spectra scaled)."""
    import scarlet_amd as scarlet

    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    n = int(g["n_sources"])
    sources = []
    for k in range(n - 1):
        image = g["image_%d" % k] if k in STARLET_OF else g["morph_%d" % k]
        h, w = image.shape
        oy, ox = (int(v) for v in g["origin_%d" % k])
        box = scarlet.Box((5, h, w), origin=(0, oy, ox))
        spectrum = scarlet.TabulatedSpectrum(frame, g["sed_%d" % k].copy() * scale, bbox=box[0],
                                             min_step=g["sed_step_minimum_%d" % k])
        morphology = scarlet.ExtendedSourceMorphology(
            frame, (oy + h // 2, ox + w // 2), image.copy(), bbox=box[1:], monotonic="angle",
            resizing=False)
        src = scarlet.FactorizedComponent(frame, spectrum, morphology)
        sources.append(scarlet.StarletSource.from_source(src) if k in STARLET_OF else src)
    np.random.seed(0)
    diffuse = scarlet.StarletSource(frame)
    diffuse.children[0]._parameters[0][...] *= scale
    plain = [s for k, s in enumerate(sources) if k not in STARLET_OF]
    keep = [s for s in sources if s not in plain[len(plain) - drop:]] if drop else sources
    return scarlet.Blend(keep + [diffuse], obs), obs


def near_a_threshold(comp):
    """Coefficients whose pre-threshold value in the oracle's last proximal evaluation lies
    within RTOL x plane peak of the plane's threshold or of zero: the only ones a comparison
    may leave out."""
    pre = comp.last_pre
    peak = np.abs(pre).max(axis=(1, 2), keepdims=True)
    t = comp.thresh[:, None, None]
    return (np.abs(pre - t) <= RTOL * peak) | (np.abs(pre - comp.floor) <= RTOL * peak)


def assert_coefficients(dev, comp, near, tol, what):
    """Device coefficients against the oracle's: equal supports and values within ``tol`` of
    the parameter's peak, except at coefficients ``near`` a threshold (``near_a_threshold``,
    collected over the iterations), of which at most 1 % may differ.

    The scale of a value's error is the peak of the whole stack, as the parity tests take the
    peak of an image: the stack is ONE parameter (one max(psi), one stopping norm), and a
    plane's own peak is no scale -- the coarse planes of the fixture's compact sources empty
    out within a few iterations (plane peaks 0.04 -> 7e-4 -> 0), so an error of 1e-7 of the
    stack is any multiple of such a plane's peak."""
    ref = comp.morph
    peak = np.abs(ref).max()
    differs = ((dev != 0) != (ref != 0)) | (np.abs(dev - ref) > tol * peak)
    print(what, "near a threshold %.3f%%, differing %d (%.4f%%), worst elsewhere %.3g of the peak"
          % (100 * near.mean(), differs.sum(), 100 * differs.mean(),
             (np.abs(dev - ref) / peak)[~differs].max()))
    assert np.all(near[differs]), (what, int((differs & ~near).sum()))
    assert differs.mean() <= 0.01, (what, differs.mean())


# -- the mirror classes -----------------------------------------------------------------------
def test_mirror_classes_against_the_fixture(g, hsc):
    import scarlet_amd as scarlet

    blend, obs = fixture_blend(g, hsc)
    assert len(blend.sources) == int(g["n_sources"])
    for k in g["starlet_of"]:
        src = blend.sources[int(k)]
        assert type(src) is scarlet.StarletSource
        spectrum, morphology = src.children
        assert type(morphology) is scarlet.StarletMorphology and not morphology.monotonic
        coeffs = morphology.parameters[0]
        assert coeffs.name == "coeffs" and coeffs.step == 1e-2 and coeffs.dtype == np.float64
        np.testing.assert_array_equal(np.asarray(coeffs), g["coeffs_%d" % k])  # bit for bit
        np.testing.assert_array_equal(morphology.transform.norm, g["norm_%d" % k])
        chain = coeffs.constraint
        assert [type(c).__name__ for c in chain.constraints] == list(g["chain_types_%d" % k])
        hard = chain.constraints[1]
        assert hard.type == str(g["l0_type_%d" % k]) and hard.thresh.shape == coeffs.shape
        np.testing.assert_array_equal(hard.thresh[:, 0, 0], g["thresh_%d" % k])
        assert chain.constraints[0].zero == 0
        once = chain(np.asarray(coeffs).copy(), 0)
        np.testing.assert_array_equal(np.packbits((once != 0).ravel()),
                                      g["chain_once_support_%d" % k])
        assert tuple(morphology.bbox.origin) == tuple(g["origin_%d" % k])
        assert tuple(morphology.bbox.shape) == tuple(g["shape_%d" % k])
        sed = spectrum.parameters[0]
        np.testing.assert_array_equal(np.asarray(sed), g["sed_%d" % k])
        assert sed.name == "spectrum" and sed.constraint.zero == float(g["sed_zero_%d" % k])
        assert sed.step.keywords["factor"] == float(g["sed_step_factor_%d" % k])
    # RandomSource under a seed: image over the whole frame first, then the spectrum
    np.random.seed(0)
    image = np.random.rand(*hsc["images"].shape[1:])
    np.random.seed(0)
    rnd = scarlet.RandomSource(blend.sources[-1].frame)
    np.testing.assert_array_equal(np.asarray(rnd.children[1].parameters[0]), image)
    np.testing.assert_array_equal(np.asarray(rnd.children[0].parameters[0]),
                                  g["sed_%d" % (int(g["n_sources"]) - 1)])
    # the model of the mirror is the reference's
    model = blend.get_model()
    assert rel_err(model, g["model"]) < RTOL
    # construction with monotonic planes works (fitting them is refused)
    mono = scarlet.StarletSource.from_source(blend.sources[1], monotonic=True)
    assert type(mono.children[1].parameters[0].constraint) is scarlet.MonotonicMaskConstraint


# -- forward and gradient through the C ABI ---------------------------------------------------
def gradient_scale(sc, comp):
    """peak per plane of the coefficient gradient's magnitude budget: the cascade of
    sum_c |sed_c| |G_c| (what the float32 sums are taken over)"""
    G = np.abs(sc.model_gradient(sc.render(sc.get_model())))
    h, w = comp.morph.shape[-2:]
    boxed = np.zeros((sc.frame_shape[0], h, w))
    fs, bs = sc.box_slices(comp)
    boxed[bs] = G[fs]
    mag = so.cascade(np.einsum("c,cyx->yx", np.abs(comp.sed), boxed), comp.morph.shape[0] - 1)
    return mag.max(axis=(1, 2), keepdims=True)


def check_forward_and_gradient(batch, sc, what):
    model, rendered, logL = batch.forward()
    ref_model = sc.get_model()
    ref_rendered = sc.render(ref_model)
    assert rel_err(model[0], ref_model) < RTOL, what
    assert rel_err(rendered[0], ref_rendered) < RTOL, what
    chi2_ref = -(sc.log_likelihood(ref_rendered) + sc.log_norm)
    assert abs(-(logL[0] + sc.log_norm) - chi2_ref) < RTOL * abs(chi2_ref), what
    g_sed, _ = batch.gradient()
    state = batch.starlet_state()
    _, grads = sc.loss_and_gradients()
    for j, k in enumerate(state["components"]):
        comp = sc.components[k]
        ref = grads[k][1]
        dev = state["gradient"][j]
        assert dev.shape == ref.shape
        peak = np.abs(ref).max(axis=(1, 2), keepdims=True)
        scale = gradient_scale(sc, comp)
        err = np.abs(dev - ref)
        print(what, "component", k, "gradient error / plane peak",
              (err.max(axis=(1, 2)) / peak[:, 0, 0]).max(), "/ magnitude budget",
              (err.max(axis=(1, 2)) / scale[:, 0, 0]).max())
        assert np.all(err <= RTOL * scale), (what, k)
        # the spectrum's gradient uses the reconstructed image like any other morphology
        mm = np.abs(comp.model_morph())
        G = np.abs(sc.model_gradient(sc.render(sc.get_model())))
        boxed = np.zeros((sc.frame_shape[0],) + mm.shape)
        fs, bs = sc.box_slices(comp)
        boxed[bs] = G[fs]
        assert np.abs(g_sed[k] - grads[k][0]).max() < RTOL * np.einsum("cyx,yx->c", boxed, mm).max()


@pytest.mark.parametrize("path", PATHS)
def test_fixture_scene_forward_and_gradient(amd, g, hsc, path):
    batch = fixture_batch(amd, g, hsc, conv_path=path)
    assert batch.conv_path == path
    model, rendered, logL = batch.forward()
    assert rel_err(model[0], g["model"]) < RTOL
    assert rel_err(rendered[0], g["rendered"]) < RTOL
    assert abs(logL[0] - float(g["logL"])) < RTOL * abs(float(g["logL"]))
    check_forward_and_gradient(batch, so.fixture_scene(g, hsc), "fixture/" + path)
    batch.close()


# box shape, origin, frame (H, W): 21^2 (S = 3); a non-square whole frame (S = 4); a box that
# overhangs the frame edge (S = 4); S = 5; and S = 6 on both sides of the regime boundary of
# starlet_source.hip -- work planes in LDS up to 20000 pixels (128^2 = 16384), in global memory
# beyond (150^2 = 22500)
SINGLE = [((21, 21), (5, 7), (40, 48)), ((40, 72), (0, 0), (40, 72)),
          ((41, 41), (-10, 30), (64, 64)), ((64, 80), (3, 5), (70, 90)),
          ((128, 128), (0, 0), (128, 128)), ((150, 150), (0, 0), (150, 150))]


def single_scene(shape, origin, frame, seed=0):
    rng = np.random.default_rng(seed)
    C = 3
    h, w = shape
    yy, xx = np.mgrid[:h, :w]
    image = np.exp(-((yy - h / 2.3) ** 2 + (xx - w / 1.9) ** 2) / (2 * (min(h, w) / 5) ** 2))
    image += 0.05 * rng.random(shape)
    S = so.get_scales(shape)
    coeffs = so.transform(image, S)
    thresh = so.thresholds(shape, 5e-3)
    sed = np.array([1.0, 2.0, 1.5])
    k1 = np.exp(-0.5 * (np.arange(-3, 4) / 1.2) ** 2)
    kernel = (k1[:, None] * k1[None, :] / k1.sum() ** 2)[None].astype(np.float32)
    comp = so.StarletComponent(sed.copy(), coeffs.copy(), origin, thresh,
                               sed_min_step=np.full(C, 1e-3))
    data = np.zeros((C,) + frame, dtype=np.float32)
    weights = (0.5 + rng.random((C,) + frame)).astype(np.float32)
    sc = so.StarletScene((C,) + frame, data, weights, kernel, [comp])
    truth = sc.render(sc.get_model())
    sc.data = (1.3 * truth + 0.05 * rng.standard_normal(truth.shape)).astype(np.float32)
    return sc, S


def single_batch(amd, sc, **kw):
    comp = sc.components[0]
    spec = amd.ComponentSpec(comp.sed, np.zeros(comp.morph.shape[1:]), comp.origin,
                             sed_min_step=comp.sed_min_step, morph_step=1e-2, prox_flags=0,
                             starlet=(comp.morph, comp.thresh))
    return amd.BlendBatch(sc.data[None], sc.weights[None], [[spec]], kernel=sc.kernel, **kw)


@pytest.mark.parametrize("shape,origin,frame", SINGLE)
def test_single_component_scenes(amd, shape, origin, frame):
    sc, S = single_scene(shape, origin, frame)
    assert S == {21: 3, 40: 4, 41: 4, 64: 5, 128: 6, 150: 6}[min(shape)]
    batch = single_batch(amd, sc, max_iter=8)
    what = "%dx%d" % shape
    check_forward_and_gradient(batch, sc, what)
    sc.loss = []
    batch.step(0, 2, e_rel=1e-3)
    comp = sc.components[0]
    left_out = np.zeros(comp.morph.shape, dtype=bool)
    for it in range(2):
        sc.step(it, 1e-3)
        left_out |= near_a_threshold(comp)
    state = batch.starlet_state()
    assert_coefficients(state["coeffs"][0], comp, left_out, 1e-4, what)
    loss = batch.loss_history()[0]
    chi, ref = loss - sc.log_norm, np.array(sc.loss) - sc.log_norm
    assert np.all(np.abs(chi - ref) <= 2e-5 * np.abs(ref)), (chi, ref)
    # what the model uses is the reconstruction of the new coefficients
    morph = batch.parameters()[1][0]
    assert rel_err(morph, so.reconstruct(state["coeffs"][0])) < RTOL
    batch.close()


# -- steps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_it", [1, 2, 12])
def test_fixture_scene_steps(amd, g, hsc, n_it):
    batch = fixture_batch(amd, g, hsc, max_iter=16)
    batch.step(0, n_it, e_rel=1e-3)
    sc = so.fixture_scene(g, hsc)
    left_out = {int(k): np.zeros(g["coeffs_%d" % k].shape, dtype=bool) for k in g["starlet_of"]}
    for it in range(n_it):
        sc.step(it, 1e-3)
        for k, mask in left_out.items():
            mask |= near_a_threshold(sc.components[k])
    loss = batch.loss_history()[0]
    chi, ref = loss - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("steps", n_it, "loss", rel.max())
    assert len(loss) == n_it and rel.max() < 2e-5
    sed, morphs = batch.parameters()
    state = batch.starlet_state()
    tol = RTOL if n_it == 1 else 1e-4  # (test_first_step_exact_structure / test_hsc_steps_vs_oracle)
    for j, k in enumerate(state["components"]):
        comp = sc.components[k]
        what = "steps %d component %d" % (n_it, k)
        assert_coefficients(state["coeffs"][j], comp, left_out[k], tol, what)
        ok = ~left_out[k]
        for name, ref_m in (("m", comp.m_morph), ("v", comp.v_morph), ("vhat", comp.vhat_morph)):
            dev = state[name][j]
            assert np.abs(dev - ref_m)[ok].max() <= 1e-3 * np.abs(ref_m).max(), (what, name)
        assert rel_err(sed[k], comp.sed) < (RTOL if n_it == 1 else 1e-4), what
    for k, comp in enumerate(sc.components):
        if k not in left_out:
            assert np.abs(morphs[k] - comp.morph).max() < (RTOL if n_it == 1 else 1e-4), k
            assert rel_err(sed[k], comp.sed) < (RTOL if n_it == 1 else 1e-4), k
    batch.close()


def test_fixed_coefficients_keep_the_gradient_out_but_not_the_prox(amd, g, hsc):
    from scarlet_amd import _lib

    specs = fixture_specs(amd, g)
    k = int(g["starlet_of"][0])
    specs[k].prox_flags |= _lib.COMPONENT_FIXED_MORPH
    batch = amd.BlendBatch(hsc["images"][None], hsc["weights"][None], [specs],
                           kernel=hsc["diff_kernel"], max_iter=4)
    batch.step(0, 2, e_rel=1e-3)
    sc = so.fixture_scene(g, hsc)
    sc.components[k].fixed = (False, True)
    for it in range(2):
        sc.step(it, 1e-3)
    state = batch.starlet_state()
    dev, ref = state["coeffs"][0], sc.components[k].morph
    # zero gradient: the coefficients only pass through the chain, which is idempotent
    once = sc.components[k].morph_prox(g["coeffs_%d" % k].astype(np.float32).astype(np.float64), 0)
    np.testing.assert_array_equal(dev != 0, ref != 0)
    assert np.abs(dev - once).max() <= 1e-7 * np.abs(once).max()
    assert np.all(state["m"][0] == 0) and np.all(state["v"][0] == 0)
    batch.close()


def test_a_blend_that_has_converged_keeps_its_coefficients(amd, g, hsc):
    """two blends in one batch; the second one's weights are so small that its loss is its
    normalisation term, which does not move: its stopping rule fires at the first chance and
    its coefficients stay as they were while the first blend goes on"""
    specs = [fixture_specs(amd, g) for _ in range(2)]
    batch = amd.BlendBatch(np.stack([hsc["images"]] * 2),
                           np.stack([hsc["weights"], hsc["weights"] * 1e-12]), specs,
                           kernel=hsc["diff_kernel"], max_iter=16)
    batch.step(0, 4, e_rel=1e-6, check_convergence=True)
    states = batch.states()
    assert states[0] == 0 and states[1] == 2
    n_star = len(g["starlet_of"])
    before = [c.copy() for c in batch.starlet_state()["coeffs"][n_star:]]
    first = [c.copy() for c in batch.starlet_state()["coeffs"][:n_star]]
    n_loss = len(batch.loss_history()[1])
    batch.step(4, 6, e_rel=1e-6, check_convergence=True)
    after = batch.starlet_state()["coeffs"]
    for a, b in zip(before, after[n_star:]):
        np.testing.assert_array_equal(a, b)
    assert any(np.any(a != b) for a, b in zip(first, after[:n_star]))
    assert len(batch.loss_history()[1]) == n_loss and len(batch.loss_history()[0]) == 10
    # and the first blend does what it does alone
    alone = fixture_batch(amd, g, hsc, max_iter=16)
    alone.step(0, 10, e_rel=1e-6, check_convergence=True)
    for a, b in zip(alone.starlet_state()["coeffs"], after[:n_star]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(alone.loss_history()[0], batch.loss_history()[0])
    batch.close()
    alone.close()


def test_calls_that_refuse_starlet_components(amd, g, hsc):
    from scarlet_amd import _lib

    batch = fixture_batch(amd, g, hsc, max_iter=4)
    lib = _lib.load()
    with pytest.raises(_lib.ScarletAmdError, match="starlet"):
        batch.set_frame_extents([(50, 40)])
    with pytest.raises(_lib.ScarletAmdError, match="starlet"):
        batch.set_iteration_base([0])
    with pytest.raises(_lib.ScarletAmdError, match="starlet|factorized image"):
        batch.component_states([0])
    with pytest.raises(_lib.ScarletAmdError, match="starlet"):
        _lib.check(lib.smi_batch_save_state(batch._h))
    with pytest.raises(_lib.ScarletAmdError, match="starlet"):
        batch.update_components([fixture_specs(amd, g)], np.ones(batch.n_components, np.int32), [])
    batch.close()
    with pytest.raises(_lib.ScarletAmdError, match="starlet|FISTA"):
        specs = fixture_specs(amd, g)
        for s in specs:
            s.fista_step = 1.0
        amd.BlendBatch(hsc["images"][None], hsc["weights"][None], [specs],
                       kernel=hsc["diff_kernel"], scheme="fista")


# -- the facade -------------------------------------------------------------------------------
def test_blend_fit_follows_the_oracle(g, hsc):
    """A whole ``Blend.fit(100, e_rel=1e-4)`` of the fixture scene against ``StarletScene.fit``:
    iteration count, loss history (early 2e-5 / whole 5e-4 / final 1e-5) and the final
    coefficients (1e-3 of the plane peak: ten times the bound the parity tests put on images
    after five iterations, for twenty times as many)."""
    blend, obs = fixture_blend(g, hsc)
    n, logL = blend.fit(100, e_rel=1e-4)
    sc = so.fixture_scene(g, hsc)
    left_out = {int(k): np.zeros(g["coeffs_%d" % k].shape, dtype=bool) for k in g["starlet_of"]}
    orig_step = sc.step

    def step(it, *a, **kw):
        orig_step(it, *a, **kw)
        for k, mask in left_out.items():
            if sc.components[k].morph.shape == mask.shape:
                mask |= near_a_threshold(sc.components[k])

    sc.step = step
    for k, comp in enumerate(sc.components):
        comp.resizing = k in left_out  # (the plain sources were built with resizing=False)
    n_ref, _ = sc.fit(100, e_rel=1e-4, resizing=True)
    chi, ref = np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm
    assert n == len(blend.loss) == n_ref, (n, n_ref)
    rel = np.abs(chi - ref) / np.abs(ref)
    print("whole fit:", n, "iterations, loss early %.3g whole %.3g final %.3g"
          % (rel[:12].max(), rel.max(), rel[-1]))
    assert rel[:12].max() < 2e-5 and rel.max() < 5e-4 and rel[-1] < 1e-5
    assert blend.loss[-1] < blend.loss[0] and logL == -blend.loss[-1]
    for k in left_out:
        coeffs = blend.sources[k].children[1].parameters[0]
        assert coeffs.m.shape == coeffs.v.shape == coeffs.vhat.shape == coeffs.shape
        assert coeffs.std.shape == coeffs.shape and coeffs.dtype == np.float64
        assert_coefficients(np.asarray(coeffs), sc.components[k], left_out[k], 1e-3,
                            "whole fit component %d" % k)


def test_refusals_through_the_facade(g, hsc):
    import scarlet_amd as scarlet
    from scarlet_amd import _lib

    uploads = _lib.load().smi_observation_uploads()

    def blend_with(change):
        blend, _ = fixture_blend(g, hsc)
        change(blend.sources[0])
        return blend

    def monotonic(src):
        src.children[1].monotonic = True

    def with_prior(src):
        class Flat(scarlet.Prior):
            def __call__(self, x):
                return 0.0

            def grad(self, x):
                return np.zeros_like(x)

        src.children[1].parameters[0].prior = Flat()

    def with_callable(src):
        src.children[1].parameters[0].step = lambda x, it=0: 1e-2

    def other_constraint(src):
        src.children[1].parameters[0].constraint = scarlet.PositivityConstraint(0)

    for change in (monotonic, with_prior, with_callable, other_constraint):
        with pytest.raises(NotImplementedError):
            blend_with(change).fit(5)
    with pytest.raises(NotImplementedError):
        fixture_blend(g, hsc)[0].fit(5, scheme="adam")
    assert _lib.load().smi_observation_uploads() == uploads  # refused before any device work


def _shrunk(parameter, inset, size):
    """the Parameter of a (planes, h, w) stack cut to the centred (size, size) box"""
    import scarlet_amd as scarlet
    from scarlet_amd.morphology import plane_thresholds

    sl = (slice(None), slice(inset, inset + size), slice(inset, inset + size))
    floor, per_plane = plane_thresholds(parameter.constraint)
    chain = scarlet.ConstraintChain(
        scarlet.PositivityConstraint(floor),
        scarlet.L0Constraint(np.broadcast_to(per_plane[:, None, None],
                                             (len(per_plane), size, size)).copy()))
    return scarlet.Parameter(np.asarray(parameter)[sl].copy(), name="coeffs", constraint=chain,
                             step=parameter.step, m=parameter.m[sl].copy(),
                             v=parameter.v[sl].copy(), vhat=parameter.vhat[sl].copy())


def test_the_update_hook_and_the_restart_after_a_shrink(g, hsc):
    import scarlet_amd as scarlet

    blend, _ = fixture_blend(g, hsc)
    src = blend.sources[2]
    morphology = src.children[1]
    coeffs = morphology.parameters[0]
    assert coeffs.shape == (5, 41, 41)
    # a non-empty border (the coarse plane lit everywhere): nothing happens
    keep = np.asarray(coeffs).copy()
    coeffs[...] = 0
    coeffs[-1] = 1.0
    morphology.update()
    assert morphology.bbox.shape == (41, 41) and morphology.parameters[0] is coeffs
    # plane 0 non-zero in the central 11^2 only: the reconstruction is that plane, the box
    # shrinks to the standard size 21 with sliced coefficients and moments
    hand = np.zeros_like(keep)
    hand[0, 15:26, 15:26] = 1 + np.arange(121).reshape(11, 11)
    coeffs[...] = hand
    coeffs.m, coeffs.v, coeffs.vhat = (np.arange(hand.size, dtype=float).reshape(hand.shape) + i
                                       for i in range(3))
    origin = tuple(morphology.bbox.origin)
    with pytest.raises(scarlet.UpdateException):
        morphology.update()
    new = morphology.parameters[0]
    assert morphology.bbox.shape == (21, 21)
    assert tuple(morphology.bbox.origin) == tuple(o + 10 for o in origin)
    np.testing.assert_array_equal(np.asarray(new), hand[:, 10:31, 10:31])
    for i, name in enumerate(("m", "v", "vhat")):
        want = (np.arange(hand.size, dtype=float).reshape(hand.shape) + i)[:, 10:31, 10:31]
        np.testing.assert_array_equal(getattr(new, name), want)
    assert new.shape[0] == 5 and new.step == coeffs.step and new.name == "coeffs"
    from scarlet_amd.morphology import plane_thresholds
    np.testing.assert_array_equal(plane_thresholds(new.constraint)[1], g["thresh_2"])
    assert new.constraint.constraints[1].thresh.shape == new.shape  # (the reference's fails here)
    # a fixed parameter is left alone
    new.fixed = True
    morphology.update()

    # the restart path: fit(10), the shrink made by hand on both sides, fit(10) again = the
    # oracle continued from the sliced state with its counter at 0
    blend, _ = fixture_blend(g, hsc)
    blend.fit(10, e_rel=1e-9)
    sc = so.fixture_scene(g, hsc)
    for it in range(10):
        sc.step(it, 1e-9)
    src = blend.sources[2]
    morphology = src.children[1]
    morphology._parameters = (_shrunk(morphology.parameters[0], 5, 31),)
    morphology.bbox.origin = tuple(o + 5 for o in morphology.bbox.origin)
    morphology.bbox.shape = (31, 31)
    src.bbox = src._joint_box(*src.children)
    comp = sc.components[2]
    sl = (slice(None), slice(5, 36), slice(5, 36))
    comp.origin = (comp.origin[0] + 5, comp.origin[1] + 5)
    comp.morph = comp.morph[sl].copy()
    comp.m_morph, comp.v_morph, comp.vhat_morph = (a[sl].copy() for a in (
        comp.m_morph, comp.v_morph, comp.vhat_morph))
    blend.fit(10, e_rel=1e-9)
    left_out = np.zeros(comp.morph.shape, dtype=bool)
    for it in range(10):
        sc.step(it, 1e-9)
        left_out |= near_a_threshold(comp)
    assert len(blend.loss) == 20
    chi, ref = np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("restart: loss", rel.max())
    assert rel.max() < 2e-5
    assert_coefficients(np.asarray(morphology.parameters[0]), comp, left_out, 1e-4, "restart")
    assert rel_err(morphology.parameters[0].v, comp.v_morph) < 1e-3


def test_fit_blends_equals_the_single_fits(g, hsc):
    import scarlet_amd as scarlet

    def make(k):
        return fixture_blend(g, hsc, drop=k, scale=1 + 0.1 * k)[0]

    single = [make(k) for k in range(2)]
    want = [b.fit(25, e_rel=1e-5) for b in single]
    many = [make(k) for k in range(2)]
    got = scarlet.fit_blends(many, 25, e_rel=1e-5)
    for a, b, r1, r2 in zip(single, many, want, got):
        assert r1 == r2
        np.testing.assert_array_equal(a.loss, b.loss)
        for p, q in zip(a.parameters, b.parameters):
            assert p.shape == q.shape
            np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
            if p.m is not None:
                np.testing.assert_array_equal(p.m, q.m)


def scene_of(blend, obs):
    """``StarletScene`` of a facade blend of factorized sources on one observation of the
    model frame: the oracle "built from the same sources" """
    import scarlet_amd as scarlet
    from oracle import pgm

    comps = []
    for src in blend.sources:
        spectrum, morphology = src.children
        sed, par = spectrum.parameters[0], morphology.parameters[0]
        kw = dict(sed_min_step=np.asarray(sed.step.keywords.get("minimum", 0), dtype=np.float64),
                  sed_zero=sed.constraint.zero)
        origin = morphology.bbox.origin[-2:]
        if isinstance(morphology, scarlet.StarletMorphology):
            thresh = par.constraint.constraints[1].thresh[:, 0, 0]
            comps.append(so.StarletComponent(
                np.asarray(sed).copy(), np.asarray(par).copy(), origin, thresh,
                sed_rel_step=sed.step.keywords["factor"], coeffs_step=par.step, **kw))
        else:
            comps.append(pgm.Component(np.asarray(sed).copy(), np.asarray(par).copy(), origin, **kw))
    data = np.asarray(obs.data, dtype=np.float32)
    weights = np.broadcast_to(np.asarray(obs.weights, dtype=np.float32), data.shape).copy()
    kernel = np.asarray(obs.renderer.diff_kernel.image, dtype=np.float32)
    return so.StarletScene(data.shape, data, weights, kernel, comps)


def test_the_wavelet_tutorial_end_to_end():
    """docs/tutorials/wavelet_model.ipynb from ``lsbg.npz``: the repository's detection as in the
    notebook, ``init_all_sources(max_components=1, min_snr=50, set_spectra=False)``, seed 0,
    ``StarletSource(model_frame)``, ``fit(200, e_rel=1e-6)``."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import wavelet_tutorial

    blend, obs = wavelet_tutorial.build()
    diffuse = blend.sources[-1]
    coeffs = diffuse.children[1].parameters[0]
    assert coeffs.shape == (7, 191, 191) and len(blend.sources) > 2
    sc = scene_of(blend, obs)
    n, logL = blend.fit(200, e_rel=1e-6)
    assert n == len(blend.loss) and np.all(np.isfinite(blend.loss)) and np.isfinite(logL)
    assert all(p.is_finite for p in blend.parameters)
    assert blend.loss[-1] < blend.loss[0]
    assert np.abs(diffuse.get_model()).max() > 0
    sc.fit(12, e_rel=1e-6, resizing=True)
    chi, ref = np.array(blend.loss[:12]) - sc.log_norm, np.array(sc.loss) - sc.log_norm
    rel = np.abs(chi - ref) / np.abs(ref)
    print("tutorial: %d iterations, logL %.1f -> %.1f, first 12 losses within %.3g"
          % (n, -blend.loss[0], logL, rel.max()))
    assert rel.max() < 2e-5
