"""The reference-style Python API end to end on the GPU: Frame / Observation.match /
FactorizedComponent / Blend.fit, against the oracle on the quickstart scene
(initial sources taken from the golden fixture, since source initialisation is
set-up code outside the loop)."""

import numpy as np
import pytest
from numpy.testing import assert_allclose

from conftest import hsc_scene

RTOL = 1e-5  # north_star: 1e-5 relative in float32

pytestmark = pytest.mark.gpu


def build_blend(hsc, resizing, shifting=False):
    import scarlet_amd as scarlet

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame(hsc["images"].shape, psf=model_psf, channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    groups = {}
    for k in range(int(hsc["n_comp"])):
        h, w = hsc["morph_%d" % k].shape
        oy, ox = hsc["origin_%d" % k]
        box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
        spectrum = scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                             min_step=hsc["min_step_%d" % k])
        center = (oy + h // 2, ox + w // 2)
        morphology = scarlet.ExtendedSourceMorphology(
            frame, center, hsc["morph_%d" % k].copy(), bbox=box[1:], monotonic="angle",
            resizing=resizing, shifting=shifting)
        comp = scarlet.FactorizedComponent(frame, spectrum, morphology)
        groups.setdefault(int(hsc["source_of"][k]), []).append(comp)
    sources = [g[0] if len(g) == 1 else scarlet.CombinedComponent(g) for g in groups.values()]
    return scarlet.Blend(sources, obs), obs


def components_of(blend):
    import scarlet_amd as scarlet

    out = []
    for src in blend.sources:
        out += [src] if isinstance(src, scarlet.FactorizedComponent) else list(src.children)
    return out


def test_render_and_loglikelihood_api(hsc):
    blend, obs = build_blend(hsc, resizing=False)
    model = blend.get_model()
    np.testing.assert_array_equal(model, hsc["model"])
    rendered = obs.render(model)
    assert np.abs(rendered - hsc["rendered"]).max() < 1e-5 * np.abs(hsc["rendered"]).max()
    assert_allclose(obs.get_log_likelihood(model), float(hsc["logL"]), rtol=1e-6)


def test_blend_fit_matches_oracle(hsc):
    blend, obs = build_blend(hsc, resizing=False)
    n, logL = blend.fit(40, e_rel=1e-4)
    sc = hsc_scene(hsc)
    n_ref, logL_ref = sc.fit(40, e_rel=1e-4)
    # bounds measured on MI355X, see test_hsc_fit_follows_the_oracle_for_all_iterations:
    # the same iterations, 8e-6 at the start, a transient of ~2e-4 around iteration 25
    assert n == len(blend.loss) == n_ref
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    assert_allclose(chi[:12], chi_ref[:12], rtol=2e-5)
    assert_allclose(chi, chi_ref, rtol=5e-4)
    assert_allclose(blend.log_likelihood[-1], logL)
    # side effects the reference promises (blend.py:153-163, 189-192)
    for p in blend.parameters:
        if p.name == "shift":
            continue
        assert p.m is not None and p.v.shape == p.shape and p.std.shape == p.shape
    for comp in components_of(blend):
        image = comp.children[1].parameters[0]
        assert image.max() == 1.0 and image.min() >= 0
    # warm start: a second call continues from the stored moments
    n2, logL2 = blend.fit(5, e_rel=1e-9)
    assert n2 == n + 5 and logL2 >= logL - 1e-3 * abs(logL)


def test_blend_fit_with_resizing_matches_oracle(hsc):
    blend, obs = build_blend(hsc, resizing=True)
    n, logL = blend.fit(45, e_rel=1e-5)
    sc = hsc_scene(hsc)
    n_ref, logL_ref = sc.fit(45, e_rel=1e-5, resizing=True)
    assert n == n_ref == 45
    comps = components_of(blend)
    # the same boxes were resized to the same shapes / origins
    for comp, c in zip(comps, sc.components):
        assert comp.children[1].parameters[0].shape == c.morph.shape
        assert tuple(comp.children[1].bbox.origin) == tuple(c.origin)
    assert any(c.morph.shape != hsc["morph_%d" % k].shape for k, c in enumerate(sc.components))
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    # measured: 9e-5 over the first 25 iterations, 1.9e-4 at most (iteration 29, after
    # the restarts), 8e-6 at the end
    assert_allclose(chi, chi_ref, rtol=5e-4)
    assert abs(chi[-1] - chi_ref[-1]) < 3e-5 * abs(chi_ref[-1])


def test_blend_fit_callback_host_stepped(hsc):
    """``callback=`` (reference blend.py:168,301-302): same trajectory as the device
    loop, called once per non-terminal iteration with the live parameters;
    StopIteration from the callback ends the fit cleanly."""
    blend, _ = build_blend(hsc, resizing=True)
    n_ref, logL_ref = blend.fit(25, e_rel=1e-5)
    loss_ref = list(blend.loss)

    blend2, _ = build_blend(hsc, resizing=True)
    seen = []

    def cb(*params, it=None):
        assert len(params) == len(blend2.parameters)
        seen.append((it, float(np.asarray(params[0]).sum())))

    n, logL = blend2.fit(25, e_rel=1e-5, callback=cb)
    assert n == n_ref and logL == logL_ref
    assert_allclose(blend2.loss, loss_ref, rtol=0, atol=0)
    # adaprox's counter restarts after every resize; one call per iteration otherwise
    assert seen[0][0] == 0 and len(seen) >= n - 3
    assert len({v for _, v in seen}) > 1  # parameters are live, not the initial ones

    blend3, _ = build_blend(hsc, resizing=False)

    def stop(*params, it=None):
        if it == 4:
            raise StopIteration

    n3, _ = blend3.fit(25, e_rel=1e-5, callback=stop)
    assert n3 == 5


def test_quickstart_initialisation_matches_reference(hsc):
    """docs/0-quickstart.ipynb / testing/deblend.py sequence: init_all_sources on the
    bundled HSC scene reproduces the reference's initial sources (golden), then fits."""
    import scarlet_amd as scarlet
    from scarlet_amd.initialization import init_all_sources

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame(hsc["images"].shape, psf=model_psf, channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    centers = [tuple(c) for c in hsc["centers"]]
    sources, skipped = init_all_sources(frame, centers, obs, max_components=2, min_snr=50,
                                        thresh=1, fallback=True, silent=True, set_spectra=True)
    assert len(skipped) == int(hsc["n_skipped"])
    blend = scarlet.Blend(sources, obs)
    comps = components_of(blend)
    assert len(comps) == int(hsc["n_comp"])
    for k, comp in enumerate(comps):
        sed = np.asarray(comp.children[0].parameters[0])
        morph = np.asarray(comp.children[1].parameters[0])
        assert morph.shape == hsc["morph_%d" % k].shape
        assert tuple(comp.children[1].bbox.origin) == tuple(hsc["origin_%d" % k])
        assert np.abs(morph - hsc["morph_%d" % k]).max() < 1e-5
        # (the least squares of set_spectra_to_match is solved in double on double renders,
        # like the reference: its normal matrices have condition numbers of 250 .. 700)
        assert np.abs(sed - hsc["sed_%d" % k]).max() < 2e-5 * np.abs(hsc["sed_%d" % k]).max()
    model = blend.get_model()
    assert np.abs(model - hsc["model"]).max() < 2e-5 * np.abs(hsc["model"]).max()
    logL0 = obs.get_log_likelihood(model)
    assert abs(logL0 - float(hsc["logL"])) < 1e-5 * abs(float(hsc["logL"]))
    n, logL = blend.fit(100, e_rel=1e-4)
    assert logL > logL0 and n <= 100


def test_initialisation_sweeps_all_detection_images_in_one_launch(hsc, monkeypatch):
    """``init_all_sources`` prepares every source's detection image -- coadd, symmetrised,
    monotonic about the source's pixel -- ahead of the loop over the sources with ONE call of
    the many-image sweep and no per-source sweep, and gives exactly the sources of the
    per-source path (``ExtendedSource`` built one by one)."""
    import scarlet_amd as scarlet
    from scarlet_amd import initialization, operator

    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5), channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    centers = [tuple(c) for c in hsc["centers"]]
    calls = {"many": 0, "one": 0}
    many, one = operator.prox_weighted_monotonic_many, operator._native_sweep

    def count_many(*a, **k):
        calls["many"] += 1
        return many(*a, **k)

    def count_one(*a, **k):
        calls["one"] += 1
        return one(*a, **k)

    monkeypatch.setattr(operator, "prox_weighted_monotonic_many", count_many)
    monkeypatch.setattr(operator, "_native_sweep", count_one)
    kw = dict(max_components=2, min_snr=50, thresh=1, fallback=True, silent=True, set_spectra=False)
    batched, _ = initialization.init_all_sources(frame, centers, obs, **kw)
    assert calls == {"many": 1, "one": 0} and not initialization._prepared
    single = [initialization.init_source(frame, c, obs, thresh=1, max_components=2, min_snr=50)
              for c in centers]
    assert calls["many"] == 1 and calls["one"] >= len(centers)
    for a, b in zip(components_of(scarlet.Blend(batched, obs)), components_of(scarlet.Blend(single, obs))):
        assert a.children[1].bbox == b.children[1].bbox
        for p, q in zip(a.parameters, b.parameters):
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)


def test_initialisation_sweeps_windows_about_the_sources_and_gives_the_same_sources(monkeypatch):
    """On a frame much larger than the sources (the benchmark's 128^2 scenes) the prepared
    sweep runs in a 65^2 window about every source's pixel (initialization.SWEEP_WINDOW): the
    result inside is the full frame's bit for bit and what lies outside is below the trimming
    threshold, so the sources equal those of the per-source path (whole-frame sweeps) exactly.
    With a window of 7^2 pixels the rim lies inside the sources and fails the test: those
    centres are swept whole, in a second launch, with the same sources again."""
    import scarlet_amd as scarlet
    from scarlet_amd import initialization, operator, synthetic

    kern = synthetic.psfs()
    channels = list("grizy")
    many = operator.prox_weighted_monotonic_many
    for seed in (1234, 1237):
        s = synthetic.make_blend(seed, kernel=kern)
        frame = scarlet.Frame((5, synthetic.H, synthetic.W),
                              psf=scarlet.GaussianPSF(sigma=(synthetic.SIGMA_MODEL,) * 5), channels=channels)
        obs = scarlet.Observation(s["data"], psf=scarlet.ImagePSF(np.repeat(kern[0], 5, axis=0)),
                                  weights=s["weights"], channels=channels).match(frame)
        centers = [(float(o[0] + m.shape[0] // 2), float(o[1] + m.shape[1] // 2))
                   for o, m in zip(s["origins"], s["morphs"])]
        for thresh, half in ((1, 32), (1, 3)):
            monkeypatch.setattr(initialization, "SWEEP_WINDOW", half)
            shapes = []

            def record(images, *a, **k):
                shapes.append(images.shape)
                return many(images, *a, **k)

            monkeypatch.setattr(operator, "prox_weighted_monotonic_many", record)
            batched, _ = initialization.init_all_sources(frame, centers, obs, max_components=1,
                                                         min_snr=50, thresh=thresh, silent=True,
                                                         set_spectra=False)
            monkeypatch.setattr(operator, "prox_weighted_monotonic_many", many)
            side = 2 * initialization.SWEEP_WINDOW + 1
            assert shapes and all(max(sh[1:]) <= side for sh in shapes if sh[1:] != (synthetic.H, synthetic.W))
            whole = sum(sh[0] for sh in shapes if sh[1:] == (synthetic.H, synthetic.W))
            if half == 32:
                assert whole < len(centers), "no source of the scene was served by its window"
            else:
                assert whole == len(centers)
            # the sources one by one: through the same window logic, and swept whole
            one_by_one = [initialization.init_source(frame, c, obs, thresh=thresh, max_components=1,
                                                     min_snr=50) for c in centers]
            with monkeypatch.context() as m:
                m.setattr(initialization, "sweep_in_window", lambda *a, **k: None)
                whole_frame = [initialization.init_source(frame, c, obs, thresh=thresh,
                                                          max_components=1, min_snr=50) for c in centers]
            b_comps = components_of(scarlet.Blend(whole_frame, obs))
            for other in (batched, one_by_one):
                a_comps = components_of(scarlet.Blend(other, obs))
                assert len(a_comps) == len(b_comps)
                for a, b in zip(a_comps, b_comps):
                    assert a.children[1].bbox == b.children[1].bbox
                    for p, q in zip(a.parameters, b.parameters):
                        assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)


def test_two_observations_equal_one(hsc):
    """the same scene observed as (g,r,i) and (z,y) by two Observations gives the same
    fit as the single 5-band Observation (loss summed over observations, blend.py:265-271)"""
    import scarlet_amd as scarlet

    blend1, _ = build_blend(hsc, resizing=False)
    n1, logL1 = blend1.fit(12, e_rel=1e-6)

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame(hsc["images"].shape, psf=model_psf, channels=filters)
    obs_a = scarlet.Observation(hsc["images"][:3], psf=scarlet.ImagePSF(hsc["psfs"][:3].copy()),
                                weights=hsc["weights"][:3], channels=filters[:3]).match(frame)
    obs_b = scarlet.Observation(hsc["images"][3:], psf=scarlet.ImagePSF(hsc["psfs"][3:].copy()),
                                weights=hsc["weights"][3:], channels=filters[3:]).match(frame)
    assert obs_a.renderer.channel_map == slice(0, 3) and obs_b.renderer.channel_map == slice(3, 5)
    blend2, _ = build_blend(hsc, resizing=False)
    blend2.observations = (obs_a, obs_b)
    n2, logL2 = blend2.fit(12, e_rel=1e-6)
    assert n1 == n2 == 12
    assert_allclose(np.array(blend2.loss), np.array(blend1.loss), rtol=1e-6)
    for p1, p2 in zip(blend1.parameters, blend2.parameters):
        assert_allclose(np.asarray(p2), np.asarray(p1), rtol=1e-5, atol=1e-7)


def test_fit_forwards_adam_constants(hsc):
    """Blend.fit(**alg_kwargs): b1, b2, eps reach the device optimizer (blend.py:165-180)"""
    blend, obs = build_blend(hsc, resizing=False)
    n, logL = blend.fit(8, e_rel=1e-9, b1=0.8, b2=0.99, eps=1e-6)
    sc = hsc_scene(hsc)
    n_ref, logL_ref = sc.fit(8, e_rel=1e-9, b1=0.8, b2=0.99, eps=1e-6)
    assert n == n_ref == 8
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=2e-4)
    default, _ = build_blend(hsc, resizing=False)
    default.fit(8, e_rel=1e-9)
    assert abs(default.loss[-1] - blend.loss[-1]) > 1e-3 * abs(blend.loss[-1] - sc.log_norm)
    with pytest.raises(ValueError):
        blend.fit(2, scheme="sgd")  # not a scheme of proxmin.adaprox
    with pytest.raises(NotImplementedError):
        blend.fit(2, no_such_option=1)


@pytest.mark.parametrize("scene", ["point_source", "point_source_moffat", "point_source_image",
                                   "point_source_bands"])
def test_point_source_tutorial_scene(scene):
    """docs/tutorials/point_source.ipynb through the facade: PointSource /
    ExtendedSource initialisation reproduces the reference's sources (golden), the
    fit follows the oracle (centres of the stars are free parameters); also on a MoffatPSF
    model PSF (source.py:92-128 takes any ``frame.psf``)."""
    import scarlet_amd as scarlet
    from conftest import golden, point_scene

    g = golden(scene)
    images = g["images"]
    filters = list("ugrizy")
    model_psf = scarlet.GaussianPSF(sigma=0.9) if "moffat" not in g else \
        scarlet.MoffatPSF(alpha=g["moffat"][0], beta=g["moffat"][1], boxsize=15)
    if "psf_image" in g:
        model_psf = scarlet.ImagePSF(g["psf_image"].copy())
    frame = scarlet.Frame(images.shape, psf=model_psf, channels=filters)
    obs = scarlet.Observation(images, psf=scarlet.ImagePSF(g["psfs"].copy()),
                              weights=np.ones_like(images) / 4, channels=filters).match(frame)
    sources = []
    for k in range(int(g["n_src"])):
        cls = scarlet.PointSource if g["is_star"][k] else scarlet.ExtendedSource
        sources.append(cls(frame, tuple(g["sky"][k]), obs))
    for k, src in enumerate(sources):
        spectrum, morphology = src.children
        assert tuple(morphology.bbox.origin[-2:]) == tuple(g["origin_%d" % k])
        assert_allclose(np.asarray(spectrum.parameters[0]), g["sed_%d" % k], rtol=2e-5)
        if g["is_star"][k]:
            assert_allclose(np.asarray(morphology.parameters[0]), g["center_%d" % k], rtol=0, atol=0)
            want = g["morph_%d" % k]  # (a cube on a model PSF that differs between the bands)
            got = morphology.get_model()
            assert_allclose(got if want.ndim == 3 else got[0], want, rtol=0, atol=1e-15)
        else:
            assert np.abs(np.asarray(morphology.parameters[0]) - g["morph_%d" % k]).max() < 1e-5
    blend = scarlet.Blend(sources, obs)
    model = blend.get_model()
    assert np.abs(model - g["model"]).max() < 2e-5 * np.abs(g["model"]).max()
    assert abs(obs.get_log_likelihood(model) - float(g["logL"])) < 1e-4 * abs(float(g["logL"]))

    n, logL = blend.fit(35, e_rel=1e-6)
    if scene == "point_source_bands":
        # a device component is a spectrum x ONE image: each star is fitted as one stand-in per
        # band, its spectrum and centre stepped on the host (hoststep.HostBandSource)
        assert [hp.kind for _, hp in blend._host] == ["band"] * int(np.sum(g["is_star"]))
    sc = point_scene(g)
    n_ref, logL_ref = sc.fit(35, e_rel=1e-6, resizing=True)
    assert n == n_ref == 35
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    assert_allclose(chi[:20], chi_ref[:20], rtol=1e-3)
    assert abs(chi[-1] - chi_ref[-1]) < 1e-2 * abs(chi_ref[-1])
    for src, c in zip(sources, sc.components):
        if isinstance(src, scarlet.PointSource):
            center = src.children[1].parameters[0]
            assert np.abs(np.asarray(center) - c.center).max() < 5e-3
            assert center.m is not None and center.std.shape == (2,)
            assert src.center is center
        else:
            assert src.children[1].parameters[0].shape == c.morph.shape
    assert logL > float(g["logL"])



def test_priors_constraints_and_step_callables_on_free_2_vectors(hsc):
    """A free 2-vector is a ``Parameter`` like any other (blend.py:120-145): a prior, a
    constraint or a step callable on a point source's centre, on the Fourier shift of an
    extended source or on a renderer's ``psf_shift`` is taken by the host from the device's
    gradient (hoststep.HostVector; rounds 1 - 5 refused them).  Each against the oracle with the
    same rule, step by step; a rule that changes nothing reproduces the device's own step."""
    import scarlet_amd as scarlet
    from scarlet_amd.initialization import init_all_sources
    from scarlet_amd.renderer import ConvolutionRenderer
    from conftest import golden, point_scene, shifting_scene

    class Pull(scarlet.Prior):
        """gradient of a quadratic well about ``x0`` (what the reference adds to the
        likelihood's gradient is whatever ``prior(x)`` returns, blend.py:120-131)"""
        def __init__(self, x0, k):
            self.x0, self.k = np.array(x0, dtype=float), k

        def __call__(self, x):
            return self.k * (np.asarray(x) - self.x0)

        def grad(self, x):
            return self(x)

    class Within(scarlet.Constraint):
        def __init__(self, x0, r):
            self.x0, self.r = np.array(x0, dtype=float), r

        def __call__(self, X, step):
            X[...] = np.clip(X, self.x0 - self.r, self.x0 + self.r)
            return X

    def halving(X, it=0):
        return 0.05 / (1 + it // 3)

    # -- point sources: constraint + step callable on one centre, a prior on another
    g = golden("point_source")
    images = g["images"]
    filters = list("ugrizy")
    frame = scarlet.Frame(images.shape, psf=scarlet.GaussianPSF(sigma=0.9), channels=filters)
    obs = scarlet.Observation(images, psf=scarlet.ImagePSF(g["psfs"].copy()),
                              weights=np.ones_like(images) / 4, channels=filters).match(frame)

    def sources_of():
        out = []
        for k in range(int(g["n_src"])):
            cls = scarlet.PointSource if g["is_star"][k] else scarlet.ExtendedSource
            out.append(cls(frame, tuple(g["sky"][k]), obs))
        return out

    stars = [k for k in range(int(g["n_src"])) if g["is_star"][k]]
    assert len(stars) >= 2
    sources = sources_of()
    c0 = np.array(sources[stars[0]].children[1].parameters[0])
    c1 = np.array(sources[stars[1]].children[1].parameters[0])
    p0 = sources[stars[0]].children[1].parameters[0]
    p0.constraint, p0.step = Within(c0, 0.02), halving
    sources[stars[1]].children[1].parameters[0].prior = Pull(c1 + 0.3, 50.0)
    blend = scarlet.Blend(sources, obs)
    n, _ = blend.fit(9, e_rel=1e-6)
    assert sorted(k for k, hp in blend._host if hp.kind == "vec") == stars[:2]
    sc = point_scene(g)
    sc.components[stars[0]].vec_rules = {"center": dict(
        prox=lambda x, step: np.clip(x, c0 - 0.02, c0 + 0.02), step=halving)}
    sc.components[stars[1]].vec_rules = {"center": dict(prior=lambda x: 50.0 * (x - (c1 + 0.3)))}
    n_ref, _ = sc.fit(9, e_rel=1e-6)
    assert n == n_ref == 9
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=1e-4)
    for k in stars[:2]:
        center = sources[k].children[1].parameters[0]
        assert np.abs(np.asarray(center) - sc.components[k].center).max() < 1e-5
        assert center.m is not None and center.std.shape == (2,)
    assert np.abs(np.asarray(p0) - c0).max() <= 0.02 + 1e-12  # the constraint held ...
    plain = sources_of()
    scarlet.Blend(plain, obs).fit(9, e_rel=1e-6)
    assert np.abs(np.asarray(plain[stars[0]].children[1].parameters[0]) - c0).max() > 0.02  # ... and bit
    # a step callable that returns the default step: the host's step is the device's (from the
    # gradient of a separate float32 evaluation: to float32 rounding)
    same = sources_of()
    for k in stars:
        same[k].children[1].parameters[0].step = lambda X, it=0: 3e-2
    scarlet.Blend(same, obs).fit(9, e_rel=1e-6)
    for k in stars:
        assert np.abs(np.asarray(same[k].children[1].parameters[0])
                      - np.asarray(plain[k].children[1].parameters[0])).max() < 2e-5

    # the spectrum of a point source is a spectrum like any other: a prior on it (here one that
    # adds nothing) sends it to the host, which reproduces the device's spectrum step
    flat = sources_of()
    for k in stars:
        flat[k].children[0].parameters[0].prior = Pull(0.0, 0.0)
    with_prior = scarlet.Blend(flat, obs)
    with_prior.fit(9, e_rel=1e-6)
    assert sorted(k for k, hp in with_prior._host if hp.kind == "sed") == stars
    for k in stars:
        assert_allclose(np.asarray(flat[k].children[0].parameters[0]),
                        np.asarray(plain[k].children[0].parameters[0]), rtol=2e-5)

    # -- the Fourier shift of an extended source under a prior
    gs = golden("hsc_shifting")
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5), channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    srcs, _ = init_all_sources(frame, [tuple(c) for c in gs["centers"]], obs, max_components=2,
                               min_snr=50, thresh=1, fallback=True, silent=True, set_spectra=True,
                               shifting=True)
    blend = scarlet.Blend(srcs, obs)
    comps = components_of(blend)
    for comp in comps:
        comp.children[1].resizing = False
    s0 = np.array(comps[0].children[1].parameters[1])
    comps[0].children[1].parameters[1].prior = Pull(s0 - 0.2, 2000.0)
    n, _ = blend.fit(7, e_rel=1e-6)
    sc = shifting_scene(gs, hsc)
    sc.components[0].vec_rules = {"shift": dict(prior=lambda x: 2000.0 * (x - (s0 - 0.2)))}
    n_ref, _ = sc.fit(7, e_rel=1e-6)
    assert n == n_ref == 7
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=3e-4)
    for comp, c in zip(comps, sc.components):
        assert np.abs(np.asarray(comp.children[1].parameters[1]) - c.shift).max() < 2e-4
    free = shifting_scene(gs, hsc)  # (the prior is in force: without it the shift ends elsewhere)
    free.fit(7, e_rel=1e-6)
    assert np.abs(free.components[0].shift - sc.components[0].shift).max() > 5e-3

    # -- psf_shift under a constraint
    gp = golden("hsc_psf_shift")
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters)
    obs.match(frame, renderer=ConvolutionRenderer(obs, frame, psf_shift=gp["psf_shift"].copy()))
    shift = obs.parameters[0]
    shift.constraint = Within(gp["psf_shift"], 0.015)
    comps = []
    for k in range(int(hsc["n_comp"])):
        h, w = hsc["morph_%d" % k].shape
        oy, ox = hsc["origin_%d" % k]
        box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
        comps.append(scarlet.FactorizedComponent(
            frame,
            scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                      min_step=hsc["min_step_%d" % k]),
            scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                             hsc["morph_%d" % k].copy(), bbox=box[1:],
                                             resizing=False)))
    blend = scarlet.Blend(comps, obs)
    n, _ = blend.fit(6, e_rel=1e-9)
    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.psf_shift = gp["psf_shift"].copy()
    lo, hi = gp["psf_shift"] - 0.015, gp["psf_shift"] + 0.015
    sc.vec_rules = {"psf_shift": dict(prox=lambda x, step: np.clip(x, lo, hi))}
    n_ref, _ = sc.fit(6, e_rel=1e-9)
    assert n == n_ref == 6
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=1e-4)
    assert np.abs(np.asarray(shift) - sc.psf_shift).max() < 2e-5
    assert np.abs(np.asarray(shift) - gp["psf_shift"]).max() <= 0.015 + 1e-12
    assert shift.m is not None


def test_relative_step_on_psf_shift_through_the_facade(hsc):
    """``Parameter.step = partial(relative_step, factor=..., minimum=...)`` (parameter.py:126-129)
    on ``psf_shift``: ``Blend.fit`` hands the rule to the device and follows the oracle with
    the same rule (round 4 refused it)."""
    from functools import partial

    import scarlet_amd as scarlet
    from scarlet_amd.parameter import relative_step
    from scarlet_amd.renderer import ConvolutionRenderer
    from conftest import golden

    gp = golden("hsc_psf_shift")
    shift0 = np.abs(gp["psf_shift"]) + 0.05
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters)
    obs.match(frame, renderer=ConvolutionRenderer(obs, frame, psf_shift=shift0.copy()))
    shift = obs.parameters[0]
    shift.step = partial(relative_step, factor=0.2, minimum=1e-3)
    comps = []
    for k in range(int(hsc["n_comp"])):
        h, w = hsc["morph_%d" % k].shape
        oy, ox = hsc["origin_%d" % k]
        box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
        comps.append(scarlet.FactorizedComponent(
            frame,
            scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                      min_step=hsc["min_step_%d" % k]),
            scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                             hsc["morph_%d" % k].copy(), bbox=box[1:],
                                             resizing=False)))
    blend = scarlet.Blend(comps, obs)
    n, _ = blend.fit(8, e_rel=1e-9)
    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.psf_shift = shift0.copy()
    sc.psf_shift_step, sc.psf_shift_rel_step = 1e-3, 0.2
    n_ref, _ = sc.fit(8, e_rel=1e-9)
    assert n == n_ref == 8
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=1e-4)
    assert np.abs(np.asarray(shift) - sc.psf_shift).max() < 2e-5
    # the rule is in force: a constant step of 1e-3 moves the shift far less
    assert np.abs(np.asarray(shift) - shift0).max() > 5 * 8 * 1e-3


def test_shifting_image_morphology(hsc):
    """A bare ``ImageMorphology(shifting=True)`` gets a FIXED zero shift in the
    reference (``fixed=self.shifting``, morphology.py:113): the Fourier shift never
    moves, so the fit equals the one without shifting."""
    import scarlet_amd as scarlet

    def blend_of(shifting):
        blend, obs = build_blend(hsc, resizing=False)
        comps = []
        for comp in components_of(blend)[:4]:
            spectrum, morphology = comp.children
            image = np.asarray(morphology.parameters[0]).copy()
            comps.append(scarlet.FactorizedComponent(
                blend.frame, spectrum,
                scarlet.ImageMorphology(blend.frame, image, bbox=morphology.bbox.copy(),
                                        shifting=shifting, resizing=False)))
        return scarlet.Blend(comps, obs)

    a, b = blend_of(False), blend_of(True)
    assert all(p.fixed for p in b.parameters if p.name == "shift")
    na, la = a.fit(8, e_rel=1e-9)
    nb, lb = b.fit(8, e_rel=1e-9)
    assert na == nb == 8 and la == lb
    morphology = b.sources[0].children[1]
    assert np.abs(morphology.get_model() - np.asarray(morphology.parameters[0])).max() < 1e-12


def test_extended_sources_with_free_shifts(hsc):
    """``init_all_sources(..., shifting=True)``: every ExtendedSource carries a free
    Fourier shift (morphology.py:673-676).  Initialisation equals the reference's
    (golden), the fit with box resizing follows the oracle, shifts and their optimizer
    state land on the ``shift`` Parameters."""
    import scarlet_amd as scarlet
    from scarlet_amd.initialization import init_all_sources
    from conftest import golden, shifting_scene

    g = golden("hsc_shifting")
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    centers = [tuple(c) for c in g["centers"]]
    sources, skipped = init_all_sources(frame, centers, obs, max_components=2, min_snr=50,
                                        thresh=1, fallback=True, silent=True, set_spectra=True,
                                        shifting=True)
    blend = scarlet.Blend(sources, obs)
    comps = components_of(blend)
    assert len(comps) == int(g["n_comp"])
    for k, comp in enumerate(comps):
        morphology = comp.children[1]
        image, shift = morphology.parameters
        assert not shift.fixed and shift.step == 1e-1
        assert_allclose(np.asarray(shift), g["shift_%d" % k], atol=1e-12)
        assert np.abs(np.asarray(image) - g["morph_%d" % k]).max() < 1e-5
        assert np.abs(morphology.get_model() - g["shifted_%d" % k]).max() < 1e-5
    model = blend.get_model()
    assert np.abs(model - g["model"]).max() < 2e-4 * np.abs(g["model"]).max()

    n, logL = blend.fit(32, e_rel=1e-6)
    sc = shifting_scene(g, hsc)
    n_ref, logL_ref = sc.fit(32, e_rel=1e-6, resizing=True)
    assert n == n_ref == 32
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    assert_allclose(chi[:15], chi_ref[:15], rtol=2e-3)
    assert abs(chi[-1] - chi_ref[-1]) < 2e-2 * abs(chi_ref[-1])
    moved = 0.0
    for k, (comp, c) in enumerate(zip(comps, sc.components)):
        image, shift = comp.children[1].parameters
        assert image.shape == c.morph.shape
        assert np.abs(np.asarray(shift) - c.shift).max() < 2e-2
        assert shift.m is not None and shift.std.shape == (2,)
        moved = max(moved, np.abs(np.asarray(shift) - g["shift_%d" % k]).max())
    assert moved > 1e-2 and logL > float(g["logL"])


# ---------------------------------------------------------------- scarlet.lite facade
def _lite_blend(hsc, g, kind):
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images = hsc["images"].astype(np.float32)
    variance = (1 / hsc["weights"]).astype(np.float32)
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    obs = lite.LiteObservation(images, variance, hsc["weights"].astype(np.float32),
                               hsc["psfs"].astype(np.float32), model_psf=model_psf[0][None])
    assert np.abs(obs.diff_kernel.image - g["diff_kernel"]).max() < 1e-6
    assert_allclose(obs.noise_rms, g["noise_rms"], rtol=1e-6)
    init = lite.init_fista_component if kind == "fista" else lite.init_adaprox_component
    sources = []
    for k in range(int(g["n_comp"])):
        morph = hsc["morph_%d" % k].astype(np.float32)
        oy, ox = (int(v) for v in hsc["origin_%d" % k])
        h, w = morph.shape
        bbox = scarlet.Box((5, h, w), origin=(0, oy, ox))
        comp = init((oy + h // 2, ox + w // 2), bbox, hsc["sed_%d" % k].astype(np.float32).copy(),
                    morph.copy(), obs, bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    return lite.LiteBlend(sources, obs)


@pytest.mark.parametrize("kind", ["fista", "adaprox"])
def test_lite_blend_fit_follows_the_reference_run(hsc, kind):
    """``scarlet.lite`` API end to end: LiteObservation / init_*_component / LiteBlend.fit
    with box resizing every 10 iterations against the run of the reference itself
    (golden): loss of every evaluation, boxes, spectra, morphologies, counter."""
    from conftest import golden

    g = golden("lite_" + kind)
    blend = _lite_blend(hsc, g, kind)
    if kind == "fista":
        assert_allclose([c._sed.step for c in blend.components], g["fista_step"], rtol=1e-6)
    it, loss = blend.fit(3, e_rel=1e-9, resize=10, reweight=False)
    assert it == int(g["it_a"]) == blend.it and len(blend.loss) == 3
    for k, c in enumerate(blend.components):
        assert np.abs(c.sed / g["a_sed_%d" % k] - 1).max() < 1e-4, k
        assert np.abs(c.morph - g["a_morph_%d" % k]).max() < 1e-4, k
    it, loss = blend.fit(25, e_rel=1e-9, resize=10, reweight=False)
    assert it == int(g["it_b"]) and len(blend.loss) == len(g["loss"]) and loss == blend.loss[-1]
    assert_allclose(blend.loss[:12], g["loss"][:12], rtol=3e-4)
    assert_allclose(blend.loss, g["loss"], rtol=5e-3)
    for k, c in enumerate(blend.components):
        assert c.morph.shape == g["b_morph_%d" % k].shape, k
        assert tuple(c.bbox.origin[1:]) == tuple(g["b_origin_%d" % k]), k
        assert np.abs(c.sed / g["b_sed_%d" % k] - 1).max() < 2e-2, k
        assert np.abs(c.morph - g["b_morph_%d" % k]).max() < 2e-2, k
    with pytest.raises(NotImplementedError):
        blend.components[0].update(0, None)


def test_lite_postprocessing_matches_the_reference(hsc):
    """weight_sources and multifit_seds on the reference's fitted FISTA state"""
    from conftest import golden
    from scarlet_amd import lite

    g = golden("lite_fista")
    blend = _lite_blend(hsc, g, "fista")
    for k, c in enumerate(blend.components):
        h = g["b_morph_%d" % k].shape[0]
        oy, ox = (int(v) for v in g["b_origin_%d" % k])
        c._morph.x = g["b_morph_%d" % k].copy()
        c._sed.x = g["b_sed_%d" % k].copy()
        c.bbox.origin, c.bbox.shape = (0, oy, ox), (5, h, h)
        c.slices = lite.models.overlapped_slices(c.model_bbox, c.bbox)
    lite.weight_sources(blend)
    for i, src in enumerate(blend.sources):
        assert tuple(src.flux_box.origin) == tuple(g["flux_origin_%d" % i])
        assert src.flux.shape == g["flux_%d" % i].shape
        scale = np.abs(g["flux_%d" % i]).max()
        assert np.abs(src.flux - g["flux_%d" % i]).max() < 2e-4 * scale, i
    seds = lite.multifit_seds(blend.observation, [c.morph for c in blend.components],
                              [c.bbox[1:] for c in blend.components])
    assert np.abs(seds - g["multifit_seds"]).max() < 2e-3 * np.abs(g["multifit_seds"]).max()
    assert blend.fit_spectra() is blend
    assert_allclose(np.stack([c.sed for c in blend.components]), np.maximum(seds, 1e-20), rtol=1e-6)


def test_lite_init_all_sources_main_matches_the_reference(hsc):
    """lite/initialization.py:321-419 on the quickstart scene: number of components per
    source, boxes, morphologies and spectra equal the reference's (golden), and the
    initialised blend fits"""
    from conftest import golden
    from scarlet_amd import lite

    g = golden("lite_init")
    blend = _lite_blend(hsc, golden("lite_fista"), "fista")
    obs = blend.observation
    sources = lite.init_all_sources_main(obs, [tuple(c) for c in g["centers"]], min_snr=50)
    assert [len(s.components) for s in sources] == list(g["n_comp_of"])
    for i, src in enumerate(sources):
        for j, c in enumerate(src.components):
            assert tuple(c.bbox.origin[1:]) == tuple(g["origin_%d_%d" % (i, j)])
            assert c.morph.shape == g["morph_%d_%d" % (i, j)].shape
            assert np.abs(c.morph - g["morph_%d_%d" % (i, j)]).max() < 1e-5, (i, j)
            ref = g["sed_%d_%d" % (i, j)]
            assert np.abs(c.sed - ref).max() <= 2e-3 * np.abs(ref).max(), (i, j)
    # the monotonic-mask variant (use_mask=True) through the GPU mask operators
    masked = lite.init_all_sources_main(obs, [tuple(c) for c in g["centers"]], min_snr=50,
                                        use_mask=True)
    assert [len(s.components) for s in masked] == list(g["mask_n_comp_of"])
    for i, src in enumerate(masked):
        for j, c in enumerate(src.components):
            assert tuple(c.bbox.origin[1:]) == tuple(g["mask_origin_%d_%d" % (i, j)])
            assert np.abs(c.morph - g["mask_morph_%d_%d" % (i, j)]).max() < 1e-5, (i, j)
            ref = g["mask_sed_%d_%d" % (i, j)]
            assert np.abs(c.sed - ref).max() <= 2e-3 * np.abs(ref).max(), (i, j)
    fitted = lite.LiteBlend(
        lite.parameterize_sources(sources, obs, lite.init_adaprox_component), obs)
    it, loss = fitted.fit(30, e_rel=1e-4)
    assert loss > fitted.loss[0] and it <= 30
    assert all(src.flux.shape[0] == 5 for src in fitted.sources)


def test_fit_blends_equals_individual_fits(hsc, monkeypatch):
    """fit_blends: several Blend objects in one device batch that stays on the device for the
    whole call (the resize hooks change its component table in place) give exactly the
    per-blend results of Blend.fit's own loop (host resize, a new batch after every
    UpdateException: ``SCARLET_AMD_BLEND_FIT=loop``; by default Blend.fit takes the resident
    path itself) -- and the observation is uploaded once, not once per hook round"""
    import scarlet_amd as scarlet
    from scarlet_amd import _lib

    def make(k):
        full, obs = build_blend(hsc, resizing=True)
        # different scenes: drop a source and rescale the spectra
        sources = list(full.sources)
        blend = scarlet.Blend(sources[:len(sources) - k], obs)
        for p in blend.parameters:
            if p.name == "spectrum":
                p *= 1 + 0.1 * k
        return blend

    single = [make(k) for k in range(3)]
    monkeypatch.setenv("SCARLET_AMD_BLEND_FIT", "loop")
    want = [b.fit(35, e_rel=1e-5) for b in single]
    monkeypatch.delenv("SCARLET_AMD_BLEND_FIT")
    # (and Blend.fit by default: the resident path for one blend)
    again = [make(k) for k in range(3)]
    assert [b.fit(35, e_rel=1e-5) for b in again] == want
    assert all(x.loss == y.loss for x, y in zip(single, again))
    many = [make(k) for k in range(3)]
    boxes = [[tuple(c.children[1].bbox.shape) for c in components_of(b)] for b in many]
    uploads = _lib.load().smi_observation_uploads()
    got = scarlet.fit_blends(many, 35, e_rel=1e-5)
    assert _lib.load().smi_observation_uploads() - uploads == 1
    # (the hooks did resize boxes in this fit)
    assert boxes != [[tuple(c.children[1].bbox.shape) for c in components_of(b)] for b in many]
    for a, b, r1, r2 in zip(single, many, want, got):
        assert r1 == r2
        assert_allclose(a.loss, b.loss, rtol=0, atol=0)
        for p, q in zip(a.parameters, b.parameters):
            assert p.shape == q.shape
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)
            if p.m is not None:
                assert_allclose(p.m, q.m, rtol=0, atol=0)
    # different frame shapes end up in different batches
    other, _ = build_blend(hsc, resizing=False)
    small = make(0)
    res = scarlet.fit_blends([other, small], 5, e_rel=1e-9)
    assert res[0][0] == res[1][0] == 5


def test_fit_blends_resident_batch_equals_rebuilt_batches_and_single_fits(monkeypatch):
    """48 scenes of the benchmark workload as Blend objects with resizing on: the batch that
    stays on the device (device-side resize test, component table changed in place, blends at
    different iteration counters paused in turn) gives what the per-round rebuilt batches give
    -- iteration counts, every loss, boxes, parameters -- and what ``Blend.fit`` gives for
    blends of it fitted alone."""
    import os
    import sys

    import scarlet_amd as scarlet

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    n = 48
    a = bench.build_facade_blends(0, n, 0)
    ra = scarlet.fit_blends(a, 60, e_rel=1e-4)
    monkeypatch.setenv("SCARLET_AMD_FIT_BLENDS", "rebuild")
    b = bench.build_facade_blends(0, n, 0)
    rb = scarlet.fit_blends(b, 60, e_rel=1e-4)
    monkeypatch.delenv("SCARLET_AMD_FIT_BLENDS")
    assert ra == rb
    resized = 0
    for x, y in zip(a, b):
        assert x.loss == y.loss
        for p, q in zip(x.parameters, y.parameters):
            assert p.shape == q.shape
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)
            if p.m is not None:
                assert_allclose(p.m, q.m, rtol=0, atol=0)
                assert_allclose(p.v, q.v, rtol=0, atol=0)
            assert callable(p.step) or p.step == q.step
        resized += sum(tuple(src.children[1].bbox.shape) != (41, 41) for src in x.sources)
    assert resized > 10 and len({r[0] for r in ra}) > 3  # boxes changed, blends stopped apart
    monkeypatch.setenv("SCARLET_AMD_BLEND_FIT", "loop")  # Blend.fit's own loop, host resize
    for i in (0, 17, 47):
        one = bench.build_facade_blends(i, i + 1, 0)[0]
        assert one.fit(60, e_rel=1e-4) == ra[i]
        assert one.loss == a[i].loss


def test_fit_blends_mixes_device_and_host_resizes(monkeypatch):
    """Blends of the stock classes have their boxes resized on the device; a blend whose
    morphologies override ``shrink_box`` (here: by calling the stock one) keeps the host's
    ``update()`` -- in the same batch, the same launches.  Both against the individual fits and
    against the batch with every resize on the host (``SCARLET_AMD_FIT_BLENDS=host-resize``)."""
    import os
    import sys

    import scarlet_amd as scarlet
    from scarlet_amd.fitting import _device_resize_covers

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    class Mine(scarlet.ExtendedSourceMorphology):
        def shrink_box(self, image, thresh=0):
            return super().shrink_box(image, thresh)

    def build():
        blends = bench.build_facade_blends(0, 12, 0)
        for i in (3, 8):
            for src in blends[i].sources:
                src.children[1].__class__ = Mine
        return blends

    a = build()
    assert [_device_resize_covers(b) for b in a] == [i not in (3, 8) for i in range(12)]
    ra = scarlet.fit_blends(a, 60, e_rel=1e-4)
    assert scarlet.fit_blends.errors == []
    monkeypatch.setenv("SCARLET_AMD_FIT_BLENDS", "host-resize")
    b = build()
    rb = scarlet.fit_blends(b, 60, e_rel=1e-4)
    monkeypatch.delenv("SCARLET_AMD_FIT_BLENDS")
    assert ra == rb
    resized = {i: 0 for i in range(12)}
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.loss == y.loss
        for p, q in zip(x.parameters, y.parameters):
            assert p.shape == q.shape and p.dtype == q.dtype
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)
            if p.m is not None:
                assert_allclose(p.m, q.m, rtol=0, atol=0)
                assert_allclose(p.vhat, q.vhat, rtol=0, atol=0)
            assert callable(p.step) or p.step == q.step
        for sx, sy in zip(x.sources, y.sources):
            assert sx.bbox == sy.bbox and sx.children[1].bbox == sy.children[1].bbox
            resized[i] += tuple(sx.children[1].bbox.shape) != (41, 41)
    assert resized[3] + resized[8] > 0 and sum(resized.values()) > resized[3] + resized[8]
    for mode in ("loop", "resident"):
        monkeypatch.setenv("SCARLET_AMD_BLEND_FIT", mode)
        for i in (0, 3, 11):
            one = build()[i]
            assert one.fit(60, e_rel=1e-4) == ra[i]
            assert one.loss == a[i].loss


def test_centre_fitting_with_resizing_on_the_resident_path(monkeypatch):
    """``MonotonicityConstraint(fit_center_radius=1)`` together with ``resizing=True``: a box
    resized on the device needs the NINE plans of its new shape (one per candidate centre), as
    the host resize registers them.  ``Blend.fit`` (resident path by default) and ``fit_blends``
    against the batch with every resize on the host and against ``Blend.fit``'s own loop."""
    import os
    import sys

    import scarlet_amd as scarlet
    from scarlet_amd.fitting import _device_resize_covers

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    def build(lo=0, hi=6):
        blends = bench.build_facade_blends(lo, hi, 0)
        for blend in blends:
            for src in blend.sources:
                src.children[1].parameters[0].constraint = scarlet.ConstraintChain(
                    scarlet.MonotonicityConstraint(neighbor_weight="angle", min_gradient=0,
                                                   fit_center_radius=1),
                    scarlet.PositivityConstraint(), scarlet.NormalizationConstraint("max"))
        return blends

    a = build()
    assert all(_device_resize_covers(b) for b in a)
    ra = scarlet.fit_blends(a, 45, e_rel=1e-4)
    assert scarlet.fit_blends.errors == []
    monkeypatch.setenv("SCARLET_AMD_FIT_BLENDS", "host-resize")
    b = build()
    rb = scarlet.fit_blends(b, 45, e_rel=1e-4)
    monkeypatch.delenv("SCARLET_AMD_FIT_BLENDS")
    assert ra == rb
    resized = 0
    for x, y in zip(a, b):
        assert x.loss == y.loss
        for p, q in zip(x.parameters, y.parameters):
            assert p.shape == q.shape
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)
        resized += sum(tuple(src.children[1].bbox.shape) != (41, 41) for src in x.sources)
    assert resized > 0
    for mode in ("loop", "resident"):
        monkeypatch.setenv("SCARLET_AMD_BLEND_FIT", mode)
        for i in (0, 5):
            one = build(i, i + 1)[0]
            assert one.fit(45, e_rel=1e-4) == ra[i]
            assert one.loss == a[i].loss


def test_blends_pause_at_their_own_hooks_and_give_the_lockstep_results(monkeypatch):
    """``fit_blends`` lets every blend run to ITS next resize hook (or the end of its budget)
    inside one device call -- the device pauses it there, ``smi_batch_set_pause_at`` -- instead of
    stopping all blends at the nearest hook of any of them.  Same results as the lock-step
    rounds (``SCARLET_AMD_FIT_BLENDS=lockstep``), bit for bit, in fewer device calls."""
    import os
    import sys

    import scarlet_amd as scarlet
    from scarlet_amd import BlendBatch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    calls = {"n": 0}
    step = BlendBatch.step

    def counting(self, *a, **k):
        calls["n"] += 1
        return step(self, *a, **k)

    monkeypatch.setattr(BlendBatch, "step", counting)
    n = 40
    a = bench.build_facade_blends(0, n, 0)
    ra = scarlet.fit_blends(a, 57, e_rel=1e-4, min_iter=3)
    own = calls["n"]
    monkeypatch.setenv("SCARLET_AMD_FIT_BLENDS", "lockstep")
    calls["n"] = 0
    b = bench.build_facade_blends(0, n, 0)
    rb = scarlet.fit_blends(b, 57, e_rel=1e-4, min_iter=3)
    assert ra == rb and own < calls["n"]
    assert len({r[0] for r in ra}) > 3 and max(r[0] for r in ra) == 57
    for x, y in zip(a, b):
        assert x.loss == y.loss
        for p, q in zip(x.parameters, y.parameters):
            assert p.shape == q.shape
            assert_allclose(np.asarray(p), np.asarray(q), rtol=0, atol=0)
            if p.m is not None:
                assert_allclose(p.v, q.v, rtol=0, atol=0)


def test_an_error_in_the_middle_of_fit_blends_leaves_consistent_objects(monkeypatch):
    """A hook round that raises (here: the second ``update_components`` of the batch): the boxes
    the device has resized so far, the parameters, moments and the losses of the iterations
    that ran still reach the Python objects before the batch is closed -- every image fits its
    box, every blend has its losses -- and the error propagates."""
    import os
    import sys

    import scarlet_amd as scarlet
    from scarlet_amd import BlendBatch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    calls = {"n": 0}
    update = BlendBatch.update_components

    def failing(self, *a, **k):
        calls["n"] += 1
        if calls["n"] == 2:
            raise RuntimeError("injected")
        return update(self, *a, **k)

    monkeypatch.setattr(BlendBatch, "update_components", failing)
    blends = bench.build_facade_blends(0, 24, 0)
    with pytest.raises(RuntimeError, match="injected"):
        scarlet.fit_blends(blends, 60, e_rel=1e-4)
    resized = 0
    for blend in blends:
        assert len(blend.loss) >= 11 and np.all(np.isfinite(blend.loss))
        for src in blend.sources:
            morphology = src.children[1]
            image = morphology.parameters[0]
            assert tuple(image.shape) == tuple(morphology.bbox.shape)
            assert image.m is not None and image.m.shape == image.shape
            resized += tuple(image.shape) != (41, 41)
    assert resized > 0


def test_fit_blends_keeps_going_when_one_blend_fails():
    """A blend whose parameters turn non-finite gets ``(n_iter, nan)`` and an entry in
    ``fit_blends.errors``; its loss history ends with the iteration that failed (the loss is
    recorded before the step, blend.py:294-299); the blends that share its device batch are
    fitted as if it were not there."""
    import os
    import sys

    import scarlet_amd as scarlet

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    alone = bench.build_facade_blends(0, 3, 0)
    want = [b.fit(25, e_rel=1e-4) for b in (alone[0], alone[2])]
    blends = bench.build_facade_blends(0, 3, 0)
    blends[1].sources[4].children[0].parameters[0][2] = np.nan   # one band of one spectrum
    got = scarlet.fit_blends(blends, 25, e_rel=1e-4)
    assert [i for i, _ in scarlet.fit_blends.errors] == [1]
    assert isinstance(scarlet.fit_blends.errors[0][1], ArithmeticError)
    assert got[1][0] == 1 and np.isnan(got[1][1]) and len(blends[1].loss) == 1
    assert [got[0], got[2]] == want
    assert blends[0].loss == alone[0].loss and blends[2].loss == alone[2].loss


def test_fit_blends_with_a_callback_or_another_scheme_fits_one_by_one(hsc):
    """``fit_blends(..., callback=...)`` and ``scheme="adam"`` are Blend.fit's host-stepped
    modes: the call goes through the blends one at a time and returns what they return."""
    import warnings

    import scarlet_amd as scarlet

    seen = []
    a, _ = build_blend(hsc, resizing=False)
    b, _ = build_blend(hsc, resizing=False)
    got = scarlet.fit_blends([a, b], 6, e_rel=1e-9, callback=lambda *X, it: seen.append(it))
    assert seen == list(range(6)) * 2 and [r[0] for r in got] == [6, 6]
    one, _ = build_blend(hsc, resizing=False)
    assert one.fit(6, e_rel=1e-9) == got[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "parity unpinned" for the published adam formulas
        c, _ = build_blend(hsc, resizing=False)
        d, _ = build_blend(hsc, resizing=False)
        assert scarlet.fit_blends([c], 5, e_rel=1e-9, scheme="adam")[0] == d.fit(5, e_rel=1e-9, scheme="adam")


def test_fit_blends_fits_unbatchable_blends_by_themselves(hsc):
    """``fit_blends`` stands for ``[b.fit() for b in blends]`` (scarlet/testing/api.py:216-224).
    A blend with a second observation of the same channels (one more term of ITS loss on the
    device) or with a free ``psf_shift`` cannot share a device batch with others; it used to
    be refused, now it is fitted by itself inside the same call, with the results of its own
    ``Blend.fit`` -- and the ordinary blends around it still share a batch."""
    import scarlet_amd as scarlet
    from scarlet_amd.renderer import ConvolutionRenderer

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame(hsc["images"].shape, psf=model_psf, channels=filters)

    def sources():
        out = []
        for k in range(int(hsc["n_comp"])):
            h, w = hsc["morph_%d" % k].shape
            oy, ox = hsc["origin_%d" % k]
            box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
            out.append(scarlet.FactorizedComponent(
                frame,
                scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                          min_step=hsc["min_step_%d" % k]),
                scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                                 hsc["morph_%d" % k].copy(), bbox=box[1:],
                                                 resizing=False)))
        return out

    def plain():
        obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                                  weights=hsc["weights"], channels=filters).match(frame)
        return scarlet.Blend(sources(), obs)

    def two_observations():
        obs1 = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                                   weights=hsc["weights"], channels=filters).match(frame)
        psfs2 = scarlet.GaussianPSF(sigma=(1.6, 1.7, 1.8), boxsize=31).get_model().astype(np.float32)
        obs2 = scarlet.Observation((hsc["images"][:3] * 0.9).astype(np.float32),
                                   psf=scarlet.ImagePSF(psfs2),
                                   weights=(hsc["weights"][:3] * 0.5).astype(np.float32),
                                   channels=filters[:3]).match(frame)
        return scarlet.Blend(sources(), [obs1, obs2])

    def shifted_psf():
        obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                                  weights=hsc["weights"], channels=filters)
        obs.match(frame, renderer=ConvolutionRenderer(obs, frame, psf_shift=np.array([0.2, -0.1])))
        return scarlet.Blend(sources(), obs)

    makers = [plain, two_observations, plain, shifted_psf]
    alone = []
    for make in makers:
        b = make()
        alone.append((b.fit(12, e_rel=1e-9), np.array(b.loss)))
    many = [make() for make in makers]
    out = scarlet.fit_blends(many, 12, e_rel=1e-9)
    assert scarlet.fit_blends.errors == []
    for b, res, (res_alone, loss_alone) in zip(many, out, alone):
        assert res[0] == res_alone[0] == 12
        assert_allclose(np.array(b.loss), loss_alone, rtol=1e-12)
        assert res[1] == res_alone[1]
    assert len(many[1]._extra_layers) == 1
    assert out[0] == out[2] and out[1] != out[0] and out[3] != out[0]


def test_psf_shift_renderer(hsc):
    """ConvolutionRenderer(psf_shift=...): rendering with the shifted kernel equals the
    reference's (golden), and the host-stepped fit (shift = free parameter of the
    observation) follows the oracle"""
    import scarlet_amd as scarlet
    from scarlet_amd.renderer import ConvolutionRenderer
    from conftest import golden

    gp = golden("hsc_psf_shift")
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters)
    obs.match(frame, renderer=ConvolutionRenderer(obs, frame, psf_shift=gp["psf_shift"].copy()))
    assert [p.name for p in obs.parameters] == ["psf_shift"]
    rendered = obs.render(gp["model"])
    assert np.abs(rendered - gp["rendered"]).max() < 1e-5 * np.abs(gp["rendered"]).max()
    assert_allclose(obs.get_log_likelihood(gp["model"]), float(gp["logL"]), rtol=1e-6)

    comps = []
    for k in range(int(hsc["n_comp"])):
        h, w = hsc["morph_%d" % k].shape
        oy, ox = hsc["origin_%d" % k]
        box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
        comps.append(scarlet.FactorizedComponent(
            frame,
            scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                      min_step=hsc["min_step_%d" % k]),
            scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                             hsc["morph_%d" % k].copy(), bbox=box[1:],
                                             resizing=False)))
    blend = scarlet.Blend(comps, obs)
    start = [np.array(p) for p in blend.parameters]
    n, logL = blend.fit(12, e_rel=1e-9)
    assert blend._psf_stepped_on_device and blend._psf is None  # (nothing left for later fits)
    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.psf_shift = gp["psf_shift"].copy()
    n_ref, logL_ref = sc.fit(12, e_rel=1e-9)
    assert n == n_ref == 12
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    assert_allclose(chi, chi_ref, rtol=1e-4)
    shift = obs.parameters[0]
    assert np.abs(np.asarray(shift) - sc.psf_shift).max() < 2e-5
    assert np.abs(np.asarray(shift) - gp["psf_shift"]).max() > 1e-3  # it moved
    assert shift.m is not None and shift.std.shape == (2,)
    # warm start: 6 + 6 iterations (moments carried on the Parameters) = 12 at once ...
    device_loss, device_shift = list(blend.loss), np.array(shift)

    def rewind():
        for p, x0 in zip(blend.parameters, start):
            p[...] = x0
            p.m = p.v = p.vhat = None
        shift[...] = gp["psf_shift"]
        shift.m = shift.v = shift.vhat = None
        blend.loss = []

    # ... and the host-stepped variant (frames beyond the fused kernel) gives the same fit
    rewind()
    opt = dict(b1=0.9, b2=0.999, eps=1e-8)
    n_host, _ = blend._fit_with_psf_shift(12, 1e-9, 1, 10, opt, None)
    assert n_host == 12
    assert_allclose(blend.loss, device_loss, rtol=1e-5)
    assert np.abs(np.asarray(shift) - device_shift).max() < 1e-5
    # the callback sees the shift after the components' parameters
    rewind()
    seen = []
    blend.fit(3, e_rel=1e-9, callback=lambda *X, it: seen.append((it, len(X), np.array(X[-1]))))
    assert [s[0] for s in seen] == [0, 1, 2] and seen[0][1] == len(blend.parameters) + 1
    assert seen[0][2].shape == (2,) and not np.array_equal(seen[0][2], seen[2][2])


# ---------------------------------------------------------------- multi-resolution (cfg 5)
def test_multiresolution_render_matches_the_reference():
    """BASELINE config 5 / tests/test_multiresolution.py: every pair of the five images
    of Multiresolution_tests.npz, union and intersection frames.  Frame.from_observations
    and ResolutionRenderer set-up must reproduce the reference's frames, and rendering
    the high-resolution image into the low-resolution observation (GPU) must equal the
    reference's rendering (golden) and pass its SDR > 10 dB criterion."""
    import scarlet_amd as scarlet
    from conftest import golden

    g = golden("multiresolution")

    def wcs(k):
        w = scarlet.LinearWCS(g["crpix_%d" % k], g["crval_%d" % k], g["pc_%d" % k], g["cdelt_%d" % k])
        w.array_shape = g["crpix_%d" % k] * 2
        return w

    def sdr(truth, x):
        return 10 * np.log10(np.sum(truth**2) ** 0.5 / np.sum((truth - x) ** 2) ** 0.5)

    worst = 0.0
    for tag in g["pairs"]:
        i, j, coverage = str(tag).split("_")
        i, j = int(i), int(j)
        obs_hr = scarlet.Observation(g["image_%d" % i][None], wcs=wcs(i),
                                     psf=scarlet.ImagePSF(g["psf_%d" % i]), channels=["lr"])
        obs_lr = scarlet.Observation(g["image_%d" % j][None], wcs=wcs(j),
                                     psf=scarlet.ImagePSF(g["psf_%d" % j]), channels=["hr"])
        frame = scarlet.Frame.from_observations([obs_lr, obs_hr], obs_id=1, coverage=coverage)
        assert tuple(frame.shape) == tuple(g["frame_shape_%s" % tag]), tag
        assert_allclose(frame.wcs.wcs.crpix, g["frame_crpix_%s" % tag])
        assert type(obs_lr.renderer).__name__ == "ResolutionRenderer"
        assert list(obs_lr.renderer._fft_shape) == list(g["fft_shape_%s" % tag])
        rendered = obs_lr.render(g["image_%d" % i][None])
        ref = g["rendered_%s" % tag]
        assert rendered.shape == ref.shape
        worst = max(worst, np.abs(rendered - ref).max() / np.abs(ref).max())
        assert np.abs(rendered - ref).max() < 1e-5 * np.abs(ref).max(), tag
        assert sdr(rendered, g["image_%d" % j]) > 10
    print("largest deviation from the reference rendering: %.2e of the peak" % worst)


def test_spectral_and_dense_evaluation_of_the_resampling_operator_agree():
    """The shift operator the reference builds (renderer.py:414-476: a phase ramp between a
    real transform and its inverse on the padded grid) is circulant along x, so the library
    evaluates A . (model . Pt) through transforms along x (path 1); the two dense products
    per band (path 0) are the same linear map.  Renderings of fixture pairs by both paths
    against the reference's rendering and against each other; an operator that is not
    circulant keeps the dense products and cannot be switched."""
    import ctypes

    import scarlet_amd as scarlet
    from conftest import golden
    from scarlet_amd import _lib

    g = golden("multiresolution")

    def wcs(k):
        w = scarlet.LinearWCS(g["crpix_%d" % k], g["crval_%d" % k], g["pc_%d" % k], g["cdelt_%d" % k])
        w.array_shape = g["crpix_%d" % k] * 2
        return w

    worst = {0: 0.0, 1: 0.0, "between": 0.0}
    for tag in ("1_3_union", "1_4_intersection", "2_4_intersection", "3_4_union", "0_2_union"):
        if tag not in list(g["pairs"]):
            continue
        i, j, coverage = tag.split("_")
        i, j = int(i), int(j)
        obs_hr = scarlet.Observation(g["image_%d" % i][None], wcs=wcs(i),
                                     psf=scarlet.ImagePSF(g["psf_%d" % i]), channels=["lr"])
        obs_lr = scarlet.Observation(g["image_%d" % j][None], wcs=wcs(j),
                                     psf=scarlet.ImagePSF(g["psf_%d" % j]), channels=["hr"])
        scarlet.Frame.from_observations([obs_lr, obs_hr], obs_id=1, coverage=coverage)
        r = obs_lr.renderer
        assert r.device_path() == 1, tag
        ref = g["rendered_%s" % tag]
        out = {}
        for path in (1, 0, 1):
            assert r.device_path(path) == path
            out[path] = obs_lr.render(g["image_%d" % i][None])
            dev = np.abs(out[path] - ref).max() / np.abs(ref).max()
            worst[path] = max(worst[path], dev)
            assert dev < 1e-5, (tag, path)
        between = np.abs(out[0] - out[1]).max() / np.abs(ref).max()
        worst["between"] = max(worst["between"], between)
        assert between < 1e-6, tag
    print("deviation from the reference rendering: spectral %.2e, dense %.2e of the peak; "
          "between the two %.2e" % (worst[1], worst[0], worst["between"]))
    # a shift operator that is not circulant
    rng = np.random.default_rng(5)
    A = rng.normal(0, 1, (1, 5, 12 * 10)).astype(np.float32)
    Pt = rng.normal(0, 1, (10, 10 * 7)).astype(np.float32)
    lib = _lib.load()
    handle = ctypes.c_void_p()
    _lib.check(lib.smi_resampler_create(_lib.ptr(A, ctypes.c_float), _lib.ptr(Pt, ctypes.c_float),
                                        1, 5, 7, 12, 10, ctypes.byref(handle)))
    try:
        path = ctypes.c_int32(-1)
        _lib.check(lib.smi_resampler_get_path(handle, ctypes.byref(path)))
        assert path.value == 0
        assert lib.smi_resampler_set_path(handle, 1) != 0
        padded = rng.normal(0, 1, (1, 12, 10)).astype(np.float32)
        out = np.empty((1, 5, 7), np.float32)
        _lib.check(lib.smi_resampler_render(handle, _lib.ptr(padded, ctypes.c_float),
                                            _lib.ptr(out, ctypes.c_float)))
        ref = np.einsum("ak,kb->ab", A[0].astype(np.float64),
                        (padded[0].astype(np.float64) @ Pt.astype(np.float64)).reshape(120, 7))
        assert np.abs(out[0] - ref).max() < 2e-6 * np.abs(ref).max()
    finally:
        lib.smi_resampler_destroy(handle)


def _lowres_operators(lowres):
    """Dense device operators from the ORACLE's matrices (independent of the facade's
    set-up): A [C][n_a][Fy Fx], Pt [Fx][Fx n_b]."""
    C, n_a = lowres.op.shape[:2]
    A = lowres.op.reshape(C, n_a, -1)
    n_b, Fx, _ = lowres.Mx.shape
    Pt = lowres.Mx.transpose(2, 1, 0).reshape(Fx, Fx * n_b)  # [x'][(x, b)]
    return np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(Pt, dtype=np.float32)


def test_lowres_term_on_the_device_matches_the_oracle():
    """smi_batch_attach_lowres: loss, low-resolution rendering and gradients of a blend
    with a second observation on a coarser grid, against the oracle (which is pinned to
    the reference's float64 evaluation and finite differences, CPU suite); then 25
    iterations of the loop against the oracle's trajectory."""
    import ctypes

    from conftest import golden
    from multires_scene import build
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, ComponentSpec

    g = golden("multires_fit")
    scene, lowres, c_hr, _ = build(g)
    lib = _lib.load()
    A, Pt = _lowres_operators(lowres)
    handle = ctypes.c_void_p()
    _lib.check(lib.smi_resampler_create(
        _lib.ptr(A, ctypes.c_float), _lib.ptr(Pt, ctypes.c_float), lowres.C, A.shape[1],
        lowres.Mx.shape[0], lowres.Fy, lowres.Fx, ctypes.byref(handle)))
    try:
        for conv_path in ("auto", "rocfft"):
            scene, lowres, c_hr, _ = build(g)
            specs = [ComponentSpec(c.sed, c.morph, c.origin, sed_min_step=0.0)
                     for c in scene.components]
            batch = BlendBatch(scene.data[None], scene.weights[None], [specs],
                               kernel=scene.kernel, max_iter=30, conv_path=conv_path)
            batch.attach_lowres(handle, lowres.channels, lowres.data, lowres.weights,
                                lowres.log_norm)
            try:
                model, rendered, logL = batch.forward()
                loss, grads = scene.loss_and_gradients()
                assert abs(-logL[0] - loss) < 2e-6 * abs(loss), conv_path
                ref_lr = lowres.render(scene.get_model())
                assert np.abs(batch.lowres_rendered() - ref_lr).max() < 1e-5 * np.abs(ref_lr).max()
                g_sed, g_morph = batch.gradient()
                for k, (r_sed, r_morph) in enumerate(grads):
                    assert np.abs(g_sed[k] - r_sed).max() < RTOL * np.abs(r_sed).max(), (conv_path, k)
                    assert np.abs(g_morph[k] - r_morph).max() < 2 * RTOL * np.abs(r_morph).max()
                # the term matters: without it the gradient is a different one
                scene.extra_observations = []
                _, without = scene.loss_and_gradients()
                assert np.abs(without[0][0] - grads[0][0]).max() > 0.1 * np.abs(grads[0][0]).max()
                scene.extra_observations = [lowres]
                scene.loss = []
                # the loop
                batch.fit(max_iter=25, e_rel=1e-9)
                n_ref, _ = scene.fit(25, e_rel=1e-9)
                hist = batch.loss_history()[0]
                assert len(hist) == n_ref == 25
                shift = lowres.log_norm + scene.log_norm
                assert_allclose(hist - shift, np.array(scene.loss) - shift, rtol=5e-4)
                assert hist[-1] < hist[0]
                seds, morphs = batch.parameters()
                for k, c in enumerate(scene.components):
                    assert np.abs(seds[k] - c.sed).max() < 1e-3 * np.abs(c.sed).max()
                    assert np.abs(morphs[k] - c.morph).max() < 2e-3
            finally:
                batch.close()
        # several observations: the same one split into two with disjoint weights is the
        # same likelihood (log_norm counts every unmasked pixel once)
        scene, lowres, c_hr, _ = build(g)
        specs = [ComponentSpec(c.sed, c.morph, c.origin, sed_min_step=0.0)
                 for c in scene.components]
        batch = BlendBatch(scene.data[None], scene.weights[None], [specs], kernel=scene.kernel,
                           max_iter=4)
        half = np.zeros(lowres.weights.shape, dtype=bool)
        half[:, ::2] = True
        import oracle.resample as resample
        for mask in (half, ~half):
            part = resample.LowResObservation.__new__(resample.LowResObservation)
            part.weights = lowres.weights * mask
            batch.attach_lowres(handle, lowres.channels, lowres.data, part.weights,
                                resample.LowResObservation.log_norm.fget(part))
        try:
            _, _, logL = batch.forward()
            loss, grads = scene.loss_and_gradients()
            assert abs(-logL[0] - loss) < 2e-6 * abs(loss)
            both = batch.lowres_rendered(0), batch.lowres_rendered(1)
            assert_allclose(both[0], both[1], rtol=0, atol=0)
            g_sed, g_morph = batch.gradient()
            for k, (r_sed, r_morph) in enumerate(grads):
                assert np.abs(g_sed[k] - r_sed).max() < RTOL * np.abs(r_sed).max()
                assert np.abs(g_morph[k] - r_morph).max() < 2 * RTOL * np.abs(r_morph).max()
        finally:
            batch.close()
    finally:
        lib.smi_resampler_destroy(handle)


def test_blend_fit_with_two_resolutions():
    """The multi-resolution tutorial's shape of problem through the facade: a
    high-resolution and a low-resolution Observation with their own WCS and PSF,
    Frame.from_observations, sources, Blend.fit.  Loss history and parameters follow the
    oracle, whose low-resolution operator is built from the REFERENCE's set-up quantities
    (golden), so the facade's own WCS / PSF-interpolation set-up is part of what is
    checked."""
    import scarlet_amd as scarlet
    from conftest import golden
    from multires_scene import build

    g = golden("multires_fit")
    gm = golden("multiresolution")
    i_hr, i_lr = int(g["i_hr"]), int(g["i_lr"])

    def wcs(k):
        w = scarlet.LinearWCS(gm["crpix_%d" % k], gm["crval_%d" % k], gm["pc_%d" % k],
                              gm["cdelt_%d" % k])
        w.array_shape = gm["crpix_%d" % k] * 2
        return w

    obs_hr = scarlet.Observation(g["data_hr"].astype(np.float32), wcs=wcs(i_hr),
                                 psf=scarlet.ImagePSF(gm["psf_%d" % i_hr]), channels=["hr"],
                                 weights=g["weights_hr"].astype(np.float32))
    obs_lr = scarlet.Observation(g["data_lr"].astype(np.float32), wcs=wcs(i_lr),
                                 psf=scarlet.ImagePSF(gm["psf_%d" % i_lr]), channels=["lr"],
                                 weights=g["weights_lr"].astype(np.float32))
    observations = [obs_lr, obs_hr]
    frame = scarlet.Frame.from_observations(observations, obs_id=1, coverage="union")
    assert tuple(frame.shape) == tuple(g["frame_shape"])
    assert list(frame.channels) == [str(c) for c in g["channels"]]
    sources = []
    for k in range(int(g["n_components"])):
        oy, ox = (int(v) for v in g["origin_%d" % k])
        spectrum = scarlet.TabulatedSpectrum(frame, g["sed_%d" % k].astype(np.float32))
        morphology = scarlet.ExtendedSourceMorphology(
            frame, (oy + 7, ox + 7), g["morph_%d" % k].copy(),
            bbox=scarlet.Box((15, 15), origin=(oy, ox)), resizing=False)
        sources.append(scarlet.FactorizedComponent(frame, spectrum, morphology))
    blend = scarlet.Blend(sources, observations)
    n, logL = blend.fit(20, e_rel=1e-9)

    scene, lowres, _, _ = build(g)
    n_ref, logL_ref = scene.fit(20, e_rel=1e-9)
    assert n == n_ref == 20
    shift = lowres.log_norm + scene.log_norm
    assert_allclose(np.array(blend.loss) - shift, np.array(scene.loss) - shift, rtol=1e-3)
    assert abs(logL - logL_ref) < 1e-4 * abs(logL_ref)
    for src, c in zip(sources, scene.components):
        sed = np.asarray(src.children[0].parameters[0])
        assert np.abs(sed - c.sed).max() < 2e-3 * np.abs(c.sed).max()
        assert src.children[1].parameters[0].m is not None


def test_multiresolution_tutorial_scene():
    """docs/tutorials/multiresolution.ipynb up to and including ``blend.fit``: 5-band HSC
    cut-out + HST F814W cut-out (gnomonic WCSs whose reference pixels lie thousands of
    pixels outside the images), ``Frame.from_observations(..., coverage="intersection",
    model_psf=GaussianPSF(0.6))``, ``ExtendedSource`` initialisation from both
    observations, ``set_spectra_to_match``.  Everything up to the fit is compared with
    the reference's own run (golden); the fit must then raise the likelihood of both
    observations.  (Source positions: bright HST peaks instead of the sep catalogue.)"""
    import scarlet_amd as scarlet
    from conftest import golden

    g = golden("multires_tutorial")

    def wcs(tag, n):
        return scarlet.TanWCS(g["crpix_" + tag], g["crval_" + tag], g["pc_" + tag],
                              g["cdelt_" + tag], array_shape=(n, n))

    obs_hst = scarlet.Observation(g["data_hst"].copy(), wcs=wcs("hst", 250),
                                  psf=scarlet.ImagePSF(g["psf_hst"].copy()),
                                  channels=[str(c) for c in g["channels_hst"]], weights=None)
    obs_hsc = scarlet.Observation(g["data_hsc"].copy(), wcs=wcs("hsc", 50),
                                  psf=scarlet.ImagePSF(g["psf_hsc"].copy()),
                                  channels=[str(c) for c in g["channels_hsc"]], weights=None)
    observations = [obs_hsc, obs_hst]
    frame = scarlet.Frame.from_observations(observations, coverage="intersection",
                                            model_psf=scarlet.GaussianPSF(sigma=0.6))
    assert tuple(frame.shape) == tuple(g["frame_shape"])
    assert_allclose(frame.wcs.wcs.crpix, g["frame_crpix"])
    assert type(obs_hsc.renderer).__name__ == str(g["hsc_renderer"])
    assert type(obs_hst.renderer).__name__ == str(g["hst_renderer"])
    assert list(obs_hsc.renderer._fft_shape) == list(g["hsc_fft_shape"])
    assert np.abs(obs_hsc.renderer.shifts - g["hsc_shifts"]).max() < 1e-7
    k = obs_hst.renderer.diff_kernel.image
    assert np.abs(k - g["hst_kernel"]).max() < 1e-6 * np.abs(g["hst_kernel"]).max()

    # the conversion pixel -> sky of the catalogue
    ra_dec = obs_hst.get_sky_coord(g["pixel_hst"])
    assert np.abs(ra_dec - g["ra_dec"]).max() < 1e-11
    sources = [scarlet.ExtendedSource(frame, sky, observations, thresh=0.1) for sky in ra_dec]
    scarlet.initialization.set_spectra_to_match(sources, observations)
    for j, src in enumerate(sources):
        assert tuple(src.bbox.origin) == tuple(g["origin_%d" % j]), j
        assert tuple(src.bbox.shape) == tuple(g["shape_%d" % j]), j
        morph = np.asarray(src.parameters[1])
        assert np.abs(morph - g["morph_%d" % j]).max() < 2e-5, j
        spectrum = np.asarray(src.parameters[0])
        assert_allclose(spectrum, g["spectrum_%d" % j], rtol=2e-4)
    blend = scarlet.Blend(sources, observations)
    model = blend.get_model()
    assert_allclose(model.sum(axis=(1, 2)), g["model_sum"], rtol=2e-4)
    rendered_hsc = obs_hsc.render(model)
    rendered_hst = obs_hst.render(model)
    assert np.abs(rendered_hsc - g["rendered_hsc"]).max() < 3e-4 * np.abs(g["rendered_hsc"]).max()
    assert np.abs(rendered_hst - g["rendered_hst"]).max() < 3e-4 * np.abs(g["rendered_hst"]).max()
    logL_hsc = obs_hsc.get_log_likelihood(model)
    logL_hst = obs_hst.get_log_likelihood(model)
    assert abs(logL_hsc - g["logL_hsc"]) < 1e-3 * abs(g["logL_hsc"])
    assert abs(logL_hst - g["logL_hst"]) < 1e-3 * abs(g["logL_hst"])

    n, logL = blend.fit(20, e_rel=1e-6)
    assert n == 20
    # the first recorded loss is the reference's initial -logL (sum over observations)
    assert abs(blend.loss[0] + g["logL_hsc"] + g["logL_hst"]) < 1e-3 * abs(blend.loss[0])
    assert logL > -blend.loss[0]
    after = blend.get_model()
    assert obs_hsc.get_log_likelihood(after) > logL_hsc
    assert obs_hst.get_log_likelihood(after) > logL_hst
    assert abs(obs_hsc.get_log_likelihood(after) + obs_hst.get_log_likelihood(after) - logL) < 2e-3 * abs(logL) + 2.0


def test_fixed_parameters(hsc):
    """Parameter(fixed=True) (parameter.py:38-39): the reference keeps it in X and hands
    adaprox a zero gradient for it (blend.py:107-115), so its value changes only through
    its proximal operator -- not at all for a spectrum above the floor or an image that
    already satisfies its constraints.  Fixed spectrum of source 0, fixed image of source 1;
    everything else follows the oracle with the same flags."""
    import scarlet_amd as scarlet

    blend, obs = build_blend(hsc, resizing=False)
    comps = components_of(blend)
    sed0 = comps[0].children[0].parameters[0]
    img1 = comps[1].children[1].parameters[0]
    sed0.fixed = True
    img1.fixed = True
    before_sed, before_img = np.array(sed0), np.array(img1)
    free_before = np.array(comps[1].children[0].parameters[0])
    n, logL = blend.fit(15, e_rel=1e-9)
    assert_array_equal = np.testing.assert_array_equal
    assert_array_equal(np.array(sed0), before_sed)
    # the image goes through its proximal chain (monotonic, normalised): a fixed point
    assert np.abs(np.array(img1) - before_img).max() < 1e-6
    assert np.abs(np.array(comps[1].children[0].parameters[0]) - free_before).max() > 1e-3
    assert sed0.m is not None and not np.any(sed0.m) and not np.any(sed0.v)

    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.components[0].fixed = (True, False)
    sc.components[1].fixed = (False, True)
    n_ref, logL_ref = sc.fit(15, e_rel=1e-9)
    assert n == n_ref == 15
    chi = np.array(blend.loss) - sc.log_norm
    chi_ref = np.array(sc.loss) - sc.log_norm
    assert_allclose(chi, chi_ref, rtol=5e-4)
    # a fixed spectrum without constraint or step, as a user would write it
    frame = obs.model_frame
    comp = comps[2]
    plain = scarlet.Parameter(np.array(comp.children[0].parameters[0]), name="spectrum", fixed=True)
    spectrum = scarlet.TabulatedSpectrum(frame, plain, bbox=comp.children[0].bbox)
    replaced = scarlet.FactorizedComponent(frame, spectrum, comp.children[1])
    blend2 = scarlet.Blend([replaced], obs)
    keep = np.array(plain)
    blend2.fit(5, e_rel=1e-9)
    assert_array_equal(np.array(plain), keep)


def test_initialisation_of_synthetic_scenes_matches_reference():
    """init_all_sources on three synthetic scenes the reference initialised itself
    (golden init_synthetic.npz): faint and bright sources, one / three / five bands,
    max_components 1 and 2, thresholds 0.5 / 1 / 2, sources near the frame edge -- the
    same source classes, boxes, morphologies, spectra, steps and initial log-likelihood."""
    import scarlet_amd as scarlet
    from conftest import golden
    from scarlet_amd.initialization import init_all_sources

    g = golden("init_synthetic")
    for t in range(int(g["n_scenes"])):
        tag = "s%d_" % t
        images, weights, psfs = g[tag + "images"], g[tag + "weights"], g[tag + "psfs"]
        C = images.shape[0]
        filters = ["f%d" % c for c in range(C)]
        max_components, min_snr, thresh = g[tag + "settings"]
        frame = scarlet.Frame(images.shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * C), channels=filters)
        obs = scarlet.Observation(images.copy(), psf=scarlet.ImagePSF(psfs.copy()),
                                  weights=weights.copy(), channels=filters).match(frame)
        centers = [tuple(c) for c in g[tag + "centers"]]
        sources, skipped = init_all_sources(
            frame, centers, obs, max_components=int(max_components), min_snr=float(min_snr),
            thresh=float(thresh), fallback=True, silent=True, set_spectra=True)
        assert list(skipped) == list(g[tag + "skipped"])
        assert [type(s).__name__ for s in sources] == [str(k) for k in g[tag + "kinds"]], t
        blend = scarlet.Blend(sources, obs)
        comps = components_of(blend)
        assert len(comps) == int(g[tag + "n_comp"])
        for k, comp in enumerate(comps):
            sed = np.asarray(comp.children[0].parameters[0])
            morph = np.asarray(comp.children[1].parameters[0])
            ref_morph, ref_sed = g[tag + "morph_%d" % k], g[tag + "sed_%d" % k]
            assert morph.shape == ref_morph.shape, (t, k)
            assert tuple(comp.children[1].bbox.origin) == tuple(g[tag + "origin_%d" % k]), (t, k)
            assert np.abs(morph - ref_morph).max() < 1e-5, (t, k)
            assert np.abs(sed - ref_sed).max() < 3e-5 * np.abs(ref_sed).max() + 1e-6, (t, k)
            step = comp.children[0].parameters[0].step
            assert_allclose(step.keywords["minimum"], g[tag + "min_step_%d" % k], rtol=1e-5)
        logL0 = obs.get_log_likelihood(blend.get_model())
        assert abs(logL0 - float(g[tag + "logL"])) < 2e-5 * abs(float(g[tag + "logL"])) + 0.05, t
        n, logL = blend.fit(30, e_rel=1e-4)
        assert logL > logL0


# ---------------------------------------------------------------- plug-in seam (seam 3)
def _fit_pair(hsc, mutate, n_it=15, **kw):
    """(built-in blend, mutated blend) after the same fit"""
    ref, _ = build_blend(hsc, resizing=False)
    ref.fit(n_it, e_rel=1e-6, **kw)
    blend, _ = build_blend(hsc, resizing=False)
    mutate(blend)
    blend.fit(n_it, e_rel=1e-6, **kw)
    return ref, blend


def test_user_constraint_subclass_reproduces_the_device_result(hsc):
    """A Python ``Constraint`` subclass is a valid proximal operator (reference
    constraint.py:39-55).  The fit degrades to the host-stepped iteration for that
    parameter (device forward + gradient, host AMSGrad + prox, hoststep.py) instead of
    raising; a subclass that re-implements the spectrum's positivity must reproduce the
    all-device result bit for bit -- losses, every parameter, every moment."""
    import scarlet_amd as scarlet

    calls = []

    class MyPositivity(scarlet.Constraint):
        def __call__(self, X, step):
            calls.append(np.shape(step))
            return np.maximum(X, 1e-20)

    def mutate(blend):
        for comp in components_of(blend):
            comp.children[0].parameters[0].constraint = MyPositivity()

    ref, blend = _fit_pair(hsc, mutate)
    assert calls and len(blend._host) == len(components_of(blend))
    assert_allclose(blend.loss, ref.loss, rtol=0, atol=0)
    for p, q in zip(ref.parameters, blend.parameters):
        assert_allclose(np.asarray(q), np.asarray(p), rtol=0, atol=0)
        if p.m is not None:
            for name in ("m", "v", "vhat"):
                assert_allclose(getattr(q, name), getattr(p, name), rtol=0, atol=0, err_msg=p.name)
            assert_allclose(np.ma.filled(q.std, 0), np.ma.filled(p.std, 0), rtol=0, atol=0)


def test_chains_the_device_cannot_express_step_on_the_host(hsc):
    """Built-in constraints in combinations the fused device chain has no slot for -- an L0
    and an L1 threshold in one chain, ``MonotonicityConstraint(fit_center_radius=2)`` -- are
    not refused: ``device_flags`` says no, and the parameter is stepped on the host with the
    reference's own operators (plug-in seam, hoststep.py) from the device's gradients."""
    import scarlet_amd as scarlet

    def sparse(blend):
        for comp in components_of(blend)[:3]:
            image = comp.children[1].parameters[0]
            image.constraint = scarlet.ConstraintChain(
                scarlet.L0Constraint(1e-3, type="absolute"), scarlet.L1Constraint(1e-4, type="absolute"),
                scarlet.PositivityConstraint())

    ref, blend = _fit_pair(hsc, sparse, n_it=8)
    assert sorted(k for k, _ in blend._host) == [0, 1, 2] and len(blend.loss) == 8
    assert np.isfinite(blend.loss).all() and blend.loss[-1] < blend.loss[0]
    for comp in components_of(blend)[:3]:
        image = np.asarray(comp.children[1].parameters[0])
        assert image.min() >= 0 and not np.any((image > 0) & (image < 1e-3 - 1e-4 - 1e-7))

    def wide_centre(blend):
        comp = components_of(blend)[0]
        image = comp.children[1].parameters[0]
        image.constraint = scarlet.ConstraintChain(
            scarlet.MonotonicityConstraint(neighbor_weight="angle", fit_center_radius=2),
            scarlet.PositivityConstraint(), scarlet.NormalizationConstraint("max"))

    ref, blend = _fit_pair(hsc, wide_centre, n_it=6)
    assert [k for k, _ in blend._host] == [0] and np.isfinite(blend.loss).all()
    assert np.asarray(components_of(blend)[0].children[1].parameters[0]).max() == 1


def test_priors_join_the_gradient_on_the_host(hsc):
    """``Parameter.prior`` (reference parameter.py:42-71; blend.py:120-131 adds ``x.prior(x)``
    to the likelihood's gradient): parameters with a prior are stepped on the host.  A prior
    that returns zeros reproduces the all-device fit bit for bit; one that pulls the image
    towards zero lowers the fitted flux and the likelihood."""
    import scarlet_amd as scarlet

    class Flat(scarlet.Prior):
        def __call__(self, x):
            return np.zeros_like(x)

        def grad(self, x):
            return np.zeros_like(x)

    class Pull(Flat):
        def __call__(self, x):
            return 50.0 * x

    def flat(blend):
        for comp in components_of(blend):
            comp.children[0].parameters[0].prior = Flat()

    ref, blend = _fit_pair(hsc, flat)
    assert len(blend._host) == len(components_of(blend))
    assert_allclose(blend.loss, ref.loss, rtol=0, atol=0)
    for p, q in zip(ref.parameters, blend.parameters):
        assert_allclose(np.asarray(q), np.asarray(p), rtol=0, atol=0)

    def pull(blend):
        components_of(blend)[0].children[0].parameters[0].prior = Pull()

    _, pulled = _fit_pair(hsc, pull)
    assert len(pulled._host) == 1
    a = np.asarray(components_of(ref)[0].children[0].parameters[0])
    b = np.asarray(components_of(pulled)[0].children[0].parameters[0])
    assert np.all(b < a) and pulled.loss[-1] > ref.loss[-1]


def test_noise_factor_draws_fresh_noise_every_iteration(hsc):
    """``Blend.fit(noise_factor=f)`` (reference observation.py:165-168, blend.py:100,
    268-270): every evaluation sees data + a draw of the pixel noise from NumPy's global
    generator and weights / (f + 1), the normalisation term stays that of the original
    weights.  With the generator seeded, the first losses equal the host evaluation of the
    same formula on the same draws."""
    blend, obs = build_blend(hsc, resizing=False)
    rendered = obs.render(blend.get_model())
    f = 1.0
    np.random.seed(11)
    want = []
    for _ in range(2):  # the second draw belongs to iteration 1, whose model we do not know
        noise = np.asarray(np.random.normal(loc=0, scale=obs.noise_rms))
        want.append(obs.log_norm + 0.5 * np.sum(
            obs.weights.astype(np.float64) / (f + 1) * (rendered - obs.data - noise) ** 2))
    np.random.seed(11)
    assert_allclose(-obs.get_log_likelihood(blend.get_model(), noise_factor=f), want[0], rtol=1e-6)
    np.random.seed(11)
    n, logL = blend.fit(4, e_rel=1e-9, noise_factor=f)
    assert n == 4 and np.isfinite(logL)
    assert_allclose(blend.loss[0], want[0], rtol=1e-6)
    quiet, _ = build_blend(hsc, resizing=False)
    quiet.fit(4, e_rel=1e-9)
    assert abs(blend.loss[0] - quiet.loss[0]) > 1e-3 * abs(quiet.loss[0])
    # the observation itself is untouched
    np.testing.assert_array_equal(obs.data, hsc["images"])


def test_other_adaprox_schemes_step_on_the_host(hsc):
    """``Blend.fit(scheme=...)`` (reference blend.py:144 forwards any scheme of
    proxmin.adaprox): the device loop is AMSGrad; every other scheme takes the device's
    gradients and steps all parameters on the host.  AdamX with the constant b1 of
    Blend.fit is AMSGrad and must reproduce the device fit; Adam fits the scene too."""
    ref, adamx = _fit_pair(hsc, lambda blend: None, n_it=10)
    adamx, _ = build_blend(hsc, resizing=False)
    adamx.fit(10, e_rel=1e-6, scheme="adamx")
    assert len(adamx._host) == 2 * len(components_of(adamx))
    assert_allclose(adamx.loss, ref.loss, rtol=2e-5)
    adam, _ = build_blend(hsc, resizing=False)
    n, logL = adam.fit(30, e_rel=1e-6, scheme="adam")
    assert n == 30 and logL > -adam.loss[0] and adam.loss[-1] < 0.2 * adam.loss[0]
    for p in adam.parameters:
        if not p.fixed and p.m is not None:
            assert p.std is not None
    # the next fit of the same blend is the device loop again
    adam.fit(3, e_rel=1e-6)
    assert adam._host == []


def test_user_step_callable_and_user_morphology_chain(hsc):
    """callable ``Parameter.step`` (reference blend.py:135-138) and a user-written chain
    for the image: host-stepped.  The constant step callable is exact; the chain divides
    by the maximum where the device multiplies by its reciprocal (<= 1 ulp per pixel and
    sub-iteration), so the image fit agrees to float32 accuracy."""
    import scarlet_amd as scarlet

    # a callable that returns what relative_step returns: numpy's mean instead of the wave tree
    def same_rule(blend):
        for comp in components_of(blend):
            sed = comp.children[0].parameters[0]
            rule = sed.step
            sed.step = lambda X, it, rule=rule: rule(X, it)

    ref, blend = _fit_pair(hsc, same_rule)
    assert len(blend._host) == len(components_of(blend))
    # (the loss passes through zero: tolerance relative to its scale)
    assert_allclose(blend.loss, ref.loss, rtol=1e-6, atol=1e-6 * abs(ref.loss[0]))

    class MyChain(scarlet.Constraint):
        def __init__(self):
            self.parts = [scarlet.MonotonicityConstraint(neighbor_weight="angle", min_gradient=0),
                          scarlet.PositivityConstraint(), scarlet.CenterOnConstraint(),
                          scarlet.NormalizationConstraint("max")]

        def __call__(self, X, step):
            for c in self.parts:
                X = c(X, step)
            return X

    def chains(blend):
        for comp in components_of(blend):
            comp.children[1].parameters[0].constraint = MyChain()

    ref, blend = _fit_pair(hsc, chains, n_it=12)
    assert [hp.kind for _, hp in blend._host] == ["morph"] * len(components_of(blend))
    chi = np.array(blend.loss) - float(hsc["log_norm"])
    chi_ref = np.array(ref.loss) - float(hsc["log_norm"])
    assert_allclose(chi, chi_ref, rtol=2e-5)
    for a, b in zip(components_of(ref), components_of(blend)):
        assert np.abs(np.asarray(a.children[1].parameters[0])
                      - np.asarray(b.children[1].parameters[0])).max() < 1e-4


def test_use_mask_on_the_device_and_foreign_chain_orders_host_stepped(hsc):
    """``MonotonicityConstraint(use_mask=True)`` (reference constraint.py:228-232) runs in the
    device chain (SMI_PROX_MONO_MASK): the fit equals the one where the same chain is hidden
    in a user ``Constraint`` and therefore stepped on the host through
    ``operator.prox_monotonic_mask``.  A chain in an order the fused device chain does not
    have runs through the host prox."""
    import scarlet_amd as scarlet

    def chain(fit_center=0):
        return scarlet.ConstraintChain(
            scarlet.MonotonicityConstraint(neighbor_weight="angle", min_gradient=0, use_mask=True,
                                           fit_center_radius=fit_center),
            scarlet.PositivityConstraint(), scarlet.CenterOnConstraint(),
            scarlet.NormalizationConstraint("max"))

    class Hidden(scarlet.Constraint):
        def __init__(self, inner):
            self.inner = inner

        def __call__(self, X, step):
            return self.inner(X, step)

    def masked(blend, wrap=lambda c: c):
        for i, comp in enumerate(components_of(blend)[:3]):
            comp.children[1].parameters[0].constraint = wrap(chain(fit_center=i == 2))

    device, _ = build_blend(hsc, resizing=False)
    masked(device)
    host, _ = build_blend(hsc, resizing=False)
    masked(host, Hidden)
    plain, _ = build_blend(hsc, resizing=False)
    results = [b.fit(12, e_rel=1e-6) for b in (device, host, plain)]
    assert len(device._host) == 0 and len(host._host) == 3
    assert [r[0] for r in results] == [12, 12, 12]
    assert_allclose(device.loss, host.loss, rtol=2e-5)  # the user chain divides by the maximum
    assert not np.allclose(device.loss, plain.loss, rtol=1e-6)  # the mask does something
    for a, b in zip(components_of(device), components_of(host)):
        assert_allclose(np.asarray(a.children[1].parameters[0]),
                        np.asarray(b.children[1].parameters[0]), atol=1e-4)

    blend, _ = build_blend(hsc, resizing=True)
    masked(blend)
    # positivity before monotonicity: not the device order
    components_of(blend)[3].children[1].parameters[0].constraint = scarlet.ConstraintChain(
        scarlet.PositivityConstraint(),
        scarlet.MonotonicityConstraint(neighbor_weight="flat", min_gradient=0.1),
        scarlet.NormalizationConstraint("max"))
    n, logL = blend.fit(25, e_rel=1e-6)
    assert len(blend._host) == 1 and n == 25 and np.isfinite(logL)
    assert logL > -blend.loss[0]
    for comp in components_of(blend)[:4]:
        image = np.asarray(comp.children[1].parameters[0])
        assert image.max() == 1.0 and image.min() >= 0
    # many blends: the host-stepped one fits alone, the others in the batch
    a, _ = build_blend(hsc, resizing=False)
    b, _ = build_blend(hsc, resizing=False)
    masked(b, Hidden)
    c, _ = build_blend(hsc, resizing=False)
    out = scarlet.fit_blends([a, b, c], 8, e_rel=1e-9)
    assert [r[0] for r in out] == [8, 8, 8] and out[0] == out[2] and out[1] != out[0]


@pytest.mark.parametrize("null_renderer", [False, True])
def test_observation_larger_than_the_model_frame(hsc, null_renderer):
    """An observation that sticks out of the model frame: the reference zero-fills the
    model there (renderer.py:130-161), so the outside pixels add a constant to the loss;
    the device loss (smi_batch_add_loss_constant) equals the host evaluation of
    Observation.get_log_likelihood on the same model, for both same-grid renderers."""
    import scarlet_amd as scarlet

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame((5, 40, 36), psf=model_psf, channels=filters)
    obs = scarlet.Observation(hsc["images"], psf=model_psf if null_renderer
                              else scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=filters).match(frame)
    assert type(obs.renderer).__name__ == ("NullRenderer" if null_renderer else "ConvolutionRenderer")
    k = 0
    h, w = hsc["morph_%d" % k].shape
    box = scarlet.Box((5, h, w), origin=(0, 5, 3))
    spectrum = scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                         min_step=hsc["min_step_%d" % k])
    morphology = scarlet.ExtendedSourceMorphology(
        frame, (5 + h // 2, 3 + w // 2), hsc["morph_%d" % k].copy(), bbox=box[1:],
        monotonic="angle", resizing=False)
    blend = scarlet.Blend([scarlet.FactorizedComponent(frame, spectrum, morphology)], obs)
    model = blend.get_model()
    if null_renderer:
        rendered = np.zeros(obs.data.shape, dtype=np.float32)
        rendered[:, :40, :36] = model
        want = -obs.log_norm - np.sum(obs.weights * (rendered - obs.data) ** 2) / 2
    else:
        want = obs.get_log_likelihood(model)
    blend.fit(1, e_rel=1e-9)
    assert blend._loss_constant > 0
    assert abs(-blend.loss[0] - want) < 1e-6 * abs(want)


def test_two_observations_of_the_same_channels(hsc):
    """``Blend._loss_func`` sums over any number of observations (blend.py:264-271).  Two
    same-grid observations that share model channels -- a second exposure of g, r, i with
    another PSF and noise next to the five-band one -- are two terms of the loss and of the
    gradient image (``smi_batch_add_observation``); the fit follows the oracle with the
    same extra term."""
    import scarlet_amd as scarlet
    from oracle import pgm

    filters = list("grizy")
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5)
    frame = scarlet.Frame(hsc["images"].shape, psf=model_psf, channels=filters)
    obs1 = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                               weights=hsc["weights"], channels=filters).match(frame)
    rng = np.random.default_rng(11)
    images2 = (hsc["images"][:3] * 0.9 + rng.normal(0, 0.05, hsc["images"][:3].shape)).astype(np.float32)
    weights2 = (hsc["weights"][:3] * rng.uniform(0.3, 0.6, hsc["weights"][:3].shape)).astype(np.float32)
    weights2[:, :5] = 0  # masked rows
    psfs2 = scarlet.GaussianPSF(sigma=(1.6, 1.7, 1.8), boxsize=31).get_model().astype(np.float32)
    obs2 = scarlet.Observation(images2, psf=scarlet.ImagePSF(psfs2), weights=weights2,
                               channels=filters[:3]).match(frame)

    def sources():
        out = []
        for k in range(int(hsc["n_comp"])):
            h, w = hsc["morph_%d" % k].shape
            oy, ox = hsc["origin_%d" % k]
            box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
            out.append(scarlet.FactorizedComponent(
                frame,
                scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                          min_step=hsc["min_step_%d" % k]),
                scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                                 hsc["morph_%d" % k].copy(), bbox=box[1:],
                                                 resizing=False)))
        return out

    blend = scarlet.Blend(sources(), [obs1, obs2])
    n, logL = blend.fit(15, e_rel=1e-9)
    assert len(blend._extra_layers) == 1 and n == 15

    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    data2 = np.zeros(hsc["images"].shape, dtype=np.float32)
    w2 = np.zeros(hsc["images"].shape, dtype=np.float32)
    data2[:3], w2[:3] = images2, weights2
    k2 = np.asarray(obs2.renderer.kernel_image(), dtype=np.float32)
    ph = max(k2.shape[1], hsc["diff_kernel"].shape[1]) | 1
    kernel2 = np.zeros((5, ph, ph), dtype=np.float32)
    kernel2[:, ph // 2, ph // 2] = 1  # unobserved channels: weight zero, any kernel
    o = ph // 2 - k2.shape[1] // 2
    kernel2[:3, o:o + k2.shape[1], o:o + k2.shape[2]] = k2
    sc.extra_observations = [pgm.SameGridObservation(data2, w2, kernel2)]
    n_ref, logL_ref = sc.fit(15, e_rel=1e-9)
    assert n_ref == 15
    off = sc.log_norm + sc.extra_observations[0].log_norm
    chi, chi_ref = np.array(blend.loss) - off, np.array(sc.loss) - off
    assert_allclose(chi[0], chi_ref[0], rtol=RTOL)
    assert_allclose(chi, chi_ref, rtol=2e-4)
    assert chi[-1] < chi[0]
    # and the single-observation fit is something else
    alone = scarlet.Blend(sources(), obs1)
    alone.fit(3, e_rel=1e-9)
    assert abs(alone.loss[0] - blend.loss[0]) > 1e-3 * abs(blend.loss[0])


def test_free_psf_shift_next_to_a_second_observation(hsc):
    """Blend.fit collects the parameters of ALL observations (blend.py:103-105): an observation
    whose ConvolutionRenderer carries a free ``psf_shift`` next to a second exposure of three of
    the bands.  On the device the shifted observation is the first layer (its kernel moves,
    ``smi_batch_set_kernel_shift``), the other one a further term of the loss
    (``smi_batch_add_observation``); whichever order the user lists them in.  Against the
    oracle: losses, the shift, its moments."""
    import scarlet_amd as scarlet
    from scarlet_amd.renderer import ConvolutionRenderer
    from conftest import golden
    from oracle import pgm

    gp = golden("hsc_psf_shift")
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    rng = np.random.default_rng(11)
    images2 = (hsc["images"][:3] * 0.9 + rng.normal(0, 0.05, hsc["images"][:3].shape)).astype(np.float32)
    weights2 = (hsc["weights"][:3] * rng.uniform(0.3, 0.6, hsc["weights"][:3].shape)).astype(np.float32)
    psfs2 = scarlet.GaussianPSF(sigma=(1.6, 1.7, 1.8), boxsize=31).get_model().astype(np.float32)

    def blend_of(shifted_first):
        obs1 = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                                   weights=hsc["weights"], channels=filters)
        obs1.match(frame, renderer=ConvolutionRenderer(obs1, frame, psf_shift=gp["psf_shift"].copy()))
        obs2 = scarlet.Observation(images2, psf=scarlet.ImagePSF(psfs2), weights=weights2,
                                   channels=filters[:3]).match(frame)
        comps = []
        for k in range(int(hsc["n_comp"])):
            h, w = hsc["morph_%d" % k].shape
            oy, ox = hsc["origin_%d" % k]
            box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
            comps.append(scarlet.FactorizedComponent(
                frame,
                scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                          min_step=hsc["min_step_%d" % k]),
                scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                                 hsc["morph_%d" % k].copy(), bbox=box[1:],
                                                 resizing=False)))
        return scarlet.Blend(comps, [obs1, obs2] if shifted_first else [obs2, obs1]), obs1, obs2

    blend, obs1, obs2 = blend_of(True)
    n, logL = blend.fit(12, e_rel=1e-9)
    assert n == 12 and blend._psf_stepped_on_device and len(blend._extra_layers) == 1

    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.psf_shift = gp["psf_shift"].copy()
    data2 = np.zeros(hsc["images"].shape, dtype=np.float32)
    w2 = np.zeros(hsc["images"].shape, dtype=np.float32)
    data2[:3], w2[:3] = images2, weights2
    k2 = np.asarray(obs2.renderer.kernel_image(), dtype=np.float32)
    ph = max(k2.shape[1], hsc["diff_kernel"].shape[1]) | 1
    kernel2 = np.zeros((5, ph, ph), dtype=np.float32)
    kernel2[:, ph // 2, ph // 2] = 1  # unobserved channels: weight zero, any kernel
    o = ph // 2 - k2.shape[1] // 2
    kernel2[:3, o:o + k2.shape[1], o:o + k2.shape[2]] = k2
    sc.extra_observations = [pgm.SameGridObservation(data2, w2, kernel2)]
    n_ref, _ = sc.fit(12, e_rel=1e-9)
    assert n_ref == 12
    off = sc.log_norm + sc.extra_observations[0].log_norm
    chi, chi_ref = np.array(blend.loss) - off, np.array(sc.loss) - off
    assert_allclose(chi[0], chi_ref[0], rtol=RTOL)
    assert_allclose(chi, chi_ref, rtol=2e-4)
    shift = obs1.parameters[0]
    assert np.abs(np.asarray(shift) - sc.psf_shift).max() < 2e-5
    assert np.abs(np.asarray(shift) - gp["psf_shift"]).max() > 1e-3  # it moved
    assert_allclose(shift.vhat, sc.vhat_psf, rtol=2e-3)
    # the order of the observations does not matter
    other, obs1b, _ = blend_of(False)
    other.fit(12, e_rel=1e-9)
    assert_allclose(other.loss, blend.loss, rtol=1e-12)
    assert_allclose(np.asarray(obs1b.parameters[0]), np.asarray(shift), rtol=0, atol=1e-15)


def test_free_psf_shifts_of_two_observations(hsc):
    """``Blend.fit`` collects the parameters of EVERY observation (blend.py:103-105): two
    observations -- bands g, r, i of one instrument, z, y of another -- whose
    ``ConvolutionRenderer``s each carry a free ``psf_shift``.  The device moves one set of
    kernels, so both shifts are stepped on the host (``Blend._fit_with_psf_shifts``; round 5
    refused).  Against the oracle with one shift per group of bands: losses, both shifts."""
    import scarlet_amd as scarlet
    from scarlet_amd.renderer import ConvolutionRenderer
    from conftest import golden

    gp = golden("hsc_psf_shift")
    filters = list("grizy")
    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=filters)
    s1, s2 = gp["psf_shift"].copy(), np.array([-0.12, 0.07])
    obs1 = scarlet.Observation(hsc["images"][:3], psf=scarlet.ImagePSF(hsc["psfs"][:3].copy()),
                               weights=hsc["weights"][:3], channels=filters[:3])
    obs1.match(frame, renderer=ConvolutionRenderer(obs1, frame, psf_shift=s1.copy()))
    obs2 = scarlet.Observation(hsc["images"][3:], psf=scarlet.ImagePSF(hsc["psfs"][3:].copy()),
                               weights=hsc["weights"][3:], channels=filters[3:])
    obs2.match(frame, renderer=ConvolutionRenderer(obs2, frame, psf_shift=s2.copy()))
    comps = []
    for k in range(int(hsc["n_comp"])):
        h, w = hsc["morph_%d" % k].shape
        oy, ox = hsc["origin_%d" % k]
        box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
        comps.append(scarlet.FactorizedComponent(
            frame,
            scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                      min_step=hsc["min_step_%d" % k]),
            scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                             hsc["morph_%d" % k].copy(), bbox=box[1:],
                                             resizing=False)))
    blend = scarlet.Blend(comps, [obs1, obs2])
    seen = []
    n, _ = blend.fit(8, e_rel=1e-9, callback=lambda *X, it: seen.append((it, len(X))))
    assert n == 8 and seen[0] == (0, len(blend.parameters) + 2)  # both shifts behind the sources'

    sc = hsc_scene(hsc)
    for c in sc.components:
        c.source = None
    sc.psf_groups = [dict(bands=[0, 1, 2], shift=s1.copy(), step=1e-2),
                     dict(bands=[3, 4], shift=s2.copy(), step=1e-2)]
    n_ref, _ = sc.fit(8, e_rel=1e-9)
    assert n_ref == 8
    assert_allclose(np.array(blend.loss) - sc.log_norm, np.array(sc.loss) - sc.log_norm, rtol=2e-4)
    for obs, start, group in ((obs1, s1, sc.psf_groups[0]), (obs2, s2, sc.psf_groups[1])):
        shift = obs.parameters[0]
        assert np.abs(np.asarray(shift) - group["shift"]).max() < 3e-5
        assert np.abs(np.asarray(shift) - start).max() > 1e-3  # it moved
        assert shift.m is not None and shift.std.shape == (2,)


def test_user_defined_linear_renderer_matches_the_device_renderer(hsc):
    """Plug-in seam (SURVEY 8b seam 3): ``Observation.match(frame, renderer=<a Renderer
    subclass>)`` (observation.py:59-112).  A user-written Python renderer -- here the PSF
    convolution re-implemented with NumPy FFTs, plus its transpose as ``adjoint`` -- is host
    code: Blend.fit renders and pulls back on the host and keeps the component updates on
    the device.  It must reproduce the fit with the built-in ConvolutionRenderer; a renderer
    without ``adjoint``, or whose ``adjoint`` is not its transpose, is refused."""
    import scarlet_amd as scarlet
    from scarlet_amd import fft
    from scarlet_amd.renderer import Renderer

    class NumpyConvolution(Renderer):
        def __init__(self, data_frame, model_frame):
            super().__init__(data_frame, model_frame)
            self.kernel = np.asarray(fft.match_psf(
                fft.Fourier(data_frame.psf.get_model().astype(np.float32)),
                fft.Fourier(model_frame.psf.get_model().astype(np.float32)), padding=10).image,
                dtype=np.float64)

        def get_model(self, *parameters):
            return lambda model: fft.convolve(fft.Fourier(np.asarray(model, np.float64)),
                                              self.kernel, axes=(1, 2)).image

        def adjoint(self, residual):
            return fft.convolve(fft.Fourier(residual), self.kernel[:, ::-1, ::-1], axes=(1, 2)).image

    class NoAdjoint(NumpyConvolution):
        adjoint = None

    class WrongAdjoint(NumpyConvolution):
        def adjoint(self, residual):
            return 2.0 * NumpyConvolution.adjoint(self, residual)

    filters = list("grizy")

    def build(renderer_cls):
        frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                              channels=filters)
        obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"]),
                                  weights=hsc["weights"], channels=filters)
        obs.match(frame) if renderer_cls is None else obs.match(frame, renderer=renderer_cls(obs, frame))
        comps = []
        for k in range(int(hsc["n_comp"])):
            h, w = hsc["morph_%d" % k].shape
            oy, ox = hsc["origin_%d" % k]
            box = scarlet.Box((5, h, w), origin=(0, int(oy), int(ox)))
            comps.append(scarlet.FactorizedComponent(
                frame,
                scarlet.TabulatedSpectrum(frame, hsc["sed_%d" % k].copy(), bbox=box[0],
                                          min_step=hsc["min_step_%d" % k]),
                scarlet.ExtendedSourceMorphology(frame, (oy + h // 2, ox + w // 2),
                                                 hsc["morph_%d" % k].copy(), bbox=box[1:])))
        return scarlet.Blend(comps, obs), obs

    device, obs_d = build(None)
    n_d, logL_d = device.fit(25, e_rel=1e-9)
    user, obs_u = build(NumpyConvolution)
    assert np.abs(obs_u.render(hsc["model"]) - hsc["rendered"]).max() < 1e-5 * np.abs(hsc["rendered"]).max()
    n_u, logL_u = user.fit(25, e_rel=1e-9)
    assert n_u == n_d == 25
    log_norm = obs_d.log_norm
    assert_allclose(np.array(user.loss) - log_norm, np.array(device.loss) - log_norm, rtol=2e-5)
    # boxes after the resize hooks of iterations 11 and 21, parameters, optimizer state
    for a, b in zip(components_of(user), components_of(device)):
        assert a.children[1].bbox == b.children[1].bbox
        for pa, pb in zip(a.parameters, b.parameters):
            assert np.abs(np.asarray(pa) - np.asarray(pb)).max() < 2e-4 * max(np.abs(np.asarray(pb)).max(), 1e-3)
            assert (pa.m is None) == (pb.m is None) and (pa.std is None) == (pb.std is None)
    # the stopping rule of the host loop
    short, _ = build(NumpyConvolution)
    ref, _ = build(None)
    assert short.fit(100, e_rel=1e-3)[0] == ref.fit(100, e_rel=1e-3)[0] < 100
    for bad in (NoAdjoint, WrongAdjoint):
        blend, _ = build(bad)
        with pytest.raises(NotImplementedError):
            blend.fit(3)
