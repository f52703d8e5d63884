"""Profile sources (GaussianSource, SpergelSource) without a GPU: the mirror classes and the
oracle (tests/profile_oracle.py) pinned to the reference's recorded results
(tests/golden/profile_source.npz, tools/make_golden_profile.py)."""

import warnings
from functools import partial

import numpy as np
import pytest

from conftest import golden

import profile_oracle as po

FILTERS = list("grizy")
GROUPS = po.GROUPS
# multiple of the Richardson error estimate |FD(h/2) - FD(h)| the oracle's gradient may be away
# from the extrapolated value (4 FD(h/2) - FD(h)) / 3: the estimate is the h^2 term of FD(h/2)
# three times over, the extrapolation removes it and leaves O(h^4); 1 x the estimate is already
# generous, and the round-off of the four likelihood values comes on top
FD_MULTIPLE = 1.0
# likelihood values entering the two differences (2 each), each rounded at eps |logL|
FD_VALUES = 4


@pytest.fixture(scope="module")
def g():
    return golden("profile_source")


def profile_indices(g):
    return [k for k in range(int(g["n_sources"])) if str(g["kinds"][k]) != "extended"]


def mirror_scene(g, hsc, dtype=np.float32):
    """The fixture's profile sources through the mirror classes, on the hsc_cosmos_35 frame."""
    import scarlet_amd as scarlet

    frame = scarlet.Frame(hsc["images"].shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * 5),
                          channels=FILTERS, dtype=dtype)
    obs = scarlet.Observation(hsc["images"], psf=scarlet.ImagePSF(hsc["psfs"].copy()),
                              weights=hsc["weights"], channels=FILTERS).match(frame)
    sources = {}
    for k in profile_indices(g):
        p = g["params_%d" % k]
        sky = tuple(g["sky_coords"][k])
        if str(g["kinds"][k]) == "gaussian":
            sources[k] = scarlet.GaussianSource(frame, sky, float(p[2]), p[3:5].copy(), obs)
        else:
            sources[k] = scarlet.SpergelSource(frame, sky, float(p[5]), float(p[2]), p[3:5].copy(), obs)
    return frame, obs, sources


# -- construction -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_sources_equal_the_fixture(g, hsc, dtype):
    import scarlet_amd as scarlet

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no DeprecationWarning from ceil(10 * array))
        frame, obs, sources = mirror_scene(g, hsc, dtype)
    kinds = set()
    for k, src in sources.items():
        spectrum, morphology = src.children
        kinds.add(type(morphology))
        assert tuple(morphology.bbox.origin) == tuple(g["origin_%d" % k])
        assert tuple(morphology.bbox.shape) == tuple(g["shape_%d" % k])
        own = morphology.parameters
        assert [p.name for p in own] == list(g["pnames_%d" % k])
        assert [str(p.dtype) for p in own] == list(g["pdtypes_%d" % k])
        assert [p.shape[0] for p in own] == list(g["pshapes_%d" % k])
        assert [bool(p.fixed) for p in own] == list(g["pfixed_%d" % k])
        steps = [float(np.asarray(p.step(p, it=0) if callable(p.step) else p.step)) for p in own]
        np.testing.assert_array_equal(steps, g["pstep0_%d" % k])
        for name, sl in zip(GROUPS, po.SLOTS):
            p = morphology.get_parameter(name)
            if p is not None:
                np.testing.assert_array_equal(np.asarray(p), g["params_%d" % k][sl])
        assert src.center is morphology.center and src.center.name == "center"
        sed = spectrum.parameters[0]
        ref_sed = g["sed64_%d" % k] if dtype == np.float64 and "sed64_%d" % k in g.files \
            else g["sed_%d" % k]
        assert sed.name == "spectrum" and sed.constraint.zero == float(g["sed_zero_%d" % k])
        # the peak value f(0) divides the spectrum: float32 round-off
        np.testing.assert_allclose(np.asarray(sed), ref_sed, rtol=2 * np.finfo(np.float32).eps)
        np.testing.assert_allclose(sed.step.keywords["minimum"], g["sed_step_minimum_%d" % k],
                                   rtol=2 * np.finfo(np.float32).eps)
        assert sed.step.keywords["factor"] == float(g["sed_step_factor_%d" % k])
        model = morphology.get_model()
        assert model.dtype == np.float64
        assert np.abs(model - g["morph_%d" % k]).max() <= 1e-12 * g["morph_%d" % k].max()
        np.testing.assert_allclose(np.asarray(morphology.integral, dtype=np.float64),
                                   g["integral_%d" % k], rtol=1e-14)
        # get_model(*parameters) takes the parameters by name
        moved = [p.copy() for p in own]
        moved[0][...] += 0.25
        assert np.abs(morphology.get_model(*moved) - model).max() > 1e-3
    assert kinds == {scarlet.GaussianMorphology, scarlet.SpergelMorphology}


def test_measure_works_on_profile_sources(g, hsc):
    import scarlet_amd as scarlet

    frame, obs, sources = mirror_scene(g, hsc)
    for k, src in sources.items():
        flux = scarlet.measure.flux(src)
        sed = np.asarray(src.children[0].parameters[0], dtype=np.float64)
        np.testing.assert_allclose(flux, sed * src.children[1].get_model().sum(), rtol=1e-6)
        assert np.all(np.isfinite(scarlet.measure.centroid(src)))


def test_plain_numbers_become_fixed_parameters():
    import scarlet_amd as scarlet

    frame = scarlet.Frame((3, 40, 50), channels=list("gri"))
    m = scarlet.GaussianMorphology(frame, (20.2, 30.7), 2.0)
    assert [p.name for p in m.parameters] == ["center", "radius", "ellipticity"]
    assert all(p.fixed and p.dtype == np.float64 for p in m.parameters)
    assert tuple(m.bbox.shape) == (20, 20) and tuple(m.bbox.origin) == (10, 21)
    s = scarlet.SpergelMorphology(frame, (20.2, 30.7), 0.5, 1.5, boxsize=31)
    assert [p.name for p in s.parameters] == ["center", "nu", "radius", "ellipticity"]
    assert all(p.fixed for p in s.parameters) and tuple(s.bbox.shape) == (31, 31)
    # a subset may be free
    free = scarlet.Parameter(np.array([2.0]), name="radius", step=scarlet.relative_step)
    m = scarlet.GaussianMorphology(frame, (20.2, 30.7), free)
    assert [p.fixed for p in m.parameters] == [True, False, True]


def test_ellipticity_quirks_are_named():
    import scarlet_amd as scarlet

    frame = scarlet.Frame((3, 40, 50), channels=list("gri"))
    obs = scarlet.Observation(np.ones((3, 40, 50), dtype=np.float32),
                              weights=np.ones((3, 40, 50), dtype=np.float32),
                              channels=list("gri")).match(frame)
    with pytest.raises(TypeError, match="ellipticity"):
        scarlet.GaussianSource(frame, (20, 30), 2.0, None, obs)
    with pytest.raises(TypeError, match="ndarray"):
        scarlet.GaussianSource(frame, (20, 30), 2.0, (0.0, 0.0), obs)
    with pytest.raises(ValueError, match="shape"):
        scarlet.SpergelSource(frame, (20, 30), 0.5, 2.0, np.zeros(3), obs)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        scarlet.GaussianSource(frame, (20, 30), 2.0, np.zeros(2), obs)
        scarlet.SpergelSource(frame, (20, 30), 0.5, 2.0, np.zeros(2), obs)


# -- update() ---------------------------------------------------------------------------------
def test_update_reproduces_the_recorded_box_table(g):
    import scarlet_amd as scarlet

    frame = scarlet.Frame((5, 58, 48), channels=FILTERS)
    assert g["box_raised"].any() and not g["box_raised"].all()
    for case, first, after, raised in zip(g["box_cases"], g["box_first"], g["box_after"],
                                          g["box_raised"]):
        center = scarlet.Parameter(case[0:2].copy(), name="center", step=0.01)
        radius = scarlet.Parameter(case[2:3].copy(), name="radius", step=0.1)
        m = scarlet.GaussianMorphology(frame, center, radius)
        assert tuple(m.bbox.origin) + (m.bbox.shape[-1],) == tuple(first)
        center[:] = case[3:5]
        radius[:] = case[5]
        moments = (radius.m, radius.v, radius.vhat)
        if raised:
            with pytest.raises(scarlet.UpdateException):
                m.update()
        else:
            m.update()
        assert tuple(m.bbox.origin) + (m.bbox.shape[-1],) == tuple(after), case
        assert m.get_model().shape == (after[2], after[2])
        assert m.parameters[1] is radius and (radius.m, radius.v, radius.vhat) == moments
        # the oracle's rule is the same
        assert po.get_box([case[3], case[4], case[5], 0, 0, 0]) == tuple(after)


# -- the oracle against the reference ----------------------------------------------------------
def test_oracle_reproduces_the_reference_model_and_likelihood(g, hsc):
    sc = po.fixture_scene(g, hsc)
    for k in profile_indices(g):
        ref = g["morph_%d" % k]
        assert np.abs(sc.components[k].morph - ref).max() <= 1e-12 * ref.max()
    model = sc.get_model()
    assert model.dtype == g["model"].dtype
    scale = np.abs(g["model"]).max()
    assert np.abs(model.astype(np.float64) - g["model"]).max() <= 1e-12 * scale
    rendered = sc.render(model)
    assert np.abs(rendered.astype(np.float64) - g["rendered"]).max() <= 1e-12 * np.abs(g["rendered"]).max()
    logL = sc.log_likelihood(rendered)
    assert abs(logL - float(g["logL"])) <= 1e-12 * abs(float(g["logL"]))
    sc64 = po.fixture_scene(g, hsc, dtype64=True)
    logL = sc64.log_likelihood(sc64.render(sc64.get_model()))
    assert abs(logL - float(g["logL64"])) <= 1e-12 * abs(float(g["logL64"]))


def richardson(fd):
    return (4 * fd[1] - fd[0]) / 3


def fd_bound(g, fd):
    """|FD(h/2) - FD(h)| times FD_MULTIPLE plus the cancellation floor of the differences: each
    of the FD_VALUES likelihood values is rounded at eps |logL|, divided by the smaller
    denominator 2 (h/2) = h, and the extrapolation weights (4 + 1) / 3 them."""
    h = float(g["fd_h"])
    floor = FD_VALUES * np.finfo(np.float64).eps * abs(float(g["logL64"])) / h * 5 / 3
    return FD_MULTIPLE * np.abs(fd[1] - fd[0]) + floor


def test_oracle_gradient_against_the_reference_finite_differences(g, hsc):
    """every profile parameter and every spectrum entry, none left out"""
    sc = po.fixture_scene(g, hsc, dtype64=True)
    grads = sc.profile_gradients()
    assert sorted(grads) == profile_indices(g)
    n = 0
    for k, (g_sed, g_par) in grads.items():
        spergel = str(g["kinds"][k]) == "spergel"
        fd = g["fd_sed_%d" % k]
        # the fixture holds d logL, the oracle's gradient is of -logL
        err = np.abs(g_sed + richardson(fd))
        print(k, "spectrum", err, fd_bound(g, fd))
        assert np.all(err <= fd_bound(g, fd)), (k, err, fd_bound(g, fd))
        n += len(err)
        fd = g["fd_param_%d" % k]
        entries = range(6 if spergel else 5)
        assert np.all(np.isfinite(fd[:, list(entries)]))
        for j in entries:
            err = abs(g_par[j] + richardson(fd[:, j]))
            print(k, j, g_par[j], err, fd_bound(g, fd[:, j]))
            assert err <= fd_bound(g, fd[:, j]), (k, j, err, fd_bound(g, fd[:, j]))
            n += 1
    assert n == 3 * (5 + 5) + (5 + 6)


def test_nu_gradient_is_the_frozen_order_one(g, hsc):
    sc = po.fixture_scene(g, hsc, dtype64=True)
    grads = sc.profile_gradients()
    (k,) = [k for k in profile_indices(g) if str(g["kinds"][k]) == "spergel"]
    frozen, unfrozen = g["fd_param_%d" % k][:, 5], g["fd_nu_unfrozen_%d" % k]
    bound = fd_bound(g, frozen)
    assert abs(grads[k][1][5] + richardson(frozen)) <= bound
    gap = abs(grads[k][1][5] + richardson(unfrozen))
    print("nu: frozen", richardson(frozen), "unfrozen", richardson(unfrozen), "bound", bound)
    assert gap > bound + fd_bound(g, unfrozen)


# -- proximal operators -----------------------------------------------------------------------
def test_proximal_operators_on_hand_cases():
    import scarlet_amd as scarlet

    frame = scarlet.Frame((3, 40, 50), channels=list("gri"))
    s = scarlet.SpergelMorphology(frame, (20.0, 30.0), 0.5, 1.5)
    radius, eps, nu = (s.get_parameter(n) for n in ("radius", "ellipticity", "nu"))
    assert s.get_parameter("center").constraint is None
    for mirror, oracle in ((radius.constraint, partial(po.prox, 1)), (eps.constraint, partial(po.prox, 2)),
                           (nu.constraint, partial(po.prox, 3))):
        for x in ([1e-3], [-2.0], [0.5], [0.6, 0.9], [3.0, -4.0], [0.6, 0.7], [-0.9], [4.5], [4.0]):
            x = np.array(x)
            np.testing.assert_array_equal(mirror(x.copy(), 0.1), oracle(x.copy()))
    np.testing.assert_array_equal(radius.constraint(np.array([1e-3]), 0), [1e-2])
    np.testing.assert_array_equal(radius.constraint(np.array([0.3]), 0), [0.3])
    out = eps.constraint(np.array([3.0, -4.0]), 0)
    np.testing.assert_allclose(out, np.array([3.0, -4.0]) / 5.5, rtol=1e-15)
    assert np.hypot(*out) < 1
    np.testing.assert_array_equal(eps.constraint(np.array([0.6, 0.7]), 0), [0.6, 0.7])
    np.testing.assert_array_equal(nu.constraint(np.array([-0.9]), 0), [-0.85])
    np.testing.assert_array_equal(nu.constraint(np.array([4.5]), 0), [4.0])


# -- refusals: all of them before the library is loaded -----------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from scarlet_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


def small_blend(**changes):
    """One free GaussianSource and one SpergelSource on a small frame; ``changes``: attributes
    set on a named parameter, e.g. ``radius=dict(step=...)``."""
    import scarlet_amd as scarlet

    rng = np.random.default_rng(3)
    frame = scarlet.Frame((3, 40, 50), channels=list("gri"))
    obs = scarlet.Observation(1 + rng.random((3, 40, 50)).astype(np.float32),
                              weights=np.ones((3, 40, 50), dtype=np.float32),
                              channels=list("gri")).match(frame)
    sources = [scarlet.GaussianSource(frame, (20, 30), 2.0, np.zeros(2), obs),
               scarlet.SpergelSource(frame, (12, 14), 0.5, 2.0, np.zeros(2), obs)]
    for name, attrs in changes.items():
        p = sources[1].children[1].get_parameter(name)
        for attr, value in attrs.items():
            setattr(p, attr, value)
    return scarlet.Blend(sources, obs), sources


def test_refusals_come_before_any_device_work(no_device):
    import scarlet_amd as scarlet
    from scarlet_amd import _lib

    class Flat(scarlet.Prior):
        def __call__(self, x):
            return 0.0

        def grad(self, x):
            return np.zeros_like(x)

    blend, _ = small_blend()
    with pytest.raises(NotImplementedError, match="scheme"):
        blend.fit(5, scheme="adam")
    for changes, word in (
            (dict(radius=dict(prior=Flat())), "prior"),
            (dict(center=dict(constraint=scarlet.PositivityConstraint())), "constraint"),
            (dict(nu=dict(constraint=scarlet.PositivityConstraint())), "constraint"),
            (dict(ellipticity=dict(step=lambda x, it=0: 0.01)), "step"),
            (dict(radius=dict(step=partial(scarlet.relative_step, axis=0))), "step")):
        blend, _ = small_blend(**changes)
        with pytest.raises(NotImplementedError, match=word):
            blend.fit(5)
        with pytest.raises(NotImplementedError, match=word):
            scarlet.fit_blends([blend], 5)

    # a profile function of the user's has no gradient
    class Exponential(scarlet.GaussianMorphology):
        def _f(self, R2, *parameters):
            return np.exp(-np.sqrt(R2))

    blend, sources = small_blend()
    frame = sources[0].frame
    own = Exponential(frame, scarlet.Parameter(np.array([20.0, 30.0]), name="center", step=0.01), 2.0)
    custom = scarlet.FactorizedComponent(frame, sources[0].children[0], own)
    with pytest.raises(NotImplementedError, match="Exponential"):
        scarlet.Blend([custom], blend.observations).fit(5)

    # FISTA and frame extents are settings of the batch; lite has no profile sources
    spec = scarlet.ComponentSpec(np.ones(3), np.zeros((21, 21)), (3, 4), profile=dict(
        kind=_lib.PROFILE_GAUSSIAN, params=[13.0, 14.0, 2.0, 0, 0, 0], step=[0.01, 0, 0.01, 0],
        rel_step=[0, 0.1, 0, 0]))
    assert spec.prox_flags == _lib.COMPONENT_PROFILE
    data = np.zeros((1, 3, 40, 50), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="FISTA"):
        scarlet.BlendBatch(data, data, [[spec]], scheme="fista")
    with pytest.raises(NotImplementedError, match="frame extents"):
        scarlet.BlendBatch(data, data, [[spec]], frame_shapes=[(30, 40)])
    from scarlet_amd import lite

    with pytest.raises(NotImplementedError, match="lite"):
        lite.LiteBlend([sources[0]], None)
    with pytest.raises(NotImplementedError, match="lite"):
        lite.LiteSource([sources[1]], np.float32)


def test_device_description_of_the_stock_sources(no_device):
    from scarlet_amd import _lib
    from scarlet_amd.blend import _profile_rules

    _, sources = small_blend()
    gauss = _profile_rules(sources[0].children[1], "amsgrad")
    assert gauss["kind"] == _lib.PROFILE_GAUSSIAN and gauss["fixed"] == 8
    np.testing.assert_array_equal(gauss["step"], [0.01, 0.0, 0.01, 0.0])
    np.testing.assert_array_equal(gauss["rel_step"], [0.0, 0.1, 0.0, 0.0])
    np.testing.assert_array_equal(gauss["params"], [20, 30, 2, 0, 0, 0])
    sperg = _profile_rules(sources[1].children[1], "amsgrad")
    assert sperg["kind"] == _lib.PROFILE_SPERGEL and sperg["fixed"] == 0
    np.testing.assert_array_equal(sperg["step"], [0.01, 0.0, 0.01, 0.01])
    np.testing.assert_array_equal(sperg["rel_step"], [0.0, 0.01, 0.0, 0.0])
    np.testing.assert_array_equal(sperg["params"], [12, 14, 2, 0, 0, 0.5])
    # the all-fixed morphology built from plain numbers
    import scarlet_amd as scarlet

    m = scarlet.GaussianMorphology(sources[0].frame, (20.2, 30.7), 2.0)
    fixed = _profile_rules(m, "amsgrad")
    assert fixed["fixed"] == 15 and not fixed["step"].any() and not fixed["rel_step"].any()


def test_exports_and_hook_coverage():
    import scarlet_amd as sa
    from scarlet_amd.fitting import _device_hook_covers

    for name in ("GaussianSource", "SpergelSource", "ProfileMorphology", "GaussianMorphology",
                 "SpergelMorphology"):
        assert hasattr(sa, name)
    # a profile source keeps its blend off the resident loop: its hook is the host's
    _, sources = small_blend()
    assert not any(_device_hook_covers(s) for s in sources)
