"""Starlet sources without a GPU: the oracle (tests/starlet_oracle.py) pinned to the
reference's recorded results, and the host-side pieces of the mirror classes."""

import numpy as np
import pytest

from conftest import golden

import starlet_oracle as so

SHAPES = [(21, 21), (41, 41), (58, 48), (191, 191), (7, 33)]


@pytest.fixture(scope="module")
def g():
    return golden("starlet_source")


def test_oracle_reproduces_the_reference_model_and_likelihood(g, hsc):
    sc = so.fixture_scene(g, hsc)
    model = sc.get_model()
    assert model.dtype == g["model"].dtype
    scale = np.abs(g["model"]).max()
    assert np.abs(model.astype(np.float64) - g["model"]).max() <= 1e-12 * scale
    rendered = sc.render(model)
    assert np.abs(rendered.astype(np.float64) - g["rendered"]).max() <= 1e-5 * np.abs(g["rendered"]).max()
    logL = sc.log_likelihood(rendered)
    assert abs(logL - float(g["logL"])) <= 1e-12 * abs(float(g["logL"]))


def test_oracle_float64_scene_reproduces_the_reference_likelihood(g, hsc):
    sc = so.fixture_scene(g, hsc, dtype64=True)
    logL = sc.log_likelihood(sc.render(sc.get_model()))
    assert abs(logL - float(g["logL64"])) <= 1e-12 * abs(float(g["logL64"]))


def test_coefficient_gradient_against_the_reference_finite_differences(g, hsc):
    """analytic cascade vs central differences (h = 1e-3) of the reference's own logL on the
    float64 frame: within 1e-7 of the plane's peak gradient (measured: ~1e-10)"""
    sc = so.fixture_scene(g, hsc, dtype64=True)
    _, grads = sc.loss_and_gradients()
    for k in g["starlet_of"]:
        g_coeffs = grads[int(k)][1]
        idx = g["fd_index_%d" % k]
        assert len(idx) >= 12
        planes = set(int(p) for p in idx[:, 0])
        assert g_coeffs.shape[0] - 1 in planes  # the last plane is among them
        for (p, y, x), fd in zip(idx, g["fd_dlogL_%d" % k]):
            peak = np.abs(g_coeffs[p]).max()
            # the fixture holds d logL, the oracle's gradient is of -logL
            err = abs(g_coeffs[p, y, x] + fd)
            print(int(k), (int(p), int(y), int(x)), err / peak)
            assert err <= 1e-7 * peak, (int(k), (int(p), int(y), int(x)), err / peak)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identity_of_the_cascade(shape):
    """<R c, g> = <c, R^T g> to 1e-13"""
    rng = np.random.default_rng(5)
    S = so.get_scales(shape)
    c = rng.standard_normal((S + 1,) + shape)
    gimg = rng.standard_normal(shape)
    lhs = np.sum(so.reconstruct(c) * gimg)
    rhs = np.sum(c * so.cascade(gimg, S))
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs), np.sqrt(c.size))


def test_oracle_transform_and_thresholds_match_the_reference(g):
    for k in g["starlet_of"]:
        coeffs = g["coeffs_%d" % k]
        image = so.reconstruct(coeffs)
        again = so.transform(image, coeffs.shape[0] - 1)
        assert np.abs(again - coeffs).max() <= 1e-12 * np.abs(coeffs).max()
        assert np.allclose(so.norm(coeffs.shape[1:]), g["norm_%d" % k], rtol=1e-12)
        assert np.allclose(so.thresholds(coeffs.shape[1:], 5e-3), g["thresh_%d" % k], rtol=1e-12)
        comp = so.StarletComponent(np.ones(5), coeffs.copy(), (0, 0), g["thresh_%d" % k])
        once = comp.morph_prox(coeffs.copy(), 0)
        assert np.array_equal(np.packbits((once != 0).ravel()), g["chain_once_support_%d" % k])
        assert np.allclose(once.sum(axis=(1, 2)), g["chain_once_sum_%d" % k], rtol=1e-12)


def test_oracle_runs_forty_iterations_with_equal_supports_in_both_state_precisions(g, hsc):
    """what makes the project's trajectory tolerances plausible for this scene: the hard
    threshold does not make it precision-sensitive"""
    a = so.fixture_scene(g, hsc)
    b = so.fixture_scene(g, hsc, state_dtype=np.float32)
    for it in range(40):
        a.step(it, 1e-3)
        b.step(it, 1e-3)
    rel = np.abs(np.array(a.loss) - np.array(b.loss)) / np.abs(np.array(a.loss))
    print("loss, float32 vs float64 state:", rel.max())
    for k in g["starlet_of"]:
        ca, cb = a.components[int(k)].morph, b.components[int(k)].morph
        assert np.array_equal(ca != 0, cb != 0)
        assert np.abs(ca - cb).max() <= 1e-4 * np.abs(ca).max()
    assert rel.max() < 1e-4


# -- the host side of the mirror classes -------------------------------------------------------
def test_starlet_thresholds_from_a_norm(g):
    from scarlet_amd.morphology import starlet_thresholds

    for k in g["starlet_of"]:
        t = starlet_thresholds(g["norm_%d" % k], 5e-3)
        assert np.array_equal(t, g["thresh_%d" % k])
    assert np.array_equal(starlet_thresholds([2.0, 1.0, 0.5], 0.1), [0.2, 0.1, 0.0])
    assert np.array_equal(starlet_thresholds([3.0], 1.0), [0.0])


def test_shrink_slices():
    from scarlet_amd.morphology import shrink_slices

    # 41^2 at (5, 7) -> 21^2 ten pixels further in
    assert shrink_slices((5, 7), (41, 41), (15, 17), (21, 21)) == (slice(10, 31), slice(10, 31))
    # leading (channel) entries are ignored
    assert shrink_slices((0, 5, 7), (5, 41, 41), (0, 15, 17), (5, 21, 21)) == \
        (slice(10, 31), slice(10, 31))
    # a new box that leaves the old one is clipped to the overlap
    assert shrink_slices((0, 0), (58, 48), (3, -2), (51, 51)) == (slice(3, 54), slice(0, 48))


def test_plane_thresholds_reads_the_chain_and_nothing_else():
    import scarlet_amd as sa
    from scarlet_amd.morphology import plane_thresholds

    per_plane = np.array([0.3, 0.1, 0.0])
    full = np.broadcast_to(per_plane[:, None, None], (3, 7, 9)).copy()
    chain = sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(full))
    floor, t = plane_thresholds(chain)
    assert floor == 0 and np.array_equal(t, per_plane)
    assert plane_thresholds(sa.ConstraintChain(sa.PositivityConstraint(0.5),
                                               sa.L0Constraint(per_plane)))[0] == 0.5
    uneven = full.copy()
    uneven[0, 3, 3] = 1.0
    for other in (
            None, sa.PositivityConstraint(0), sa.L0Constraint(full),
            sa.ConstraintChain(sa.L0Constraint(full), sa.PositivityConstraint(0)),
            sa.ConstraintChain(sa.PositivityConstraint(0), sa.L1Constraint(0.1)),
            sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(full, type="relative")),
            sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(uneven)),
            sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(full), repeat=2)):
        assert plane_thresholds(other) is None


class _Bare:
    """a StarletMorphology as ``_starlet_rules`` sees it, made without the device transform"""

    def __init__(self, coeffs, monotonic=False):
        self._parameters = (coeffs,)
        self.monotonic = monotonic


def _coeffs(**kw):
    import scarlet_amd as sa

    per_plane = np.array([0.3, 0.1, 0.0])
    full = np.broadcast_to(per_plane[:, None, None], (3, 8, 8)).copy()
    kw.setdefault("constraint", sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(full)))
    kw.setdefault("step", 1e-2)
    return sa.Parameter(np.zeros((3, 8, 8)), name="coeffs", **kw)


def test_component_description_and_refusals_need_no_device():
    import scarlet_amd as sa
    from scarlet_amd.blend import _starlet_rules

    step, floor, t = _starlet_rules(_Bare(_coeffs()), "amsgrad")
    assert (step, floor) == (1e-2, 0.0) and np.array_equal(t, [0.3, 0.1, 0.0])
    # fixed coefficients without a step are described with a step that is never used
    assert _starlet_rules(_Bare(_coeffs(step=None, fixed=True)), "amsgrad")[0] == 0.0

    class Flat(sa.Prior):
        def __call__(self, x):
            return 0.0

        def grad(self, x):
            return np.zeros_like(x)

    for bare, scheme in (
            (_Bare(_coeffs(), monotonic=True), "amsgrad"),
            (_Bare(_coeffs()), "adam"),
            (_Bare(_coeffs(prior=Flat())), "amsgrad"),
            (_Bare(_coeffs(step=lambda x, it=0: 1e-2)), "amsgrad"),
            (_Bare(_coeffs(step=sa.relative_step)), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.PositivityConstraint(0))), "amsgrad"),
            (_Bare(_coeffs(constraint=None)), "amsgrad")):
        with pytest.raises(NotImplementedError):
            _starlet_rules(bare, scheme)


def test_component_spec_of_a_starlet_component():
    import scarlet_amd as sa
    from scarlet_amd import _lib

    coeffs = np.arange(3 * 4 * 5, dtype=np.float64).reshape(3, 4, 5)
    spec = sa.ComponentSpec(np.ones(2), np.zeros((4, 5)), (1, 2), morph_step=1e-2,
                            prox_flags=_lib.COMPONENT_FIXED_MORPH | _lib.PROX_MONOTONIC,
                            starlet=(coeffs, [0.2, 0.1, 0.0]), sed_floor=0.0)
    assert spec.prox_flags == _lib.COMPONENT_STARLET | _lib.COMPONENT_FIXED_MORPH
    assert spec.star_coeffs.dtype == np.float32 and spec.star_coeffs.shape == (3, 4, 5)
    assert spec.star_thresh.dtype == np.float32 and spec.sed_floor == 0.0
    plain = sa.ComponentSpec(np.ones(2), np.zeros((4, 5)), (1, 2))
    assert plain.star_coeffs is None and plain.sed_floor is None
    with pytest.raises(AssertionError):
        sa.ComponentSpec(np.ones(2), np.zeros((4, 4)), (1, 2), starlet=(coeffs, [0.2, 0.1, 0.0]))


def test_exports_and_hook_coverage():
    import scarlet_amd as sa
    from scarlet_amd.fitting import _device_hook_covers

    for name in ("StarletSource", "RandomSource", "StarletMorphology"):
        assert hasattr(sa, name)
    # a starlet source keeps its blend off the resident loop: its hook is the host's
    made = sa.StarletSource.__new__(sa.StarletSource)
    morphology = sa.StarletMorphology.__new__(sa.StarletMorphology)
    spectrum = sa.TabulatedSpectrum.__new__(sa.TabulatedSpectrum)
    made._children = [spectrum, morphology]
    assert not _device_hook_covers(made)
