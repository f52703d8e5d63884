"""Monotonic starlet sources without a GPU: the oracle extension (tests/starlet_monotonic_oracle.py)
against what the reference recorded in tests/golden/starlet_monotonic.npz, the attributes of the
mirror classes, and the rules ``Blend.fit`` reads off a ``StarletMorphology(monotonic=True)``."""

import numpy as np
import pytest

from conftest import golden

import starlet_monotonic_oracle as smo


@pytest.fixture(scope="module")
def g():
    return golden("starlet_source")


@pytest.fixture(scope="module")
def gm():
    return golden("starlet_monotonic")


def test_oracle_reproduces_the_reference_constraint(gm):
    """float64 like the reference's coefficients; np.array_equal takes -0.0 (the reference's
    ``model * valid`` of a negative pixel) for the 0 it is"""
    for k in gm["starlet_of"]:
        assert str(gm["constraint_type_%d" % k]) == "MonotonicMaskConstraint"
        rule = (int(gm["center_radius_%d" % k]), float(gm["variance_%d" % k]),
                int(gm["max_iter_%d" % k]))
        for name in ("coeffs", "perturbed"):
            stack = gm["%s_%d" % (name, k)]
            assert stack.dtype == np.float64
            out, interpolated = smo.mask_planes(stack, *rule)
            want = gm["once_%d" % k if name == "coeffs" else "perturbed_once_%d" % k]
            print("source", k, name, "kept", (want != 0).mean(), "interpolated", interpolated)
            assert np.array_equal(out, want)
        assert interpolated > 0  # the perturbed stacks go through the interpolation passes
        comp = smo.MonotonicStarletComponent(np.ones(5), gm["perturbed_%d" % k].copy(), (0, 0), *rule)
        assert comp.center == tuple(gm["center_%d" % k])
        assert np.array_equal(comp.morph_prox(comp.morph.copy(), 0), gm["perturbed_once_%d" % k])


def test_oracle_reproduces_the_reference_model_and_likelihood(g, gm, hsc):
    sc = smo.fixture_scene(g, gm, hsc)
    model = sc.get_model()
    assert model.dtype == gm["model"].dtype
    scale = np.abs(gm["model"]).max()
    assert np.abs(model.astype(np.float64) - gm["model"]).max() <= 1e-12 * scale
    rendered = sc.render(model)
    assert np.abs(rendered.astype(np.float64) - gm["rendered"]).max() <= 1e-5 * np.abs(gm["rendered"]).max()
    logL = sc.log_likelihood(rendered)
    assert abs(logL - float(gm["logL"])) <= 1e-12 * abs(float(gm["logL"]))


def test_the_shrink_hook_recentres(g, gm, hsc):
    sc = smo.fixture_scene(g, gm, hsc)
    comp = sc.components[2]
    assert comp.morph.shape == (5, 41, 41) and comp.center == (20, 20)
    hand = np.zeros_like(comp.morph)
    hand[0, 15:26, 15:26] = 1 + np.arange(121).reshape(11, 11)
    comp.morph = hand
    origin = comp.origin
    assert smo.shrink_component(comp)
    assert comp.morph.shape == (5, 21, 21) and comp.center == (10, 10)
    assert comp.origin == (origin[0] + 10, origin[1] + 10)
    # the operator is the one about the new middle
    want, _ = smo.mask_planes(comp.morph, comp.center_radius, comp.variance, comp.max_iter)
    assert np.array_equal(comp.morph_prox(comp.morph.copy(), 0), want)
    # (the fill starts at the maximum of the window about (10, 10) and drops what lies above it)
    assert want[0, 11, 11] == hand[0, 21, 21] and want[0, 15, 15] == 0


def test_mirror_classes_agree_with_the_fixture(gm):
    """the constraint StarletMorphology(monotonic=True) builds, without the device transform"""
    import scarlet_amd as sa

    for k in gm["starlet_of"]:
        shape = tuple(int(n) for n in gm["shape_%d" % k])
        morphology = sa.StarletMorphology.__new__(sa.StarletMorphology)
        morphology.monotonic = True
        constraint = sa.MonotonicMaskConstraint(tuple(n // 2 for n in shape), center_radius=1)
        assert tuple(constraint.center) == tuple(gm["center_%d" % k])
        assert constraint.center_radius == int(gm["center_radius_%d" % k])
        assert constraint.variance == float(gm["variance_%d" % k])
        assert constraint.max_iter == int(gm["max_iter_%d" % k])
        assert type(constraint).__name__ == str(gm["constraint_type_%d" % k])
        assert float(gm["step_%d" % k]) == 1e-2


class _Bare:
    """a StarletMorphology as ``_starlet_rules`` sees it, made without the device transform"""

    def __init__(self, coeffs, monotonic=True):
        self._parameters = (coeffs,)
        self.monotonic = monotonic


def _coeffs(shape=(3, 9, 8), **kw):
    import scarlet_amd as sa

    kw.setdefault("constraint", sa.MonotonicMaskConstraint((shape[1] // 2, shape[2] // 2)))
    kw.setdefault("step", 1e-2)
    return sa.Parameter(np.zeros(shape), name="coeffs", **kw)


def test_rules_of_monotonic_coefficients_need_no_device():
    import scarlet_amd as sa
    from scarlet_amd.blend import _starlet_rules

    step, floor, rule = _starlet_rules(_Bare(_coeffs()), "amsgrad")
    assert (step, floor) == (1e-2, 0.0)
    assert type(rule) is sa.MonotonicPlanes and rule == (1, 0.0, 3)
    custom = sa.MonotonicMaskConstraint((np.int64(4), 4), center_radius=0, variance=0.25, max_iter=0)
    assert _starlet_rules(_Bare(_coeffs(constraint=custom)), "amsgrad")[2] == (0, 0.25, 0)
    assert _starlet_rules(_Bare(_coeffs(step=None, fixed=True)), "amsgrad")[0] == 0.0

    class Flat(sa.Prior):
        def __call__(self, x):
            return 0.0

        def grad(self, x):
            return np.zeros_like(x)

    class Mine(sa.MonotonicMaskConstraint):
        pass

    full = np.zeros((3, 9, 8))
    chain = sa.ConstraintChain(sa.PositivityConstraint(0), sa.L0Constraint(full))
    for bare, scheme in (
            (_Bare(_coeffs(constraint=chain)), "amsgrad"),  # the flag without the constraint
            (_Bare(_coeffs(), monotonic=False), "amsgrad"),  # the constraint without the flag
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4, 3)))), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4.0, 4.0)))), "amsgrad"),
            (_Bare(_coeffs(constraint=Mine((4, 4)))), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4, 4), center_radius=-1))), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4, 4), center_radius=1.5))), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4, 4), variance=-1.0))), "amsgrad"),
            (_Bare(_coeffs(constraint=sa.MonotonicMaskConstraint((4, 4), max_iter=-1))), "amsgrad"),
            (_Bare(_coeffs(constraint=None)), "amsgrad"),
            (_Bare(_coeffs()), "adam"),
            (_Bare(_coeffs(prior=Flat())), "amsgrad"),
            (_Bare(_coeffs(step=lambda x, it=0: 1e-2)), "amsgrad"),
            (_Bare(_coeffs(step=sa.relative_step)), "amsgrad")):
        with pytest.raises(NotImplementedError):
            _starlet_rules(bare, scheme)


def test_component_spec_of_a_monotonic_starlet_component():
    import scarlet_amd as sa
    from scarlet_amd import _lib

    coeffs = np.arange(3 * 4 * 5, dtype=np.float64).reshape(3, 4, 5)
    spec = sa.ComponentSpec(np.ones(2), np.zeros((4, 5)), (1, 2), morph_step=1e-2, prox_flags=0,
                            starlet=(coeffs, sa.MonotonicPlanes(1, 0.0, 3)))
    assert spec.prox_flags == _lib.COMPONENT_STARLET
    assert spec.star_monotonic == (1, 0.0, 3) and np.array_equal(spec.star_thresh, np.zeros(3))
    thresholded = sa.ComponentSpec(np.ones(2), np.zeros((4, 5)), (1, 2), prox_flags=0,
                                   starlet=(coeffs, [0.2, 0.1, 0.0]))
    assert thresholded.star_monotonic is None
    with pytest.raises(AssertionError):
        sa.ComponentSpec(np.ones(2), np.zeros((4, 5)), (1, 2),
                         starlet=(coeffs, sa.MonotonicPlanes(-1, 0.0, 3)))
    names = [name for name, _ in _lib.Components._fields_]
    assert names[-4:] == ["star_monotonic", "star_center_radius", "star_variance", "star_max_iter"]
