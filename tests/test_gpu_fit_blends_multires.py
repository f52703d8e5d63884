"""``fit_blends`` with two-resolution blends in device batches (tests/multires_batch_cases.py):
every blend gets the bits of its own ``Blend.fit`` -- iteration counts, loss histories,
parameters, optimizer moments, boxes, low-resolution renderings -- whatever list it is in,
in whatever order, on either side of a cut of its group, and whether its batch mates stop
before it or after it."""

import numpy as np
import pytest

import multires_batch_cases as mc
import scarlet_amd as scarlet
import scarlet_amd.fitting as fitting
from scarlet_amd.blend import _flatten

pytestmark = pytest.mark.gpu

N_ITER, E_REL = 25, 1e-4
# At this e_rel the members of EARLY_AMPLITUDES stop at different iterations (see
# test_members_that_stop_at_different_iterations, which asserts it)
EARLY_E_REL = 1e-2
EARLY_AMPLITUDES = (5.0, 0.2, 20.0, 1.0, 50.0)


def snapshot(blend, result):
    """Everything a fit leaves on a blend, as arrays."""
    out = dict(n=np.array(result[0]), logL=np.array(result[1]), loss=np.array(blend.loss))
    for k, c in enumerate(_flatten(blend.sources)):
        out["box origin %d" % k] = np.array(c.children[1].bbox.origin)
        out["box shape %d" % k] = np.array(c.children[1].bbox.shape)
        for j, p in enumerate(c.children[0]._parameters + c.children[1]._parameters):
            tag = "component %d parameter %d " % (k, j)
            out[tag + "value"] = np.array(p)
            for name in ("m", "v", "vhat", "std"):
                state = getattr(p, name)
                out[tag + name] = np.array(np.nan if state is None else state, dtype=np.float64)
    model = blend.get_model()
    for j, obs in enumerate(blend.observations):
        if type(obs.renderer) is scarlet.ResolutionRenderer:
            out["low-resolution rendering %d" % j] = np.array(obs.render(model))
    return out


def assert_same(got, ref, what):
    assert got.keys() == ref.keys(), what
    for key in ref:
        assert np.array_equal(got[key], ref[key], equal_nan=True), (what, key)


_alone = {}


def alone(name, make):
    """Every blend of list ``name`` through its own ``Blend.fit`` (once per module)."""
    if name not in _alone:
        blends = make()
        _alone[name] = [snapshot(b, b.fit(N_ITER, e_rel=E_REL)) for b in blends]
    return _alone[name]


def batched(blends, e_rel=E_REL, **kw):
    report = {}
    results = scarlet.fit_blends(blends, N_ITER, e_rel=e_rel, _report=report, **kw)
    assert scarlet.fit_blends.errors == []
    return [snapshot(b, r) for b, r in zip(blends, results)], report


@pytest.mark.parametrize("name", list(mc.LISTS))
def test_every_blend_gets_the_bits_of_its_own_fit(name):
    ref = alone(name, mc.LISTS[name])
    got, report = batched(mc.LISTS[name]())
    groups, why = fitting.plan_fit_blends(mc.LISTS[name](), N_ITER, e_rel=E_REL)
    assert report["groups"] == groups and report["alone"] == why
    assert report["batches"] == len(groups)
    assert report["batches"] == {"first": 1, "classes": 5, "single": 2, "psf_shift": 1}[name]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert r["n"] > 1 and np.isfinite(r["loss"]).all()
        assert_same(g, r, (name, i))


def test_blend_fit_keeps_the_bits_of_its_round_loop(monkeypatch):
    """``Blend.fit`` of such a blend used to be the loop of ``Blend._fit_rounds`` (a batch per
    round, hooks on the host, the resampler's own tables); it still is with this switch."""
    ref = alone("classes", mc.LISTS["classes"])
    monkeypatch.setenv("SCARLET_AMD_BLEND_FIT", "loop")
    for i, blend in enumerate(mc.LISTS["classes"]()):
        assert_same(snapshot(blend, blend.fit(N_ITER, e_rel=E_REL)), ref[i], i)


def test_the_order_of_the_list_does_not_matter():
    ref = alone("classes", mc.LISTS["classes"])
    got, report = batched(mc.LISTS["classes"]()[::-1])
    assert report["batches"] == 5
    for i, (g, r) in enumerate(zip(got[::-1], ref)):
        assert_same(g, r, i)


def test_a_cut_group_has_the_same_bits(monkeypatch):
    ref = alone("first", mc.LISTS["first"])
    each = 2 * 11 * 54 * 31 * 8
    monkeypatch.setattr(fitting, "LOWRES_OPERATOR_CAP", 3 * each)
    got, report = batched(mc.LISTS["first"]())
    assert [idx for _, idx in report["groups"]] == [[0, 1, 2], [3, 4]]
    assert report["batches"] == 2
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, i)


def test_a_list_of_one_has_the_same_bits():
    ref = alone("classes", mc.LISTS["classes"])
    blends = mc.LISTS["classes"]()
    for i in (2, 7):  # a member of the group of five; the blend with two observations
        got, report = batched([blends[i]])
        assert report["batches"] == 1
        assert_same(got[0], ref[i], i)


def test_members_that_stop_at_different_iterations():
    """Amplitudes of 0.2 to 50 at e_rel = 1e-2: members 0, 2 and 4 (the bright ones) stop
    first, member 3 in the middle of the run, member 1 (the faintest) near its end and before
    the budget is used up; a member that has stopped keeps its term, and those that go on do
    not see it."""
    make = lambda: mc.first_five(EARLY_AMPLITUDES)  # noqa: E731
    ref = []
    for b in make():
        ref.append(snapshot(b, b.fit(N_ITER, e_rel=EARLY_E_REL)))
    counts = [int(r["n"]) for r in ref]
    print("iterations:", counts)
    assert max(counts[0], counts[2], counts[4]) < counts[3] < counts[1] < N_ITER
    got, report = batched(make(), e_rel=EARLY_E_REL)
    assert report["batches"] == 1
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, i)
