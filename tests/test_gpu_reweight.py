"""lite.weight_blends on the device: bit for bit the NumPy oracle (tests/reweight_oracle.py)
and ``weight_sources``, on the reference's fitted scene and on small synthetic blends at the
edges of the kernel's tile, stamp and box handling."""

from types import SimpleNamespace

import numpy as np
import pytest

import reweight_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _golden_blend(hsc, g):
    """The fitted FISTA scene of the golden in float32, with the golden's own stamp."""
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images = hsc["images"].astype(np.float32)
    weights = hsc["weights"].astype(np.float32)
    obs = lite.LiteObservation(images, (1 / weights).astype(np.float32), weights,
                               hsc["psfs"].astype(np.float32), model_psf=None)
    obs.diff_kernel = SimpleNamespace(image=g["diff_kernel"].astype(np.float32))
    sources = []
    for k in range(int(g["n_comp"])):
        morph = g["b_morph_%d" % k].astype(np.float32)
        oy, ox = (int(v) for v in g["b_origin_%d" % k])
        h, w = morph.shape
        comp = lite.init_fista_component((oy + h // 2, ox + w // 2),
                                         scarlet.Box((5, h, w), origin=(0, oy, ox)),
                                         g["b_sed_%d" % k].astype(np.float32), morph, obs,
                                         bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    return lite.LiteBlend(sources, obs)


def test_golden_scene(hsc):
    """43 x 43 stamp, ten sources, four boxes across the edges of the 58 x 48 frame: the
    device equals the oracle and ``weight_sources`` bit for bit, and the reference's fluxes
    within the tolerance of the host test."""
    from scarlet_amd import lite

    g = golden("lite_fista")
    blend, copy = _golden_blend(hsc, g), _golden_blend(hsc, g)
    assert lite.weight_blends([blend]) is None
    got = cases.fluxes(blend)
    cases.assert_same(got, cases.oracle(blend))
    lite.weight_sources(copy)
    cases.assert_same(got, cases.fluxes(copy))
    worst = cases.check_against_golden(got, g)
    print("worst relative deviation from the golden: %.3g" % worst)


@pytest.mark.parametrize("mask_footprint", [True, False])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_edge_blends(name, mask_footprint):
    from scarlet_amd import lite

    blend, copy = cases.make_blend(name), cases.make_blend(name)
    stats = {}
    want = cases.oracle(blend, mask_footprint, stats)
    # the clamps act in this case's family (test_reweight_host.test_cases_exercise_the_clamps
    # checks all three per frame size); here: the case is not trivial
    assert stats["clamped"] + stats["zeroed"] > 0
    lite.weight_blends([blend], mask_footprint)
    got = cases.fluxes(blend)
    cases.assert_same(got, want)
    lite.weight_sources(copy, mask_footprint)
    cases.assert_same(got, cases.fluxes(copy))


def test_the_cases_reach_every_rule():
    """Over the set of edge cases the oracle clamps a ratio to 1, zeroes one where the total
    is 0 and meets a masked pixel (checked on the CPU)."""
    stats = {}
    for name in cases.CASES:
        cases.oracle(cases.make_blend(name), stats=stats)
    assert stats["clamped"] > 0 and stats["zeroed"] > 0 and stats["masked"] > 0, stats


@pytest.mark.parametrize("name", ["33x31-bcast", "7x5-15x15"])
def test_float64(name):
    from scarlet_amd import lite

    blend, copy = (cases.make_blend(name, dtype=np.float64) for _ in range(2))
    lite.weight_blends([blend])
    got = cases.fluxes(blend)
    assert got[0][0].dtype == np.float64
    cases.assert_same(got, cases.oracle(blend))
    lite.weight_sources(copy)
    cases.assert_same(got, cases.fluxes(copy))


def _catalogue():
    return [cases.make_blend("7x5-3x3"), cases.make_blend("33x31-bcast"),
            cases.make_blend("7x5-3x3", mixed=True), cases.make_blend("64x65-C1"),
            cases.make_blend("33x31-bcast", dtype=np.float64), cases.make_blend("7x5-3x3", seed=1),
            cases.make_blend("31x33-big-psf"), cases.make_blend("33x31-bcast", seed=2)]


def test_mixed_catalogue():
    """Three frame sizes, three stamp shapes, a float64 and a mixed-dtype blend: all at once
    equals one by one, a forced-small byte budget equals the default, input order is kept."""
    from scarlet_amd import lite
    from scarlet_amd.lite import measure

    groups, fallback = measure.plan_blends(_catalogue())
    assert fallback == [2] and len(groups) == 5 and max(len(v) for v in groups.values()) == 2
    together, alone, small = _catalogue(), _catalogue(), _catalogue()
    lite.weight_blends(together)
    for b in alone:
        lite.weight_blends([b])
    lite.weight_blends(small, _working_set_bytes=1)  # one blend per chunk
    for i, (a, b, c) in enumerate(zip(together, alone, small)):
        cases.assert_same(cases.fluxes(a), cases.fluxes(b))
        cases.assert_same(cases.fluxes(a), cases.fluxes(c))
        if i != 2:
            cases.assert_same(cases.fluxes(a), cases.oracle(a))
    # the mixed-dtype blend got what weight_sources gives
    ref = _catalogue()[2]
    lite.weight_sources(ref)
    cases.assert_same(cases.fluxes(together[2]), cases.fluxes(ref))
    # results are arrays of their own
    assert together[0].sources[0].flux.base is None


def test_a_bad_plan_is_refused():
    """smi_reweight_* validates the plan on the host: nothing out of range is launched."""
    from scarlet_amd import _lib
    from scarlet_amd.lite import measure

    blend = cases.make_blend("7x5-3x3")
    key = measure._group_key(blend)

    def packed():
        return measure._pack([measure._plan_blend(blend)], key, True)

    def broken(table, field, value, row=0):
        p = packed()
        p[table][field][row] = value
        return p

    bad = [broken("sources", "h", 8), broken("sources", "x0", -1), broken("sources", "out_off", -1),
           broken("sources", "out_off", 10 ** 9), broken("sources", "blend", 1),
           broken("sources", "n_comp", 100), broken("comps", "morph_off", 10 ** 9),
           broken("comps", "stride", 1), broken("comps", "sed_off", -1), broken("comps", "h", -1),
           broken("comps", "y0", -1), broken("blends", "h", 0), broken("blends", "image_off", 1),
           broken("blends", "stamp_off", 1), broken("blends", "n_comp", -1)]
    for p in bad:
        with pytest.raises(_lib.ScarletAmdError, match="status -1"):
            measure._run_chunk(p, key, 0)
    for k in ((key[0], key[1], 4, 3), (key[0], key[1], 201, 201), (key[0], 0, 3, 3)):
        with pytest.raises(_lib.ScarletAmdError, match="status -1"):
            measure._run_chunk(packed(), k, 0)
    with pytest.raises(_lib.ScarletAmdError, match="status -1"):
        measure._run_chunk(packed(), key, 1 << 20)  # no such device


def test_fit_blends_reweights_with_the_batch(hsc):
    """``fit_blends(blends, 5, reweight=True)`` leaves the fluxes ``weight_sources`` gives
    after ``fit_blends(copies, 5, reweight=False)``."""
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    def blends():
        out = []
        model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
        for h, w in ((58, 48), (52, 40)):
            images = np.ascontiguousarray(hsc["images"][:, :h, :w], np.float32)
            weights = np.ascontiguousarray(hsc["weights"][:, :h, :w], np.float32)
            obs = lite.LiteObservation(images, (1 / weights).astype(np.float32), weights,
                                       hsc["psfs"].astype(np.float32), model_psf=model_psf[0][None])
            sources = []
            for k in range(int(hsc["n_comp"])):
                morph = hsc["morph_%d" % k].astype(np.float32)
                oy, ox = (int(v) for v in hsc["origin_%d" % k])
                mh, mw = morph.shape
                comp = lite.init_fista_component(
                    (oy + mh // 2, ox + mw // 2), scarlet.Box((5, mh, mw), origin=(0, oy, ox)),
                    hsc["sed_%d" % k].astype(np.float32).copy(), morph.copy(), obs, bg_thresh=0.25)
                sources.append(lite.LiteSource([comp], images.dtype))
            out.append(lite.LiteBlend(sources, obs))
        return out

    batched, copies = blends(), blends()
    got = lite.fit_blends(batched, 5, e_rel=1e-9, reweight=True)
    want = lite.fit_blends(copies, 5, e_rel=1e-9, reweight=False)
    assert got == want and lite.fit_blends.errors == []
    for a, b in zip(batched, copies):
        assert all(s.flux is None for s in b.sources)
        lite.weight_sources(b)
        cases.assert_same(cases.fluxes(a), cases.fluxes(b))
