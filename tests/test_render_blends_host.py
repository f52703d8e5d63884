"""The host side of scarlet.render_blends: the plan and its reasons beside plan_measure_blends',
the packed tables, byte counts and chunks, and the float64 oracle's own identities.  No GPU."""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import render_blends_cases as rc
import render_blends_oracle as ro


@pytest.fixture(scope="module")
def cat():
    return rc.catalogue()


@pytest.fixture(scope="module")
def planned(cat):
    """Per device case ``name -> (blend, key, plan, oracle)``, computed once and only read."""
    import scarlet_amd as scarlet
    from scarlet_amd import rendering

    blends = [b for _, b, _ in cat]
    groups, _ = scarlet.plan_render_blends(blends)
    out = {}
    for key, idx in groups.items():
        for i in idx:
            if cat[i][2] == "device":
                plan = rendering.plan_blend(blends[i], key)
                out[cat[i][0]] = (blends[i], key, plan, ro.blend(plan, key))
    return out


def test_plan_groups_and_reasons(cat):
    import scarlet_amd as scarlet

    blends = [b for _, b, _ in cat]
    groups, fallback = scarlet.plan_render_blends(blends)
    names = {key: [cat[i][0] for i in idx] for key, idx in groups.items()}
    assert names == {(3, 5, 5): ["tiny", "list map", "slice map", "zero weight", "not finite",
                                 "stock"],
                     (1, 5, 9): ["tiles"], (3, 1, 1): ["null", "subset null"],
                     (2, 63, 63): ["limit"], (3, 11, 11): ["lobes", "clamped"],
                     (6, 5, 5): ["six"], (2, 5, 5): ["alone", "apart"]}
    assert list(groups) == [(3, 5, 5), (1, 5, 9), (3, 1, 1), (2, 63, 63), (3, 11, 11), (6, 5, 5),
                            (2, 5, 5)]
    refused = {cat[i][0]: why for i, why in fallback.items()}
    assert sorted(refused) == sorted(n for n, _, e in cat if e not in ("device", "runtime"))
    for name, _, expect in cat:
        if name in refused:
            assert refused[name].startswith(expect), (name, refused[name])
    # the two differences from plan_measure_blends, and nothing else
    m_groups, m_fallback = scarlet.plan_measure_blends(blends)
    m_refused = {cat[i][0]: why for i, why in m_fallback.items()}
    assert {n: m_refused[n] for n in set(m_refused) - set(refused)} == {
        "zero weight": "a weight that is zero, negative or not finite",
        "subset null": "a NullRenderer of a subset of the frame's bands"}
    assert {n: why for n, why in m_refused.items() if n in refused} == refused
    for key, idx in m_groups.items():
        assert [i for i in groups[key] if i in idx] == idx


def test_more_reasons():
    """What the catalogue does not hold: weights that are negative or not finite, data that are
    not a plain float32 array."""
    import numpy.ma as ma

    import scarlet_amd as scarlet
    from init_blends_cases import scene
    from measure_sources_cases import component

    rng = np.random.RandomState(5)

    def reason(change):
        frame, obs = scene(1, (2, 25, 31), (5, 5), [])
        change(obs)
        groups, fallback = scarlet.plan_render_blends(
            [scarlet.Blend([component(frame, rng, (3, 4, 5, 5))], [obs])])
        assert not groups
        return fallback[0]

    def negative(obs):
        obs.weights[1, 2, 3] = -1

    def infinite(obs):
        obs.weights[0, 0, 0] = np.inf

    def masked(obs):
        obs.data = ma.masked_invalid(obs.data)

    def wide(obs):
        obs.data = obs.data.astype(np.float64)

    assert reason(negative) == reason(infinite) == "a weight that is negative or not finite"
    assert reason(masked) == reason(wide) == "data that are not a plain float32 array"


def test_packed_tables_bytes_and_chunks(planned):
    """Offsets, counts and buffer sizes of two blends of one group packed together, with and
    without the sources; the regions and tile counts of hand-worked boxes; chunks at a small
    budget."""
    from scarlet_amd import _catalog, measure, rendering

    key = (3, 5, 5)
    plans = [planned["tiny"][2], planned["list map"][2]]
    for flags, n_sources in ((0, 0), (rendering.MASK, 0), (rendering.SOURCES, 6),
                             (rendering.REWEIGHT | rendering.MASK, 6)):
        packed = rendering.pack(plans, key, flags)
        blends, src, comps, bands = (packed[n] for n in ("blends", "sources", "comps", "bands"))
        assert len(blends) == 2 and len(src) == n_sources and len(comps) == 6 and len(bands) == 5
        assert [tuple(b) for b in blends] == [(9, 11, 0, 4, 0, 3, 0),
                                              (25, 31, 4, 2, 3, 2, 3 * 99)]
        assert packed["n_out"] == 3 * 99 + 2 * 775
        assert_array_equal(bands["channel"], [0, 1, 2, 0, 2])
        assert_array_equal(bands["stamp_off"], 25 * np.arange(5))
        assert_array_equal(bands["weight_off"], [0, 99, 198, 297, 297 + 775])
        assert packed["data"].size == packed["weights"].size == 3 * 99 + 2 * 775
        assert packed["data"].dtype == packed["weights"].dtype == np.float32
        assert_array_equal(packed["data"][:99], planned["tiny"][0].observations[0].data[0].ravel())
        assert_array_equal(comps["sed_off"], 3 * np.arange(6))
        sizes = [13 * 17, 5 * 9, 1, 5 * 6, 11 * 9, 7 * 7]
        assert_array_equal(comps["morph_off"], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    # the sources: those with components, in order; every region clipped to its frame
    assert_array_equal(src["blend"], [0, 0, 0, 0, 1, 1])
    assert_array_equal(src["comp0"], np.arange(6))
    assert_array_equal(src["n_comp"], 1)
    assert tuple(src[0])[:4] == (-2, -3, 13, 17) and tuple(src[4])[:4] == (4, 6, 11, 9)
    regions = [(0, 0, 9, 11), (0, 2, 6, 9), (2, 3, 5, 5), (4, 0, 5, 6), (2, 4, 15, 13),
               (13, 18, 11, 11)]
    bands_of = [3, 3, 3, 3, 2, 2]
    cubes = [n * r[2] * r[3] for n, r in zip(bands_of, regions)]
    assert_array_equal(src["out_off"], np.concatenate([[0], np.cumsum(cubes)[:-1]]))
    assert packed["n_source_out"] == sum(cubes)
    out_off, got, offsets = packed["layout"][0]
    assert out_off == 0 and got == regions[:2] + [(0, 0, 0, 0)] + regions[2:4]
    assert offsets == [0, cubes[0], None, cubes[0] + cubes[1], sum(cubes[:3])]
    assert rendering._BLEND_DESC.itemsize == 32 and rendering._SOURCE_DESC.itemsize == 40

    region, tiles = rendering.region_of, rendering._tiles
    assert region((3, 5, 17, 17), (25, 31), 5, 9) == (1, 1, 21, 25)
    assert region((40, 40, 3, 3), (9, 11), 5, 5)[2:] == (0, 0) and tiles(0, 7) == 0
    assert tiles(21, 25) == 4 and tiles(16, 16) == 1 and tiles(17, 16) == 2 and tiles(9, 11) == 1
    for rect, hw, kh, kw in (((3, 5, 17, 17), (25, 31), 5, 9), ((9, 11, 15, 15), (33, 37), 63, 63),
                             ((-2, -3, 13, 17), (9, 11), 5, 5), ((40, 40, 3, 3), (9, 11), 5, 5)):
        assert tiles(*region(rect, hw, kh, kw)[2:]) == measure._region_tiles(rect, hw, kh, kw)

    # bytes: the outputs and the float64 total are counted
    plan = planned["list map"][2]
    plain = rendering._plan_bytes(plan, key, 0)
    with_sources = rendering._plan_bytes(plan, key, rendering.SOURCES)
    with_flux = rendering._plan_bytes(plan, key, rendering.REWEIGHT)
    assert plain >= 2 * 775 * 16  # data, weights, rendered and residual of two bands
    cubes = 2 * (15 * 13 + 11 * 11)
    assert with_sources - plain == 2 * 40 + 4 * cubes + 12 * 2 * (1 + 1)
    assert with_flux - with_sources == 4 * cubes + 8 * 2 * 775
    group = [planned[n][2] for n in ("tiny", "list map", "slice map")]
    need = [rendering._plan_bytes(p, key, 0) for p in group]
    assert _catalog.chunks(list(enumerate(need)), need[0] + need[1]) == [[0, 1], [2]]
    assert _catalog.chunks(list(enumerate(need)), 1) == [[0], [1], [2]]


def test_oracle_rendering_is_the_float64_fft(planned):
    """The oracle's scene and per-source renderings equal ConvolutionRenderer.render_float64 (host
    float64 FFT) of the float64 models to 1e-12 of the largest pixel; a NullRenderer's are the
    model's bands themselves, through its channel map."""
    import scarlet_amd as scarlet

    for name, (blend, key, plan, oracle) in planned.items():
        frame = blend.frame
        models = [None if isinstance(s, scarlet.NullSource) else s.get_model(frame=frame)
                  for s in blend.sources]
        assert all(m is None or m.dtype == np.float64 for m in models)
        scene = sum(m for m in models if m is not None)
        for model, R in [(scene, oracle["R"])] + [(m, o["R"]) for m, o in
                                                  zip(models, oracle["sources"]) if o is not None]:
            at = 0
            for obs in blend.observations:
                n = obs.shape[0]
                if type(obs.renderer) is scarlet.NullRenderer:
                    want = obs.renderer.map_channels(model)
                else:
                    want = obs.renderer.render_float64(model)
                assert want.shape == R[at:at + n].shape
                assert np.abs(R[at:at + n] - want).max() <= 1e-12 * np.abs(want).max(), name
                at += n
        assert [o is None for o in oracle["sources"]] == [m is None for m in models]


def test_oracle_identities(planned):
    """``alone``: the ratio is exactly 1 wherever the rendering is positive; ``apart``: exact zeros
    in the middle of the frame; ``clamped``: every branch of the ratio rules is visited; the ratio
    bound is zero where nothing moves and reaches both sides of a denominator at zero."""
    _, _, plan, oracle = planned["alone"]
    (src,) = oracle["sources"]
    y0, x0, h, w = src["region"]
    crop = (slice(None), slice(y0, y0 + h), slice(x0, x0 + w))
    assert_array_equal(src["R"], oracle["R"])
    positive = src["R"][crop] > 0
    assert positive.sum() > 100
    assert np.all(ro.ratio(src["R"][crop], oracle["R"][crop])[positive] == 1)
    assert_array_equal(src["flux"][positive], oracle["image"][crop][positive])

    _, _, plan, oracle = planned["apart"]
    middle = (slice(None),) + rc.MIDDLE
    assert oracle["R"][middle].size > 0 and not oracle["R"][middle].any()
    assert not oracle["R_bound"][middle].any()
    assert oracle["R"].any(axis=(1, 2)).all()

    _, _, plan, oracle = planned["clamped"]
    negative = zero_total = above = 0
    for src in oracle["sources"]:
        y0, x0, h, w = src["region"]
        crop = (slice(None), slice(y0, y0 + h), slice(x0, x0 + w))
        R_k, R_tot = src["R"][crop], oracle["R"][crop]
        negative += int((R_k < 0).sum())
        zero_total += int((R_tot <= 0).sum())
        above += int(((R_k > R_tot) & (R_tot > 0)).sum())
    assert negative >= 1 and zero_total >= 1 and above >= 1, (negative, zero_total, above)

    a, b = np.array([1.0, 1.0, -1.0, 3.0]), np.array([2.0, 1e-20, 1e-20, 2.0])
    assert_array_equal(ro.ratio(a, b), [0.5, 1, 0, 1])
    assert_array_equal(ro.ratio_bound(a, b, 0.0, 0.0), [0, 0, 0, 0])
    assert_array_equal(ro.ratio_bound(a, b, 0.0, 1e-19), [0, 1, 0, 0])
    assert_array_equal(ro.ratio_bound(a, np.array([2.0, 2.0, 2.0, 2.0]), 0.5, 0.0),
                       [0.25, 0.25, 0, 0])


def test_host_loop_shapes():
    """``render_blend_host`` needs the GPU for a convolution; a NullRenderer's blend does not:
    shapes, the channel map, regions, the NullSource and the ratio rules of the loop."""
    import scarlet_amd as scarlet
    from scarlet_amd import rendering

    cat = rc.catalogue()
    by_name = {name: blend for name, blend, _ in cat}
    blend = by_name["subset null"]
    res = rendering.render_blend_host(blend, reweight=True)
    (obs,) = blend.observations
    model = blend.get_model()
    assert_array_equal(res["rendered"][0], model[1:3])
    assert_array_equal(res["residual"][0], obs.data - model[1:3])
    assert res["chi2"][0].shape == (2,)
    want = obs.get_log_likelihood(model[1:3])
    assert abs(res["log_likelihood"] - want) <= 1e-6 * abs(want)
    assert [s["region"] for s in res["sources"]] == [(4, 6, 11, 9), (0, 20, 7, 11)]
    for s in res["sources"]:
        assert s["rendered"][0].shape == s["flux"][0].shape == (2,) + s["region"][2:]
        assert s["flux"][0].dtype == np.float32
    assert res["sources"][0]["flux"][0][0, 1, 1] == 0  # the pixel (5, 7) without weight
    unmasked = rendering.render_blend_host(blend, reweight=True, mask_footprint=False)
    # (the source is alone there: the ratio is 1 up to the float32 model of the scene)
    assert abs(unmasked["sources"][0]["flux"][0][0, 1, 1] - obs.data[0, 5, 7]) <= 1e-6 * abs(
        obs.data[0, 5, 7])

    blend = scarlet.Blend([scarlet.NullSource(by_name["null"].frame)] + by_name["null"].sources,
                          by_name["null"].observations)
    res = rendering.render_blend_host(blend, sources=True)
    assert res["sources"][0]["region"] == (0, 0, 0, 0)
    assert res["sources"][0]["rendered"][0].shape == (3, 0, 0)
    assert "flux" not in res["sources"][1]
