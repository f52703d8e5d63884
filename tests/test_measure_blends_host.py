"""The host side of scarlet.measure_blends: the plan and its reasons, the packed tables, the row
type, the table made from the sums (on the oracle's records), and the oracle itself against the
float64 FFT rendering and the reference S/N formula.  No GPU."""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import measure_sources_cases as mc
import measure_sources_oracle as mo

U = 2.0 ** -52


@pytest.fixture(scope="module")
def cat():
    return mc.catalogue()


@pytest.fixture(scope="module")
def planned(cat):
    """Per device case ``(name, blend, key, plan, oracle)``, computed once and only read."""
    import scarlet_amd as scarlet
    from scarlet_amd import measure

    blends = [b for _, b, _ in cat]
    groups, _ = scarlet.plan_measure_blends(blends)
    out = []
    for key, idx in groups.items():
        for i in idx:
            if cat[i][2] != "device":
                continue
            plan = measure.plan_blend(blends[i], key)
            out.append((cat[i][0], blends[i], key, plan, mo.blend(plan)))
    return out


def test_plan_groups_and_reasons(cat):
    import scarlet_amd as scarlet

    groups, fallback = scarlet.plan_measure_blends([b for _, b, _ in cat])
    names = {key: [cat[i][0] for i in idx] for key, idx in groups.items()}
    assert names == {(3, 5, 5): ["tiny", "list map", "slice map", "not finite"],
                     (1, 5, 9): ["tiles"], (3, 1, 1): ["null"], (2, 63, 63): ["limit"],
                     (3, 11, 11): ["lobes"], (6, 5, 5): ["six"]}
    assert list(groups) == [(3, 5, 5), (1, 5, 9), (3, 1, 1), (2, 63, 63), (3, 11, 11), (6, 5, 5)]
    refused = {cat[i][0]: why for i, why in fallback.items()}
    assert sorted(refused) == sorted(n for n, _, e in cat if e not in ("device", "runtime"))
    for name, _, expect in cat:
        if name in refused:
            assert refused[name].startswith(expect), (name, refused[name])
    assert scarlet.plan_measure_blends([mc.leaves_the_box()]) == (
        {}, {0: "a component's box leaves its source's box"})


def test_more_reasons():
    """What the catalogue does not hold: a 65 x 65 stamp, two stamp shapes in one blend, float64
    frames, masked weights, a NullRenderer of some of the bands, a morphology with a plane per band."""
    import numpy.ma as ma

    import scarlet_amd as scarlet
    from init_blends_cases import scene
    from scarlet_amd import fft

    rng = np.random.RandomState(5)

    def reason(blend):
        groups, fallback = scarlet.plan_measure_blends([blend])
        assert not groups
        return fallback[0]

    frame, obs = scene(1, (2, 25, 31), (5, 5), [])
    src = mc.component(frame, rng, (3, 4, 5, 5))
    obs.renderer.diff_kernel = fft.Fourier(np.ones((2, 65, 65), np.float32))
    assert reason(scarlet.Blend([src], [obs])) == "difference-kernel stamp beyond 63 x 63"

    channels = ["c0", "c1", "c2", "c3"]
    frame = scarlet.Frame((4, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 4), channels=channels)
    a = mc._subset(2, (4, 25, 31), (5, 5), channels[:2], frame)
    b = mc._subset(3, (4, 25, 31), (7, 7), channels[2:], frame)
    src = mc.component(frame, rng, (3, 4, 5, 5))
    assert reason(scarlet.Blend([src], [a, b])) == "ConvolutionRenderers with different stamp shapes"

    frame, obs = scene(4, (2, 25, 31), (5, 5), [])
    obs.weights = ma.masked_equal(obs.weights, 0)
    src = mc.component(frame, rng, (3, 4, 5, 5))
    assert reason(scarlet.Blend([src], [obs])) == "weights that are not a plain float32 array"

    frame = scarlet.Frame((2, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 2),
                          channels=["a", "b"], dtype=np.float64)
    obs = scarlet.Observation(np.zeros((2, 25, 31)), psf=frame.psf, channels=["a", "b"]).match(frame)
    src = mc.component(frame, rng, (3, 4, 5, 5))
    assert reason(scarlet.Blend([src], [obs])) == "frame dtype float64 is not float32"

    frame = scarlet.Frame((3, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 3), channels=channels[:3])
    obs = scarlet.Observation(np.zeros((2, 25, 31), np.float32), psf=frame.psf,
                              channels=channels[1:3]).match(frame)
    src = mc.component(frame, rng, (3, 4, 5, 5))
    assert reason(scarlet.Blend([src], [obs])) == "a NullRenderer of a subset of the frame's bands"

    frame, obs = scene(5, (2, 25, 31), (5, 5), [])
    box = scarlet.Box((2, 5, 5), origin=(0, 3, 4))
    per_band = scarlet.FactorizedComponent(
        frame, scarlet.TabulatedSpectrum(frame, np.ones(2, np.float32), bbox=box[0]),
        scarlet.ImageMorphology(frame, rng.uniform(0.1, 1, (2, 5, 5)), bbox=box))
    assert reason(scarlet.Blend([per_band], [obs])) == "a morphology with an image per band"


def test_table_dtype():
    from scarlet_amd import measure

    dt = measure.table_dtype(3, 5)
    shapes = {name: dt[name].shape for name in dt.names}
    assert shapes == dict(n_components=(), box=(4,), flux=(3,), sums=(3, 5), peak=(3,),
                          peak_value=(), centroid=(3,), moments=(3, 3), rendered_flux=(5,),
                          rendered_sq=(5,), rendered_var=(5,), snr=())
    floats = [n for n in dt.names if n not in ("n_components", "box", "peak")]
    assert all(dt[n].base == np.float64 for n in floats)
    assert all(dt[n].base.kind == "i" for n in ("n_components", "box", "peak"))


def test_packed_tables(planned):
    """Offsets, counts and buffer sizes of two blends of one group packed together; the tile
    counts of hand-worked boxes."""
    from scarlet_amd import _catalog, measure

    by_name = {p[0]: p for p in planned}
    key = (3, 5, 5)
    plans = [by_name["tiny"][3], by_name["list map"][3]]
    packed = measure.pack(plans, key)
    src, comps, bands = packed["sources"], packed["comps"], packed["bands"]
    assert len(src) == 4 + 2 and len(comps) == 6 and len(bands) == 3 + 2
    # the null source of "tiny" (row 2) is not a device source
    assert [(rows, list(live), c_obs) for rows, live, c_obs in packed["layout"]] == [
        (5, [0, 1, 3, 4], 3), (2, [0, 1], 2)]
    assert_array_equal(src["comp0"], np.arange(6))
    assert_array_equal(src["n_comp"], 1)
    assert_array_equal(src["band0"], [0, 0, 0, 0, 3, 3])
    assert_array_equal(src["n_band"], [3, 3, 3, 3, 2, 2])
    assert tuple(src[0])[:6] == (-2, -3, 13, 17, 9, 11)
    assert tuple(src[4])[:6] == (4, 6, 11, 9, 25, 31)
    assert_array_equal(bands["channel"], [0, 1, 2, 0, 2])  # the list channel_map spelled out
    assert_array_equal(bands["stamp_off"], 25 * np.arange(5))
    assert_array_equal(bands["weight_off"], [0, 99, 198, 297, 297 + 775])
    assert_array_equal(comps["sed_off"], 3 * np.arange(6))
    sizes = [13 * 17, 5 * 9, 1, 5 * 6, 11 * 9, 7 * 7]
    assert_array_equal(comps["morph_off"], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert packed["seds"].size == 18 and packed["seds"].dtype == np.float64
    assert packed["morphs"].size == sum(sizes) and packed["morphs"].dtype == np.float64
    assert packed["stamps"].size == 5 * 25 and packed["stamps"].dtype == np.float32
    assert packed["weights"].size == 3 * 99 + 2 * 775 and packed["weights"].dtype == np.float32
    assert packed["n_record"] == 6 * 3 * 8 and packed["n_rendered"] == (4 * 3 + 2 * 2) * 3
    assert measure._SOURCE_DESC.itemsize == 40
    assert measure._COMP_DESC.itemsize == 32 and measure._BAND_DESC.itemsize == 24

    tiles = measure._region_tiles
    assert tiles((3, 5, 17, 17), (25, 31), 1, 1) == 4      # one pixel into a second tile
    assert tiles((2, 4, 16, 16), (25, 31), 1, 1) == 1
    assert tiles((12, 20, 3, 3), (25, 31), 5, 9) == 1      # 7 x 11 grown
    assert tiles((3, 5, 17, 17), (25, 31), 5, 9) == 2 * 2  # 21 x 25 grown
    assert tiles((9, 11, 15, 15), (33, 37), 63, 63) == 3 * 3  # the whole frame
    assert tiles((-2, -3, 13, 17), (9, 11), 5, 5) == 1     # clipped to the 9 x 11 frame
    assert tiles((40, 40, 3, 3), (9, 11), 5, 5) == 0       # out of reach
    # chunks: runs within the budget, a blend beyond it alone
    assert _catalog.chunks([(0, 5), (1, 5), (2, 20), (3, 1)], 10) == [[0, 1], [2], [3]]


def test_oracle_model_is_get_model(planned):
    """The oracle's model has the bits of ``src.get_model()``."""
    import scarlet_amd as scarlet

    for name, blend, key, plan, oracle in planned:
        for src, o in zip(blend.sources, oracle):
            if isinstance(src, scarlet.NullSource):
                assert o is None
                continue
            model = src.get_model()
            assert model.dtype == np.float64
            assert_array_equal(o["cube"], model, err_msg=name)


def test_fill_table_on_oracle_records(planned):
    """The table made from the oracle's records: flux and centroid within the summation bound of
    the per-source functions, the peak exactly, the central moments those of measure.moments
    about each band's centroid."""
    import scarlet_amd as scarlet
    from scarlet_amd import measure

    for name, blend, key, plan, oracle in planned:
        packed = measure.pack([plan], key)
        live = [o for o in oracle if o is not None]
        records = np.stack([o["records"] for o in live])
        rendered = np.concatenate([o["rendered"] for o in live])
        (table,) = measure.fill_table(packed["layout"], packed["sources"], records, rendered)
        assert table.dtype == measure.table_dtype(key[0], len(plan["bands"]))
        assert len(table) == len(blend.sources)
        for row, src in zip(table, blend.sources):
            if isinstance(src, scarlet.NullSource):
                assert row["n_components"] == 0
                assert row.tobytes() == bytes(row.dtype.itemsize)
                continue
            model = src.get_model()
            _, h, w = model.shape
            n = h * w
            assert row["n_components"] == len(measure._leaves(src))
            assert tuple(row["box"]) == (src.bbox.origin[1], src.bbox.origin[2], h, w)
            # two orders of the same n positive terms: (n + 4) u sum|terms|
            want = measure.flux(src)
            assert np.all(np.abs(row["flux"] - want) <= (n + 4) * U * want), name
            assert tuple(row["peak"]) == tuple(measure.max_pixel(src)), name
            assert row["peak_value"] == model.max()
            # the centroid is a ratio of two such sums: twice the bound, and a rounding each
            got, want = row["centroid"], measure.centroid(src)
            origin = np.array(src.bbox.origin)
            scale = np.maximum(np.abs(want - origin), 1.0)
            assert np.all(np.abs(got - want) <= 2 * (key[0] * n + 8) * U * scale), name
            y, x = np.indices((h, w), dtype=np.float64)
            for c in range(key[0]):
                m = model[c]
                F = m.sum()
                center = ((x * m).sum() / F, (y * m).sum() / F)  # (c1, c0): x first
                mom = measure.moments(m, N=2, centroid=center)
                want = np.array([mom[0, 2], mom[1, 1], mom[2, 0]])
                # M = S2 - S1 S1' / F with |S1 S1' / F| <= max(Syy, Sxx) (Cauchy-Schwarz): each
                # of the three terms carries (n + 4) u of that, and so does the direct sum
                bound = 8 * (n + 4) * U * max(row["sums"][c, 2], row["sums"][c, 4], 1e-300)
                assert np.all(np.abs(row["moments"][c] - want) <= bound), (name, c)


def test_oracle_rendering_is_the_float64_fft(planned):
    """The oracle's R equals ConvolutionRenderer.render_float64 (host float64 FFT) to 1e-12 of
    the largest pixel; a NullRenderer's R is the model's band itself."""
    import scarlet_amd as scarlet

    for name, blend, key, plan, oracle in planned:
        frame = blend.frame
        for src, o in zip(blend.sources, oracle):
            if o is None:
                continue
            full = src.get_model(frame=frame)
            at = 0
            for obs in blend.observations:
                n = obs.shape[0]
                R = o["R"][at:at + n]
                at += n
                if type(obs.renderer) is scarlet.NullRenderer:
                    assert_array_equal(R, obs.renderer.map_channels(full))
                else:
                    want = obs.renderer.render_float64(full)
                    assert np.abs(R - want).max() <= 1e-12 * np.abs(want).max(), name


def test_snr_formula_and_condition(planned):
    """snr_of_sums on the oracle's sums is the reference formula (measure.snr's, in float64) on
    the oracle's cubes; and in every case and observed band sum|R| <= 10 |sum R|: the condition
    under which the S/N bound of the GPU test holds."""
    from scarlet_amd import measure

    for name, blend, key, plan, oracle in planned:
        var = np.stack([1.0 / np.asarray(w, np.float64) for _, _, w in plan["bands"]])
        for o in oracle:
            if o is None:
                continue
            R = o["R"]
            signal = R.reshape(-1)
            weight = (R / R.sum(axis=(-2, -1))[:, None, None]).reshape(-1)
            want = (signal * weight).sum() / np.sqrt((var.reshape(-1) * weight * weight).sum())
            got = measure.snr_of_sums(*o["rendered"].T)
            assert_allclose(got, want, rtol=1e-12)
            assert np.all(o["rendered_abs"][:, 0] <= 10 * np.abs(o["rendered"][:, 0])), name
