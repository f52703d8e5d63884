"""scarlet.measure_blends on the GPU: the catalogue of tests/measure_sources_cases.py against the
float64 oracle and the per-source functions, independence of list, order and chunking, the
fallback, and the validation of the C entry.

Measured on one MI355X (the figures the tests print): the largest error of a sum is 0.024 of its
bound; the device's S/N lies at most 3.5e-16 (relative) from the oracle's, ``measure.snr`` (float32
rendering through the FFT) at most 1.6e-7."""

import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import measure_sources_cases as mc
import measure_sources_oracle as mo

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


@pytest.fixture(scope="module")
def runs():
    """The catalogue, its tables in one call, the plans and oracle records of the device cases:
    computed once and only read."""
    import scarlet_amd as scarlet
    from scarlet_amd import measure

    cat = mc.catalogue()
    blends = [b for _, b, _ in cat]
    report = {}
    tables = scarlet.measure_blends(blends, _report=report)
    groups, _ = scarlet.plan_measure_blends(blends)
    device = {}
    for key, idx in groups.items():
        for i in idx:
            if cat[i][2] == "device":
                plan = measure.plan_blend(blends[i], key)
                device[i] = (key, plan, mo.blend(plan))
    return dict(cat=cat, blends=blends, tables=tables, report=report, device=device)


def _sources(runs):
    """Every source with components of the device cases:
    ``((name, blend), source, row, key, plan, rect, K, oracle)``."""
    for i, (key, plan, oracle) in runs["device"].items():
        name, blend, _ = runs["cat"][i]
        for src, row, (rect, comps), o in zip(blend.sources, runs["tables"][i], plan["sources"], oracle):
            if o is not None:
                yield (name, blend), src, row, key, plan, rect, len(comps), o


def _bounds(key, plan, rect, K, o):
    """The bound of every sum: (n + kh kw K + 4) 2^-52 sum|terms|, n the pixels summed --
    recursive summation of the same terms in two orders.  ``(model (C, 6), rendered (bands, 3))``."""
    _, kh, kw = key
    n_box = rect[2] * rect[3]
    n_region = mo.region_pixels(rect, plan["shape"], kh, kw)
    return ((n_box + kh * kw * K + 4) * U * o["records_abs"],
            (n_region + kh * kw * K + 4) * U * o["rendered_abs"])


def test_report_and_shapes(runs):
    from scarlet_amd import measure

    assert runs["report"]["launches"] == 3
    assert len(runs["tables"]) == len(runs["cat"])
    for (name, blend, _), table in zip(runs["cat"], runs["tables"]):
        C_obs = sum(o.shape[0] for o in blend.observations)
        assert table.dtype == measure.table_dtype(blend.frame.C, C_obs), name
        assert len(table) == len(blend.sources)


def test_sums_against_the_oracle(runs):
    worst = 0.0
    for (name, blend), src, row, key, plan, rect, K, o in _sources(runs):
        model_bound, rendered_bound = _bounds(key, plan, rect, K, o)
        got = np.concatenate([row["flux"][:, None], row["sums"]], axis=1)
        err = np.abs(got - o["records"][:, :6])
        worst = max(worst, float((err / np.maximum(model_bound, 1e-300)).max()))
        assert np.all(err <= model_bound), (name, err, model_bound)
        got = np.stack([row["rendered_flux"], row["rendered_sq"], row["rendered_var"]], axis=1)
        err = np.abs(got - o["rendered"])
        worst = max(worst, float((err / np.maximum(rendered_bound, 1e-300)).max()))
        assert np.all(err <= rendered_bound), (name, err, rendered_bound)
    print("largest error of a sum over its bound: %.3g" % worst)


def test_peak_is_exact(runs):
    from scarlet_amd import measure

    ties = 0
    for (name, blend), src, row, key, plan, rect, K, o in _sources(runs):
        cube = o["cube"]
        at = np.unravel_index(np.argmax(cube), cube.shape)
        want = (at[0], at[1] + rect[0], at[2] + rect[1])
        assert tuple(row["peak"]) == want == tuple(measure.max_pixel(src)), name
        assert row["peak_value"] == cube.max(), name
        ties += int((cube == cube.max()).sum() == 4)
    assert ties == 1  # the tie across two bands and two pixels is among them


def test_snr_against_the_oracle(runs):
    """First-order propagation: the S/N lies within four times the largest relative bound among
    its sums (valid while sum|R| <= 10 |sum R|, which the host test checks)."""
    from scarlet_amd import measure

    worst = 0.0
    for (name, blend), src, row, key, plan, rect, K, o in _sources(runs):
        _, rendered_bound = _bounds(key, plan, rect, K, o)
        rel = float((rendered_bound / np.abs(o["rendered"])).max())
        want = measure.snr_of_sums(*o["rendered"].T)
        err = abs(row["snr"] - want) / abs(want)
        worst = max(worst, err)
        assert err <= 4 * rel, (name, row["snr"], want, rel)
    print("largest relative S/N distance from the oracle: %.3g" % worst)


def test_alone_in_chunks_and_reversed(runs):
    """A blend's table has the same bits alone, in the whole catalogue, in chunks and in the
    reversed list."""
    import scarlet_amd as scarlet
    from scarlet_amd import _catalog, measure

    blends, tables = runs["blends"], runs["tables"]
    device = sorted(runs["device"])
    for i in device:
        (alone,) = scarlet.measure_blends([blends[i]])
        assert alone.tobytes() == tables[i].tobytes(), runs["cat"][i][0]
    picked = [blends[i] for i in device]
    # a budget of one byte: every blend a chunk of its own
    report = {}
    for i, table in zip(device, scarlet.measure_blends(picked, _working_set_bytes=1, _report=report)):
        assert table.tobytes() == tables[i].tobytes(), runs["cat"][i][0]
    assert report["fallback"] == []
    # a budget that holds two blends of the largest group, not three
    group = [i for i in device if runs["device"][i][0] == (3, 5, 5)]
    need = [measure._plan_bytes(runs["device"][i][1], (3, 5, 5)) for i in group]
    assert len(group) == 3
    budget = need[0] + need[1]
    assert _catalog.chunks(list(zip(group, need)), budget) == [group[:2], group[2:]]
    for i, table in zip(group, scarlet.measure_blends([blends[i] for i in group],
                                                      _working_set_bytes=budget)):
        assert table.tobytes() == tables[i].tobytes(), runs["cat"][i][0]
    for i, table in zip(device[::-1], scarlet.measure_blends(picked[::-1])):
        assert table.tobytes() == tables[i].tobytes(), runs["cat"][i][0]


def test_against_the_per_source_functions(runs):
    """flux and centroid within the summation bound of measure.flux and measure.centroid; the
    S/N as near measure.snr -- which renders in float32 through the FFT -- as that is to the
    oracle, plus the device's own bound."""
    from scarlet_amd import measure

    worst = 0.0
    for (name, blend), src, row, key, plan, rect, K, o in _sources(runs):
        model_bound, rendered_bound = _bounds(key, plan, rect, K, o)
        assert np.all(np.abs(row["flux"] - measure.flux(src)) <= model_bound[:, 0]), name
        # the centroid: ratios of sums over all bands, each within the sum of its bands' bounds
        want = measure.centroid(src)
        origin = np.array(src.bbox.origin, np.float64)
        total = o["records"][:, 0].sum()
        C = key[0]
        num_bound = np.array([(C - 1) * model_bound[:, 0].sum(), model_bound[:, 1].sum(),
                              model_bound[:, 2].sum()])
        scale = np.abs(want - origin)
        bound = (num_bound + scale * model_bound[:, 0].sum()) / total * 2 + 4 * U * np.abs(want)
        assert np.all(np.abs(row["centroid"] - want) <= bound), (name, row["centroid"], want)
        loop = measure.snr(src, blend.observations)
        oracle = measure.snr_of_sums(*o["rendered"].T)
        rel = float((rendered_bound / np.abs(o["rendered"])).max())
        worst = max(worst, abs(loop - oracle) / abs(oracle))
        assert abs(row["snr"] - loop) <= abs(loop - oracle) + 4 * rel * abs(oracle), name
    print("largest relative distance of measure.snr from the oracle: %.3g" % worst)


def test_fallback_rows_and_report(runs):
    """Refused blends and the one whose values are not finite get the rows of the per-source
    functions; ``_report`` names them, in list order."""
    from scarlet_amd import measure

    cat, twin = runs["cat"], mc.catalogue()
    fallback = runs["report"]["fallback"]
    assert [cat[i][0] for i, _ in fallback] == [n for n, _, e in cat if e != "device"]
    for i, why in fallback:
        if cat[i][2] == "runtime":
            assert why == "at run time: a model value that is not finite"
        else:
            assert why.startswith(cat[i][2])
        want = measure.measure_sources(twin[i][1])
        got = runs["tables"][i]
        assert got.dtype == want.dtype
        for field in got.dtype.names:
            assert_array_equal(got[field], want[field], err_msg="%s %s" % (cat[i][0], field))


def test_c_entry_validates_before_any_launch(runs):
    """An out-of-range offset, a stamp side of 65, an even stamp and buffers one element short:
    an error, and the outputs untouched.  The tables are checked on the host; nothing is
    launched."""
    from scarlet_amd import _lib, measure

    lib = _lib.load()
    key = (3, 5, 5)
    i = [c[0] for c in runs["cat"]].index("tiny")
    packed = measure.pack([runs["device"][i][1]], key)

    def call(key=key, short=None, **tables):
        p = dict(packed, **tables)
        records = np.full(p["n_record"], -7.0)
        rendered = np.full(p["n_rendered"], -7.0)
        args = [0, *key]
        for name in ("sources", "comps", "bands"):
            args += [len(p[name]), p[name].ctypes.data]
        for name, ct in (("seds", ctypes.c_double), ("morphs", ctypes.c_double),
                         ("stamps", ctypes.c_float), ("weights", ctypes.c_float)):
            args += [_lib.ptr(p[name], ct), p[name].size - (short == name)]
        args += [_lib.ptr(records, ctypes.c_double), records.size - (short == "records"),
                 _lib.ptr(rendered, ctypes.c_double), rendered.size - (short == "rendered")]
        rc = lib.smi_measure_sources_f32(*args)
        return rc, np.all(records == -7.0) and np.all(rendered == -7.0)

    rc, untouched = call()
    assert rc == 0 and not untouched  # the tables themselves are good
    bad = []
    for field, table, row, value in (("morph_off", "comps", -1, packed["morphs"].size),
                                     ("sed_off", "comps", 0, -1),
                                     ("weight_off", "bands", 2, packed["weights"].size - 98),
                                     ("stamp_off", "bands", 1, packed["stamps"].size - 24),
                                     ("channel", "bands", 0, 3), ("comp0", "sources", 3, 4),
                                     ("n_band", "sources", 0, 4), ("h", "sources", 1, 0),
                                     ("y0", "comps", 1, -2)):
        changed = packed[table].copy()
        changed[field][row] = value
        bad.append(("%s.%s" % (table, field), call(**{table: changed})))
    bad.append(("65", call(key=(3, 65, 5))))
    bad.append(("even", call(key=(3, 4, 5))))
    bad.append(("stamp shape beyond the buffer", call(key=(3, 5, 7))))
    for name in ("seds", "morphs", "stamps", "weights", "records", "rendered"):
        bad.append((name + " one short", call(short=name)))
    for what, (rc, untouched) in bad:
        assert rc < 0 and untouched, what
