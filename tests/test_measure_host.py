"""lite.measure_blends without a GPU: the host measurement of lite/catalog.py against the
``fsum`` oracle, against ``scarlet_amd.measure`` and against the reference's ``snr``; the
fields derived from given sums; the planning; the table's dtype."""

import numpy as np
import pytest

import measure_cases
import measure_oracle as oracle
import reweight_cases


def _row(C):
    from scarlet_amd.lite import catalog

    return np.zeros(1, catalog.table_dtype(C))[0]


def _positive(C=3, h=9, w=14, seed=5):
    rng = np.random.RandomState(seed)
    return rng.uniform(0.1, 2.0, (C, h, w)), rng.uniform(0.0, 1.5, (C, h, w))


@pytest.mark.parametrize("blend", ["33x31-C7", "multi-tile"])
def test_host_records_are_within_the_bound_of_the_exact_sums(blend):
    """``records_of`` adds the oracle's float64 terms in NumPy's order: each sum lies within
    ``(N + 1) 2^-53 sum |t|`` of their ``fsum`` (the bound of any summation order, derived in
    test_gpu_measure), and the peak is the first maximum of the band."""
    from scarlet_amd.lite import catalog

    b = measure_cases.make_blend() if blend == "multi-tile" else reweight_cases.make_blend(blend)
    seen = 0
    for flux, model, origin in oracle.cubes(b):
        if origin is None or flux.size == 0:
            continue
        rec = catalog.records_of(flux, model)
        want, bound = oracle.exact_sums(flux, model)
        assert (np.abs(rec[:, :8] - want) <= bound).all()
        for band in range(flux.shape[0]):
            at = int(np.argmax(flux[band]))
            assert rec[band, 9] == at and rec[band, 8] == flux[band].reshape(-1)[at]
        seen += 1
    assert seen >= 3


def test_rows_agree_with_scarlet_amd_measure_on_positive_cubes():
    """flux, centroid, max_pixel and moments of ``scarlet_amd.measure`` on a positive float64
    cube.  Both sides add N = h w positive float64 terms per sum, each within N u of the exact
    sum relatively (u = 2^-53): flux within 2 N u; the centroid, a quotient of two such sums,
    within 5 N u.  A central moment is a raw second sum minus products of first sums -- at most
    four terms, none larger than ``sum (y^2 + x^2) f`` (Cauchy-Schwarz), each carrying at most
    (2 + 5 + 5) N u of relative error -- so it lies within 64 N u of that magnitude."""
    from scarlet_amd import measure
    from scarlet_amd.lite import catalog

    flux, model = _positive()
    C, h, w = flux.shape
    N, u = h * w, 2.0 ** -53
    row = _row(C)
    catalog.fill_row(row, 2, (7, -3, h, w), catalog.records_of(flux, model), np.ones(C), band0=0)
    assert row["n_components"] == 2 and tuple(row["box"]) == (7, -3, h, w)
    np.testing.assert_allclose(row["flux"], measure.flux(flux), rtol=2 * N * u)
    centre = measure.centroid(flux)
    np.testing.assert_allclose(row["centroid"], centre[1:] + (7, -3), rtol=5 * N * u)
    peak = measure.max_pixel(flux)
    assert tuple(row["peak"]) == (peak[0], peak[1] + 7, peak[2] - 3)
    assert row["peak_value"] == flux[peak]
    # moments takes centroid = (x, y): measure.py's own argument order
    want = measure.moments(flux, N=2, centroid=(centre[2], centre[1]))
    y, x = np.indices((h, w))
    scale = ((y * y + x * x) * flux).sum(axis=(1, 2))
    for k, key in enumerate([(0, 2), (1, 1), (2, 0)]):  # (power of x, power of y): yy, yx, xx
        assert (np.abs(row["moments"][:, k] - want[key]) <= 64 * N * u * scale).all(), key


def test_snr_is_the_reference_formula():
    """Reference scarlet/measure.py:89-102 restated literally (measure_oracle.reference_snr)
    on M: a handful of float64 operations on sums of N positive terms, within 16 N u."""
    from scarlet_amd.lite import catalog

    flux, model = _positive(C=4, seed=9)
    noise = np.array([0.5, 1.0, 2.0, 0.25])
    rec = catalog.records_of(flux, model)
    got = catalog.snr_of(rec[:, 0], rec[:, 1], noise)
    N = model[0].size
    np.testing.assert_allclose(got, oracle.reference_snr(model, noise), rtol=16 * N * 2.0 ** -53)
    row = _row(4)
    catalog.fill_row(row, 1, (0, 0) + flux.shape[1:], rec, noise)
    assert row["snr"] == got


def test_derived_fields_from_given_sums():
    from scarlet_amd.lite import catalog

    C = 2
    # a null source: nothing is touched
    row = _row(C)
    catalog.fill_row(row, 0, (5, 5, 3, 3), np.ones((C, catalog.RECORD)), np.ones(C))
    assert row.tobytes() == _row(C).tobytes()
    # an empty box: sums 0, centroid 0 / 0, signal-to-noise 0
    row = _row(C)
    catalog.fill_row(row, 1, (4, -2, 0, 7), None, np.ones(C), band0=3)
    assert row["n_components"] == 1 and tuple(row["box"]) == (4, -2, 0, 7)
    assert (row["flux"] == 0).all() and (row["sums"] == 0).all() and row["snr"] == 0
    assert np.isnan(row["centroid"]).all() and tuple(row["peak"]) == (0, 0, 0)
    # known sums: two pixels of flux 1 at (y, x) = (0, 0) and (2, 4) in band 0, nothing in band 1
    rec = np.zeros((C, catalog.RECORD))
    rec[0] = (3, 5, 2, 2, 4, 4, 8, 16, 1, 0)
    rec[1] = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    row = _row(C)
    catalog.fill_row(row, 1, (10, 20, 3, 5), rec, np.array([2.0, 7.0]), band0=1)
    assert tuple(row["centroid"]) == (11.0, 22.0)
    assert tuple(row["moments"][0]) == (2.0, 4.0, 8.0) and tuple(row["moments"][1]) == (0, 0, 0)
    assert tuple(row["peak"]) == (1, 10, 20) and row["peak_value"] == 1
    # band 1 has S = 0 and is left out: (Q / S) / sqrt(n^2 Q / S^2) = sqrt(Q) / n
    assert row["snr"] == pytest.approx(np.sqrt(5) / 2.0, rel=1e-15)
    assert catalog.snr_of([0, 0], [0, 0], [1, 1]) == 0
    # a zero total divides as NumPy does
    rec[0] = (3, 5, 0, 1, -1, 0, 0, 0, 1, 0)
    row = _row(C)
    catalog.fill_row(row, 1, (0, 0, 3, 5), rec, np.ones(C))
    assert row["centroid"][0] == np.inf and row["centroid"][1] == -np.inf
    # the peak: the lower band wins a tie, a later band wins when larger
    rec = np.zeros((C, catalog.RECORD))
    rec[0, 8:], rec[1, 8:] = (2.0, 7), (2.0, 3)
    row = _row(C)
    catalog.fill_row(row, 1, (0, 0, 3, 5), rec, np.ones(C))
    assert tuple(row["peak"]) == (0, 1, 2)
    rec[1, 8] = 2.5
    catalog.fill_row(row, 1, (0, 0, 3, 5), rec, np.ones(C))
    assert tuple(row["peak"]) == (1, 0, 3) and row["peak_value"] == 2.5


def test_plan_is_the_plan_of_weight_blends():
    from scarlet_amd import lite
    from scarlet_amd.lite import measure

    def blends():
        return [reweight_cases.make_blend("7x5-3x3"), measure_cases.make_blend(),
                reweight_cases.make_blend("7x5-3x3", mixed=True),
                reweight_cases.make_blend("33x31-bcast", dtype=np.float64),
                reweight_cases.make_blend("7x5-3x3", seed=1)]

    got = lite.plan_measure_blends(blends())
    assert got == measure.plan_blends(blends())
    assert got[1] == [2] and list(got[0].values())[0] == [0, 4]


@pytest.mark.parametrize("C", [1, 7])
def test_table_dtype(C):
    from scarlet_amd.lite import catalog

    dt = catalog.table_dtype(C)
    want = [("n_components", "<i4", ()), ("box", "<i4", (4,)), ("flux", "<f8", (C,)),
            ("sums", "<f8", (C, 5)), ("model_flux", "<f8", (C,)), ("model_sq", "<f8", (C,)),
            ("peak", "<i4", (3,)), ("peak_value", "<f8", ()), ("centroid", "<f8", (2,)),
            ("moments", "<f8", (C, 3)), ("snr", "<f8", ())]
    assert list(dt.names) == [n for n, _, _ in want]
    for name, base, shape in want:
        field = dt.fields[name][0]
        assert (field.base.str, field.shape) == (base, shape), name
    table = np.zeros(3, dt)
    assert table["flux"].shape == (3, C) and table["moments"].shape == (3, C, 3)


def test_a_chunk_is_filled_like_its_rows():
    """``_fill_chunk`` derives a whole chunk at once: every row has the bits ``fill_row`` gives
    it alone, null sources and empty boxes included, in the order of ``blend.sources``."""
    from scarlet_amd.lite import catalog, measure

    blends = [reweight_cases.make_blend("33x31-C7"), reweight_cases.make_blend("33x31-C7", seed=1)]
    key = measure._group_key(blends[0])
    plans = [measure._plan_blend(b) for b in blends]
    packed = measure._pack(plans, key, True)
    cubes = [c for b in blends for c in oracle.cubes(b) if c[2] is not None and c[0].size]
    records = np.array([catalog.records_of(f, m) for f, m, _ in cubes])
    assert len(records) == len(packed["results"]) == 12
    tables = [np.zeros(len(b.sources), catalog.table_dtype(7)) for b in blends]
    catalog._fill_chunk(plans, tables, packed, records)
    k = 0
    for b, table in zip(blends, tables):
        noise = np.asarray(b.observation.noise_rms, np.float64)
        for row, src, (flux, model, origin) in zip(table, b.sources, oracle.cubes(b)):
            want = _row(7)
            if origin is not None:
                rec = None
                if flux.size:
                    rec, k = records[k], k + 1
                catalog.fill_row(want, len(src.components), tuple(origin[1:]) + flux.shape[1:],
                                 rec, noise, band0=origin[0])
            assert row.tobytes() == want.tobytes()
    assert [r["n_components"] for r in tables[0]] == [2, 1, 1, 1, 1, 1, 0, 1]
