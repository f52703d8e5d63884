"""lite.measure_blends on the device: known answers to the bit, the first maximum, the eight
raw sums of every edge and multi-tile case within the bound of a reordered sum around their
``fsum``, the derived fields on the reference's fitted scene, ``keep_flux``, and bits that do
not depend on where a blend stands in a catalogue.

The bound.  The device and ``measure_oracle`` add the same N float64 terms t_i per sum (N the
pixels of the flux box): value x integer weight, the weight exact, the product exact for
float32 data and rounded once, identically on both sides, for float64 data.  A floating-point
sum of N numbers in ANY order is the exact sum of t_i (1 + d_i) with |d_i| <= (1 + u)^(N-1) - 1
(Higham, Accuracy and Stability, 4.2), u = 2^-53, so it lies within ((1 + u)^(N-1) - 1) sum|t_i|
of the exact sum; ``fsum`` is the exact sum rounded once, within u sum|t_i|.  For N u < 0.01 the
two together stay below (N + 1) u sum|t_i| -- which also has room for the exact products of
float64 data (another u sum|t_i|) when N >= 2.  Zeros added for lanes without a pixel change
nothing.  ``measure_oracle.exact_sums`` returns the ``fsum`` and this bound."""

from types import SimpleNamespace

import numpy as np
import pytest

import measure_cases
import measure_oracle as oracle
import reweight_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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


def _same_tables(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, i
        assert x.tobytes() == y.tobytes(), i


def _check_against_oracle(table, blend, mask_footprint=True):
    """Rows of ``table`` against the oracle's cubes of ``blend``: null rows all zero, boxes,
    the eight raw sums within the bound, the peak exact.  Returns the largest error / bound."""
    zero = np.zeros(1, table.dtype)[0].tobytes()
    worst = 0.0
    for row, src, (flux, model, origin) in zip(table, blend.sources,
                                               oracle.cubes(blend, mask_footprint)):
        if origin is None:
            assert row.tobytes() == zero
            continue
        assert row["n_components"] == len(src.components)
        assert tuple(row["box"]) == tuple(origin[1:]) + flux.shape[1:]
        got = oracle.table_sums(row)
        if flux.size == 0:
            assert (got == 0).all() and tuple(row["peak"]) == (0, 0, 0) and row["snr"] == 0
            continue
        want, bound = oracle.exact_sums(flux, model)
        err = np.abs(got - want)
        share = (err / np.maximum(bound, 1e-300)).max(axis=0)
        print("largest |sum - fsum| / bound per sum:", np.round(share, 3))
        assert (err <= bound).all(), share
        worst = max(worst, float(share.max()))
        at, value = oracle.first_peak(flux)
        assert tuple(row["peak"]) == tuple(a + o for a, o in zip(at, origin))
        assert row["peak_value"] == value
    return worst


# ------------------------------------------------------------------ known answers
def _closed_forms(h, w):
    """sum 1, y, x, y^2, y x, x^2 over an h x w box."""
    sy, sx = h * (h - 1) // 2, w * (w - 1) // 2
    return (h * w, w * sy, h * sx, w * ((h - 1) * h * (2 * h - 1) // 6), sy * sx,
            h * ((w - 1) * w * (2 * w - 1) // 6))


@pytest.mark.parametrize("shape", [(1, 1), (32, 32), (33, 33), (35, 64)])
def test_known_answers(shape):
    """f = 1 and M = the integer spectrum on the whole flux box: every sum and every partial
    sum is an integer far below 2^53, so the table holds the closed forms to the bit -- one
    tile, an exact tile, one pixel over both ways, 2 x 2 ragged tiles."""
    from scarlet_amd import lite

    h, w = shape
    blend = measure_cases.flat_blend(h, w, origin=(3, 1))
    assert lite.plan_measure_blends([blend])[1] == []
    (table,) = lite.measure_blends([blend])
    assert table.shape == (1,) and table.dtype == lite.catalog.table_dtype(3)
    row = table[0]
    n, sy, sx, syy, syx, sxx = _closed_forms(h, w)
    assert row["n_components"] == 1 and tuple(row["box"]) == (3, 1, h, w)
    assert np.array_equal(row["flux"], [n] * 3)
    assert np.array_equal(row["sums"], [[sy, sx, syy, syx, sxx]] * 3)
    assert np.array_equal(row["model_flux"], [n, 2 * n, 3 * n])
    assert np.array_equal(row["model_sq"], [n, 4 * n, 9 * n])
    assert tuple(row["peak"]) == (0, 3, 1) and row["peak_value"] == 1
    # 3 sy / 3 n and 3 sx / 3 n are (h - 1) / 2 and (w - 1) / 2: exact quotients
    assert tuple(row["centroid"]) == (3 + (h - 1) / 2, 1 + (w - 1) / 2)
    assert blend.sources[0].flux is None and blend.sources[0].flux_box is None


@pytest.mark.parametrize("planted, first", [
    ([(1, 4, 5), (1, 9, 2)], (1, 4, 5)),         # inside one tile
    ([(0, 7, 2), (0, 5, 33)], (0, 5, 33)),       # either side of a vertical tile edge
    ([(0, 32, 3), (0, 31, 40)], (0, 31, 40)),    # either side of a horizontal tile edge
    ([(2, 1, 1), (0, 20, 50)], (0, 20, 50)),     # two bands
    ([(2, 34, 63)], (2, 34, 63)),                # alone in the last pixel of the last tile
], ids=["tile", "across-x", "across-y", "bands", "last-pixel"])
def test_peak_is_the_first_maximum(planted, first):
    """Equal maxima: the first in (band, y, x) order wins, as ``np.argmax``."""
    from scarlet_amd import lite

    h, w = 35, 64
    blend = measure_cases.flat_blend(h, w, origin=(3, 1), planted=[(p, 7.0) for p in planted])
    row = lite.measure_blends([blend])[0][0]
    assert tuple(row["peak"]) == (first[0], first[1] + 3, first[2] + 1) and row["peak_value"] == 7
    n, sy, sx, syy, syx, sxx = _closed_forms(h, w)
    want = np.array([[n, sy, sx, syy, syx, sxx]] * 3, np.float64)
    for b, y, x in planted:  # f = the image: 6 more than 1 at every planted pixel, all exact
        want[b] += 6 * np.array([1, y, x, y * y, y * x, x * x])
    assert np.array_equal(row["flux"], want[:, 0]) and np.array_equal(row["sums"], want[:, 1:])


# ------------------------------------------------------------------ raw sums within the bound
@pytest.mark.parametrize("mask_footprint", [True, False])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_edge_blends(name, mask_footprint):
    """The eight raw sums per (source, band) within ``(N + 1) 2^-53 sum|t|`` of their ``fsum``
    (derivation: module docstring), peak and box exact, on blends whose images have both
    signs -- and the boxes are those ``weight_sources`` sets on a copy."""
    from scarlet_amd import lite

    blend, copy = cases.make_blend(name), cases.make_blend(name)
    (table,) = lite.measure_blends([blend], mask_footprint)
    _check_against_oracle(table, blend, mask_footprint)
    lite.weight_sources(copy, mask_footprint)
    for row, src in zip(table, copy.sources):
        if not src.is_null:
            assert tuple(row["box"]) == tuple(src.flux_box.origin[1:]) + tuple(src.flux_box.shape[1:])


@pytest.mark.parametrize("name", ["33x31-bcast", "7x5-15x15"])
def test_edge_blends_float64(name):
    from scarlet_amd import lite

    blend = cases.make_blend(name, dtype=np.float64)
    (table,) = lite.measure_blends([blend])
    _check_against_oracle(table, blend)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_multi_tile_sources(dtype):
    """64 x 65 frame, 5 x 5 stamp with negative lobes: flux boxes of 35 x 64 (two components),
    33 x 33 in the frame's corner, a null source and a small one -- the same bound."""
    from scarlet_amd import lite

    blend = measure_cases.make_blend(dtype, corner=(3, -2))
    (table,) = lite.measure_blends([blend])
    boxes = [None if r["n_components"] == 0 else tuple(r["box"]) for r in table]
    assert boxes == [None if b is None else (b[0] + 3, b[1] - 2, b[2], b[3])
                     for b in measure_cases.FLUX_BOXES]
    _check_against_oracle(table, blend)


# ------------------------------------------------------------------ derived fields
def _quotient(a, da, b, db):
    """Bound of |a' / b' - a / b| for |a' - a| <= da, |b' - b| <= db < |b|."""
    return (da + abs(a / b) * db) / (abs(b) - db)


def _product(a, da, b, db):
    return abs(a) * db + abs(b) * da + da * db


def test_derived_fields_on_the_golden_scene(hsc):
    """43 x 43 stamp, ten sources, positive models: flux, centroid, moments, peak and snr against
    the host measurement (``catalog.records_of`` / ``fill_row``) of ``src.flux`` and M from
    ``weight_sources``.

    Bound.  Device and host sums both lie within e = (N + 1) u sum|t| of the exact sum, so they
    differ by at most 2 e (``d`` below, per band and sum); flux is such a sum.  With A = sum_b
    S_y, B = sum_b S_0 (C-term float64 sums: another C u |A| per side), c = A / B, the
    quotient rule gives dc = (dA + |c| dB) / (B - dB), plus u |c| per side for the division.
    A central moment, e.g. S_yy - 2 c S_y + c^2 S_0, is a sum of products of quantities with
    known bounds: the product rule |a| db + |b| da + da db per product, added up, plus 8 u
    times the sum of the terms' magnitudes for the host's own few roundings on both sides.
    snr = P / sqrt(D) with P = sum_b Q / S and D = sum_b n^2 Q / S^2: the quotient rule twice
    per band, d sqrt(D) = dD / (2 sqrt(D - dD)), the quotient rule once more, and 16 u per
    operation chain for the roundings."""
    from scarlet_amd import lite
    from scarlet_amd.lite import catalog

    g = golden("lite_fista")
    blend, copy = _golden_blend(hsc, g), _golden_blend(hsc, g)
    (table,) = lite.measure_blends([blend])
    lite.weight_sources(copy)
    obs = copy.observation
    noise = np.asarray(obs.noise_rms, np.float64)
    C = obs.images.shape[0]
    assert len(table) == 10
    for row, src in zip(table, copy.sources):
        model = catalog._source_model(copy, src)
        _, y0, x0 = src.flux_box.origin
        _, h, w = src.flux_box.shape
        want = np.zeros(1, table.dtype)[0]
        rec = catalog.records_of(src.flux, model)
        catalog.fill_row(want, 1, (y0, x0, h, w), rec, noise)
        d = 2 * oracle.exact_sums(src.flux, model)[1]  # (C, 8): M, M^2, f, y f, x f, yy, yx, xx
        assert tuple(row["box"]) == (y0, x0, h, w) and tuple(row["peak"]) == tuple(want["peak"])
        assert row["peak_value"] == want["peak_value"]
        assert (np.abs(row["flux"] - want["flux"]) <= d[:, 2]).all()
        S0, Sy, Sx = rec[:, 2], rec[:, 3], rec[:, 4]
        B = S0.sum()
        dB = d[:, 2].sum() + 2 * C * U * np.abs(S0).sum()
        assert abs(B) > dB
        c, dc = [], []
        for k, S in ((3, Sy), (4, Sx)):
            A = S.sum()
            dA = d[:, k].sum() + 2 * C * U * np.abs(S).sum()
            c.append(A / B)
            dc.append(_quotient(A, dA, B, dB) + 2 * U * abs(A / B))
        assert abs(row["centroid"][0] - want["centroid"][0]) <= dc[0] + 2 * U * abs(want["centroid"][0])
        assert abs(row["centroid"][1] - want["centroid"][1]) <= dc[1] + 2 * U * abs(want["centroid"][1])
        (cy, cx), (dcy, dcx) = c, dc
        for b in range(C):
            e = d[b]
            # yy: S_yy - 2 cy S_y + cy^2 S_0
            terms = [(rec[b, 5], e[5]), (2 * cy * Sy[b], 2 * _product(cy, dcy, Sy[b], e[3])),
                     (cy * cy * S0[b], _product(cy * cy, _product(cy, dcy, cy, dcy), S0[b], e[2]))]
            bound = sum(t[1] for t in terms) + 8 * U * sum(abs(t[0]) for t in terms)
            assert abs(row["moments"][b, 0] - want["moments"][b, 0]) <= bound
            # xx
            terms = [(rec[b, 7], e[7]), (2 * cx * Sx[b], 2 * _product(cx, dcx, Sx[b], e[4])),
                     (cx * cx * S0[b], _product(cx * cx, _product(cx, dcx, cx, dcx), S0[b], e[2]))]
            bound = sum(t[1] for t in terms) + 8 * U * sum(abs(t[0]) for t in terms)
            assert abs(row["moments"][b, 2] - want["moments"][b, 2]) <= bound
            # yx: S_yx - cy S_x - cx S_y + cy cx S_0
            terms = [(rec[b, 6], e[6]), (cy * Sx[b], _product(cy, dcy, Sx[b], e[4])),
                     (cx * Sy[b], _product(cx, dcx, Sy[b], e[3])),
                     (cy * cx * S0[b], _product(cy * cx, _product(cy, dcy, cx, dcx), S0[b], e[2]))]
            bound = sum(t[1] for t in terms) + 8 * U * sum(abs(t[0]) for t in terms)
            assert abs(row["moments"][b, 1] - want["moments"][b, 1]) <= bound
        # snr
        S, Q, dS, dQ = rec[:, 0], rec[:, 1], d[:, 0], d[:, 1]
        assert (S > 0).all()
        P = dP = D = dD = 0.0
        for b in range(C):
            q, dq = Q[b] / S[b], _quotient(Q[b], dQ[b], S[b], dS[b]) + 2 * U * Q[b] / S[b]
            q2, dq2 = q / S[b], _quotient(q, dq, S[b], dS[b]) + 2 * U * q / S[b]
            n2 = noise[b] * noise[b]
            P, dP = P + q, dP + dq
            D, dD = D + n2 * q2, dD + n2 * dq2 + 4 * U * n2 * q2
        dP += 2 * C * U * P
        dD += 2 * C * U * D
        root, droot = np.sqrt(D), dD / (2 * np.sqrt(D - dD)) + 2 * U * np.sqrt(D)
        bound = _quotient(P, dP, root, droot) + 16 * U * P / root
        assert abs(row["snr"] - want["snr"]) <= bound
        assert row["snr"] > 0 and np.isfinite(row["centroid"]).all()


# ------------------------------------------------------------------ keep_flux
def test_keep_flux():
    from scarlet_amd import lite

    def blends():
        return [measure_cases.make_blend(), cases.make_blend("33x31-C7"),
                cases.make_blend("7x5-3x3", mixed=True)]

    kept, plain, weighted = blends(), blends(), blends()
    with_cubes = lite.measure_blends(kept, keep_flux=True)
    lite.weight_blends(weighted)
    for a, b in zip(kept, weighted):
        cases.assert_same(cases.fluxes(a), cases.fluxes(b))
    without = lite.measure_blends(plain)
    assert all(s.flux is None and s.flux_box is None for b in plain for s in b.sources)
    _same_tables(with_cubes, without)


# ------------------------------------------------------------------ placement independence
def _catalogue():
    return [cases.make_blend("7x5-3x3"), cases.make_blend("33x31-bcast"),
            cases.make_blend("7x5-3x3", mixed=True), measure_cases.make_blend(),
            cases.make_blend("33x31-bcast", dtype=np.float64), cases.make_blend("7x5-3x3", seed=1),
            measure_cases.make_blend(seed=1), cases.make_blend("33x31-bcast", seed=2)]


def test_bits_do_not_depend_on_the_catalogue():
    """Alone = in a list of eight = one blend per chunk = the same call again, bit for bit;
    float32, float64 and a mixed-dtype fallback blend in one list each get the row they get
    alone, and the fallback's rows stay within the bound."""
    from scarlet_amd import lite

    groups, fallback = lite.plan_measure_blends(_catalogue())
    assert fallback == [2] and sorted(len(v) for v in groups.values()) == [1, 2, 4]
    together = lite.measure_blends(_catalogue())
    again = lite.measure_blends(_catalogue())
    alone = [lite.measure_blends([b])[0] for b in _catalogue()]
    small = lite.measure_blends(_catalogue(), _working_set_bytes=1)  # one blend per chunk
    _same_tables(together, again)
    _same_tables(together, alone)
    _same_tables(together, small)
    eight = [measure_cases.make_blend(seed=s % 2) for s in range(8)]
    tables = lite.measure_blends(eight)
    _same_tables(tables, [together[3], together[6]] * 4)
    # the fallback blend: float32 images, float64 morphologies -- the oracle of its float32 twin
    # does not apply, so its cubes come from weight_sources on a copy
    ref = _catalogue()[2]
    lite.weight_sources(ref)
    for row, src in zip(together[2], ref.sources):
        if src.is_null or src.flux.size == 0:
            continue
        model = lite.catalog._source_model(ref, src)
        want, bound = oracle.exact_sums(src.flux, model)
        assert (np.abs(oracle.table_sums(row) - want) <= bound).all()
        at, value = oracle.first_peak(src.flux)
        assert tuple(row["peak"]) == tuple(a + o for a, o in zip(at, src.flux_box.origin))
        assert row["peak_value"] == value


# ------------------------------------------------------------------ refusals
def test_a_bad_plan_is_refused():
    """smi_lite_measure_* validates plan and buffers on the host: nothing out of range is
    launched."""
    import ctypes

    from scarlet_amd import _lib
    from scarlet_amd.lite import catalog, measure

    blend = cases.make_blend("7x5-3x3")
    key = measure._group_key(blend)

    def packed():
        return measure._pack([measure._plan_blend(blend)], key, True)

    def broken(table, field, value, row=0):
        p = packed()
        p[table][field][row] = value
        return p

    records, out = catalog._run_chunk(packed(), key, 0, True)  # the plan itself is fine
    assert records.shape == (6, 3, catalog.RECORD) and out.size == packed()["n_out"]
    bad = [broken("sources", "h", 8), broken("sources", "x0", -1), broken("sources", "blend", 1),
           broken("sources", "n_comp", 100), broken("comps", "morph_off", 10 ** 9),
           broken("comps", "stride", 1), broken("comps", "sed_off", -1), broken("comps", "h", -1),
           broken("blends", "h", 0), broken("blends", "image_off", 1), broken("blends", "n_comp", -1)]
    for p in bad:
        for keep in (False, True):
            with pytest.raises(_lib.ScarletAmdError, match="status -1"):
                catalog._run_chunk(p, key, 0, keep)
    # the cube offsets count only when there is a cube buffer
    for value in (-1, 10 ** 9):
        with pytest.raises(_lib.ScarletAmdError, match="status -1"):
            catalog._run_chunk(broken("sources", "out_off", value), key, 0, True)
        got, _ = catalog._run_chunk(broken("sources", "out_off", value), key, 0, False)
        assert got.tobytes() == records.tobytes()
    for k in ((key[0], key[1], 4, 3), (key[0], key[1], 201, 201), (key[0], 0, 3, 3)):
        with pytest.raises(_lib.ScarletAmdError, match="status -1"):
            catalog._run_chunk(packed(), k, 0, False)
    with pytest.raises(_lib.ScarletAmdError, match="status -1"):
        catalog._run_chunk(packed(), key, 1 << 20, False)  # no such device

    # buffer sizes, through the C entry itself
    def call(p, out, n_out, rec, n_rec):
        _, C, kh, kw = key
        args = [0, C, kh, kw]
        for name in ("blends", "sources", "comps"):
            args += [len(p[name]), p[name].ctypes.data]
        for arr in (p["images"], p["stamps"], p["seds"], p["morphs"]):
            args += [_lib.ptr(arr, ctypes.c_float), arr.size]
        args += [_lib.ptr(out, ctypes.c_float), n_out, _lib.ptr(rec, ctypes.c_double), n_rec]
        return _lib.load().smi_lite_measure_f32(*args)

    p = packed()
    rec = np.zeros(records.size, np.float64)
    cube = np.zeros(p["n_out"], np.float32)
    assert call(p, None, 0, rec, rec.size) == 0 and rec.tobytes() == records.tobytes()
    assert call(p, cube, cube.size, rec, rec.size) == 0 and cube.tobytes() == out.tobytes()
    assert call(p, None, 0, rec, rec.size - 1) == -1       # a record buffer one entry short
    assert call(p, None, 0, None, rec.size) == -1
    assert call(p, None, 0, rec, -1) == -1
    assert call(p, None, cube.size, rec, rec.size) == -1   # a size without a buffer
    assert call(p, cube, cube.size - 1, rec, rec.size) == -1
    assert call(p, cube, -1, rec, rec.size) == -1
