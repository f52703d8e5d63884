"""``lite.fit_spectra_blends`` without a GPU: the host solve against ``lstsq``, the plan (keys,
order, every reason for the per-blend path), chunking, the packed tables, the tile plan the
kernel walks, and the conditioning of every test case (the GPU tolerance is derived from it)."""

import numpy as np
import pytest
from numpy.testing import assert_allclose

import fit_spectra_cases as cases

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def _spectra():
    from scarlet_amd.lite import spectra

    return spectra


# ------------------------------------------------------------------------------ solve
def _designs():
    rng = np.random.RandomState(3)
    full = rng.uniform(0.1, 1.0, (40, 4))
    zero = full.copy()
    zero[:, 2] = 0
    twin = full.copy()
    twin[:, 3] = twin[:, 1]
    return {"full rank": full, "zero column": zero, "duplicated column": twin,
            "one component": full[:, :1]}


@pytest.mark.parametrize("name", list(_designs()))
def test_solve_spectra_is_the_minimum_norm_solution_of_lstsq(name):
    design = _designs()[name]
    rng = np.random.RandomState(4)
    data = rng.normal(0.5, 1.0, (3, design.shape[0]))  # three bands, one design
    gram = np.broadcast_to(design.T @ design, (3,) + (design.shape[1],) * 2)
    rhs = data @ design
    got = _spectra()._solve_spectra(gram, rhs, np.float64)
    want = np.stack([np.linalg.lstsq(design, d, rcond=None)[0] for d in data])
    assert got.shape == want.shape and got.dtype == np.float64
    assert (want < 0).any() or name == "one component"  # the clip acts
    assert_allclose(got, np.where(want < 0, 0, want), rtol=1e-9, atol=1e-9 * np.abs(want).max())
    if name == "zero column":
        assert np.all(got[:, 2] == 0)
    if name == "duplicated column":
        assert_allclose(got[:, 1], got[:, 3], rtol=1e-9)
    single = _spectra()._solve_spectra(gram, rhs, np.float32)
    assert single.dtype == np.float32 and np.all(single >= 0)
    assert np.array_equal(single, np.where(single < 0, 0, got.astype(np.float32)))


def test_solve_spectra_clips_after_the_cast():
    got = _spectra()._solve_spectra([[[2.0]], [[2.0]]], [[-1.0], [3.0]], np.float32)
    assert got.tolist() == [[0.0], [1.5]]


# ------------------------------------------------------------------------------- plan
def _even(dtype=np.float32):
    blend = cases.make_blend("7x5-3x3", dtype)
    blend.observation.diff_kernel.image = np.ones((3, 4, 3), dtype) / 12
    return blend


def _half():
    blend = cases.make_blend("7x5-3x3")
    blend.observation.images = blend.observation.images.astype(np.float16)
    return blend


def _two_band_stamp():
    blend = cases.make_blend("7x5-3x3")
    blend.observation.diff_kernel.image = blend.observation.diff_kernel.image[:2]
    return blend


def _list_spectrum():
    blend = cases.make_blend("7x5-3x3")
    blend.components[1]._sed.x = list(blend.components[1].sed)
    return blend


def _short_spectrum():
    blend = cases.make_blend("7x5-3x3")
    blend.components[1]._sed.x = blend.components[1].sed[:2].copy()
    return blend


def _no_components():
    from scarlet_amd import lite

    blend = cases.make_blend("7x5-3x3")
    return lite.LiteBlend([lite.LiteSource([], np.float32)], blend.observation)


FALLBACKS = [
    (_even, "even"),
    (_half, "neither float32 nor float64"),
    (lambda: cases.reweight_cases.make_blend("7x5-3x3", mixed=True), "mixed dtypes"),
    (_two_band_stamp, "not a stamp per band"),
    (_list_spectrum, "not spectrum x morphology arrays"),
    (_short_spectrum, "all bands"),
    (_no_components, "no components"),
] + [(lambda n=n: cases.make_blend(n), why) for n, why in cases.PAST_REASON.items()]


def test_plan_keys_and_order():
    from scarlet_amd import lite

    names = ["33x31-bcast", "7x5-none", "union-15", "7x5-3x3", "disjoint", "64x65-C1", "union-17"]
    blends = [cases.make_blend(n) for n in names] + [cases.make_blend("union-15", np.float64)]
    groups, fallback = lite.plan_fit_spectra_blends(blends)
    assert fallback == []
    assert list(groups.items()) == [
        ((F32, 3, 5, 5), [0]), ((F32, 3, 1, 1), [1]), ((F32, 2, 3, 3), [2, 4, 6]),
        ((F32, 3, 3, 3), [3]), ((F32, 1, 7, 5), [5]), ((F64, 2, 3, 3), [7])]


@pytest.mark.parametrize("k", range(len(FALLBACKS)))
def test_every_reason_for_the_per_blend_path(k):
    from scarlet_amd import lite

    make, why = FALLBACKS[k]
    blends = [cases.make_blend("7x5-3x3"), make(), cases.make_blend("7x5-5x9")]
    groups, fallback = lite.plan_fit_spectra_blends(blends)
    assert list(groups.values()) == [[0], [2]]
    assert [i for i, _ in fallback] == [1] and why in fallback[0][1], fallback


def test_clip_sends_a_component_the_data_do_not_reach_through_the_loop():
    """Its exact spectrum is 0, so whether ``clip=True`` drops it in the loop hangs on the sign
    of the loop's round-off: only the loop gives the loop's survivors.  Without ``clip`` the
    floor covers it either way and the device takes the blend."""
    from scarlet_amd import lite

    sp = _spectra()
    names = list(cases.NAMES)
    blends = [cases.make_blend(n) for n in names]
    assert lite.plan_fit_spectra_blends(blends)[1] == []
    groups, fallback = lite.plan_fit_spectra_blends(blends, clip=True)
    assert [names[i] for i, _ in fallback] == list(cases.reweight_cases.CASES)
    assert all("do not reach" in why for _, why in fallback)
    assert sorted(i for idx in groups.values() for i in idx) == list(range(8, len(names)))
    # frame 10 x 10, 3 x 3 stamp: far off alone; far off but touching a second one's grown box;
    # off the frame by less than the stamp's half; an empty box
    boxes = [(2, 2, 5, 5), (30, 0, 3, 3), (50, 0, 3, 3), (54, 2, 3, 3), (10, 3, 3, 3),
             (80, 80, 0, 3)]
    assert sp._out_of_reach(boxes, (10, 10), 3, 3) == [1]
    # (no stamp: the neighbours stop touching, and the box on the frame's edge is off it)
    assert sp._out_of_reach(boxes, (10, 10), 1, 1) == [1, 2, 3, 4]
    assert sp._out_of_reach(boxes[:1], (10, 10), 3, 3) == []


def test_the_limits_are_module_constants_the_cases_sit_on():
    sp = _spectra()
    assert (sp.TILE, sp.MAX_STAMP) == (cases.T, 63)
    assert sp.MAX_COMPONENTS >= 64 and sp.MAX_PRESENT >= 32
    at = {"present-32": sp.MAX_PRESENT, "components-64": sp.MAX_COMPONENTS}
    for name, limit in at.items():
        blend = cases.make_blend(name)
        assert sp._spectra_key(blend)[0] is not None, name
        boxes, union = sp._geometry(blend)
        if name == "present-32":
            assert sp._max_present(boxes, union, 3, 3) == limit
        else:
            assert len(boxes) == limit and sp._max_present(boxes, union, 3, 3) <= sp.MAX_PRESENT
    assert cases.OWN["stamp-63"]["stamp"][1] == sp.MAX_STAMP
    assert sp._spectra_key(cases.make_blend("stamp-63"))[0] == (F32, 1, 63, 63)


def test_no_components_surfaces_the_exception_of_the_loop():
    """(multifit_seds fails on its empty list of boxes before it touches the device)"""
    from scarlet_amd import lite

    with pytest.raises(IndexError):
        _no_components().fit_spectra()
    with pytest.raises(IndexError):
        lite.fit_spectra_blends([_no_components()])


def test_fit_spectra_and_the_batch_share_one_tail():
    """``LiteBlend._set_spectra``: in place, clipped at 0, then ``prox_sed`` or the drop."""
    blend = cases.make_blend("7x5-3x3")
    arrays = [c.sed for c in blend.components]
    K, C = len(arrays), 3
    seds = np.ones((K, C), np.float32)
    seds[0] = -1
    seds[2, 1] = -2
    first = blend.sources[0].components[1]
    assert blend._set_spectra(seds, False) is blend
    assert all(c.sed is a for c, a in zip(blend.components, arrays))
    assert arrays[0].tolist() == [np.float32(1e-20)] * 3 and arrays[2][1] == np.float32(1e-20)
    blend._set_spectra(seds, True)
    assert len(blend.components) == K - 1 and blend.components[0] is first
    assert blend.sources[0].components == [first]
    assert [c for s in blend.sources for c in s.components] == blend.components


# --------------------------------------------------------------------------- chunking
GROUP = ["union-15", "disjoint", "union-17", "present-32", "components-64"]


def test_chunks_at_a_middle_budget_and_at_one_byte():
    sp = _spectra()
    key = (F32, 2, 3, 3)
    plans = [sp._plan_blend(cases.make_blend(n))[1] for n in GROUP]
    need = [sp._plan_bytes(p, key) for p in plans]
    # union-15: 2 x 20 x 20 image + 2 morphologies of 81 in float32; 18 taps, one tile and the
    # output of 2 bands x (4 + 2) sums in float64
    assert need[0] == (800 + 162) * 4 + (18 + 2 * 2 * 6) * 8

    from scarlet_amd import _catalog

    def ids(chunks):
        return [[GROUP[plans.index(p)] for p in c] for c in chunks]

    items = [(p, sp._plan_bytes(p, key)) for p in plans]
    assert ids(_catalog.chunks(items, sum(need))) == [GROUP]
    assert ids(_catalog.chunks(items, 1)) == [[n] for n in GROUP]
    middle = need[0] + need[1] + need[2]
    chunks = _catalog.chunks(items, middle)
    assert 1 < len(chunks) < len(GROUP) and chunks[0] == plans[:3]
    assert [p for c in chunks for p in c] == plans
    for c, nxt in zip(chunks, chunks[1:] + [None]):
        used = sum(need[plans.index(p)] for p in c)
        assert used <= middle or len(c) == 1
        if nxt is not None:  # greedy: the next blend did not fit any more
            assert used + need[plans.index(nxt[0])] > middle


def test_packed_tables_of_a_two_blend_chunk():
    sp = _spectra()
    key = (F32, 2, 3, 3)
    blends = [cases.make_blend("union-15"), cases.make_blend("union-16")]
    packed = sp._pack([sp._plan_blend(b)[1] for b in blends], key)
    #        h   w   y0 x0 fh  fw  comp0 n  image stamp out
    assert packed["blends"].tolist() == [(20, 20, 1, 2, 15, 15, 0, 2, 0, 0, 0),
                                         (20, 20, 1, 2, 16, 16, 2, 2, 800, 18, 12)]
    assert packed["comps"].tolist() == [(1, 2, 9, 9, 0), (7, 8, 9, 9, 81), (1, 2, 9, 9, 162),
                                        (8, 9, 9, 9, 243)]
    assert packed["blends"].dtype.itemsize == 56 and packed["comps"].dtype.itemsize == 24
    assert packed["n_out"] == 24
    assert packed["images"].dtype == F32 and packed["images"].size == 1600
    assert np.array_equal(packed["images"][800:], blends[1].observation.images.reshape(-1))
    assert packed["stamps"].dtype == F64 and packed["stamps"].size == 36
    assert np.array_equal(packed["stamps"][18:],
                          blends[1].observation.diff_kernel.image.astype(np.float64).reshape(-1))
    assert packed["morphs"].dtype == F32 and packed["morphs"].size == 324
    assert np.array_equal(packed["morphs"][243:], blends[1].components[1].morph.reshape(-1))


def test_a_broadcast_or_missing_stamp_is_packed_per_band():
    sp = _spectra()
    for name, key in (("33x31-bcast", (F32, 3, 5, 5)), ("7x5-none", (F32, 3, 1, 1))):
        blend = cases.make_blend(name)
        stamps = sp._pack([sp._plan_blend(blend)[1]], key)["stamps"].reshape(key[1:])
        assert np.array_equal(stamps[0], stamps[2])
        if name == "7x5-none":
            assert np.all(stamps == 1)


# -------------------------------------------------------------------------- tile plan
@pytest.mark.parametrize("name", cases.NAMES)
def test_tile_plan_covers_every_pixel_once_and_keeps_every_overlap(name):
    """Every pixel of the union box lies in exactly one tile, and on every tile where the
    convolved columns of two components are both non-zero, both are present."""
    from scipy.signal import convolve2d

    sp = _spectra()
    blend = cases.make_blend(name)
    (dtype, C, kh, kw), _ = sp._spectra_key(blend)
    boxes, (uy, ux, fh, fw) = sp._geometry(blend)
    tiles = sp._tile_plan(boxes, (uy, ux, fh, fw), kh, kw)
    seen = np.zeros((fh, fw), int)
    for ty, tx, th, tw, _ in tiles:
        assert 0 < th <= sp.TILE and 0 < tw <= sp.TILE
        seen[ty:ty + th, tx:tx + tw] += 1
    assert np.all(seen == 1)
    assert [(t[0], t[1]) for t in tiles] == [(y, x) for y in range(0, fh, sp.TILE)
                                             for x in range(0, fw, sp.TILE)]
    support = []  # where a column can be non-zero: the box convolved with a full stamp
    for y0, x0, h, w in boxes:
        full = np.zeros((fh, fw))
        full[y0 - uy:y0 - uy + h, x0 - ux:x0 - ux + w] = 1
        support.append(convolve2d(full, np.ones((kh, kw)), mode="same") > 0)
    for ty, tx, th, tw, present in tiles:
        assert present == sorted(present) and len(present) <= sp.MAX_PRESENT
        for k, s in enumerate(support):
            if s[ty:ty + th, tx:tx + tw].any():
                assert k in present, (name, ty, tx, k)
    assert sp._max_present(boxes, (uy, ux, fh, fw), kh, kw) == max(len(t[4]) for t in tiles)


def test_the_disjoint_pair_shares_no_tile_pixel():
    sp = _spectra()
    boxes, union = sp._geometry(cases.make_blend("disjoint"))
    for ty, tx, th, tw, present in sp._tile_plan(boxes, union, 3, 3):
        grown = [(y0 - union[0] - 1, x0 - union[1] - 1, h + 2, w + 2) for y0, x0, h, w in boxes]
        a, b = grown
        assert a[1] + a[3] <= b[1]  # along x the grown boxes do not meet


# ----------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_is_well_conditioned(name, dtype):
    """The bound of the GPU test is 8 cond^2 n 2^-53; the cap is the one
    test_every_joint_fit_is_well_conditioned uses."""
    _, cond, n_pix = cases.oracle(cases.make_blend(name, dtype))
    assert cond <= 1e3, (name, cond)
    assert 8 * cond ** 2 * n_pix * 2.0 ** -53 < 2.0 ** -23


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", cases.NAMES)
def test_tables_solve_and_tail_reach_the_oracle(name, dtype, monkeypatch):
    """Everything but the kernel: with the sums formed by NumPy from the packed tables, the
    batch leaves the oracle's spectra within the bound the GPU test applies."""
    from scarlet_amd import lite

    sp = _spectra()
    monkeypatch.setattr(sp, "_run_chunk", lambda packed, key, device:
                        cases.sums_of_tables(packed, key))
    blend = cases.make_blend(name, dtype)
    seds64, cond, n_pix = cases.oracle(blend)
    lite.fit_spectra_blends([blend])
    got = np.stack([c.sed for c in blend.components])
    assert got.dtype == dtype
    assert cases.ratio_to_bound(got, seds64, cond, n_pix, dtype) <= 1


def test_the_reference_fitted_scene_is_planned_and_well_conditioned(hsc):
    from conftest import golden
    from scarlet_amd import lite

    g = golden("lite_fista")
    blend = cases.hsc_blend(hsc, g)
    assert lite.plan_fit_spectra_blends([blend]) == ({(F32, 5, 43, 43): [0]}, [])
    seds64, cond, n_pix = cases.oracle(blend)
    assert cond <= 1e3 and 8 * cond ** 2 * n_pix * 2.0 ** -53 < 2.0 ** -23
    # the oracle itself stands where the reference's own multifit_seds does
    ref = g["multifit_seds"]
    assert np.abs(np.where(seds64 < 0, 0, seds64) - ref).max() < 2e-3 * np.abs(ref).max()


def test_the_clip_acts_in_the_cases():
    """Images of both signs: some least-squares spectra are negative, in the small cases and
    in tiled ones."""
    negative = [n for n in cases.NAMES if (cases.oracle(cases.make_blend(n))[0] < 0).any()]
    assert set(negative) & set(cases.reweight_cases.CASES) and set(negative) & set(cases.OWN)
    assert "components-64" in negative
