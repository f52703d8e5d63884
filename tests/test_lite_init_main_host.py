"""``lite.init_blends_main`` without a GPU: the relative-cosine table and the level order of
the sweep kernel against the radial tables and the sequential sweep they replace, the CPU
restatement tests/init_main_oracle.py against the reference's run on hsc_cosmos_35
(tests/golden/lite_init.npz), the classes of the cases of tests/init_main_cases.py, and the
planning of the device batches."""

from types import SimpleNamespace

import numpy as np
import pytest

import init_cases
import init_main_cases as mc
import init_main_oracle as mo
from conftest import golden


@pytest.fixture(scope="module")
def cases():
    return {name: mc.make_case(name) for name in mc.CASES}


@pytest.fixture(scope="module")
def oracles(cases):
    return {name: mc.run_oracle(c) for name, c in cases.items()}


def _frames_and_centres(cases):
    seen = []
    for c in cases.values():
        for center in c.centers:
            item = (c.obs.images.shape[1:], tuple(center))
            if item not in seen:
                seen.append(item)
    return seen


def table_weights(shape, center):
    """The (8, N) float64 weights as the sweep kernel derives them: the entries of the
    relative-cosine table where the neighbour lies in the frame and strictly nearer the
    centre, zeros elsewhere, added in direction order and divided in float64."""
    from scarlet_amd.lite import initialization as li
    from scarlet_amd.operator import NEIGHBOR_COORDS

    h, w = shape
    cy, cx = center
    ry, rx = h + 2, w + 1  # (a table larger than the frame, as in a chunk of several frames)
    table = li._relative_cosines(ry, rx)
    Y, X = np.mgrid[:h, :w]
    Y, X = Y - cy, X - cx
    cosw = np.zeros((8, h, w))
    for i, (dy, dx) in enumerate(NEIGHBOR_COORDS):
        ny, nx = Y + dy, X + dx
        counts = ((cy + ny >= 0) & (cy + ny < h) & (cx + nx >= 0) & (cx + nx < w)
                  & (ny * ny + nx * nx < Y * Y + X * X))
        cosw[i] = np.where(counts, table[Y + ry, X + rx, i], 0.0)
    total = np.zeros((h, w))
    for i in range(8):
        total = total + cosw[i]
    total[total == 0] = 1
    return (cosw / total).reshape(8, h * w)


def test_cases_cover_what_the_issue_names(cases):
    shapes = {c.obs.images.shape[1:] for c in cases.values()}
    assert {(9, 11), (10, 12), (32, 36), (33, 37)} <= shapes
    assert {c.obs.images.dtype for c in cases.values()} == {np.dtype("f4"), np.dtype("f8")}
    pairs = _frames_and_centres(cases)
    for (h, w), want in [((9, 11), (0, 0)), ((9, 11), (8, 10)), ((9, 11), (4, 10)),
                         ((10, 12), (5, 6)), ((10, 12), (4, 6)), ((32, 36), (16, 18)),
                         ((32, 36), (15, 17)), ((32, 36), (31, 35)), ((33, 37), (16, 18)),
                         ((33, 37), (16, 19)), ((33, 37), (17, 0))]:
        assert ((h, w), want) in pairs
    stamps = {np.shape(c.obs.diff_kernel.image) for c in cases.values()}
    assert {(2, 3, 3), (1, 7, 5)} <= stamps
    assert {c.obs.psfs.shape[1:] for c in cases.values()} == {(3, 3), (5, 5), (7, 7)}
    assert any(c.detect is not None for c in cases.values())
    assert {c.options.get("percentile", 25) for c in cases.values()} == {25, 30}
    assert float(np.float32(0.3)) != 0.3  # the level is rounded to the data type


def test_table_weights_equal_the_radial_tables(cases):
    from scarlet_amd.operator import getRadialMonotonicWeights

    for shape, center in _frames_and_centres(cases):
        want = getRadialMonotonicWeights(shape, "angle", center)
        got = table_weights(shape, center)
        assert init_cases.same_bits(got, want), (shape, center)
        assert init_cases.same_bits(got.astype(np.float32), want.astype(np.float32))
        assert init_cases.same_bits(got, mo.angle_weights(shape, center)), (shape, center)


def test_every_weighted_neighbour_has_a_smaller_level(cases):
    from scarlet_amd.lite import initialization as li
    from scarlet_amd.operator import NEIGHBOR_COORDS

    for (h, w), (cy, cx) in _frames_and_centres(cases):
        weights = table_weights((h, w), (cy, cx)).reshape(8, h, w)
        Y, X = np.mgrid[:h, :w]
        Y, X = Y - cy, X - cx
        level = li._sweep_level(Y, X)
        assert level[cy, cx] == -1 and (np.delete(level.reshape(-1), cy * w + cx) >= 0).all()
        assert level.max() <= 3 * max(h, w)
        for i, (dy, dx) in enumerate(NEIGHBOR_COORDS):
            ys, xs = np.nonzero(weights[i] > 0)
            assert (level[ys + dy, xs + dx] < level[ys, xs]).all(), ((h, w), (cy, cx), i)
        # every pixel but the centre has a weighted neighbour
        assert ((weights > 0).sum(axis=0).reshape(-1) > 0).sum() == h * w - 1


def level_sweep(image, center):
    """The sweep of lite_init_main.hip in NumPy: level after level, every pixel of a level at
    once, the terms in direction order with one rounded multiply and one rounded add each."""
    from scarlet_amd.lite import initialization as li
    from scarlet_amd.operator import NEIGHBOR_COORDS

    h, w = image.shape
    weights = table_weights(image.shape, center).astype(image.dtype).reshape(8, h, w)
    Y, X = np.mgrid[:h, :w]
    level = li._sweep_level(Y - center[0], X - center[1])
    out = image.copy()
    for L in range(level.max() + 1):
        ys, xs = np.nonzero(level == L)
        ref = np.zeros(len(ys), image.dtype)
        for i, (dy, dx) in enumerate(NEIGHBOR_COORDS):
            on = weights[i, ys, xs] > 0
            term = out[ys[on] + dy, xs[on] + dx] * weights[i, ys[on], xs[on]]
            ref[on] = ref[on] + term
        lim = ref * image.dtype.type(1)
        out[ys, xs] = np.where(lim < out[ys, xs], lim, out[ys, xs])
    return out


def test_level_sweep_equals_the_sequential_sweep(cases):
    checked = 0
    for c in cases.values():
        detect = c.detect
        if detect is None:
            detect = mo.coadd(c.obs.images, np.asarray(c.obs.noise_rms))
        for center in c.centers:
            sym = mo.symmetrise(detect, center)
            assert init_cases.same_bits(level_sweep(sym, center), mo.sweep(sym, center)), \
                (c.name, center)
            checked += 1
    assert checked >= 30


def test_symmetry_equals_the_operator(cases):
    from scarlet_amd.operator import prox_uncentered_symmetry

    for c in cases.values():
        detect = mo.coadd(c.obs.images, np.asarray(c.obs.noise_rms))
        for center in c.centers:
            want = prox_uncentered_symmetry(detect.copy(), 0, center, "sdss")
            assert init_cases.same_bits(mo.symmetrise(detect, center), want), (c.name, center)
    # a corner centre keeps one pixel; an even extent shortens the sub-array by one more
    assert mo.centred_slices((9, 11), (0, 0)) == (slice(None, -8), slice(None, -10))
    assert mo.centred_slices((10, 12), (4, 6)) == (slice(None, -1), slice(1, None))
    assert mo.centred_slices((10, 12), (5, 6)) is None


def test_oracle_gives_every_case_its_classes(cases, oracles):
    for name, c in cases.items():
        assert [s["kind"] for s in oracles[name]] == c.kinds, name
    for name, k in mc.CLIPPED.items():
        (src,) = oracles[name]
        assert not src["components"][k][2].any() and src["components"][1 - k][2].all()
    (src,) = oracles["negative-centre"]
    sed = src["components"][0][2]
    assert sed[0] == 0 and sed[1] > 0


def test_every_snr_is_clear_of_the_class_threshold(cases):
    """A float64 sum and NumPy's pairwise sum in the data type pick the same class."""
    from scarlet_amd.lite import calculate_snr

    for c in cases.values():
        edge = 2 * c.options["min_snr"]
        for center in c.centers:
            snr = float(calculate_snr(c.obs.images, c.obs.variance, c.obs.psfs, center))
            assert abs(snr - edge) >= 1e-3 * edge and abs(snr - round(snr)) >= 1e-4 or \
                abs(np.floor(snr) - edge) >= 1, (c.name, center, snr)


def test_oracle_reproduces_the_reference(hsc):
    from test_lite_init_host import _hsc_observation

    g = golden("lite_init")
    obs = _hsc_observation(hsc)
    centers = [tuple(int(v) for v in c) for c in g["centers"]]
    sources = mo.of_observation(obs, centers, min_snr=50)
    assert [len(s["components"]) for s in sources] == list(g["n_comp_of"])
    for i, src in enumerate(sources):
        for j, (origin, morph, sed) in enumerate(src["components"]):
            assert tuple(origin[1:]) == tuple(g["origin_%d_%d" % (i, j)]), (i, j)
            ref = g["morph_%d_%d" % (i, j)]
            assert morph.shape == ref.shape and np.abs(morph - ref).max() < 1e-5, (i, j)
            ref = g["sed_%d_%d" % (i, j)]
            assert np.abs(sed - ref).max() <= 2e-3 * np.abs(ref).max(), (i, j)


# ------------------------------------------------------------------ planning
def _dark(frame, dtype=np.float32, C=1):
    """An observation of zeros (planning reads shapes and dtypes only)."""
    psfs = np.ones((C, 3, 3)) / 9
    return init_cases._observation(np.zeros((C,) + frame, dtype), psfs,
                                   np.ones((1, 3, 3)), np.ones((7, 7)))


def test_plan_groups_by_dtypes_and_bands(cases):
    from scarlet_amd import lite

    names = ["9x11-classes", "9x11-f64", "33x37-centre", "moat", "32x36-f64", "32x36-even"]
    group = [cases[n] for n in names]
    groups, fallback = lite.plan_init_blends_main(
        [c.obs for c in group], [c.centers for c in group], [c.detect for c in group])
    f4, f8 = np.dtype("f4"), np.dtype("f8")
    assert fallback == []
    assert list(groups.items()) == [((f4, f4, 2), [0, 3]), ((f8, f8, 2), [1, 4]),
                                    ((f4, f4, 5), [2]), ((f4, f4, 3), [5])]
    groups, fallback = lite.plan_init_blends_main([group[0].obs], [[]])
    assert list(groups.values()) == [[0]] and fallback == []


def _reason(obs, centers=((1, 1),), detect=None, **kw):
    from scarlet_amd import lite

    groups, fallback = lite.plan_init_blends_main([obs], [list(centers)],
                                                  None if detect is None else [detect], **kw)
    assert not groups and len(fallback) == 1 and fallback[0][0] == 0
    return fallback[0][1]


def test_plan_names_every_fallback(cases):
    from scarlet_amd import Box

    case = mc.make_case("moat")
    obs = case.obs
    assert "use_mask" in _reason(obs, use_mask=True)
    for percentile in (0, 100, 150, -5):
        assert "percentile" in _reason(obs, percentile=percentile)
    assert "dtype" in _reason(obs, detect=np.zeros((33, 37), np.float64))
    assert "frame's shape" in _reason(obs, detect=np.zeros((37, 33), np.float32))
    assert "frame's shape" in _reason(obs, detect=np.zeros((1, 33, 37), np.float32))
    other = mc.make_case("moat").obs
    other.noise_rms = other.noise_rms.astype(np.float64)
    assert "noise_rms" in _reason(other)
    assert "detect" not in _reason(other, use_mask=True)
    # ... but a passed detection image of the images' dtype needs no coadd
    from scarlet_amd import lite
    groups, _ = lite.plan_init_blends_main([other], [[(1, 1)]], [np.zeros((33, 37), np.float32)])
    assert list(groups.values()) == [[0]]
    # what init_blends refuses
    other = mc.make_case("moat").obs
    other.diff_kernel = SimpleNamespace(image=np.ones((2, 2, 3), np.float32))
    assert "even" in _reason(other)
    other = mc.make_case("moat").obs
    other.images = other.images.astype(np.float16)
    assert "float32 nor float64" in _reason(other)
    other = mc.make_case("moat").obs
    other.bbox = Box(other.images.shape, origin=(0, 2, 0))
    assert "box" in _reason(other)
    other = mc.make_case("moat").obs
    other.variance = other.variance.astype(np.float64)
    assert "variance" in _reason(other)
    other = mc.make_case("moat").obs
    other.psfs = other.psfs[:, :2]
    other.psfs = other.psfs.astype(np.float64)
    assert "PSFs" in _reason(other)
    other = mc.make_case("moat").obs
    other.diff_kernel = SimpleNamespace(image=np.ones((1, 257, 3), np.float32))
    assert "stamp beyond" in _reason(other)


def test_plan_states_the_lds_limit():
    from scarlet_amd import lite
    from scarlet_amd.lite import initialization as li

    # 160 KiB per CU, 1 KiB of it for the kernel's reductions
    assert li._max_sweep_pixels(np.float32) == (160 * 1024 - 1024) // 4 == 40704
    assert li._max_sweep_pixels(np.float64) == (160 * 1024 - 1024) // 8 == 20352
    for frame, dtype, fits in [((201, 202), np.float32, True), ((202, 202), np.float32, False),
                               ((142, 143), np.float64, True), ((143, 143), np.float64, False)]:
        groups, fallback = lite.plan_init_blends_main([_dark(frame, dtype)], [[(0, 0)]])
        assert bool(groups) == fits, (frame, dtype)
        if not fits:
            reason = fallback[0][1]
            assert str(frame[0] * frame[1]) in reason and "160 KiB" in reason
            assert str(li._max_sweep_pixels(dtype)) in reason and np.dtype(dtype).name in reason


def test_plan_refuses_bad_catalogues(cases):
    from scarlet_amd import lite

    c = cases["9x11-classes"]
    for bad in [(9, 2), (4, 11), (-1, 0), (0, -1)]:
        with pytest.raises(ValueError, match=r"blend 1: centre \(%d, %d\) lies outside its 9 x 11"
                           % bad):
            lite.plan_init_blends_main([c.obs, c.obs], [[(4, 4)], [(4, 4), bad]])
    with pytest.raises(ValueError, match="one entry per blend, got 2, 1 and 2"):
        lite.plan_init_blends_main([c.obs, c.obs], [c.centers])
    with pytest.raises(ValueError, match="one entry per blend, got 1, 1 and 2"):
        lite.plan_init_blends_main([c.obs], [c.centers], [None, None])
    # the same refusals before init_blends_main touches a device
    with pytest.raises(ValueError, match=r"blend 0: centre \(9, 2\)"):
        lite.init_blends_main([c.obs], [[(4, 4), (9, 2)]])


def test_chunks_follow_the_working_set(cases):
    from scarlet_amd import _catalog, lite
    from scarlet_amd.lite import initialization as li

    group = [cases[n] for n in mc.GROUP]
    (key, idx), = lite.plan_init_blends_main(
        [c.obs for c in group], [c.centers for c in group], [c.detect for c in group])[0].items()
    assert idx == [0, 1, 2, 3, 4]
    assert len({c.obs.images.shape[1:] for c in group}) == 3
    items = [(i, li._main_bytes(c.obs, len(c.centers), key)) for i, c in enumerate(group)]
    # detection image, images, variance, four frames per source, stamps, the cosine table
    assert items[0][1] == ((1 + 4 + 4 * 3) * 120 * 4 + 2 * 9 * (4 + 4 + 8) + 64 * 19 * 23)
    middle = items[0][1] + items[1][1]
    assert _catalog.chunks(items, middle) == [[0, 1], [2, 3], [4]]
    assert _catalog.chunks(items, _catalog.WORKING_SET_BYTES) == [[0, 1, 2, 3, 4]]
    assert _catalog.chunks(items, 1) == [[0], [1], [2], [3], [4]]
