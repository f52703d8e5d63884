"""``lite.init_blends`` without a GPU: the CPU restatement tests/init_oracle.py against the
reference's run on hsc_cosmos_35 (tests/golden/detect.npz), the planning of the device
batches, and the two conditions on the cases of tests/init_cases.py that the GPU tests rely
on."""

from types import SimpleNamespace

import numpy as np
import pytest

import init_cases
import init_oracle
import wavelet_oracle as wo
from conftest import golden


def _hsc_observation(hsc):
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images = hsc["images"].astype(np.float32)
    weights = hsc["weights"].astype(np.float32)
    variance = (1 / weights).astype(np.float32)
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    return lite.LiteObservation(images, variance, weights, hsc["psfs"].astype(np.float32),
                                model_psf=model_psf[0][None])


def test_oracle_reproduces_the_reference(hsc):
    from scarlet_amd import wavelet

    g = golden("detect")
    obs = _hsc_observation(hsc)
    detect = wo.coadd(obs.images)
    w = wo.transform(detect, wavelet.get_scales(detect.shape, 5))
    wavelets = wo.support(detect.dtype, w, np.median(np.sqrt(obs.variance)))[0] * w
    centers = [tuple(int(v) for v in c) for c in g["init_centers"]]
    sources = init_oracle.of_observation(obs, centers, wavelets, min_snr=50)
    assert [len(s["components"]) for s in sources] == list(g["init_n_comp_of"])
    for i, src in enumerate(sources):
        for j, (origin, morph, sed) in enumerate(src["components"]):
            assert tuple(origin) + (len(sed),) + morph.shape == tuple(g["init_box_%d_%d" % (i, j)])
            ref = g["init_morph_%d_%d" % (i, j)]
            assert morph.shape == ref.shape and np.abs(morph - ref).max() < 1e-5, (i, j)
            ref = g["init_sed_%d_%d" % (i, j)]
            assert np.abs(sed - ref).max() <= 1e-5 * np.abs(ref).max(), (i, j)


# ------------------------------------------------------------------ the cases
@pytest.fixture(scope="module")
def cases():
    return {name: init_cases.make_case(name) for name in init_cases.CASES}


@pytest.fixture(scope="module")
def oracles(cases):
    return {name: init_cases.run_oracle(c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def configurations():
    return [(label, case, options, init_cases.run_oracle(case, options, wavelets))
            for label, case, options, wavelets in init_cases.configurations()]


def test_every_snr_is_clear_of_the_class_thresholds(configurations):
    """A float64 sum and NumPy's float32 pairwise sum pick the same class: every centre's
    calculate_snr, in every configuration a GPU test runs, is at least 1e-3 (relative) away
    from min_snr and 2 min_snr, and -- the class is taken from floor(snr) -- from the integers
    min_snr and 2 min_snr step over."""
    from scarlet_amd.lite import calculate_snr

    seen = 0
    for label, c, options, _ in configurations:
        min_snr = options["min_snr"]
        for center in c.centers:
            snr = float(calculate_snr(c.obs.images, c.obs.variance, c.obs.psfs, center))
            seen += 1
            for edge in (min_snr, 2 * min_snr):
                assert abs(snr - edge) >= 1e-3 * edge, (label, center, snr)
    assert seen >= 30


def test_every_joint_fit_is_well_conditioned(configurations):
    seen = 0
    for label, _, _, sources in configurations:
        for s in sources:
            if s is not None and s["kind"] == "two":
                seen += 1
                assert s["cond"] <= 1e3, (label, s["cond"])
    assert seen >= 12


def test_blob_scenes_hold_joint_fits_and_single_components(configurations):
    kinds = {label: ["none" if s is None else s["kind"] for s in sources]
             for label, _, _, sources in configurations if label.startswith("blob")}
    for label, k in kinds.items():
        assert "two" in k, (label, k)


def test_cases_take_the_classes_they_are_named_for(cases, oracles):
    for name, c in cases.items():
        kinds = ["none" if s is None else s["kind"] for s in oracles[name]]
        assert kinds == c.kinds, name
        for s in oracles[name]:
            if s is not None and s["kind"] == "two":
                assert s["kept"] == init_cases.KEPT.get(name, (True, True)), name
    # the mask of one kept pixel, and the boxes of bulge and disk that differ
    (_, morph, _), = oracles["spike"][0]["components"]
    assert np.count_nonzero(morph) == 1 and morph[10, 10] == 1
    two = oracles["33x37-boxes"][1]["components"]
    assert two[0][1].shape != two[1][1].shape
    # the flat top: the seed moved to the first of the equal pixels, its equals are left out
    (_, morph, _), = oracles["flat-top-one"][0]["components"]
    half = morph.shape[0] // 2
    assert morph[half - 1, half - 1] == 1 and morph[half, half] == 0
    # the moat stops the fill: nothing beyond Chebyshev distance 3
    (_, morph, _), = oracles["moat-one"][0]["components"]
    y, x = np.nonzero(morph)
    assert max(np.abs(y - 10).max(), np.abs(x - 10).max()) == 3
    # the spiral is followed to its end
    (_, morph, _), = oracles["serpentine"][0]["components"]
    assert np.count_nonzero(morph) == len(init_cases.spiral(15)) > 90


# ------------------------------------------------------------------ planning
def test_plan_groups_and_fallback_reasons(cases):
    from scarlet_amd import lite

    names = ["9x11-classes", "33x37-boxes", "9x11-f64", "33x37-f32-wavelets", "flat-top"]
    obs = [cases[n].obs for n in names]
    centers = [cases[n].centers for n in names]
    wavelets = [cases[n].wavelets for n in names]
    wavelets[4] = None
    groups, fallback = lite.plan_init_blends(obs, centers, wavelets)
    f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
    assert groups == {(f64, f32, f32, 2): [0, 4], (f64, f32, f32, 5): [1],
                      (f64, f64, f64, 2): [2], (f32, f32, f32, 2): [3]}
    assert list(groups) == [(f64, f32, f32, 2), (f64, f32, f32, 5), (f64, f64, f64, 2),
                            (f32, f32, f32, 2)]
    assert fallback == []

    def variant(**changes):
        c = init_cases.make_case("9x11-classes")
        for k, v in changes.items():
            setattr(c.obs, k, v)
        return c.obs

    base = cases["9x11-classes"]
    even = variant(diff_kernel=SimpleNamespace(image=np.ones((2, 4, 3), np.float32)))
    half = variant(images=base.obs.images.astype(np.float16))
    flat = variant(images=base.obs.images[0])
    wide = variant(diff_kernel=SimpleNamespace(image=np.ones((2, 257, 3), np.float32)))
    groups, fallback = lite.plan_init_blends([even, base.obs, half, flat, wide],
                                             [base.centers] * 5, [base.wavelets] * 5)
    assert groups == {(f64, f32, f32, 2): [1]}
    assert [i for i, _ in fallback] == [0, 2, 3, 4]
    reasons = dict(fallback)
    assert "even" in reasons[0] and "float32 nor float64" in reasons[2]
    assert "ndim" in reasons[3] and "limits" in reasons[4]
    groups, fallback = lite.plan_init_blends([base.obs], [base.centers],
                                             [base.wavelets.astype(np.float16)])
    assert not groups and "wavelets" in fallback[0][1]


def test_plan_refuses_a_centre_outside_the_frame(cases):
    from scarlet_amd import lite

    c = cases["9x11-classes"]
    for bad in ((9, 0), (0, 11), (-1, 3), (3, -1)):
        with pytest.raises(ValueError, match=r"blend 1: centre \(%d, %d\)" % bad):
            lite.plan_init_blends([c.obs, c.obs], [c.centers, [(1, 1), bad]])
    with pytest.raises(ValueError, match="one entry per blend"):
        lite.plan_init_blends([c.obs], [c.centers, c.centers])


def test_the_group_of_the_gpu_test_is_one_group(cases):
    """The cases the GPU test batches together share one device group, and the budgets it
    uses cut them into one, several multi-blend and one-blend chunks."""
    from scarlet_amd import _catalog
    from scarlet_amd import lite
    from scarlet_amd.lite import initialization as li

    group = [cases[n] for n in init_cases.GROUP]
    assert all(c.options == group[0].options for c in group)
    groups, fallback = lite.plan_init_blends([c.obs for c in group], [c.centers for c in group],
                                             [c.wavelets for c in group])
    (key, idx), = groups.items()
    assert idx == [0, 1, 2, 3, 4] and fallback == []
    assert len({c.obs.images.shape for c in group}) == 3
    assert len({c.obs.diff_kernel.image.shape for c in group}) == 2
    assert len({c.obs.psfs.shape for c in group}) == 3
    assert len({len(c.centers) for c in group}) == 3
    items = [(i, li._init_bytes(c.obs, len(c.centers), 4, key)) for i, c in enumerate(group)]
    middle = init_cases.group_budget(group, key)
    assert _catalog.chunks(items, middle) == [[0, 1], [2, 3], [4]]


def test_plan_of_an_empty_catalogue_and_of_a_blend_without_centres(cases):
    from scarlet_amd import lite

    assert lite.plan_init_blends([], []) == ({}, [])
    assert lite.init_blends([], []) == []
    c = cases["9x11-classes"]
    groups, fallback = lite.plan_init_blends([c.obs], [[]])
    assert list(groups.values()) == [[0]] and fallback == []
    assert lite.init_blends([c.obs], [[]]) == [[]]  # (no device work for it)


def test_chunks_follow_the_budget():
    from scarlet_amd import _catalog
    from scarlet_amd.lite import initialization as li

    key = (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float32), 2)
    obs = SimpleNamespace(images=np.zeros((2, 10, 10), np.float32),
                          diff_kernel=SimpleNamespace(image=np.zeros((1, 7, 5), np.float32)))
    need = li._init_bytes(obs, 3, 6, key)
    assert need == ((6 + 3) * 100 * 8 + 2 * 2 * 100 * 4 + 2 * 7 * 5 * (8 + 8)
                    + 3 * 3 * 7 * 100)
    assert li._n_planes(obs, np.zeros((4, 10, 10)), 5) == 4
    assert li._n_planes(obs, None, 2) == 3  # what get_detect_wavelets makes
    items = [(i, need) for i in range(5)]
    assert _catalog.chunks(items, 2 * need) == [[0, 1], [2, 3], [4]]
    assert _catalog.chunks(items, 1) == [[0], [1], [2], [3], [4]]
    assert _catalog.chunks(items, 1 << 40) == [[0, 1, 2, 3, 4]]
    assert _catalog.chunks([], 1) == []


def test_descriptor_layouts_and_offsets():
    """The records are the C structs of include/scarlet_amd.h, and packed buffers follow
    each other without gaps."""
    from scarlet_amd import _catalog
    from scarlet_amd.lite import initialization as li

    sizes = {li._COADD_DESC: 72, li._SNR_DESC: 40, li._TAPS_DESC: 48, li._MASK_DESC: 40,
             li._CROP_DESC: 48, li._FIT_DESC: 96}
    for desc, size in sizes.items():
        assert desc.itemsize == size
    assert li._COADD_DESC.fields["n_pix"][1] == 48 and li._FIT_DESC.fields["image_off"][1] == 64
    off, total = _catalog.offsets([6, 0, 10])
    assert list(off) == [0, 6, 6] and total == 16
    assert li._plane_selection(slice(None, -1), 4) == (0, 3, 1)
    assert li._plane_selection(slice(2, -1), 4) == (2, 1, 1)
    assert li._plane_selection(slice(2, -1), 3)[1] == 0
    assert li._plane_selection(slice(None, None, -1), 3) == (2, 3, -1)


def test_boxes_follow_the_loop():
    """_monotonic_box is init_monotonic_morph's box arithmetic: bounds -> grown box -> the
    standard odd box around the centre."""
    from scarlet_amd import Box
    from scarlet_amd.lite import initialization as li

    assert li._monotonic_box(np.array([4, 4, 5, 5], np.int32), 0.0, (4, 5), 5) is None
    assert li._monotonic_box(np.array([4, 4, 5, 5], np.int32), 0.7, (4, 5), 5) == \
        Box((21, 21), origin=(-6, -5))
    # 13 rows below the centre, grown by 5: size 2 * 19 -> 41
    assert li._monotonic_box(np.array([10, 23, 8, 12], np.int32), 1.0, (10, 10), 5) == \
        Box((41, 41), origin=(-10, -10))
    # a box that misses the centre (grow 0): the smallest box
    assert li._monotonic_box(np.array([11, 12, 11, 12], np.int32), 1.0, (10, 10), 0) == \
        Box((21, 21), origin=(0, 0))


def test_normal_equations_give_the_minimum_norm_solution():
    from scarlet_amd.lite import initialization as li

    rng = np.random.RandomState(3)
    a, b, img = rng.rand(50), rng.rand(50), rng.rand(50)

    def sums(a, b):
        return np.array([a @ a, a @ b, b @ b, a @ img, b @ img])

    packed = np.array([[sums(a, b), sums(a, a)], [sums(a, 0 * b), sums(-a, b)]])
    got = li._solve_pairs(packed, np.float64)
    assert got.shape == (2, 2, 2)
    for n, c, (u, v) in ((0, 0, (a, b)), (0, 1, (a, a)), (1, 0, (a, 0 * b)), (1, 1, (-a, b))):
        want = np.linalg.lstsq(np.stack([u, v], axis=1), img, rcond=None)[0]
        want[want < 0] = 0
        assert np.allclose(got[n, :, c], want, rtol=1e-9, atol=1e-12), (n, c)
    assert li._solve_pairs(np.zeros((0, 3, 5)), np.float32).shape == (0, 2, 3)
