"""``lite.init_blends`` on the GPU against the per-blend loop ``init_all_sources_wavelets``
(bit for bit, but for the spectra of joint fits) and against the CPU restatement
tests/init_oracle.py, on the small scenes of tests/init_cases.py; a mixed catalogue; the
reference's run on hsc_cosmos_35; malformed plans at the C entries."""

import ctypes

import numpy as np
import pytest

import init_cases
from conftest import golden

pytestmark = pytest.mark.gpu


def _joint(oracle):
    return [s is not None and s["kind"] == "two" for s in oracle]


@pytest.mark.parametrize("name", list(init_cases.CASES))
def test_case_equals_the_loop_and_the_oracle(name):
    from scarlet_amd import lite

    case = init_cases.make_case(name)
    before = case.wavelets.copy()
    (batch,) = lite.init_blends([case.obs], [case.centers], wavelets=[case.wavelets],
                                **case.options)
    assert init_cases.same_bits(case.wavelets, before)
    loop = init_cases.run_loop(case)
    oracle = init_cases.run_oracle(case)
    kinds = ["none" if s is None else s["kind"] for s in oracle]
    assert kinds == case.kinds
    init_cases.assert_matches_loop(batch, loop, _joint(oracle))
    worst = init_cases.assert_matches_oracle(batch, loop, oracle)
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)


def test_one_group_of_five_blends_in_one_two_and_five_chunks():
    """Five blends of one device group -- three frame shapes, two stamp shapes, three PSF
    sizes, three, two and one source -- in one chunk: every offset past the first blend's is
    in use.  Equal to the loop and the oracle; a budget that cuts the group into chunks of
    two, two and one blend and a budget of one byte give the same bits."""
    from scarlet_amd import _catalog, lite
    from scarlet_amd.lite import initialization as li

    group = [init_cases.make_case(n) for n in init_cases.GROUP]
    observations = [c.obs for c in group]
    centers = [c.centers for c in group]
    wavelets = [c.wavelets for c in group]
    options = group[0].options
    (key, idx), = lite.plan_init_blends(observations, centers, wavelets)[0].items()
    assert idx == [0, 1, 2, 3, 4]
    middle = init_cases.group_budget(group, key)
    items = [(i, li._init_bytes(c.obs, len(c.centers), 4, key)) for i, c in enumerate(group)]
    assert _catalog.chunks(items, middle) == [[0, 1], [2, 3], [4]]
    assert _catalog.chunks(items, _catalog.WORKING_SET_BYTES) == [[0, 1, 2, 3, 4]]

    batch = lite.init_blends(observations, centers, wavelets=wavelets, **options)
    worst = 0.0
    for i, case in enumerate(group):
        loop = init_cases.run_loop(case)
        oracle = init_cases.run_oracle(case)
        assert ["none" if s is None else s["kind"] for s in oracle] == case.kinds
        init_cases.assert_matches_loop(batch[i], loop, _joint(oracle))
        worst = max(worst, init_cases.assert_matches_oracle(batch[i], loop, oracle))
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)
    for budget in (middle, 1):
        chunked = lite.init_blends(observations, centers, wavelets=wavelets,
                                   _working_set_bytes=budget, **options)
        for i, case in enumerate(group):  # the spectra of joint fits included
            init_cases.assert_matches_loop(chunked[i], batch[i], [False] * len(case.centers))
    # the blends in another order: other offsets, the same sources
    order = [3, 1, 4, 0, 2]
    shuffled = lite.init_blends([observations[i] for i in order], [centers[i] for i in order],
                                wavelets=[wavelets[i] for i in order], **options)
    for at, i in enumerate(order):
        init_cases.assert_matches_loop(shuffled[at], batch[i], [False] * len(centers[i]))


def test_mixed_catalogue():
    """Seven device blends of five frame shapes, float32 and float64 -- one of them without
    centres -- and one whose variance is float64 next to float32 images, which takes the
    loop; wavelets as None, host arrays and device tensors; one chunk per group and one
    chunk per blend give the same bits; passed wavelets stay as they were.  (Chunks of
    several blends: test_one_group_of_five_blends_in_one_two_and_five_chunks.)"""
    import torch

    from scarlet_amd import detect, lite

    options = init_cases.MIXED_OPTIONS
    cases = [init_cases.make_case(n) for n in init_cases.MIXED]
    cases += [init_cases.make_blob("blob32"), init_cases.make_blob("blob64")]
    other = init_cases.make_case("flat-top")
    other.obs.variance = other.obs.variance.astype(np.float64)
    cases += [other, init_cases.make_case("serpentine")]  # (15 x 15: the fifth frame shape)
    observations = [c.obs for c in cases]
    centers = [c.centers for c in cases]
    centers[7] = []
    blob64 = cases[5].obs
    d_blob64 = detect.get_detect_wavelets(blob64.images, blob64.variance, scales=5, device=True)
    wavelets = [c.wavelets for c in cases]
    wavelets[1] = torch.from_numpy(cases[1].wavelets).to("cuda")
    wavelets[5] = d_blob64
    kept = [None if w is None else (w.clone() if torch.is_tensor(w) else w.copy())
            for w in wavelets]

    groups, fallback = lite.plan_init_blends(observations, centers, wavelets)
    assert [i for i, _ in fallback] == [6] and "variance" in fallback[0][1]
    assert sorted(i for idx in groups.values() for i in idx) == [0, 1, 2, 3, 4, 5, 7]
    assert len(groups) == 6  # the four cases differ in dtype or bands; blob32, blob64
    assert len({o.images.shape[1:] for o in observations}) == 5

    batch = lite.init_blends(observations, centers, wavelets=wavelets, **options)
    chunked = lite.init_blends(observations, centers, wavelets=wavelets, _working_set_bytes=1,
                               **options)
    for w, k in zip(wavelets, kept):
        if w is not None:
            assert torch.equal(w, k) if torch.is_tensor(w) else init_cases.same_bits(w, k)
    assert len(batch) == len(observations) and batch[7] == [] and chunked[7] == []
    host = [w.cpu().numpy() if torch.is_tensor(w) else w for w in wavelets]
    host[4] = detect.get_detect_wavelets(cases[4].obs.images, cases[4].obs.variance, scales=5)
    worst = 0.0
    for i in range(7):
        loop = lite.init_all_sources_wavelets(observations[i], centers[i],
                                              wavelets=host[i].copy(), **options)
        oracle = init_cases.run_oracle(cases[i], options, host[i])
        init_cases.assert_matches_loop(batch[i], loop, _joint(oracle))
        worst = max(worst, init_cases.assert_matches_oracle(batch[i], loop, oracle))
        # chunking changes nothing, the spectra of joint fits included
        init_cases.assert_matches_loop(chunked[i], batch[i], [False] * len(centers[i]))
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)


def test_even_stamp_is_planned_for_the_loop():
    from types import SimpleNamespace

    from scarlet_amd import lite

    case = init_cases.make_case("flat-top")
    case.obs.diff_kernel = SimpleNamespace(image=np.ones((2, 2, 3), np.float32))
    groups, fallback = lite.plan_init_blends([case.obs], [case.centers], [case.wavelets])
    assert not groups and fallback[0][0] == 0 and "even" in fallback[0][1]


def test_even_stamp_takes_the_loop():
    """The fallback is the loop itself: what it raises for an even stamp, init_blends raises."""
    from types import SimpleNamespace

    from scarlet_amd import lite

    case = init_cases.make_case("flat-top")
    case.obs.diff_kernel = SimpleNamespace(image=np.ones((2, 2, 3), np.float32))
    with pytest.raises(ValueError, match="odd height and width"):
        init_cases.run_loop(case)
    with pytest.raises(ValueError, match="odd height and width"):
        lite.init_blends([case.obs], [case.centers], wavelets=[case.wavelets], **case.options)


def test_centre_outside_the_frame_is_refused_before_any_device_work():
    from scarlet_amd import lite

    case = init_cases.make_case("9x11-classes")
    with pytest.raises(ValueError, match=r"blend 0: centre \(9, 2\)"):
        lite.init_blends([case.obs], [[(4, 4), (9, 2)]], wavelets=[case.wavelets])


def test_golden_scene_and_a_fit_started_from_it(hsc):
    from scarlet_amd import lite
    from test_gpu_lite_wavelets import _observation

    g = golden("detect")
    obs = _observation(hsc)
    centers = [tuple(int(v) for v in c) for c in g["init_centers"]]
    (sources,) = lite.init_blends([obs], [centers], min_snr=50)
    assert [len(s.components) for s in sources] == list(g["init_n_comp_of"])
    for i, src in enumerate(sources):
        for j, c in enumerate(src.components):
            assert tuple(c.bbox.origin) + tuple(c.bbox.shape) == \
                tuple(g["init_box_%d_%d" % (i, j)]), (i, j)
            ref = g["init_morph_%d_%d" % (i, j)]
            assert c.morph.shape == ref.shape
            assert np.abs(c.morph - ref).max() < 1e-5, (i, j)
            ref = g["init_sed_%d_%d" % (i, j)]
            assert np.abs(c.sed - ref).max() <= 1e-5 * np.abs(ref).max(), (i, j)
    blend = lite.LiteBlend(lite.parameterize_sources(sources, obs, lite.init_adaprox_component),
                           obs)
    lite.fit_blends([blend], 5, e_rel=1e-9, reweight=False)
    assert len(blend.loss) >= 2 and np.all(np.isfinite(blend.loss))


# ------------------------------------------------------------------ malformed plans
@pytest.mark.parametrize("step,field,value,message", [
    ("coadd", "first", (0, 3, 0), "plane selection outside the tensor"),
    ("coadd", "wavelet_off", 1, "wavelets outside their buffer"),
    ("coadd", "n_pix", -99, "frame extent"),
    ("snr", "image_off", 1, "frame outside the image buffer"),
    ("snr", "cy", 9, "centre outside its frame"),
    ("snr", "psf_off", -1, "PSF outside its buffer"),
    ("taps", "cy", 9, "centre outside its frame"),
    ("taps", "plane_off", 1 << 40, "plane outside its buffer"),
    ("taps", "kh", 4, "odd height and width"),
    ("masks", "cx", -1, "centre outside its frame"),
    ("masks", "h", -3, "plane extent"),
    ("masks", "valid_off", 50, "valid map outside its buffer"),
    ("crop", "bh", -1, "box extent"),
    ("crop", "out_off", 1 << 33, "morphology outside the output buffer"),
    ("fit", "a_y0", -7, "leaves the union box"),
    ("fit", "b_w", 22, "leaves the union box"),
    ("fit", "b_off", 512, "morphology outside its buffer"),
    ("fit", "stamp_off", 1, "stamp outside its buffer"),
])
def test_malformed_plan_is_refused_before_any_launch(step, field, value, message):
    """A bad descriptor returns SMI_ERR_INVALID; the output buffers keep their fill.  (The
    same tables with the field left alone are what the other tests launch.)"""
    import torch

    from scarlet_amd import _lib
    from scarlet_amd.lite import initialization as li

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    plane = torch.ones(4 * 9 * 11, dtype=torch.float64, device=dev)  # 4 planes, or 2 bands x 2
    stamps = torch.ones(2 * 9, dtype=torch.float64, device=dev)
    out = torch.full((1024,), -7.0, dtype=torch.float64, device=dev)
    valid = torch.full((99,), 9, dtype=torch.uint8, device=dev)
    visited = torch.zeros(99, dtype=torch.int32, device=dev)
    flags = [torch.zeros(99, dtype=torch.uint8, device=dev) for _ in range(2)]
    bounds = torch.full((4,), -7, dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = {
        "coadd": (li._COADD_DESC, (4, (0, 0, 2), (3, 2, 1), (1, 1, 1), (0, 0), 99, 0, 0)),
        "snr": (li._SNR_DESC, (9, 11, 4, 5, 3, 3, 0, 0)),
        "taps": (li._TAPS_DESC, (9, 11, 4, 5, 3, 3, 0, 0, 0)),
        "masks": (li._MASK_DESC, (9, 11, 4, 5, 0, 0, 0)),
        "crop": (li._CROP_DESC, (9, 11, -6, -5, 21, 21, 0, 0, 0)),
        "fit": (li._FIT_DESC, (9, 11, -6, -5, 21, 21, -6, -5, 21, 21, -6, -5, 21, 21, 3, 3,
                               0, 0, 0, 441)),
    }
    table = np.zeros(1, good[step][0])
    table[0] = good[step][1]
    table[field] = value
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    head = [1, table.ctypes.data, d_table.data_ptr()]
    if step == "coadd":
        status = lib.smi_lite_init_coadd_f64(*head, vp(plane), 396, vp(out), 297, None)
    elif step == "snr":
        status = lib.smi_lite_init_snr_f64(2, *head, vp(plane), vp(plane), 198, vp(stamps), 18,
                                           vp(out), 2, None)
    elif step == "taps":
        status = lib.smi_lite_init_taps_f64(2, *head, vp(plane), 99, vp(stamps), 18, vp(out), 512,
                                            None)
    elif step == "masks":
        status = lib.smi_lite_init_masks_f64(*head, vp(plane), 99, vp(visited), vp(flags[0]),
                                             vp(flags[1]), 99, vp(valid), 99, vp(bounds), vp(out),
                                             1, None)
    elif step == "crop":
        status = lib.smi_lite_init_crop_f64(*head, vp(plane), 99, vp(valid), 99, vp(out), 512,
                                            None)
    else:
        status = lib.smi_lite_init_fit_f64(2, *head, vp(out), 882, vp(plane), 1, 198, vp(stamps),
                                           18, vp(out[900:]), 10, None)
    torch.cuda.synchronize()
    assert status < 0
    with pytest.raises(_lib.ScarletAmdError, match=message):
        _lib.check(status)
    assert bool((out == -7).all()) and bool((valid == 9).all()) and bool((bounds == -7).all())
