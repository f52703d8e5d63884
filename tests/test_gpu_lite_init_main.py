"""``lite.init_blends_main`` on the GPU against the per-blend loop ``init_all_sources_main``
(bit for bit, but for the spectra of joint fits) and against the CPU restatement
tests/init_main_oracle.py, on the small scenes of tests/init_main_cases.py; one group in
several chunkings; a mixed catalogue; the reference's run on hsc_cosmos_35; malformed task
tables at the new C entries."""

import ctypes

import numpy as np
import pytest

import init_cases
import init_main_cases as mc
from conftest import golden

pytestmark = pytest.mark.gpu


def _joint(oracle):
    return [s["kind"] == "two" for s in oracle]


def _check(batch, case, loop=None):
    """``batch`` against the loop and the oracle of ``case``; the largest ratio of the joint
    spectra's rule."""
    loop = mc.run_loop(case) if loop is None else loop
    oracle = mc.run_oracle(case)
    assert [s["kind"] for s in oracle] == case.kinds
    init_cases.assert_matches_loop(batch, loop, _joint(oracle))
    return init_cases.assert_matches_oracle(batch, loop, oracle)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_equals_the_loop_and_the_oracle(name):
    case = mc.make_case(name)
    before = None if case.detect is None else case.detect.copy()
    (batch,) = mc.run_batch([case])
    if before is not None:
        assert init_cases.same_bits(case.detect, before)
    worst = _check(batch, case)
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)
    if name in mc.CLIPPED:
        assert not batch[0].components[mc.CLIPPED[name]].sed.any()


@pytest.mark.parametrize("name", list(mc.LARGE))
def test_large_frame_equals_the_loop(name):
    """More LDS than a kernel gets by default, levels wider than the workgroup."""
    case = mc.LARGE[name]()
    (batch,) = mc.run_batch([case])
    loop = mc.run_loop(case)
    assert [len(s.components) for s in loop] == [1] * len(case.centers)
    boxes = [s.components[0].bbox.shape[1] for s in batch]
    print("boxes:", boxes)
    assert max(boxes) > 100
    init_cases.assert_matches_loop(batch, loop, [False] * len(case.centers))


def test_one_group_of_five_blends_in_one_three_and_five_chunks():
    """Five blends of one device group -- three frame shapes, two stamp shapes, three PSF
    sizes, one to four sources, a passed detection image -- in one chunk: every offset past
    the first blend's is in use.  Equal to the loop and the oracle; a budget that cuts the
    group into chunks of two, two and one blend, a budget of one byte and another order of the
    blends give the same bits, the spectra of joint fits included."""
    from scarlet_amd import _catalog, lite
    from scarlet_amd.lite import initialization as li

    group = [mc.make_case(n) for n in mc.GROUP]
    observations = [c.obs for c in group]
    centers = [c.centers for c in group]
    detect = [c.detect for c in group]
    (key, idx), = lite.plan_init_blends_main(observations, centers, detect)[0].items()
    assert idx == [0, 1, 2, 3, 4] and len({o.images.shape[1:] for o in observations}) == 3
    items = [(i, li._main_bytes(c.obs, len(c.centers), key)) for i, c in enumerate(group)]
    middle = items[0][1] + items[1][1]
    assert _catalog.chunks(items, middle) == [[0, 1], [2, 3], [4]]

    batch = mc.run_batch(group)
    assert _catalog.Launcher.last.launches == ["main_coadd", "snr", "taps", "taps", "main_sweep",
                                               "crop", "main_split", "fit"]
    worst = max(_check(batch[i], case) for i, case in enumerate(group))
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)
    for budget in (middle, 1):
        chunked = mc.run_batch(group, _working_set_bytes=budget)
        for i, case in enumerate(group):
            init_cases.assert_matches_loop(chunked[i], batch[i], [False] * len(case.centers))
    order = [3, 1, 4, 0, 2]
    shuffled = mc.run_batch([group[i] for i in order])
    for at, i in enumerate(order):
        init_cases.assert_matches_loop(shuffled[at], batch[i], [False] * len(centers[i]))


def test_mixed_catalogue():
    """Float32 and float64 groups of two, three and five bands, a blend without centres, a
    blend whose detection image is float64 next to float32 images, which takes the loop, and
    passed detection images, which come back unchanged; one chunk per group and one chunk per
    blend give the same bits."""
    from scarlet_amd import lite

    names = ["9x11-classes", "32x36-f64", "passed-detect", "33x37-centre", "9x11-f64",
             "32x36-even", "negative-centre", "moat"]
    cases = [mc.make_case(n) for n in names]
    observations = [c.obs for c in cases]
    centers = [c.centers for c in cases]
    centers[7] = []
    detect = [c.detect for c in cases]
    detect[6] = detect[6].astype(np.float64)
    kept = [None if d is None else d.copy() for d in detect]
    options = dict(min_snr=mc.MIN_SNR)

    groups, fallback = lite.plan_init_blends_main(observations, centers, detect)
    assert [i for i, _ in fallback] == [6] and "dtype" in fallback[0][1]
    f4, f8 = np.dtype("f4"), np.dtype("f8")
    assert groups == {(f4, f4, 2): [0, 2, 7], (f8, f8, 2): [1, 4], (f4, f4, 5): [3],
                      (f4, f4, 3): [5]}

    batch = lite.init_blends_main(observations, centers, detect=detect, **options)
    chunked = lite.init_blends_main(observations, centers, detect=detect, _working_set_bytes=1,
                                    **options)
    for d, k in zip(detect, kept):
        assert d is None or init_cases.same_bits(d, k)
    assert len(batch) == 8 and batch[7] == [] and chunked[7] == []
    worst = 0.0
    for i in range(6):
        worst = max(worst, _check(batch[i], cases[i]))
        init_cases.assert_matches_loop(chunked[i], batch[i], [False] * len(centers[i]))
    print("largest |batch - oracle| / max(|loop - oracle|, floor):", worst)
    # the fallback is the loop itself
    loop = lite.init_all_sources_main(observations[6], centers[6], detect=detect[6], **options)
    init_cases.assert_matches_loop(batch[6], loop, [False])
    init_cases.assert_matches_loop(chunked[6], loop, [False])


def test_use_mask_takes_the_loop():
    from scarlet_amd import lite

    case = mc.make_case("moat")
    (batch,) = lite.init_blends_main([case.obs], [case.centers], use_mask=True, **case.options)
    loop = lite.init_all_sources_main(case.obs, case.centers, use_mask=True, **case.options)
    init_cases.assert_matches_loop(batch, loop, [False])


def test_golden_scene_and_a_fit_started_from_it(hsc):
    from scarlet_amd import lite
    from test_lite_init_host import _hsc_observation

    g = golden("lite_init")
    obs = _hsc_observation(hsc)
    centers = [tuple(int(v) for v in c) for c in g["centers"]]
    (sources,) = lite.init_blends_main([obs], [centers], min_snr=50)
    assert [len(s.components) for s in sources] == list(g["n_comp_of"])
    for i, src in enumerate(sources):
        for j, c in enumerate(src.components):
            assert tuple(c.bbox.origin[1:]) == tuple(g["origin_%d_%d" % (i, j)]), (i, j)
            ref = g["morph_%d_%d" % (i, j)]
            assert c.morph.shape == ref.shape and np.abs(c.morph - ref).max() < 1e-5, (i, j)
            ref = g["sed_%d_%d" % (i, j)]
            assert np.abs(c.sed - ref).max() <= 2e-3 * np.abs(ref).max(), (i, j)
    blend = lite.LiteBlend(lite.parameterize_sources(sources, obs, lite.init_adaprox_component),
                           obs)
    lite.fit_blends([blend], 5, e_rel=1e-9, reweight=False)
    print("losses:", blend.loss)
    assert len(blend.loss) >= 2 and np.all(np.isfinite(blend.loss))


# ------------------------------------------------------------------ malformed task tables
@pytest.mark.parametrize("step,field,value,message", [
    ("main_coadd", "image_off", 1, "frame outside the image buffer"),
    ("main_coadd", "nr2_off", 1, "noise levels outside their buffer"),
    ("main_coadd", "detect_off", -1, "detection image outside its buffer"),
    ("main_coadd", "n_pix", -99, "frame extent"),
    ("main_coadd", "bands", 0, "bands"),
    ("main_sweep", "plane_off", 1, "plane outside its buffer"),
    ("main_sweep", "out_off", 1 << 40, "swept plane outside the output buffer"),
    ("main_sweep", "cy", 9, "centre outside its frame"),
    ("main_sweep", "cx", -1, "centre outside its frame"),
    ("main_sweep", "h", -3, "plane extent"),
    ("main_sweep", "w", 2314, "frame beyond the LDS image"),  # 9 x 2314 = 20826 > 20352
    ("main_sweep", "w", 12, "frame beyond the cosine table"),
    ("main_split", "bh", -1, "box extent"),
    ("main_split", "morph_off", 1 << 33, "morphology outside its buffer"),
    ("main_split", "bulge_off", 440, "shared with another morphology"),
    ("main_split", "disk_off", 883, "shared with another morphology"),
])
def test_malformed_table_is_refused_before_any_launch(step, field, value, message):
    """A bad descriptor returns SMI_ERR_INVALID; the output buffers keep their fill.  (The
    same tables with the field left alone are what the other tests launch.)"""
    import torch

    from scarlet_amd import _lib
    from scarlet_amd.lite import initialization as li

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    plane = torch.ones(2 * 9 * 11, dtype=torch.float64, device=dev)  # two bands, or a plane
    nr2 = torch.ones(2, dtype=torch.float64, device=dev)
    cosines = torch.ones(17 * 21 * 8, dtype=torch.float64, device=dev)
    out = torch.full((3 * 441,), -7.0, dtype=torch.float64, device=dev)
    bounds = torch.full((4,), -7, dtype=torch.int32, device=dev)
    peaks = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = {
        "main_coadd": (li._MAIN_COADD_DESC, (2, 0, 99, 0, 0, 0)),
        "main_sweep": (li._MAIN_SWEEP_DESC, (9, 11, 4, 5, 0, 0, 0.5)),
        "main_split": (li._MAIN_SPLIT_DESC, (21, 21, 0, 441, 882)),
    }
    table = np.zeros(1, good[step][0])
    table[0] = good[step][1]
    table[field] = value
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    head = [1, table.ctypes.data, d_table.data_ptr()]
    if step == "main_coadd":
        status = lib.smi_lite_init_main_coadd_f64(*head, vp(plane), 198, vp(nr2), 2, vp(out), 99,
                                                  None)
    elif step == "main_sweep":
        status = lib.smi_lite_init_main_sweep_f64(*head, vp(plane), 99, vp(cosines), 17 * 21 * 8,
                                                  8, 10, vp(out), 99, vp(bounds), vp(peaks), 1,
                                                  None)
    else:
        status = lib.smi_lite_init_main_split_f64(*head, vp(out), 3 * 441, 0.25, None)
    torch.cuda.synchronize()
    assert status < 0
    with pytest.raises(_lib.ScarletAmdError, match=message):
        _lib.check(status)
    assert bool((out == -7).all()) and bool((bounds == -7).all()) and bool((peaks == -7).all())


def test_cosine_table_of_the_wrong_size_is_refused():
    import torch

    from scarlet_amd import _lib
    from scarlet_amd.lite import initialization as li

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    plane = torch.ones(99, dtype=torch.float32, device=dev)
    cosines = torch.ones(17 * 21 * 8, dtype=torch.float64, device=dev)
    out = torch.full((99,), -7.0, dtype=torch.float32, device=dev)
    bounds = torch.full((4,), -7, dtype=torch.int32, device=dev)
    peaks = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    table = np.zeros(1, li._MAIN_SWEEP_DESC)
    table[0] = (9, 11, 4, 5, 0, 0, 0.5)
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    status = lib.smi_lite_init_main_sweep_f32(1, table.ctypes.data, d_table.data_ptr(), vp(plane),
                                              99, vp(cosines), 17 * 21 * 8, 8, 11, vp(out), 99,
                                              vp(bounds), vp(peaks), 1, None)
    torch.cuda.synchronize()
    with pytest.raises(_lib.ScarletAmdError, match="cosine table"):
        _lib.check(status)
    assert bool((out == -7).all())
