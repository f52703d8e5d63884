"""initialization.init_blends on the GPU against the loop of init_all_sources: the catalogue of
tests/init_blends_cases.py under three option sets, the scenes the reference initialised itself,
invariance to list, order and chunking, and the validation of every kernel entry."""

import ctypes

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import init_blends_cases as ic

pytestmark = pytest.mark.gpu


def _columns(cat):
    return [c[1] for c in cat], [c[2] for c in cat], [c[3] for c in cat]


def _spectra(result):
    import scarlet_amd as scarlet

    out = []
    for s in result[0]:
        for c in (s.children if isinstance(s, scarlet.CombinedComponent) else [s]):
            out.append(np.array(c.children[0].parameters[0]))
    return out


@pytest.fixture(scope="module")
def runs():
    """Per option set and ``set_spectra``: (catalogue, init_blends of it, the loop's results on a
    second, equal catalogue), computed once and only read by the tests."""
    from scarlet_amd import initialization as init

    cache = {}

    def get(name, set_spectra):
        key = (name, set_spectra)
        if key not in cache:
            opts = dict(ic.OPTIONS[name], silent=True, set_spectra=set_spectra)
            cat, twin = ic.catalogue(), ic.catalogue()
            report = {}
            got = init.init_blends(*_columns(cat), _report=report, **opts)
            launches = (report["launches"], report["fallback"])
            want = [init.init_all_sources(f, c, o, **opts) for f, c, o in zip(*_columns(twin))]
            cache[key] = (cat, got, want, launches)
        return cache[key]

    return get


@pytest.mark.parametrize("name", sorted(ic.OPTIONS))
def test_every_case_equals_the_loop(runs, name):
    """Classes, skipped, boxes, centres, steps, flags and chains equal; morphologies and the
    pixel spectra of set_spectra=False bit for bit -- refused and fallen-back blends included,
    in list order."""
    cat, got, want, launches = runs(name, False)
    assert len(got) == len(want) == len(cat)
    # the last chunk took its three launches, and the loop only the blends meant for it
    assert launches[0] == ["psf_snr", "sweep", "crop"]
    assert [cat[i][0] for i, _ in launches[1]] == [c[0] for c in cat if c[4] != "device"]
    assert [why.startswith("at run time") for _, why in launches[1]] == [
        c[4] == "runtime" for c in cat if c[4] != "device"]
    for case, a, b in zip(cat, got, want):
        try:
            ic.same_sources(a, b, spectra="equal")
        except AssertionError as exc:
            raise AssertionError("blend '{}' ({}): {}".format(case[0], name, exc))


def test_option_sets_reach_every_class_and_branch(runs):
    """The cases mean something: two components, one, compact; a lit single pixel; a fixed box."""
    import scarlet_amd as scarlet

    _, got, _, _ = runs("two", False)
    kinds = {type(s) for sources, _ in got for s in sources}
    assert kinds == {scarlet.MultiExtendedSource, scarlet.SingleExtendedSource,
                     scarlet.CompactExtendedSource}
    cat, got, _, _ = runs("box", False)
    assert all(s.children[1].bbox.shape == (15, 15) for sources, _ in got for s in sources)
    null = [k for k, c in enumerate(cat) if c[0] == "null"][0]
    faint = np.asarray(got[null][0][2].children[1].parameters[0])
    floor = np.asarray(scarlet.CompactExtendedSource.init_morph(cat[null][1], cat[null][2][2], 15)[0])
    assert faint[7, 7] == 1 and np.array_equal(faint, np.maximum(floor, faint == 1))


@pytest.mark.parametrize("name", sorted(ic.OPTIONS))
def test_spectra_of_set_spectra(runs, name):
    """set_spectra=True: the device's normal equations.  Per blend the longdouble solution by
    direct convolution is the truth; the loop's distance from it, relative to each component's
    largest band, is measured, and the device may lie at most 4 x that far plus one float32
    rounding of the value.  Measured over the three option sets (float32 parameters, so both
    are the rounding of the cast): loop <= 5.4e-08, device <= 5.4e-08, equal blend by blend;
    before the cast see test_device_sums_against_longdouble.  Blends the loop took are the loop's own answer up to
    the order of its threaded BLAS sums."""
    from scarlet_amd import initialization as init

    cat, got, want, launches = runs(name, True)
    assert launches[0][-2:] == ["spectra_tiles", "spectra_reduce"] and len(launches[0]) <= 5
    took = {cat[i][0]: why for i, why in launches[1]}
    assert sorted(took) == sorted(c[0] for c in cat if c[4] != "device" or c[0] in ic.SPECTRA_RUNTIME)
    assert all("identical" in took[n] for n in ic.SPECTRA_RUNTIME)
    worst = [0.0, 0.0]
    for case, a, b in zip(cat, got, want):
        ic.same_sources(a, b, spectra=None)
        x, y = np.array(_spectra(a)), np.array(_spectra(b))
        assert x.dtype == y.dtype == np.float32
        if case[0] in took:
            ok = np.isfinite(y)  # (the loop's own answer for the band with the NaN pixel is NaN)
            assert_array_equal(np.isfinite(x), ok)
            scale = np.abs(np.where(ok, y, 0)).max(axis=1, keepdims=True)
            assert np.all(np.abs(x - y)[ok] <= (2.0 ** -23 * np.abs(y) + 1e-10 * scale)[ok]), case[0]
            continue
        comps = init._components(b[0])
        sp = init.pack_spectra([(0, case[1], case[3], b[0])], [0])  # (sets the spectra to 1)
        for c, row in zip(comps, y):
            c.children[0].parameters[0][:] = row
        assert sp["loop"] == {}
        truth, ratios = ic.longdouble_spectra(sp, 0, case[3].data, case[3].weights)
        assert (np.abs(ratios - 0.1) > 1e-3).all(), case[0]  # the cases keep clear of the rule
        truth = ic.constrained(comps, truth)
        d_loop, d_device = ic.spectra_distance(y, truth), ic.spectra_distance(x, truth)
        print("%-6s %-5s K=%d loop %.3g device %.3g" % (case[0], name, len(comps), d_loop, d_device))
        worst = [max(worst[0], d_loop), max(worst[1], d_device)]
        scale = np.abs(truth).max(axis=1, keepdims=True)
        assert (np.abs(x - truth) <= 4 * d_loop * scale + 2.0 ** -24 * np.abs(truth)).all(), case[0]
    print("worst: loop %.3g device %.3g" % tuple(worst))


def test_device_sums_against_longdouble(runs):
    """The sums themselves, before any cast: the (G, r, sum m w, sum m) tables of the two spectra
    launches against the longdouble restatement.  Every entry is a sum of at most 64 x 48
    products of one sign pattern the rounding of which is at most n eps of the sum of the
    absolute values; asserted at 1e-12 of the largest entry of its kind."""
    import torch

    from scarlet_amd import _catalog, initialization as init

    cat, got, _, _ = runs("two", False)
    for case, (sources, _) in zip(cat, got):
        if case[4] != "device" or case[0] in ic.SPECTRA_RUNTIME:
            continue
        frame, obs = case[1], case[3]
        sp = init.pack_spectra([(0, frame, obs, sources)], [0])
        dv = _catalog.Launcher(0, pad=1)
        K, C = int(sp["blends"][0]["n_comp"]), frame.C
        d_data, d_weights = dv.cat([obs.data], np.float32), dv.cat([obs.weights], np.float32)
        d_morphs, d_stamps = dv.cat(sp["morphs"], np.float64), dv.cat(sp["stamps"], np.float64)
        d_part, d_sums = dv.empty(sp["n_part"], np.float64), dv.empty(sp["n_out"], np.float64)
        init._call(dv, "spectra_tiles", sp["blends"], sp["components"], sp["work"], d_data,
                   d_weights, obs.data.size, d_stamps, sp["n_stamp"], d_morphs, sp["n_morph"],
                   d_part, sp["n_part"], sp["n_out"])
        init._call(dv, "spectra_reduce", sp["blends"], d_part, sp["n_part"], d_sums, sp["n_out"])
        torch.cuda.synchronize()
        sums = d_sums.cpu().numpy().reshape(C, K * K + 3 * K)
        want = ic.normal_equations(sp, 0, obs.data, obs.weights, np.longdouble)
        for lo, hi in ((0, K * K), (K * K, K * K + K), (K * K + K, K * K + 2 * K),
                       (K * K + 2 * K, K * K + 3 * K)):
            err = np.abs(sums[:, lo:hi] - want[:, lo:hi]).max()
            assert err <= 1e-12 * np.abs(want[:, lo:hi]).max(), (case[0], lo, float(err))
        # G is written symmetric, bit for bit
        G = sums[:, :K * K].reshape(C, K, K)
        assert_array_equal(G, G.transpose(0, 2, 1))


def test_bits_do_not_depend_on_list_order_or_chunks(runs):
    """A blend alone, in the catalogue, in the reversed catalogue and in chunks of one blend:
    identical bits, spectra included, for every blend the device takes (the loop's own solve
    adds its sums in no fixed order: its blends are compared without the spectra)."""
    from scarlet_amd import initialization as init

    opts = dict(ic.OPTIONS["two"], silent=True, set_spectra=True)
    cat, whole, _, _ = runs("two", True)
    rev = ic.catalogue()[::-1]
    reversed_ = init.init_blends(*_columns(rev), **opts)[::-1]
    small = init.init_blends(*_columns(ic.catalogue()), _working_set_bytes=1, **opts)
    fresh = ic.catalogue()
    alone = [init.init_blends([c[1]], [c[2]], [c[3]], **opts)[0] for c in fresh]
    for case, a, b, c, d in zip(cat, whole, reversed_, small, alone):
        device = case[4] == "device" and case[0] not in ic.SPECTRA_RUNTIME
        for other in (b, c, d):
            ic.same_sources(a, other, spectra="equal" if device else None)


@pytest.mark.parametrize("name", ["box", "plain"])
def test_no_flux_warnings_are_the_loops(name, caplog):
    """'No flux in morphology model' where the cut-out is empty -- not where the whole plane
    is --, as the loop decides it: the same messages in the same order."""
    import logging

    from scarlet_amd import initialization as init

    opts = dict(ic.OPTIONS[name], silent=True, set_spectra=False)
    logs = []
    for run in (lambda cat: init.init_blends(*_columns(cat), **opts),
                lambda cat: [init.init_all_sources(f, c, o, **opts) for f, c, o in zip(*_columns(cat))]):
        cat = [c for c in ic.catalogue() if c[4] == "device"]
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            run(cat)
        logs.append([r.getMessage() for r in caplog.records if "No flux" in r.getMessage()])
    assert logs[0] == logs[1]


def test_plan_named_the_blends_the_loop_took(runs):
    from scarlet_amd import initialization as init

    cat, got, want, _ = runs("plain", False)
    _, fallback = init.plan_init_blends(*_columns(cat), **ic.OPTIONS["plain"])
    assert [cat[i][0] for i, _ in fallback] == [c[0] for c in cat if c[4] == "refused"]
    assert sum(c[4] == "runtime" for c in cat) <= 3


def test_synthetic_scenes_match_the_reference():
    """The three scenes the reference initialised itself (golden init_synthetic.npz) as a
    catalogue, with the assertions and tolerances test_initialisation_of_synthetic_scenes_
    matches_reference applies to the loop.  The scenes carry different settings and a call takes
    one set: the catalogue runs once per scene's settings and that scene is checked."""
    import scarlet_amd as scarlet
    from conftest import golden
    from scarlet_amd.initialization import init_blends, plan_init_blends

    g = golden("init_synthetic")

    def build():
        frames, centers, observations = [], [], []
        for t in range(int(g["n_scenes"])):
            tag = "s%d_" % t
            images, weights, psfs = g[tag + "images"], g[tag + "weights"], g[tag + "psfs"]
            C = images.shape[0]
            filters = ["f%d" % c for c in range(C)]
            frame = scarlet.Frame(images.shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * C),
                                  channels=filters)
            obs = scarlet.Observation(images.copy(), psf=scarlet.ImagePSF(psfs.copy()),
                                      weights=weights.copy(), channels=filters).match(frame)
            frames.append(frame)
            observations.append(obs)
            centers.append([tuple(c) for c in g[tag + "centers"]])
        return frames, centers, observations

    for t in range(int(g["n_scenes"])):
        tag = "s%d_" % t
        max_components, min_snr, thresh = g[tag + "settings"]
        opts = dict(max_components=int(max_components), min_snr=float(min_snr),
                    thresh=float(thresh), fallback=True, silent=True, set_spectra=True)
        frames, centers, observations = build()
        assert plan_init_blends(frames, centers, observations, **opts)[1] == []
        sources, skipped = init_blends(frames, centers, observations, **opts)[t]
        obs = observations[t]
        assert list(skipped) == list(g[tag + "skipped"])
        assert [type(s).__name__ for s in sources] == [str(k) for k in g[tag + "kinds"]], t
        blend = scarlet.Blend(sources, obs)
        comps = [c for s in blend.sources
                 for c in (s.children if isinstance(s, scarlet.CombinedComponent) else [s])]
        assert len(comps) == int(g[tag + "n_comp"])
        for k, comp in enumerate(comps):
            sed = np.asarray(comp.children[0].parameters[0])
            morph = np.asarray(comp.children[1].parameters[0])
            ref_morph, ref_sed = g[tag + "morph_%d" % k], g[tag + "sed_%d" % k]
            assert morph.shape == ref_morph.shape, (t, k)
            assert tuple(comp.children[1].bbox.origin) == tuple(g[tag + "origin_%d" % k]), (t, k)
            assert np.abs(morph - ref_morph).max() < 1e-5, (t, k)
            assert np.abs(sed - ref_sed).max() < 3e-5 * np.abs(ref_sed).max() + 1e-6, (t, k)
            step = comp.children[0].parameters[0].step
            assert_allclose(step.keywords["minimum"], g[tag + "min_step_%d" % k], rtol=1e-5)
        logL0 = obs.get_log_likelihood(blend.get_model())
        assert abs(logL0 - float(g[tag + "logL"])) < 2e-5 * abs(float(g[tag + "logL"])) + 0.05, t


def test_fit_blends_raises_every_log_likelihood(runs):
    import scarlet_amd as scarlet

    opts = dict(ic.OPTIONS["plain"], silent=True, set_spectra=True)
    cat = [c for c in ic.catalogue() if c[4] == "device"]
    results = scarlet.init_blends(*_columns(cat), **opts)
    blends = [scarlet.Blend(sources, c[3]) for c, (sources, _) in zip(cat, results)]
    before = [c[3].get_log_likelihood(b.get_model()) for c, b in zip(cat, blends)]
    fitted = scarlet.fit_blends(blends, 30, e_rel=1e-4)
    for case, lo, (_, logL) in zip(cat, before, fitted):
        assert logL > lo, case[0]


# ---------------------------------------------------------------- validation of the entries
def _entry(step):
    from scarlet_amd import _lib

    return getattr(_lib.load(), "smi_init_sources_%s_f32" % step), _lib


def _call(step, table, sizes, comps=None, work=None):
    """The entry with a table and buffer sizes and pointers that are never followed: the
    validation answers before anything is launched."""
    fn, _lib = _entry(step)
    keep = np.zeros(8)
    p = ctypes.c_void_p(keep.ctypes.data)
    t = ctypes.c_void_p(table.ctypes.data)
    if step == "psf_snr":
        args = [p, p, sizes[0], p, sizes[1], p, sizes[2]]
    elif step == "sweep":
        args = [p, p, sizes[0], p, sizes[1], p, sizes[2], p, p, sizes[3]]
    elif step == "crop":
        args = [p, sizes[0], p, sizes[1], p, sizes[2], p, sizes[3]]
    elif step == "spectra_tiles":
        c, w = ctypes.c_void_p(comps.ctypes.data), ctypes.c_void_p(work.ctypes.data)
        args = [len(comps), c, c, len(work), w, w, p, p, sizes[0], p, sizes[1], p, sizes[2], p,
                sizes[3], sizes[4]]
    else:
        args = [p, sizes[0], p, sizes[1]]
    return fn(len(table), t, t, *args, None), _lib


# a 9 x 11 frame of 3 bands: one source in the middle with a 5 x 5 stamp, a 21 x 21 box that leaves
# the frame on all sides, one 15 x 15 component on one tile
_BLEND = (9, 11, 0, 0, 9, 11, 3, 5, 5, 1, 0, 0, 0, 0, 0, 0)
GOOD = {
    "psf_snr": ((9, 11, 4, 5, 5, 5, 3, 0, 0, 0, 0), (297, 75, 9)),
    "sweep": ((9, 11, 4, 5, 3, 0, 0, 0, 0, 1.0), (297, 3, 99, 1)),
    "crop": ((9, 11, -6, -5, 21, 2, 0, 0, 0, 25.0), (99, 441, 882, 1)),
    "spectra_tiles": (_BLEND, (297, 75, 225, 12, 12)),
    "spectra_reduce": (_BLEND, (12, 12)),
}
GOOD_COMPONENT, GOOD_WORK = (-3, -2, 15, 15, 0), (0, 0)
# (entry, fields changed -- "c." a field of the component, "work" the tile of the work list --,
# buffer sizes or None for the good ones, what the entry has to answer)
BAD = [
    ("psf_snr", dict(ph=65), None, "stamp extent"),
    ("psf_snr", dict(cy=9), None, "centre outside its frame"),
    ("psf_snr", dict(bands=0), None, "bands"),
    ("psf_snr", dict(cube_off=1), None, "cube outside the data buffers"),
    ("psf_snr", dict(psf_off=1), None, "stamps outside their buffer"),
    ("psf_snr", dict(out_off=1), None, "sums outside the output buffer"),
    ("psf_snr", dict(h=1 << 15), None, "frame extent"),
    ("sweep", dict(h=200, w=200), (5 * 40000, 3, 40000, 1), "frame beyond the LDS image"),
    ("sweep", dict(cx=11), None, "centre outside its frame"),
    ("sweep", dict(cube_off=-1), None, "cube outside the data buffers"),
    ("sweep", dict(spec_off=1), None, "spectrum outside its buffer"),
    ("sweep", dict(out_off=1), None, "swept plane outside the output buffer"),
    ("sweep", dict(), (297, 3, 99, 0), "results outside the output buffers"),
    ("crop", dict(side=20), None, "box side"), ("crop", dict(side=4097), None, "box side"),
    ("crop", dict(layers=3), None, "one or two layers"),
    ("crop", dict(percentile=100.0), None, "percentile outside"),
    ("crop", dict(plane_off=1), None, "plane outside its buffer"),
    ("crop", dict(floor_off=1), None, "floor outside its buffer"),
    ("crop", dict(out_off=1), None, "cut-out outside the output buffer"),
    ("crop", dict(y0=1 << 20), None, "box origin"),
    ("crop", dict(), (99, 441, 882, 0), "flags outside their buffer"),
    ("spectra_tiles", dict(kh=65), (297, 3 * 65 * 5, 225, 12, 12), "stamp beyond the kernel's limit"),
    ("spectra_tiles", dict(kw=4), None, "odd height and width"),
    ("spectra_tiles", dict(n_comp=65), None, "components of a blend"),
    ("spectra_tiles", dict(n_comp=0), None, "components of a blend"),
    ("spectra_tiles", dict(n_comp=33), (297, 75, 225, 3564, 3564), "components present on one tile"),
    ("spectra_tiles", dict(n_comp=2), (297, 75, 225, 30, 30), "component range"),
    ("spectra_tiles", dict(fh=10), None, "region outside its frame"),
    ("spectra_tiles", dict(x0=1), None, "region outside its frame"),
    ("spectra_tiles", dict(bands=0), None, "bands"),
    ("spectra_tiles", dict(cube_off=1), None, "cube outside the data buffers"),
    ("spectra_tiles", dict(stamp_off=1), None, "stamps outside their buffer"),
    ("spectra_tiles", dict(part_off=1), None, "tile sums outside their buffer"),
    ("spectra_tiles", dict(out_off=1), None, "sums outside the output buffer"),
    ("spectra_tiles", {"c.morph_off": 1}, None, "morphology outside its buffer"),
    ("spectra_tiles", {"c.h": 0}, None, "component extent"),
    ("spectra_tiles", {"c.y0": 1 << 25}, None, "component origin"),
    ("spectra_tiles", dict(work=1), None, "work list"),
    ("spectra_reduce", dict(n_comp=65), None, "components of a blend"),
    ("spectra_reduce", dict(fw=0), None, "region outside its frame"),
    ("spectra_reduce", dict(part_off=1), None, "tile sums outside their buffer"),
    ("spectra_reduce", dict(out_off=1), None, "sums outside the output buffer"),
]


def malformed(step, change, sizes):
    """``(status, _lib)`` of the entry for its good table with ``change`` applied."""
    from scarlet_amd import initialization as init

    dtype = {"psf_snr": init._PSF_SNR_DESC, "sweep": init._SWEEP_DESC, "crop": init._CROP_DESC,
             "spectra_tiles": init._SPECTRA_BLEND, "spectra_reduce": init._SPECTRA_BLEND}[step]
    table = np.zeros(1, dtype)
    table[0] = GOOD[step][0]
    comps = np.zeros(33 if change.get("n_comp") == 33 else 1, init._SPECTRA_COMPONENT)
    comps[:] = GOOD_COMPONENT
    work = np.array([GOOD_WORK], np.int32)
    for field, value in change.items():
        if field == "work":
            work[0, 1] = value
        elif field.startswith("c."):
            comps[field[2:]] = value
        else:
            table[field] = value
    return _call(step, table, GOOD[step][1] if sizes is None else sizes, comps, work)


@pytest.mark.parametrize("step,change,sizes,answer", BAD)
def test_entries_refuse_malformed_tables(step, change, sizes, answer):
    """Each malformed table is refused for the reason meant: the entry reached that check, so
    the rest of the table -- the good one -- passed the checks before it."""
    status, _lib = malformed(step, change, sizes)
    assert status < 0
    assert answer in _lib.load().smi_last_error().decode()
    with pytest.raises(_lib.ScarletAmdError):
        _lib.check(status)
