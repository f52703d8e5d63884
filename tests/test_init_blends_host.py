"""The host side of initialization.init_blends, without a GPU: the plan and its refusals, the
descriptor records against the C structs, packing and chunking, the box rule, the component
count and its near-integer rule, the conditions the test catalogue has to meet, and a NumPy
restatement of the three kernels against the loop's own host functions."""

import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import init_blends_cases as ic
from conftest import ROOT


def _columns(cat):
    return [c[1] for c in cat], [c[2] for c in cat], [c[3] for c in cat]


@pytest.fixture(scope="module")
def cat():
    return ic.catalogue()


# ---------------------------------------------------------------- plan
def test_plan_takes_and_refuses_what_the_cases_say(cat):
    from scarlet_amd import initialization as init

    for name, opts in ic.OPTIONS.items():
        groups, fallback = init.plan_init_blends(*_columns(cat), **opts)
        taken = sorted(i for idx in groups.values() for i in idx)
        assert taken == [i for i, c in enumerate(cat) if c[4] != "refused"]
        assert [i for i, _ in fallback] == [i for i, c in enumerate(cat) if c[4] == "refused"]
        reasons = {cat[i][0]: why for i, why in fallback}
        assert "observations" in reasons["two observations"]
        assert "even" in reasons["even stamp"]
        assert "outside the frame" in reasons["off the frame"]
        # groups: dtype, bands, PSF stamp shape; list order inside a group
        for key, idx in groups.items():
            assert idx == sorted(idx)
            for i in idx:
                obs = cat[i][3]
                assert key == ("<f4", cat[i][1].C) + tuple(obs.psf.bbox.shape[1:])


def test_plan_never_loads_the_library(cat, monkeypatch):
    from scarlet_amd import _lib, initialization as init

    def boom():
        raise AssertionError("plan_init_blends touched the library")

    monkeypatch.setattr(_lib, "load", boom)
    init.plan_init_blends(*_columns(cat))


def _one(cat, name="odd"):
    return next(c for c in cat if c[0] == name)


def test_every_refusal_reason(cat):
    import scarlet_amd as scarlet
    from scarlet_amd import initialization as init

    _, frame, centers, obs, _ = _one(cat)
    base = init._options({})

    def why(frame=frame, centers=centers, obs=obs, **opts):
        return init._refusal(frame, centers, obs, dict(base, **opts))

    assert why() is None
    assert why(obs=[obs]) is None  # a sequence holding one
    assert "max_components" in why(max_components=3)
    assert "thresh" in why(thresh=-1)
    assert "no centres" in why(centers=[])
    assert "outside the frame" in why(centers=[(25.6, 3)])
    assert why(centers=[(24.4, 30.4)]) is None
    assert "boxsize" in why(boxsize=1 << 14)
    assert "min_snr" in why(min_snr=0)
    # another renderer, another dtype, no PSF, a frame the observation is not matched to
    C = frame.C
    channels = list(frame.channels)

    class Mine(scarlet.ConvolutionRenderer):
        pass

    f2, o2 = ic.scene(2, (5, 25, 31), (11, 11), [])
    o2.match(f2, renderer=Mine(o2, f2))
    assert "neither" in init._refusal(f2, centers, o2, base)
    f3, o3 = ic.scene(2, (5, 25, 31), (11, 11), [])
    o3.match(f3, renderer=scarlet.ConvolutionRenderer(o3, f3, psf_shift=np.zeros((C, 2))))
    assert "psf_shift" in init._refusal(f3, centers, o3, base)
    assert "not matched" in init._refusal(f2, centers, obs, base)
    f64 = scarlet.Frame(frame.shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * C), channels=channels,
                        dtype=np.float64)
    o64 = scarlet.Observation(obs.data.copy(), psf=obs.psf, weights=obs.weights.copy(),
                              channels=channels).match(f64)
    assert "float32" in init._refusal(f64, centers, o64, base)
    big = scarlet.Frame((1, 143, 143), psf=scarlet.GaussianPSF(sigma=(0.8,)), channels=["a"])
    obig = scarlet.Observation(np.zeros((1, 143, 143), np.float32),
                               psf=scarlet.ImagePSF(ic.gaussian_stamps(1, 5, 5)),
                               channels=["a"]).match(big)
    assert "20352" in init._refusal(big, [(5, 5)], obig, base)
    small = scarlet.Frame((1, 159, 128), psf=scarlet.GaussianPSF(sigma=(0.8,)), channels=["a"])
    osmall = scarlet.Observation(np.zeros((1, 159, 128), np.float32),
                                 psf=scarlet.ImagePSF(ic.gaussian_stamps(1, 5, 5)),
                                 channels=["a"]).match(small)
    assert init._refusal(small, [(5, 5)], osmall, base) is None  # exactly 20352 pixels
    wide = scarlet.Observation(np.zeros((1, 9, 11), np.float32),
                               psf=scarlet.ImagePSF(ic.gaussian_stamps(1, 65, 65)), channels=["a"])
    fw = scarlet.Frame((1, 9, 11), psf=scarlet.GaussianPSF(sigma=(0.8,)), channels=["a"])
    assert "63" in init._refusal(fw, [(5, 5)], wide.match(fw), base)
    # an observation that covers a part of the frame only
    part = scarlet.Observation(np.zeros((3, 25, 31), np.float32),
                               psf=scarlet.ImagePSF(ic.gaussian_stamps(3, 5, 5)),
                               channels=channels[:3]).match(frame)
    assert "cover" in init._refusal(frame, centers, part, base)


def test_plan_refuses_lists_of_different_length(cat):
    from scarlet_amd import initialization as init

    frames, centers, observations = _columns(cat)
    with pytest.raises(ValueError):
        init.plan_init_blends(frames, centers[:-1], observations)
    with pytest.raises(TypeError):
        init.plan_init_blends(frames, centers, observations, percentile=3)


# ---------------------------------------------------------------- records, packing, chunks
def _c_struct(name):
    """[(field, C type)] of a struct of include/scarlet_amd.h"""
    text = open(os.path.join(ROOT, "include", "scarlet_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_records_are_the_c_structs():
    from scarlet_amd import initialization as init

    kinds = {"int32_t": np.dtype(np.int32), "int64_t": np.dtype(np.int64), "double": np.dtype("f8")}
    for name, dtype in (("smi_init_sources_psf_snr", init._PSF_SNR_DESC),
                        ("smi_init_sources_sweep", init._SWEEP_DESC),
                        ("smi_init_sources_crop", init._CROP_DESC),
                        ("smi_init_sources_spectra_blend", init._SPECTRA_BLEND),
                        ("smi_init_sources_spectra_component", init._SPECTRA_COMPONENT)):
        fields = _c_struct(name)
        assert [f for f, _ in fields] == list(dtype.names)
        offset = 0
        for field, ctype in fields:  # natural alignment, as the C compiler lays it out
            size = kinds[ctype].itemsize
            offset = (offset + size - 1) // size * size
            assert dtype.fields[field] == (kinds[ctype], offset), (name, field)
            offset += size
        assert dtype.itemsize == (offset + 7) // 8 * 8


def _device_blends(cat):
    return [(c[1], c[2], c[3]) for c in cat if c[4] != "refused"]


def test_packed_tables_stay_inside_their_buffers(cat):
    from scarlet_amd import initialization as init

    blends = _device_blends(cat)
    pk = init.pack_chunk(blends, init._options(ic.OPTIONS["two"]))
    names = [c[0] for c in cat if c[4] != "refused"]
    assert [names[k] for k in pk["loop"]] == ["nan"]  # the only run-time fallback of the cases
    assert pk["n_cube"] == sum(b[0].C * b[0].shape[1] * b[0].shape[2] for b in blends)
    assert sum(d.size for d in pk["data"]) == sum(v.size for v in pk["var"]) == pk["n_cube"]
    ends = 0
    for s, (t, u) in enumerate(zip(pk["psf_snr"], pk["sweep"])):
        frame = blends[pk["src_blend"][s]][0]
        assert (t["h"], t["w"], t["bands"]) == (u["h"], u["w"], u["bands"]) == (
            frame.shape[1], frame.shape[2], frame.C)
        assert 0 <= t["cy"] < t["h"] and 0 <= t["cx"] < t["w"]
        assert t["cube_off"] + frame.C * t["h"] * t["w"] <= pk["n_cube"]
        assert t["psf_off"] + frame.C * t["ph"] * t["pw"] <= pk["n_psf"]
        assert t["out_off"] + 3 * frame.C <= pk["n_snr"]
        assert u["spec_off"] + frame.C <= len(pk["spectra"])
        assert u["out_off"] == ends and u["thresh"] == 0.5
        ends += t["h"] * t["w"]
    assert ends == pk["n_plane"]
    # zero-weight pixels go up with a negated variance, all others positive
    wide = names.index("wide")
    assert_array_equal(pk["var"][wide] < 0, blends[wide][2].weights == 0)
    assert (pk["var"][wide] < 0).sum() == 4 * 5


def test_small_chunks_pack_a_blend_to_the_same_bytes(cat):
    from scarlet_amd import _catalog, initialization as init

    opts = init._options(ic.OPTIONS["two"])
    blends = _device_blends(cat)
    whole = init.pack_chunk(blends, opts)
    items = [(i, init._blend_bytes(b[0], len(b[1]), 21)) for i, b in enumerate(blends)]
    assert _catalog.chunks(items, 1) == [[i] for i in range(len(blends))]
    assert _catalog.chunks(items, 1 << 40) == [list(range(len(blends)))]
    two = _catalog.chunks(items, items[0][1] + items[1][1])
    assert two[0] == [0, 1] and sum(two, []) == list(range(len(blends)))
    first = 0
    for k, blend in enumerate(blends):
        alone = init.pack_chunk([blend], opts)
        n = len(alone["src_blend"])
        assert alone["data"][0].tobytes() == whole["data"][k].tobytes()
        assert alone["var"][0].tobytes() == whole["var"][k].tobytes()
        assert alone["psfs"][0].tobytes() == whole["psfs"][k].tobytes()
        if k in whole["loop"]:
            assert set(alone["loop"]) == {0} and n == 0
            continue
        sub = whole["sweep"][first:first + n].copy()
        for field, table in (("cube_off", alone["sweep"]), ("spec_off", alone["sweep"]),
                             ("out_off", alone["sweep"])):
            sub[field] -= sub[field][0] - table[field][0]
        assert sub.tobytes() == alone["sweep"].tobytes()
        lo = whole["sweep"]["spec_off"][first]
        assert whole["spectra"][lo:lo + len(alone["spectra"])].tobytes() == alone["spectra"].tobytes()
        first += n


# ---------------------------------------------------------------- host decisions
def test_box_rule_is_that_of_trim_morphology():
    from scarlet_amd import initialization as init

    rng = np.random.RandomState(3)
    for trial in range(40):
        h, w = rng.randint(5, 60, 2)
        morph = np.zeros((h, w))
        pixel = (rng.randint(h), rng.randint(w))
        if trial % 4:
            y0, x0 = rng.randint(h), rng.randint(w)
            morph[y0:y0 + rng.randint(1, 30), x0:x0 + rng.randint(1, 30)] = 1
        boxsize = None if trial % 3 else int(rng.randint(1, 40))
        ys, xs = np.nonzero(morph > 0)
        bounds = (ys.min(), ys.max(), xs.min(), xs.max()) if len(ys) else (0, -1, 0, -1)
        _, bbox = init.trim_morphology(pixel, morph.copy(), bg_thresh=0, boxsize=boxsize)
        origin, side = init.trim_box(bounds, pixel, boxsize)
        assert bbox.shape == (side, side) and tuple(bbox.origin) == origin


def test_component_count_and_the_near_integer_rule():
    from scarlet_amd import initialization as init

    def count(ratio, **kw):
        opts = init._options(dict(dict(min_snr=10.0, max_components=2, min_components=0), **kw))
        sums = np.array([[ratio * 10.0 * 3.0, 1.0, 9.0]])  # snr = num / sqrt(den)
        return init.component_count(sums, opts)

    assert [count(r) for r in (0.5, 1.5, 2.5, 7.0, -3.0)] == [0, 1, 2, 2, 0]
    assert count(0.5, min_components=1) == 1 and count(7.0, max_components=1) == 1
    assert count(1 + 0.9e-4) is None and count(1 - 0.9e-4) is None and count(2 * (1 + 0.9e-4)) is None
    assert count(1 + 1.1e-4) == 1 and count(1 - 1.1e-4) == 0 and count(2 * (1 - 1.1e-4)) == 1
    assert count(np.nan) is None and count(np.inf) is None
    assert count(0.5, fallback=False) == 2 and count(np.nan, fallback=False, max_components=1) == 1


def test_cases_keep_clear_of_the_run_time_rules(cat):
    """Every snr / min_snr at least 1 % from every component count it could tip (and one
    beyond), so that the run-time fallbacks trigger only in the cases meant for them; at most
    three of those."""
    assert sum(c[4] == "runtime" for c in cat) <= 3
    for opts in ic.OPTIONS.values():
        min_snr = opts.get("min_snr", 50)
        counts = range(0, opts.get("max_components", 1) + 2)
        for name, frame, centers, obs, expect in cat:
            if expect != "device":
                continue
            for center in centers:
                ratio = ic.snr_ratio(frame, center, obs, min_snr)
                assert np.isfinite(ratio)
                assert all(abs(ratio - k) >= 0.01 * max(k, 1) for k in counts), (name, center)


def test_snr_ratio_of_the_cases_is_the_loops(cat):
    from scarlet_amd import initialization as init

    for name, frame, centers, obs, expect in cat:
        if expect != "device":
            continue
        for center in centers:
            _, snr = init.get_psf_spectrum(center, obs, compute_snr=True)
            assert abs(ic.snr_ratio(frame, center, obs, 10.0) * 10.0 - snr) <= 1e-5 * abs(snr) + 1e-6


# ---------------------------------------------------------------- the kernels, restated
def _sweep_numpy(data, var, spec, pixel, thresh):
    """The sweep kernel in NumPy, operation by operation: coadd, symmetry, the 'flat' sweep level
    by level in the order of lite_init_main.hip, trim."""
    from scarlet_amd.lite.initialization import _sweep_level

    C, h, w = data.shape
    v = np.abs(var)
    wt = np.where(v > 0, (np.float32(1) / np.where(v > 0, v, 1)).astype(np.float64), 0.0)
    wt = wt * spec[:, None, None]
    img = np.zeros((h, w))
    for c in range(C):
        img = img + wt[c] * data[c].astype(np.float64)
    std2 = np.zeros((h, w))
    for c in range(C):
        std2 = std2 + spec[c] * wt[c]
    cy, cx = pixel
    if (cy, cx) == (h // 2, w // 2):
        ys, xs = slice(None), slice(None)
    else:
        def rng(n, c):
            d = 2 * (c - n // 2) + (n % 2 == 0)
            return slice(max(d, 0), n + d if d < 0 else n)
        ys, xs = rng(h, cy), rng(w, cx)
    img[ys, xs] = np.minimum(img[ys, xs], img[ys, xs][::-1, ::-1])
    Y, X = np.mgrid[:h, :w]
    Y, X = Y - cy, X - cx
    level = _sweep_level(Y, X)
    r2 = Y * Y + X * X
    dirs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    for L in range(level.max() + 1):
        new = {}
        for y, x in zip(*np.nonzero(level == L)):
            nb = [(y + dy, x + dx) for dy, dx in dirs
                  if 0 <= y + dy < h and 0 <= x + dx < w and r2[y + dy, x + dx] < r2[y, x]]
            ref = 0.0
            for q in nb:
                ref = ref + img[q] * (1.0 / len(nb))
            if ref < img[y, x]:
                new[(y, x)] = ref
        for q, val in new.items():
            img[q] = val
    with np.errstate(invalid="ignore"):
        img[~(img > np.sqrt(std2) * thresh)] = 0
    return img


def test_numpy_restatement_of_the_sweep_equals_the_loop(cat):
    """What the sweep kernel computes, restated in NumPy from the packed tables, is bit for bit
    what the loop's host functions and the sequential sweep give: coadd, symmetry, level order
    and trim.  (The sequential sweep itself is restated with the weights of
    getRadialMonotonicWeights in radial order, as the native operator applies them.)"""
    from scarlet_amd import initialization as init, operator

    blends = _device_blends(cat)
    opts = init._options(ic.OPTIONS["two"])
    pk = init.pack_chunk(blends, opts)
    off = np.cumsum([0] + [d.size for d in pk["data"]])
    checked = 0
    for s, k in enumerate(pk["src_blend"]):
        frame, centers, obs = blends[k]
        if frame.shape[1] * frame.shape[2] > 33 * 37:
            continue
        t = pk["sweep"][s]
        C, h, w = t["bands"], t["h"], t["w"]
        assert t["cube_off"] == off[k]
        spec = pk["spectra"][t["spec_off"]:t["spec_off"] + C]
        got = _sweep_numpy(pk["data"][k], pk["var"][k], spec, (t["cy"], t["cx"]), t["thresh"])
        # the loop: build_initialization_image, prox_uncentered_symmetry, sequential sweep, trim
        coadd, std = init.build_initialization_image((obs,), spectra=pk["src_spec"][s])
        pixel = (int(t["cy"]), int(t["cx"]))
        profile = operator.prox_uncentered_symmetry(coadd.copy(), 0, center=pixel, algorithm="sdss")
        weights = operator.getRadialMonotonicWeights((h, w), "flat", pixel)
        order = operator.sort_by_radius((h, w), pixel)[1:]
        offsets = [dy * w + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
        flat = profile.reshape(-1)
        for p in order:
            ref = 0.0
            for i, o in enumerate(offsets):
                if weights[i, p] != 0:
                    ref = ref + flat[p + o] * weights[i, p]
            if ref < flat[p]:
                flat[p] = ref
        with np.errstate(invalid="ignore"):
            profile[~(profile > std * t["thresh"])] = 0
        assert_array_equal(got, profile)
        checked += 1
    assert checked >= 8


# ---------------------------------------------------------------- spectra
def test_seen_rule_and_the_near_tenth_rule():
    from scarlet_amd import initialization as init

    def seen(*ratios):
        r = np.array(ratios, np.float64)
        return init.seen_components(r * 3.0 * 400.0, np.full(len(r), 3.0), 400.0)

    assert_array_equal(seen(0.5, 0.05, 0.2), [0, 2])
    assert_array_equal(seen(0.05), [])
    assert seen(0.5, 0.1 + 0.9e-6) is None and seen(0.1 - 0.9e-6, 0.5) is None
    assert_array_equal(seen(0.1 + 1.2e-6, 0.1 - 1.2e-6), [0])
    assert seen(np.nan, 0.5) is None
    assert init.seen_components(np.array([1.0]), np.array([0.0]), 400.0) is None
    # a singular matrix and a non-finite solution are the loop's
    K = 2
    sums = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 400.0, 400.0, 1.0, 1.0]])
    assert "singular" in init.solve_spectra(sums, K, np.full((1, 2, 2), 400.0, np.float32))
    sums = np.array([[2.0, 1.0, 1.0, 2.0, 3.0, 3.0, 400.0, 400.0, 1.0, 1.0]])
    np.testing.assert_allclose(init.solve_spectra(sums, K, np.full((1, 2, 2), 400.0, np.float32)),
                               [[1.0], [1.0]], rtol=1e-14)


def _hand_blends(cat):
    """(name, frame, observation, hand-built components) of the cases the device takes."""
    out = []
    for n, (name, frame, centers, obs, expect) in enumerate(cat):
        if expect != "refused" and name not in ic.SPECTRA_RUNTIME and name != "nan":
            out.append((name, frame, obs, ic.hand_components(frame, centers, seed=n)))
    return out


def test_packed_spectra_tables_and_chunks(cat):
    from scarlet_amd import initialization as init

    hand = _hand_blends(cat)
    offs = np.cumsum([0] + [b[1].C * b[1].shape[1] * b[1].shape[2] for b in hand])
    sp = init.pack_spectra([(k, b[1], b[2], b[3]) for k, b in enumerate(hand)], offs)
    assert sp["loop"] == {} and len(sp["blends"]) == len(hand)
    part_end = out_end = at = 0
    for b, (bl, (name, frame, obs, comps)) in enumerate(zip(sp["blends"], hand)):
        K, C = len(comps), frame.C
        assert (bl["h"], bl["w"], bl["bands"], bl["n_comp"]) == (*frame.shape[1:], C, K)
        assert bl["y0"] >= 0 and bl["x0"] >= 0 and bl["fh"] > 0 and bl["fw"] > 0
        assert bl["y0"] + bl["fh"] <= bl["h"] and bl["x0"] + bl["fw"] <= bl["w"]
        stamp = (1, 1) if name == "null" else obs.renderer.diff_kernel.image.shape[1:]
        assert (bl["kh"], bl["kw"]) == stamp
        tiles = -(-bl["fh"] // 16) * -(-bl["fw"] // 16)
        E = K * K + 3 * K
        assert bl["part_off"] == part_end and bl["out_off"] == out_end and bl["cube_off"] == offs[b]
        part_end, out_end = part_end + tiles * C * E, out_end + C * E
        assert_array_equal(sp["work"][at:at + tiles], [(b, t) for t in range(tiles)])
        at += tiles
        for d, comp in zip(sp["components"][bl["comp0"]:bl["comp0"] + K], comps):
            assert (d["y0"], d["x0"]) == tuple(comp.bbox.origin[1:]) and (d["h"], d["w"]) == (15, 15)
        # alone, the blend packs to the same bytes but for where its buffers start
        alone = init.pack_spectra([(0, frame, obs, comps)], [0])
        sub = sp["blends"][b:b + 1].copy()
        for field in ("comp0", "cube_off", "stamp_off", "part_off", "out_off"):
            sub[field] = 0
        assert sub.tobytes() == alone["blends"].tobytes()
        comps_sub = sp["components"][bl["comp0"]:bl["comp0"] + K].copy()
        comps_sub["morph_off"] -= comps_sub["morph_off"][0]
        assert comps_sub.tobytes() == alone["components"].tobytes()
        assert all(x.tobytes() == y.tobytes()
                   for x, y in zip(alone["morphs"], sp["morphs"][bl["comp0"]:bl["comp0"] + K]))
        assert alone["stamps"][0].tobytes() == sp["stamps"][b].tobytes()
    assert (part_end, out_end, at) == (sp["n_part"], sp["n_out"], len(sp["work"]))
    # the limits, and the loop's screen for identical models
    frame, obs = hand[1][1], hand[1][2]
    many = ic.hand_components(frame, [(12, 14)] * 65)
    assert "65 components" in init.pack_spectra([(0, frame, obs, many)], [0])["loop"][0]
    crowd = [ic.hand_components(frame, [(12, 14)], seed=s)[0] for s in range(33)]
    assert "reach one tile" in init.pack_spectra([(0, frame, obs, crowd)], [0])["loop"][0]
    twins = ic.hand_components(frame, [(12, 14), (5, 5)]) + ic.hand_components(frame, [(12, 14)])
    assert "identical" in init.pack_spectra([(0, frame, obs, twins)], [0])["loop"][0]


def test_numpy_restatement_of_the_normal_equations_equals_the_loop(cat):
    """The weighted normal equations restated in NumPy from the packed tables -- direct taps,
    columns clipped to the frame, sums over the region -- solved by solve_spectra, against
    set_spectra_to_match on hand-built components, both measured against the longdouble
    solution.  The bound of the GPU test: 4 x the loop's distance plus one float32 rounding.
    Measured here, as distances relative to a component's largest band: loop 2.8e-8 .. 4.5e-8,
    restatement the same figures (both are float32 parameters: the rounding of that cast)."""
    from scarlet_amd import initialization as init

    hand = _hand_blends(cat)
    assert len(hand) >= 5
    for name, frame, obs, comps in hand:
        sp = init.pack_spectra([(0, frame, obs, comps)], [0])
        assert sp["loop"] == {}, name
        K = len(comps)
        truth, ratios = ic.longdouble_spectra(sp, 0, obs.data, obs.weights)
        truth = ic.constrained(comps, truth)
        # the cases keep every seen ratio away from 0.1
        assert (np.abs(ratios - 0.1) > 1e-3).all(), name
        sums = ic.normal_equations(sp, 0, obs.data, obs.weights)
        mine = ic.constrained(comps, init.solve_spectra(sums, K, obs.weights).astype(np.float32))
        init.set_spectra_to_match(comps, obs)
        loop = np.array(ic.spectra_of(comps))
        assert loop.dtype == np.float32
        d_loop = ic.spectra_distance(loop, truth)
        d_mine = ic.spectra_distance(mine.astype(np.float32), truth)
        print("%-6s K=%d loop %.3g restatement %.3g" % (name, K, d_loop, d_mine))
        scale = np.abs(truth).max(axis=1, keepdims=True)
        bound = 4 * d_loop * scale + 2.0 ** -24 * np.abs(truth)
        assert (np.abs(mine.astype(np.float32) - truth) <= bound).all(), name


# ---------------------------------------------------------------- validation without a device
def test_entries_refuse_malformed_tables_without_launching():
    """The same malformed tables as the GPU test: the validation answers SMI_ERR_INVALID, with
    the reason meant, before it looks for a device, so this runs anywhere."""
    import test_gpu_init_blends as g

    assert {step for step, _, _, _ in g.BAD} == set(g.GOOD)
    for step, change, sizes, answer in g.BAD:
        status, _lib = g.malformed(step, change, sizes)
        assert status < 0, (step, change)
        message = _lib.load().smi_last_error().decode()
        assert answer in message and "no HIP device" not in message, (step, change, message)
