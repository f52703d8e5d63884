"""scarlet.render_blends on the GPU: the catalogue of tests/render_blends_cases.py against the
float64 oracle, the reference's own runs, the per-call loop and the identities of the ratio rules;
independence of list, order and chunking; the fallback; the validation of the C entry.

Measured on one MI355X (the figures the tests print): the largest error over its bound is 0.989
for a scene, 0.988 for a source's rendering, 0.994 for a flux (the float32 rounding of the value
is nearly all of each bound) and 0.0022 for chi2; the reference's renderings of hsc_cosmos_35 and
render_loss are met to 1.1e-7 and 2.9e-8 of the largest value, their log-likelihoods to 2.0e-8
and 2.2e-12 (relative); the loop lies up to 2.0e-7 of the largest value from the oracle, the
device 5.1e-8."""

import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import render_blends_cases as rc
import render_blends_oracle as ro
from conftest import golden

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # tests/test_gpu_parity.py: renderings, relative to the largest value


@pytest.fixture(scope="module")
def runs():
    """The catalogue, its results in one call with everything asked for, the plans and oracles of
    the device cases: computed once and only read."""
    import scarlet_amd as scarlet
    from scarlet_amd import rendering

    cat = rc.catalogue()
    blends = [b for _, b, _ in cat]
    report = {}
    results = scarlet.render_blends(blends, reweight=True, _report=report)
    groups, _ = scarlet.plan_render_blends(blends)
    device = {}
    for key, idx in groups.items():
        for i in idx:
            if cat[i][2] == "device":
                plan = rendering.plan_blend(blends[i], key)
                device[i] = (key, plan, ro.blend(plan, key))
    return dict(cat=cat, blends=blends, results=results, report=report, device=device)


def _crop(region):
    y0, x0, h, w = region
    return (slice(None), slice(y0, y0 + h), slice(x0, x0 + w))


def _cases(runs):
    """``(name, blend, result, key, plan, oracle)`` of every device case."""
    for i, (key, plan, oracle) in runs["device"].items():
        name, blend, _ = runs["cat"][i]
        yield name, blend, runs["results"][i], key, plan, oracle


def _bytes(res):
    """Every array of a result, in a fixed order, as bytes."""
    parts = list(res["rendered"]) + list(res["residual"]) + list(res["chi2"])
    parts.append(np.float64(res["log_likelihood"]))
    for src in res.get("sources", ()):
        parts += [np.array(src["region"])] + list(src["rendered"]) + list(src.get("flux", ()))
    return [np.ascontiguousarray(p).tobytes() for p in parts]


def test_report_and_shapes(runs):
    report = runs["report"]
    assert report["launches"] == 3 and report["chunks"] == len(report["groups"]) == 7
    assert len(report["launch_ms"]) == 3 and min(report["launch_ms"]) >= 0
    assert sum(report["launch_ms"]) > 0
    assert len(runs["results"]) == len(runs["cat"])
    for name, blend, res, key, plan, oracle in _cases(runs):
        _, H, W = blend.frame.shape
        assert len(res["rendered"]) == len(res["residual"]) == len(res["chi2"]) == len(
            blend.observations)
        for obs, R, r, c in zip(blend.observations, res["rendered"], res["residual"], res["chi2"]):
            assert R.shape == r.shape == (obs.shape[0], H, W) and R.dtype == r.dtype == np.float32
            assert c.shape == (obs.shape[0],) and c.dtype == np.float64
        assert isinstance(res["log_likelihood"], float)
        assert len(res["sources"]) == len(blend.sources)
        for src, planned in zip(res["sources"], plan["regions"]):
            assert src["region"] == tuple(planned)
            for obs, R, f in zip(blend.observations, src["rendered"], src["flux"]):
                assert R.shape == f.shape == (obs.shape[0],) + src["region"][2:], name
                assert R.dtype == f.dtype == np.float32
    (i,) = [i for i, c in enumerate(runs["cat"]) if c[0] == "tiny"]
    null = runs["results"][i]["sources"][2]
    assert null["region"] == (0, 0, 0, 0) and null["rendered"][0].shape == (3, 0, 0)
    assert null["flux"][0].shape == (3, 0, 0)


def test_against_the_oracle(runs):
    """rendered, of the scene and of every source, within one float32 rounding of the value plus
    the float64 sum bound; the flux within the bound of the moved ratio and one rounding more;
    chi2 and the log-likelihood within the bound of chi2's terms; the residual bit for bit."""
    worst = dict(rendered=0.0, source=0.0, flux=0.0, chi2=0.0)
    visited = dict(negative=0, zero_total=0, above=0)
    for name, blend, res, key, plan, o in _cases(runs):
        got = np.concatenate(res["rendered"])
        err = np.abs(got - o["R"])
        assert np.all(err <= o["rendered_bound"]), (name, float((err / o["rendered_bound"]).max()))
        worst["rendered"] = max(worst["rendered"], float((err / o["rendered_bound"]).max()))
        for obs, R, r in zip(blend.observations, res["rendered"], res["residual"]):
            assert r.tobytes() == (obs.data - R).tobytes(), name
        chi2 = np.concatenate(res["chi2"])
        err = np.abs(chi2 - o["chi2"])
        assert np.all(err <= o["chi2_bound"]), (name, err, o["chi2_bound"])
        worst["chi2"] = max(worst["chi2"], float((err / np.maximum(o["chi2_bound"], 1e-300)).max()))
        at, want = 0, 0.0
        for obs in blend.observations:
            want -= obs.log_norm + o["chi2"][at:at + obs.shape[0]].sum() / 2
            at += obs.shape[0]
        bound = o["chi2_bound"].sum() / 2 + 4 * len(chi2) * ro.U * (abs(want) + o["chi2"].sum())
        assert abs(res["log_likelihood"] - want) <= bound, name
        for src, so in zip(res["sources"], o["sources"]):
            if so is None:
                continue
            crop = _crop(so["region"])
            got = np.concatenate(src["rendered"])
            err = np.abs(got - so["R"][crop])
            assert np.all(err <= so["rendered_bound"]), name
            worst["source"] = max(worst["source"], float((err / so["rendered_bound"]).max()))
            got = np.concatenate(src["flux"])
            err = np.abs(got - so["flux"])
            assert np.all(err <= so["flux_bound"]), (name, float((err / so["flux_bound"]).max()))
            worst["flux"] = max(worst["flux"], float((err / so["flux_bound"]).max()))
            if name == "clamped":
                R_k, R_tot = so["R"][crop], o["R"][crop]
                visited["negative"] += int((R_k < 0).sum())
                visited["zero_total"] += int((R_tot <= 0).sum())
                visited["above"] += int(((R_k > R_tot) & (R_tot > 0)).sum())
    assert min(visited.values()) >= 1, visited
    print("largest error over its bound:", {k: "%.3g" % v for k, v in worst.items()})


def test_options_select_outputs_and_keep_the_bits(runs):
    """The defaults return no sources, ``sources=True`` no flux; what they return has the bits of
    the full call.  Without ``mask_footprint`` the image is the data itself: the pixel without
    weight of ``subset null`` gets its share."""
    import scarlet_amd as scarlet

    picked = sorted(runs["device"])
    blends = [runs["blends"][i] for i in picked]
    plain = scarlet.render_blends(blends)
    with_sources = scarlet.render_blends(blends, sources=True)
    unmasked = scarlet.render_blends(blends, reweight=True, mask_footprint=False)
    for i, a, b, c in zip(picked, plain, with_sources, unmasked):
        name, full = runs["cat"][i][0], runs["results"][i]
        assert "sources" not in a and all("flux" not in s for s in b["sources"])
        assert _bytes(a) == _bytes(dict(full, sources=())), name
        stripped = dict(full, sources=[dict(region=s["region"], rendered=s["rendered"])
                                       for s in full["sources"]])
        assert _bytes(b) == _bytes(stripped), name
        key, plan, _ = runs["device"][i]
        o = ro.blend(plan, key, mask_footprint=False)
        for src, so in zip(c["sources"], o["sources"]):
            if so is not None:
                err = np.abs(np.concatenate(src["flux"]) - so["flux"])
                assert np.all(err <= so["flux_bound"]), name
        if name == "subset null":
            masked, free = full["sources"][0]["flux"][0], c["sources"][0]["flux"][0]
            assert masked[0, 1, 1] == 0 and free[0, 1, 1] == blends[picked.index(i)].observations[
                0].data[0, 5, 7] != 0
            differ = masked != free
            assert differ.sum() == 1 and differ[0, 1, 1]


def _facade_blend(scarlet, images, weights, psfs, model_psf, components):
    """A Blend of FactorizedComponents ``(sed, morph, origin)`` on the frame of ``images``."""
    C = images.shape[0]
    channels = ["b%d" % c for c in range(C)]
    frame = scarlet.Frame(images.shape, psf=scarlet.ImagePSF(model_psf), channels=channels)
    obs = scarlet.Observation(images, psf=scarlet.ImagePSF(psfs), weights=weights,
                              channels=channels).match(frame)
    sources = []
    for sed, morph, (oy, ox) in components:
        h, w = morph.shape
        box = scarlet.Box((C, h, w), origin=(0, int(oy), int(ox)))
        sources.append(scarlet.FactorizedComponent(
            frame, scarlet.TabulatedSpectrum(frame, np.asarray(sed, np.float32), bbox=box[0]),
            scarlet.ImageMorphology(frame, np.asarray(morph, np.float64), bbox=box[1:])))
    return scarlet.Blend(sources, [obs])


@pytest.mark.parametrize("name", ["hsc_cosmos_35", "render_loss"])
def test_against_the_reference(name):
    """The reference's own runs, rebuilt through the facade: ``rendered`` within 1e-5 of the
    largest value of the golden rendering, the log-likelihood within 1e-5 of the golden one (the
    tolerances of test_hsc_forward_vs_golden_and_oracle)."""
    import scarlet_amd as scarlet

    g = golden(name)
    if name == "hsc_cosmos_35":
        comps = [(g["sed_%d" % k], g["morph_%d" % k], g["origin_%d" % k])
                 for k in range(int(g["n_comp"]))]
        blend = _facade_blend(scarlet, g["images"], g["weights"], g["psfs"].copy(),
                              g["model_psf"].copy(), comps)
    else:  # a model cube: one component per band with a unit spectrum
        C = g["model"].shape[0]
        comps = [(np.eye(C)[c], g["model"][c], (0, 0)) for c in range(C)]
        blend = _facade_blend(scarlet, g["images"].astype(np.float32), None, g["obs_psf"].copy(),
                              g["model_psf"].copy(), comps)
    report = {}
    (res,) = scarlet.render_blends([blend], _report=report)
    assert report["fallback"] == [] and report["chunks"] == 1
    (rendered,) = res["rendered"]
    err = np.abs(rendered.astype(np.float64) - g["rendered"]).max() / np.abs(g["rendered"]).max()
    logL = float(g["logL"])
    print("%s: rendered %.3g of the largest value, log-likelihood %.3g relative"
          % (name, err, abs(res["log_likelihood"] - logL) / abs(logL)))
    assert err < RTOL
    assert abs(res["log_likelihood"] - logL) < 1e-5 * abs(logL)


def test_against_the_loop(runs):
    """``obs.render(blend.get_model())`` and ``obs.render(src.get_model(frame=...))`` on the
    region render in float32 through the FFT: within 1e-5 of the largest value."""
    from scarlet_amd import rendering

    loop_worst = device_worst = 0.0
    for name, blend, res, key, plan, o in _cases(runs):
        frame = blend.frame
        scale = np.abs(o["R"]).max()
        at = 0
        for obs, got in zip(blend.observations, res["rendered"]):
            n = obs.shape[0]
            want = rendering._host_render(obs, blend.get_model())
            assert np.abs(got - want).max() < RTOL * scale, name
            loop_worst = max(loop_worst, np.abs(want - o["R"][at:at + n]).max() / scale)
            device_worst = max(device_worst, np.abs(got - o["R"][at:at + n]).max() / scale)
            at += n
        for src, got, so in zip(blend.sources, res["sources"], o["sources"]):
            if so is None:
                continue
            crop = _crop(so["region"])
            full = src.get_model(frame=frame)
            own = np.abs(so["R"]).max()  # (the source's own largest value: the smaller scale)
            for obs, R in zip(blend.observations, got["rendered"]):
                want = rendering._host_render(obs, full)[crop]
                assert np.abs(R - want).max() < RTOL * own, name
    print("largest distance from the oracle over the largest value: loop %.3g, device %.3g"
          % (loop_worst, device_worst))


def test_identities(runs):
    """``alone``: the flux is the image wherever the rendering is positive.  ``apart``: exact
    zeros in the middle; no flux wherever the scene is zero.  ``tiles``: positive models, so the
    fluxes of all sources add up to the image within one float32 rounding per source."""
    by_name = {name: (blend, res, o) for name, blend, res, _, _, o in _cases(runs)}

    blend, res, o = by_name["alone"]
    (src,), (so,) = res["sources"], o["sources"]
    crop = _crop(src["region"])
    positive = so["R"][crop] > 4 * so["R_bound"]  # (positive on the device as well)
    assert positive.sum() > 100
    image = o["image"].astype(np.float32)[crop]
    assert_array_equal(src["flux"][0][positive], image[positive])

    blend, res, o = by_name["apart"]
    middle = (slice(None),) + rc.MIDDLE
    assert not res["rendered"][0][middle].any()
    assert_array_equal(res["residual"][0][middle], blend.observations[0].data[middle])
    n_dark = 0
    for src in res["sources"]:
        crop = _crop(src["region"])
        dark = o["R"][crop] == 0
        n_dark += int(dark.sum())
        assert not src["flux"][0][dark].any()
        assert np.all(blend.observations[0].data[crop][dark] != 0)  # (there was flux to share)
    assert n_dark >= 1

    blend, res, o = by_name["tiles"]
    total = np.zeros(o["image"].shape)
    covered = np.zeros(o["image"].shape, bool)
    unclamped = np.ones(o["image"].shape, bool)
    slack = o["R_bound"].copy()
    for src, so in zip(res["sources"], o["sources"]):
        crop = _crop(src["region"])
        total[crop] += np.concatenate(src["flux"]).astype(np.float64)
        covered[crop] = True
        unclamped[crop] &= so["R"][crop] > 4 * so["R_bound"]
        slack[crop] += so["R_bound"]
    lit = covered & unclamped & (o["R"] > 4 * o["R_bound"])
    assert lit.sum() > 400
    # Where nothing is clamped the ratios are R_k / R, and the R_k add up to R within `slack`, the
    # bounds of all of them (R itself at least 3 / 4 of the oracle's): the ratios add up to 1
    # within 4 slack / R.  Every flux carries a division, a product and one float32 rounding of
    # its own share of the image: n_sources float32 roundings bound them all.
    n = len(res["sources"])
    bound = np.abs(o["image"]) * (n * ro.U32 + 4 * n * ro.U + 4 * slack / o["R"].clip(1e-300))
    assert np.all(np.abs(total - o["image"])[lit] <= bound[lit])


def test_alone_in_chunks_and_reversed(runs):
    """A blend's outputs have the same bits alone, in the whole catalogue, with every blend a
    chunk of its own, with two blends to a chunk, and in the reversed list."""
    import scarlet_amd as scarlet
    from scarlet_amd import _catalog, rendering

    blends, results = runs["blends"], runs["results"]
    device = sorted(runs["device"])
    want = {i: _bytes(results[i]) for i in device}
    for i in device:
        (alone,) = scarlet.render_blends([blends[i]], reweight=True)
        assert _bytes(alone) == want[i], runs["cat"][i][0]
    picked = [blends[i] for i in device]
    report = {}
    for i, res in zip(device, scarlet.render_blends(picked, reweight=True, _working_set_bytes=1,
                                                    _report=report)):
        assert _bytes(res) == want[i], runs["cat"][i][0]
    assert report["fallback"] == [] and report["chunks"] == len(device)
    key = (3, 5, 5)
    group = [i for i in device if runs["device"][i][0] == key]
    flags = rendering.SOURCES | rendering.REWEIGHT | rendering.MASK
    need = [rendering._plan_bytes(runs["device"][i][1], key, flags) for i in group]
    assert len(group) == 5
    budget = need[0] + need[1]  # holds the first two blends, not three
    chunks = _catalog.chunks(list(zip(group, need)), budget)
    assert chunks[0] == group[:2] and sum(chunks, []) == group
    report = {}
    for i, res in zip(group, scarlet.render_blends([blends[i] for i in group], reweight=True,
                                                   _working_set_bytes=budget, _report=report)):
        assert _bytes(res) == want[i], runs["cat"][i][0]
    assert report["chunks"] == len(chunks) >= 2
    for i, res in zip(device[::-1], scarlet.render_blends(picked[::-1], reweight=True)):
        assert _bytes(res) == want[i], runs["cat"][i][0]


def test_source_renderings_are_the_ones_measure_blends_sums(runs):
    """A source's rendering has the bits ``measure_blends`` sums: summed in any order in float64
    the float32 images give ``rendered_flux`` within the roundings of the images."""
    import scarlet_amd as scarlet

    picked = [i for i in sorted(runs["device"]) if runs["cat"][i][0] in ("tiles", "lobes", "six")]
    tables = scarlet.measure_blends([runs["blends"][i] for i in picked])
    for i, table in zip(picked, tables):
        res = runs["results"][i]
        for row, src in zip(table, res["sources"]):
            images = np.concatenate(src["rendered"]).astype(np.float64)
            n = images[0].size
            bound = (ro.U32 + (n + 4) * ro.U) * np.abs(images).sum(axis=(1, 2))
            assert np.all(np.abs(images.sum(axis=(1, 2)) - row["rendered_flux"]) <= bound)


def test_fallback_results_and_report(runs):
    """Refused blends and the one whose values are not finite come back from the host loop in
    position; ``_report`` names them with the reasons of ``plan_render_blends``."""
    import scarlet_amd as scarlet
    from scarlet_amd import rendering

    cat, twin = runs["cat"], rc.catalogue()
    fallback = runs["report"]["fallback"]
    _, refused = scarlet.plan_render_blends(runs["blends"])
    assert [cat[i][0] for i, _ in fallback] == [n for n, _, e in cat if e != "device"]
    for i, why in fallback:
        if cat[i][2] == "runtime":
            assert why == "at run time: a model value that is not finite"
        else:
            assert why == refused[i] and why.startswith(cat[i][2])
        want = rendering.render_blend_host(twin[i][1], reweight=True)
        got = runs["results"][i]
        assert sorted(got) == sorted(want)
        for field in ("rendered", "residual", "chi2"):
            for a, b in zip(got[field], want[field]):
                assert_array_equal(a, b, err_msg="%s %s" % (cat[i][0], field))
        assert_array_equal(got["log_likelihood"], want["log_likelihood"])
        for a, b in zip(got["sources"], want["sources"]):
            assert a["region"] == b["region"]
            for field in ("rendered", "flux"):
                for x, y in zip(a[field], b[field]):
                    assert_array_equal(x, y, err_msg="%s %s" % (cat[i][0], field))


def test_c_entry_validates_before_any_launch(runs):
    """Each descriptor field out of range, each buffer one element short, an even stamp and a
    stamp of 65: an error, and the outputs untouched.  The tables are checked on the host; nothing
    is launched."""
    from scarlet_amd import _lib, rendering

    lib = _lib.load()
    key = (3, 5, 5)
    names = [c[0] for c in runs["cat"]]
    plans = [runs["device"][names.index(n)][1] for n in ("tiny", "list map")]
    flags = rendering.SOURCES | rendering.REWEIGHT | rendering.MASK
    packed = rendering.pack(plans, key, flags)
    sizes = dict(rendered=packed["n_out"], residual=packed["n_out"], chi2=len(packed["bands"]),
                 source_rendered=packed["n_source_out"], flux=packed["n_source_out"])
    outputs = (("rendered", ctypes.c_float), ("residual", ctypes.c_float),
               ("chi2", ctypes.c_double), ("source_rendered", ctypes.c_float),
               ("flux", ctypes.c_float))

    def call(key=key, flags=flags, short=None, **tables):
        p = dict(packed, **tables)
        out = {name: np.full(sizes[name], -7, np.float64 if ct is ctypes.c_double else np.float32)
               for name, ct in outputs}
        args = [0, *key, flags]
        for name in ("blends", "sources", "comps", "bands"):
            args += [len(p[name]), p[name].ctypes.data]
        for name, ct in (("seds", ctypes.c_double), ("morphs", ctypes.c_double),
                         ("stamps", ctypes.c_float), ("data", ctypes.c_float),
                         ("weights", ctypes.c_float)):
            args += [_lib.ptr(p[name], ct), p[name].size - (short == name)]
        for name, ct in outputs:
            args += [_lib.ptr(out[name], ct), out[name].size - (short == name)]
        rc_ = lib.smi_render_sources_f32(*args, None)
        return rc_, all(np.all(a == -7) for a in out.values())

    rc_, untouched = call()
    assert rc_ == 0 and not untouched  # the tables themselves are good
    n_out, n_src = packed["n_out"], packed["n_source_out"]
    bad = []
    for field, table, row, value in (
            ("morph_off", "comps", -1, packed["morphs"].size), ("sed_off", "comps", 0, -1),
            ("h", "comps", 2, 0), ("w", "comps", 2, 1 << 15), ("y0", "comps", 1, -2),
            ("x0", "comps", 1, 1 << 25),
            ("weight_off", "bands", 2, packed["weights"].size - 98),
            ("stamp_off", "bands", 1, packed["stamps"].size - 24), ("channel", "bands", 0, 3),
            ("channel", "bands", 4, -1),
            ("fh", "blends", 0, 0), ("fw", "blends", 1, 32), ("fh", "blends", 1, 1 << 25),
            ("comp0", "blends", 1, 5), ("n_comp", "blends", 0, 7), ("band0", "blends", 1, 2),
            ("n_band", "blends", 0, 2), ("n_band", "blends", 1, 3), ("n_band", "blends", 1, -1),
            ("out_off", "blends", 1, n_out - 2 * 775 + 1), ("out_off", "blends", 0, -1),
            ("blend", "sources", 0, 2), ("blend", "sources", 5, -1), ("h", "sources", 1, 0),
            ("w", "sources", 1, 1 << 15), ("y0", "sources", 3, -(1 << 25)),
            ("x0", "sources", 0, -2), ("comp0", "sources", 3, 4), ("comp0", "sources", 4, 3),
            ("n_comp", "sources", 0, 0), ("n_comp", "sources", 5, 2),
            ("out_off", "sources", 5, n_src - 2 * 121 + 1), ("out_off", "sources", 2, -1)):
        changed = packed[table].copy()
        changed[field][row] = value
        bad.append(("%s.%s[%d] = %d" % (table, field, row, value), call(**{table: changed})))
    bad.append(("65", call(key=(3, 65, 5))))
    bad.append(("even", call(key=(3, 4, 5))))
    bad.append(("stamp shape beyond the buffer", call(key=(3, 5, 7))))
    bad.append(("no bands", call(key=(0, 5, 5))))
    bad.append(("unknown flag", call(flags=flags | 8)))
    bad.append(("sources without the flag", call(flags=rendering.MASK)))
    for name in ("seds", "morphs", "stamps", "data", "weights", "rendered", "residual", "chi2",
                 "source_rendered", "flux"):
        bad.append((name + " one short", call(short=name)))
    for what, (rc_, untouched) in bad:
        assert rc_ < 0 and untouched, what
