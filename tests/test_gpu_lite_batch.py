"""Ragged frames (smi_batch_set_frame_extents) and scarlet_amd.lite.fit_blends: blends of
different frame sizes in one device batch give what each blend gives alone."""

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ C ABI: frame extents
def _specs(g):
    from scarlet_amd import ComponentSpec

    return [ComponentSpec(g["sed_%d" % k].astype(np.float32), g["morph_%d" % k].astype(np.float32),
                          tuple(int(v) for v in g["origin_%d" % k]),
                          sed_min_step=g["min_step_%d" % k].astype(np.float32))
            for k in range(int(g["n_comp"]))]


def _crop(g, h, w):
    return (np.ascontiguousarray(g["images"][:, :h, :w], np.float32),
            np.ascontiguousarray(g["weights"][:, :h, :w], np.float32))


@pytest.mark.parametrize("conv_path,fft_shape", [("fused", (96, 96)), ("rocfft", (120, 108))])
def test_frame_extents_match_unpadded_batches(hsc, conv_path, fft_shape):
    from scarlet_amd import BlendBatch, _lib

    g = golden("hsc_cosmos_35")
    kernel = g["diff_kernel"].astype(np.float32)
    frames = [(58, 48), (52, 40)]  # the quickstart blend and a crop of it
    # (+6 rows: the padded frame keeps the fused kernel's variant -- its count of all-padding
    # blocks -- which lite.fit_blends groups by)
    H, W = 58 + 6, 48 + 13
    data = np.full((2, 5, H, W), 3.0, np.float32)  # finite, non-zero padding of weight 0
    weights = np.zeros_like(data)
    for b, (h, w) in enumerate(frames):
        data[b, :, :h, :w], weights[b, :, :h, :w] = _crop(g, h, w)
    # components overhang the true bottom and right edges of both frames
    assert any(o[0] + m.shape[0] > 52 for o, m in ((c.origin, c.morph) for c in _specs(g)))
    ragged = BlendBatch(data, weights, [_specs(g), _specs(g)], kernel=kernel, max_iter=8,
                        fft_shape=fft_shape, conv_path=conv_path, log_norm=False,
                        frame_shapes=frames)
    assert ragged.fft_shape == fft_shape and ragged.conv_path == conv_path
    m_r, r_r, logL_r = ragged.forward()
    gs_r, gm_r = ragged.gradient()
    ragged.step(0, 5, e_rel=1e-3)
    sed_r, morph_r = ragged.parameters()
    loss_r = ragged.loss_history()
    n = int(g["n_comp"])
    for b, (h, w) in enumerate(frames):
        d, wt = _crop(g, h, w)
        one = BlendBatch(d[None], wt[None], [_specs(g)], kernel=kernel, max_iter=8,
                         fft_shape=fft_shape, conv_path=conv_path, log_norm=False)
        m, r, logL = one.forward()
        np.testing.assert_array_equal(m_r[b, :, :h, :w], m[0])
        np.testing.assert_array_equal(r_r[b, :, :h, :w], r[0])
        np.testing.assert_allclose(logL_r[b], logL[0], rtol=1e-9)
        gs, gm = one.gradient()
        np.testing.assert_array_equal(gs_r[b * n:(b + 1) * n], gs)
        for k in range(n):
            np.testing.assert_array_equal(gm_r[b * n + k], gm[k])
        one.step(0, 5, e_rel=1e-3)
        sed, morph = one.parameters()
        np.testing.assert_array_equal(sed_r[b * n:(b + 1) * n], sed)
        for k in range(n):
            np.testing.assert_array_equal(morph_r[b * n + k], morph[k])
        np.testing.assert_allclose(loss_r[b], one.loss_history()[0], rtol=1e-9)
        one.close()
    # combinations the extents do not cover are refused
    with pytest.raises(_lib.ScarletAmdError):
        ragged.resize_test()
    if conv_path == "fused":
        with pytest.raises(_lib.ScarletAmdError):
            ragged.add_observation(data, weights, kernel)
    with pytest.raises(_lib.ScarletAmdError):
        ragged.set_frame_extents([(H + 1, W), (1, 1)])
    ragged.close()


def test_fft_shape_for_agrees_with_the_batch(hsc):
    from scarlet_amd import BlendBatch
    from scarlet_amd.batch import fft_shape_for

    g = golden("hsc_cosmos_35")
    kernel = g["diff_kernel"].astype(np.float32)
    for h, w in ((58, 48), (52, 40), (20, 90)):
        d, wt = _crop(g, h, w) if w <= 48 else (np.ones((5, h, w), np.float32),) * 2
        for path in ("auto", "rocfft"):
            batch = BlendBatch(d[None], wt[None], [_specs(g)[:1]], kernel=kernel, max_iter=1,
                               conv_path=path)
            assert batch.fft_shape == fft_shape_for(h, w, kernel.shape, path), (h, w, path)
            batch.close()


# ------------------------------------------------------------------ lite.fit_blends
def _quickstart_blend(g, kind, h, w):
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images, weights = _crop(g, h, w)
    variance = (1 / weights).astype(np.float32)
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    obs = lite.LiteObservation(images, variance, weights, g["psfs"].astype(np.float32),
                               model_psf=model_psf[0][None])
    init = lite.init_fista_component if kind == "fista" else lite.init_adaprox_component
    sources = []
    for k in range(int(g["n_comp"])):
        morph = g["morph_%d" % k].astype(np.float32)
        oy, ox = (int(v) for v in g["origin_%d" % k])
        mh, mw = morph.shape
        assert oy + mh // 2 < h and ox + mw // 2 < w
        bbox = scarlet.Box((5, mh, mw), origin=(0, oy, ox))
        comp = init((oy + mh // 2, ox + mw // 2), bbox, g["sed_%d" % k].astype(np.float32).copy(),
                    morph.copy(), obs, bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    return lite.LiteBlend(sources, obs)


def _synthetic_blend(seed, kind, h, w):
    import scarlet_amd as scarlet
    from scarlet_amd import lite, synthetic

    s = synthetic.make_blend(seed)
    images = np.ascontiguousarray(s["data"][:, :h, :w], np.float32)
    weights = np.ascontiguousarray(s["weights"][:, :h, :w], np.float32)
    psfs = np.repeat(s["obs_psf"], images.shape[0], axis=0).astype(np.float32)
    obs = lite.LiteObservation(images, (1 / weights).astype(np.float32), weights, psfs,
                               model_psf=s["model_psf"].astype(np.float32))
    init = lite.init_fista_component if kind == "fista" else lite.init_adaprox_component
    sources = []
    for k in range(len(s["morphs"])):
        morph = np.asarray(s["morphs"][k], np.float32)
        oy, ox = (int(v) for v in s["origins"][k])
        mh, mw = morph.shape
        if not (0 <= oy + mh // 2 < h and 0 <= ox + mw // 2 < w):
            continue
        bbox = scarlet.Box((images.shape[0], mh, mw), origin=(0, oy, ox))
        comp = init((oy + mh // 2, ox + mw // 2), bbox, np.asarray(s["seds"][k], np.float32).copy(),
                    morph.copy(), obs, bg_thresh=0.25)
        sources.append(lite.LiteSource([comp], images.dtype))
    return lite.LiteBlend(sources, obs)


QUICKSTART_CROPS = [(58, 48), (54, 44), (52, 40), (56, 42), (58, 40)]
SYNTHETIC_CROPS = [(1, 64, 72), (2, 60, 56)]


def _blends(kind, same_shape=False):
    g = golden("hsc_cosmos_35")
    if same_shape:
        return [_quickstart_blend(g, kind, 58, 48) for _ in range(3)]
    out = [_quickstart_blend(g, kind, h, w) for h, w in QUICKSTART_CROPS]
    out += [_synthetic_blend(seed, kind, h, w) for seed, h, w in SYNTHETIC_CROPS]
    return out


def _state(blend, kind):
    out = []
    for c in blend.components:
        out.append(("box", (tuple(c.bbox.origin), tuple(c.bbox.shape))))
        for p in (c._sed, c._morph):
            names = ("x", "z", "t") if kind == "fista" else ("x", "m", "v", "vhat")
            out.extend((n, np.asarray(getattr(p, n))) for n in names)
    return out


def _assert_same(a, b, kind, loss_rtol=1e-9):
    assert a.it == b.it and len(a.loss) == len(b.loss)
    np.testing.assert_allclose(a.loss, b.loss, rtol=loss_rtol)
    for (na, va), (nb, vb) in zip(_state(a, kind), _state(b, kind)):
        assert na == nb
        if na == "box":
            assert va == vb
        else:
            np.testing.assert_array_equal(va, vb, err_msg=na)


@pytest.mark.parametrize("kind", ["fista", "adaprox"])
def test_fit_blends_equals_single_fits(kind):
    from scarlet_amd import lite
    from scarlet_amd.lite.fitting import group_keys

    e_rel = 1e-3
    batched, single = _blends(kind), _blends(kind)
    keys = group_keys(batched, 30, e_rel)
    shapes = {b.observation.images.shape for b in batched}
    assert len(shapes) >= 3
    assert any(len({b.observation.images.shape for b, k in zip(batched, keys) if k == key}) > 1
               for key in keys)  # some device batches mix frame sizes
    out = lite.fit_blends(batched, 30, e_rel=e_rel, resize=10)
    ref = []
    for b in single:
        try:
            ref.append(b.fit(30, e_rel=e_rel, resize=10))
        except ArithmeticError:  # (fit_blends reports it and goes on)
            ref.append(None)
    failed = {i for i, r in enumerate(ref) if r is None}
    assert {i for i, _ in lite.fit_blends.errors} == failed
    assert len(failed) < len(single) // 2
    its = [b.it for i, b in enumerate(single) if i not in failed]
    print("iterations", kind, [b.it for b in single], "failed", sorted(failed))
    assert min(its) < 30 and max(its) == 30  # some stop early, others run to max_iter
    for i, ((it, loss), a, b) in enumerate(zip(out, batched, single)):
        if i in failed:
            assert np.isnan(loss)
            continue
        assert (it, loss) == (b.it, b.loss[-1]) and it == ref[i][0]
        np.testing.assert_allclose(loss, ref[i][1], rtol=1e-9)
        _assert_same(a, b, kind)
    # a second call continues where the first stopped
    ok = [i for i in range(len(single)) if i not in failed]
    lite.fit_blends([batched[i] for i in ok], 45, e_rel=e_rel, resize=10)
    for i in ok:
        single[i].fit(45, e_rel=e_rel, resize=10)
        _assert_same(batched[i], single[i], kind)


@pytest.mark.parametrize("kind", ["fista", "adaprox"])
def test_fit_blends_same_shape_is_bit_identical(kind):
    from scarlet_amd import lite

    batched, single = _blends(kind, True), _blends(kind, True)
    lite.fit_blends(batched, 20, e_rel=1e-9, resize=10)
    for b in single:
        b.fit(20, e_rel=1e-9, resize=10)
    for a, b in zip(batched, single):
        assert a.loss == b.loss
        _assert_same(a, b, kind, loss_rtol=0)


def test_fit_blends_partitions_do_not_matter():
    from scarlet_amd import lite

    one, two = _blends("adaprox"), _blends("adaprox")
    r1 = lite.fit_blends(one, 25, e_rel=1e-3, resize=10, devices=None)
    r2 = lite.fit_blends(two, 25, e_rel=1e-3, resize=10, devices=[0, 0])
    failed = {i for i, r in enumerate(r1) if np.isnan(r[1])}
    assert failed == {i for i, r in enumerate(r2) if np.isnan(r[1])}
    for i, (a, b) in enumerate(zip(one, two)):
        if i in failed:  # (its state depends on when its batch mates resized)
            continue
        assert r1[i] == r2[i] and a.loss == b.loss
        _assert_same(a, b, "adaprox", loss_rtol=0)


def test_fit_blends_refuses_before_touching_any_blend():
    from scarlet_amd import lite
    from scarlet_amd.bbox import Box

    assert lite.fit_blends([], 10) == []
    blends = _blends("adaprox")[:3]
    before = [(b.it, list(b.loss), [c.sed.copy() for c in b.components]) for b in blends]
    bad = blends[2]
    bad.components[0].floor = 1e-10  # LiteBlend._spec refuses it
    with pytest.raises(NotImplementedError):
        lite.fit_blends(blends, 10)
    bad.components[0].floor = 1e-20
    obs = bad.observation
    obs.bbox = Box(obs.images.shape, origin=(0, 3, 0))
    with pytest.raises(NotImplementedError):
        lite.fit_blends(blends, 10)
    for b, (it, loss, seds) in zip(blends, before):
        assert b.it == it and b.loss == loss
        for c, s in zip(b.components, seds):
            np.testing.assert_array_equal(c.sed, s)
