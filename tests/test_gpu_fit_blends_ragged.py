"""``fit_blends`` with frames of different sizes on the GPU (scenes: fit_blends_ragged_cases.py).

C level: a ``BlendBatch`` with frame extents for all kinds (``frame_kinds="all"``) gives every
blend, whatever kinds of components it holds, the bits of its own unpadded batch.  Facade: a
blend fitted in a ragged list is bit for bit the blend ``Blend.fit`` fits alone -- loss history, parameters, moments, boxes.

Summation orders: on the fused convolution path the loss of a band is summed per thread over
row pairs in an order that does not depend on the padded frame, and the normalisation term is
summed over the own frame (``log_norm_extents_kernel``), so losses are equal bit for bit and are
held to that.  On the rocFFT path ``residual_kernel`` cuts the pixels of the PADDED
plane into blocks of 256, so the partial sums of the loss group other pixels than in the
unpadded batch: there the loss (and only the loss) is held to rtol 1e-9, the bound
tests/test_gpu_lite_batch.py::test_frame_extents_match_unpadded_batches uses for it."""

import copy

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import fit_blends_ragged_cases as fc

pytestmark = pytest.mark.gpu

N_ITER = 25  # past the resize hooks after iterations 11 and 22 (of a call that restarted)
E_REL = 1e-6


# ------------------------------------------------------------------ C ABI: every component kind
def _pair(kind):
    """Two blends of scene A (31 x 24 and 27 x 29) as ``_Run``s: cubes and specs."""
    from scarlet_amd.fitting import _classify

    blends = [fc.make_blend(fc.FRAMES[i], 100 + i, kind) for i in (0, 3)]
    runs = []
    for b in blends:
        why, run = _classify(b)
        assert why is None
        runs.append(run)
    return runs


def _state(batch):
    """Everything a step changes, of every kind of component: arrays with a row per component,
    and arrays of single components under ``name@k``."""
    sed, morph = batch.parameters()
    out = dict(sed=sed)
    out.update({"morph@%d" % k: m for k, m in enumerate(morph)})
    out.update({"model_morph@%d" % k: m for k, m in enumerate(batch.model_morphologies())})
    out.update({"center_" + k: v for k, v in batch.centers().items()})
    if batch._star:
        for name, planes in batch.starlet_state().items():
            if name != "components":
                out.update({"star_%s@%d" % (name, k): p for k, p in zip(batch._star, planes)})
    if batch._profile:
        out.update({"prof_" + k: v for k, v in batch.profile_state().items() if k != "components"})
    return out


def _rows(state, lo, hi):
    """The entries of ``_state`` that belong to components [lo, hi), counted from ``lo``."""
    out = {}
    for name, value in state.items():
        if "@" not in name:
            out[name] = value[lo:hi]
            continue
        base, k = name.split("@")
        if lo <= int(k) < hi:
            out["%s@%d" % (base, int(k) - lo)] = value
    return out


@pytest.mark.parametrize("conv_path", ["fused", "rocfft"])
@pytest.mark.parametrize("kind", fc.KINDS)
def test_frame_extents_match_unpadded_batches_for_every_kind(kind, conv_path):
    from scarlet_amd import BlendBatch
    from scarlet_amd.batch import _conv_plan, fft_shape_for
    from scarlet_amd.fitting import _pad_cubes

    runs = _pair(kind)
    frames = [r.obs[0].shape[1:] for r in runs]
    H, W = max(f[0] for f in frames), max(f[1] for f in frames)
    assert (H, W) not in frames  # both blends are padded
    kernel = runs[0].obs[2]
    if conv_path == "fused":
        plans = {_conv_plan(h, w, kernel.shape) for h, w in frames + [(H, W)]}
        assert len(plans) == 1
        fft_shape = tuple(plans.pop()[1:3])
    else:
        fft_shape = fft_shape_for(H, W, kernel.shape, "rocfft")
    data = _pad_cubes([r.obs[0] for r in runs])
    data[0, :, :, frames[0][1]:] = 3.0  # finite, non-zero padding of weight 0
    data[1, :, frames[1][0]:, :] = -2.0
    weights = _pad_cubes([r.obs[1] for r in runs])
    kw = dict(kernel=kernel, max_iter=8, fft_shape=fft_shape, conv_path=conv_path)
    ragged = BlendBatch(data, weights, [r.specs for r in runs], frame_shapes=frames,
                        frame_kinds="all", **kw)
    assert ragged.fft_shape == fft_shape and ragged.conv_path == conv_path
    n = [len(r.specs) for r in runs]
    first = [0, n[0], n[0] + n[1]]

    m_r, r_r, logL_r = ragged.forward()
    gs_r, gm_r = ragged.gradient()
    grad_r = _state(ragged)
    ragged.step(0, 5, e_rel=1e-3)
    after_r = _state(ragged)
    loss_r = ragged.loss_history()
    margin_r, pull_r = ragged.resize_test()
    for b, (run, (h, w)) in enumerate(zip(runs, frames)):
        lo, hi = first[b], first[b + 1]
        one = BlendBatch(run.obs[0][None], run.obs[1][None], [run.specs], **kw)
        m, r, logL = one.forward()
        assert_array_equal(m_r[b, :, :h, :w], m[0])
        assert not m_r[b, :, h:, :].any() and not m_r[b, :, :, w:].any()  # nothing rendered beyond
        assert_array_equal(r_r[b, :, :h, :w], r[0])
        gs, gm = one.gradient()
        assert_array_equal(gs_r[lo:hi], gs)
        for k in range(n[b]):
            assert_array_equal(gm_r[lo + k], gm[k])
        # no gradient from beyond the own frame: the image components' boxes (the second one
        # crosses the bottom and the right edge)
        crossing = 0
        for k in range(3):
            oy, ox = run.specs[k].origin
            bh, bw = run.specs[k].morph.shape
            yy, xx = np.mgrid[oy:oy + bh, ox:ox + bw]
            beyond = (yy >= h) | (xx >= w)
            crossing += int(beyond.any())
            assert not gm_r[lo + k][beyond].any()
            assert gm_r[lo + k][~beyond].any()
        assert crossing >= 1
        want = _state(one)
        got = _rows(grad_r, lo, hi)
        assert sorted(got) == sorted(want)
        for name, value in got.items():
            assert_array_equal(value, want[name], err_msg="gradient() %s" % name)
        one.step(0, 5, e_rel=1e-3)
        want = _state(one)
        got = _rows(after_r, lo, hi)
        assert sorted(got) == sorted(want)
        for name, value in got.items():
            assert_array_equal(value, want[name], err_msg="step() %s" % name)
        print(kind, conv_path, b, "logL", logL_r[b], logL[0], "loss", loss_r[b], one.loss_history()[0])
        if conv_path == "fused":
            assert logL_r[b] == logL[0]
            assert_array_equal(loss_r[b], one.loss_history()[0])
        else:  # (module docstring: the blocks of the loss's partial sums follow the padded plane)
            assert_allclose(logL_r[b], logL[0], rtol=1e-9)
            assert_allclose(loss_r[b], one.loss_history()[0], rtol=1e-9)
        # the resize test reads a component's own box, moments and step
        margin, pull = one.resize_test()
        assert_array_equal(margin_r[lo:hi], margin)
        assert_array_equal(pull_r[lo:hi], pull)
        one.close()
    ragged.close()


def test_the_narrower_extents_keep_their_contract():
    """``frame_kinds="image"``, the default and the lite loop's call: image components only, no
    resize test -- what callers of ``smi_batch_set_frame_extents`` have relied on."""
    from scarlet_amd import BlendBatch, _lib
    from scarlet_amd.fitting import _pad_cubes

    for kind in ("image", "point", "shifting", "starlet"):
        runs = _pair(kind)
        frames = [r.obs[0].shape[1:] for r in runs]
        args = (_pad_cubes([r.obs[0] for r in runs]), _pad_cubes([r.obs[1] for r in runs]),
                [r.specs for r in runs])
        kw = dict(kernel=runs[0].obs[2], max_iter=2, frame_shapes=frames)
        if kind == "image":
            batch = BlendBatch(*args, **kw)
            with pytest.raises(_lib.ScarletAmdError, match="resize_test"):
                batch.resize_test()
            batch.close()
            continue
        with pytest.raises(_lib.ScarletAmdError, match="frame extents"):
            BlendBatch(*args, **kw)
    runs = _pair("profile")
    with pytest.raises(NotImplementedError, match="frame extents"):
        BlendBatch(_pad_cubes([r.obs[0] for r in runs]), _pad_cubes([r.obs[1] for r in runs]),
                   [r.specs for r in runs], kernel=runs[0].obs[2],
                   frame_shapes=[r.obs[0].shape[1:] for r in runs])


# ------------------------------------------------------------------ fit_blends
def _fit_alone(blends, skip=()):
    """Deep copies of ``blends``, each fitted by ``Blend.fit``: (copies, results)."""
    copies = [copy.deepcopy(b) for b in blends]
    results = [None if i in skip else c.fit(N_ITER, e_rel=E_REL) for i, c in enumerate(copies)]
    return copies, results


def _crossing(blend, frame):
    """The components whose box reaches beyond the blend's own frame."""
    from scarlet_amd.blend import _flatten

    out = []
    for c in _flatten(blend.sources):
        box = c.children[1].bbox
        (y0, x0), (bh, bw) = box.origin[-2:], box.shape[-2:]
        if y0 + bh > frame[0] or x0 + bw > frame[1]:
            out.append((bh, bw))
    return out


def test_ragged_scene_a_is_one_batch_and_equals_the_solo_fits():
    import scarlet_amd as scarlet

    blends = fc.scene_a(fifth=False)
    before = [_crossing(b, f) for b, f in zip(blends, fc.FRAMES)]
    alone, want = _fit_alone(blends)
    report = {}
    got = scarlet.fit_blends(blends, N_ITER, e_rel=E_REL, _report=report)
    assert scarlet.fit_blends.errors == []
    assert report["batches"] == 1 and report["alone"] == {}
    assert [idx for _, idx in report["groups"]] == [[0, 1, 2, 3]]
    assert report["groups"] == scarlet.plan_fit_blends(fc.scene_a(fifth=False), N_ITER)[0]
    assert got == want
    for i, (a, b) in enumerate(zip(blends, alone)):
        fc.assert_same_fit(a, b, "blend %d" % i)
    # the scene does what it was built for: boxes have grown across their own frame's edges
    after = [_crossing(b, f) for b, f in zip(blends, fc.FRAMES)]
    assert all(b == [(11, 11)] for b in before)
    grown = [(21, 21) in a for a in after]
    print("boxes beyond their own frame after the fit:", after)
    assert all(grown)
    # with the fifth blend: its own plan, its own batch
    five = fc.scene_a()
    scarlet.fit_blends(five, 12, e_rel=E_REL, _report=report)
    assert report["batches"] == 2 and [idx for _, idx in report["groups"]] == [[0, 1, 2, 3], [4]]


@pytest.mark.parametrize("kind", [k for k in fc.KINDS if k != "image"])
def test_ragged_variants_equal_the_solo_fits(kind):
    """Point sources and free shifts (a batch per round, ``_fit_group_rebuilt``), starlet and
    profile components: one group, every blend what ``Blend.fit`` makes of it alone.

    Point sources: bit for bit what ``fit_blends`` makes of the blend alone, an unpadded batch
    of one.  Against ``Blend.fit`` the centre and its moments are held to rtol 1e-12 (the bound
    of tests/test_gpu_facade.py::test_fit_blends_fits_unbatchable_blends_by_themselves), as for
    equal frames: no sum changes its order, but ``Blend.fit`` keeps a centre on the device,
    relative to its box, over a hook that resizes nothing, while ``fit_blends`` opens a batch
    per round and takes it over the host, ``box + (centre - box)``, which costs the last bit
    (blend.py, ``_fit_rounds``).  Everything else of these blends is compared exactly."""
    import scarlet_amd as scarlet

    blends = fc.scene_a(kind, fifth=False)
    alone, want = _fit_alone(blends)
    singles = [copy.deepcopy(b) for b in blends] if kind == "point" else []
    report = {}
    got = scarlet.fit_blends(blends, N_ITER, e_rel=E_REL, _report=report)
    assert scarlet.fit_blends.errors == []
    assert [idx for _, idx in report["groups"]] == [[0, 1, 2, 3]] and report["alone"] == {}
    assert got == want
    for i, (a, b) in enumerate(zip(blends, alone)):
        fc.assert_same_fit(a, b, "%s blend %d" % (kind, i),
                           last_bit=("center",) if kind == "point" else ())
    for i, single in enumerate(singles):
        assert scarlet.fit_blends([single], N_ITER, e_rel=E_REL) == [got[i]]
        fc.assert_same_fit(blends[i], single, "point blend %d, a batch of one" % i)
    assert all((21, 21) in _crossing(b, f) for b, f in zip(blends, fc.FRAMES))


def test_a_blend_of_the_ragged_batch_follows_the_oracle():
    """The ragged path is the algorithm, not only consistent with itself: blend 0 of scene A,
    fitted in the list, against oracle/pgm.py at the tolerance
    tests/test_gpu_facade.py::test_blend_fit_with_resizing_matches_oracle holds ``Blend.fit`` to."""
    import scarlet_amd as scarlet
    from scarlet_amd.blend import _flatten

    blends = fc.scene_a(fifth=False)
    scene = fc.oracle_scene(blends[0])
    with np.errstate(all="ignore"):
        n_ref, _ = scene.fit(N_ITER, e_rel=E_REL, resizing=True)
    got = scarlet.fit_blends(blends, N_ITER, e_rel=E_REL)
    assert got[0][0] == n_ref == N_ITER
    for comp, c in zip(_flatten(blends[0].sources), scene.components):
        assert comp.children[1].parameters[0].shape == c.morph.shape
        assert tuple(comp.children[1].bbox.origin) == tuple(c.origin)
    assert scene.components[2].morph.shape == (21, 21)
    chi = np.array(blends[0].loss) - scene.log_norm
    chi_ref = np.array(scene.loss) - scene.log_norm
    print("chi / chi_ref - 1:", np.abs(chi / chi_ref - 1).max())
    assert_allclose(chi, chi_ref, rtol=5e-4)


def test_a_failing_blend_leaves_its_group_mates_alone():
    import scarlet_amd as scarlet

    blends = fc.scene_a(fifth=False, nan_at=1)
    alone, want = _fit_alone(blends, skip=(1,))
    report = {}
    got = scarlet.fit_blends(blends, N_ITER, e_rel=E_REL, _report=report)
    assert report["batches"] == 1
    assert [i for i, _ in scarlet.fit_blends.errors] == [1]
    assert isinstance(scarlet.fit_blends.errors[0][1], ArithmeticError)
    assert got[1][0] == len(blends[1].loss) and np.isnan(got[1][1])
    for i in (0, 2, 3):
        assert got[i] == want[i]
        fc.assert_same_fit(blends[i], alone[i], "blend %d" % i)


def test_two_shards_on_one_gpu_equal_the_single_device_call():
    import scarlet_amd as scarlet

    one = fc.scene_a(fifth=False)
    two = fc.scene_a(fifth=False)
    want = scarlet.fit_blends(one, N_ITER, e_rel=E_REL)
    report = {}
    got = scarlet.fit_blends(two, N_ITER, e_rel=E_REL, devices=[0, 0], _report=report)
    assert [idx for _, idx in report["groups"]] == [[0, 1], [2, 3]] and report["batches"] == 2
    assert got == want
    for i, (a, b) in enumerate(zip(two, one)):
        fc.assert_same_fit(a, b, "blend %d" % i)
