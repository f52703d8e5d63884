"""``fit_blends`` with frames of different sizes, the host side: what ``plan_fit_blends`` says
about the scenes of tests/fit_blends_ragged_cases.py, and what ``_open_batch`` hands to
``BlendBatch`` -- padded cubes, the members' own convolution plan and the extents for a ragged
group, exactly the old call for a group of equal frames.  No GPU."""

import numpy as np
import pytest

import fit_blends_ragged_cases as fc

HOST_KINDS = [k for k in fc.KINDS if k != "starlet"]  # (the starlet transform needs the device)


class Recorder:
    """Stands in for ``BlendBatch``: keeps what it was opened with."""
    opened = []

    def __init__(self, data, weights, specs, **kwargs):
        self.data, self.weights, self.specs, self.kwargs = data, weights, specs, kwargs
        Recorder.opened.append(self)

    def add_loss_constant(self, constant):
        self.constant = constant

    def set_optimizer(self, **opt):
        self.opt = opt

    def close(self):
        pass


@pytest.fixture
def recorder(monkeypatch):
    from scarlet_amd import blend, fitting

    Recorder.opened = []
    monkeypatch.setattr(fitting, "BlendBatch", Recorder)
    monkeypatch.setattr(blend.Blend, "_upload_state", staticmethod(lambda batch, comps: None))
    return Recorder


def _open(blends):
    from scarlet_amd.blend import _flatten
    from scarlet_amd.fitting import _classify, _open_batch

    runs = [_classify(b)[1] for b in blends]
    flat = [c for r in runs for c in _flatten(r.blend.sources)]
    report = {}
    batch = _open_batch(runs, [r.specs for r in runs], flat, 7, 0, dict(b1=0.9, b2=0.999, eps=1e-8),
                        report)
    assert report == {"batches": 1}
    return runs, batch


def test_conv_plan_is_shared_by_both_fit_blends():
    from scarlet_amd import batch, fitting
    from scarlet_amd.lite import fitting as lite_fitting

    assert lite_fitting._conv_plan is batch._conv_plan is fitting._conv_plan
    # what it returned where it lived before
    for h, w, kshape in ((58, 48, (5, 41, 41)), (31, 24, (1, 11, 11)), (70, 66, (1, 11, 11))):
        fy, fx = batch.fft_shape_for(h, w, kshape, "fused")
        zb = min(fy // 16 - (h + 15) // 16, fx // 16 - (w + 15) // 16, 2)
        assert batch._conv_plan(h, w, kshape) == ("fused", fy, fx, zb)
    assert batch._conv_plan(600, 600, (1, 11, 11)) == (
        ("rocfft",) + batch.fft_shape_for(600, 600, (1, 11, 11), "rocfft") + (0,))
    assert batch._conv_plan(40, 50, None) == (None, 40, 50, 0)


@pytest.mark.parametrize("kind", HOST_KINDS)
def test_scene_a_is_one_group_and_the_fifth_blend_another(kind):
    import scarlet_amd as scarlet
    from scarlet_amd.batch import _conv_plan

    blends = fc.scene_a(kind)
    kshape = (1, fc.STAMP, fc.STAMP)  # one stamp for all bands: the PSFs are the same in each
    plans = [_conv_plan(h, w, kshape) for h, w in fc.FRAMES]
    assert len(set(plans)) == 1 and plans[0][0] == "fused"
    other = _conv_plan(*fc.OTHER_FRAME, kshape)
    assert other != plans[0]
    groups, alone = scarlet.plan_fit_blends(blends, 25, e_rel=1e-6)
    assert alone == {}
    assert groups == [((fc.C, kshape, plans[0]), [0, 1, 2, 3]), ((fc.C, kshape, other), [4])]


def test_scene_a_does_what_it_was_built_for():
    from scarlet_amd.blend import _flatten

    for blend, (h, w) in zip(fc.scene_a(), fc.FRAMES + [fc.OTHER_FRAME]):
        inside, edge, grower = [c.children[1].bbox for c in _flatten(blend.sources)]
        (y0, x0), (bh, bw) = inside.origin, inside.shape
        assert y0 > 0 and x0 > 0 and y0 + bh < h and x0 + bw < w
        (y0, x0), (bh, bw) = edge.origin, edge.shape
        assert y0 + bh > h and x0 + bw > w           # crosses the own frame's edges ...
        assert y0 < h and x0 < w
        if (h, w) != fc.OTHER_FRAME:                   # ... inside the padded plane where it can
            assert (y0 + bh <= 31 or h == 31) and (x0 + bw <= 31 or w == 31)
        (y0, x0), (bh, bw) = grower.origin, grower.shape
        assert y0 + bh < h and x0 + bw < w             # inside now; 21 x 21 about it is not
        assert y0 + bh // 2 + 10 >= h and x0 + bw // 2 + 10 >= w
    # the oracle on the first blend: the box of the grower has grown at the first resize hook
    scene = fc.oracle_scene(fc.scene_a()[0])
    with np.errstate(all="ignore"):
        scene.fit(12, e_rel=1e-6, resizing=True)
    assert [c.morph.shape for c in scene.components] == [(9, 9), (11, 11), (21, 21)]
    origin = scene.components[2].origin
    assert origin[0] + 21 > fc.FRAMES[0][0] and origin[1] + 21 > fc.FRAMES[0][1]


def test_null_renderer_blends_group_by_their_frame():
    import scarlet_amd as scarlet

    blends = fc.scene_b()
    groups, alone = scarlet.plan_fit_blends(blends + fc.scene_b()[:1])
    assert alone == {}
    assert groups == [((fc.C, None, (None, 31, 24, 0)), [0, 2]), ((fc.C, None, (None, 24, 31, 0)), [1])]


def test_blends_fitted_alone_and_their_reasons():
    import scarlet_amd as scarlet

    blends = fc.scene_a(fifth=False)
    image = blends[1].sources[0].children[1].parameters[0]
    image.step = lambda X, it=0: 0.01  # a step rule of the user's: stepped on the host
    groups, alone = scarlet.plan_fit_blends(blends, 25)
    assert alone == {1: "parameters the host updates"}
    assert [idx for _, idx in groups] == [[0, 2, 3]]
    # a callback or another scheme: every blend through Blend.fit, one at a time
    groups, alone = scarlet.plan_fit_blends(blends, 25, callback=lambda *p, it=None: None)
    assert groups == [] and sorted(alone) == [0, 1, 2, 3]
    assert all("callback" in why for why in alone.values())
    groups, alone = scarlet.plan_fit_blends(blends, 25, scheme="adam")
    assert groups == [] and all("adam" in why for why in alone.values())
    # options adaprox does not have are refused as by fit_blends
    with pytest.raises(NotImplementedError, match="unsupported"):
        scarlet.plan_fit_blends(blends, 25, momentum=0.5)
    with pytest.raises(ValueError, match="devices"):
        scarlet.plan_fit_blends(blends, 25, devices="all")
    # every shard of a list of devices has groups of its own
    groups, alone = scarlet.plan_fit_blends(fc.scene_a(fifth=False), 25, devices=[0, 1])
    assert [idx for _, idx in groups] == [[0, 1], [2, 3]] and alone == {}


def test_equal_frames_open_the_batch_they_opened_before(recorder):
    import scarlet_amd as scarlet

    blends = fc.equal_frames(3)
    groups, alone = scarlet.plan_fit_blends(blends, 25)
    assert [idx for _, idx in groups] == [[0, 1, 2]] and alone == {}
    runs, batch = _open(blends)
    assert recorder.opened == [batch]
    # no extents, no explicit plan: the arguments of the call as it was
    assert batch.kwargs.get("frame_shapes") is None
    assert sorted(batch.kwargs) == ["device", "kernel", "max_iter"]
    assert batch.kwargs["max_iter"] == 7 and batch.kwargs["device"] == 0
    np.testing.assert_array_equal(batch.data, np.stack([r.obs[0] for r in runs]))
    np.testing.assert_array_equal(batch.weights, np.stack([r.obs[1] for r in runs]))
    np.testing.assert_array_equal(batch.kwargs["kernel"], np.stack([r.obs[2] for r in runs]))


@pytest.mark.parametrize("kind", HOST_KINDS)
def test_ragged_group_is_padded_and_keeps_its_members_plan(recorder, kind):
    from scarlet_amd.batch import _conv_plan

    blends = fc.scene_a(kind, fifth=False)
    runs, batch = _open(blends)
    assert batch.kwargs["frame_shapes"] == fc.FRAMES and batch.kwargs["frame_kinds"] == "all"
    kshape = runs[0].obs[2].shape
    smallest = _conv_plan(24, 31, kshape)
    largest = _conv_plan(31, 31, kshape)
    assert smallest == largest
    assert (batch.kwargs["conv_path"],) + tuple(batch.kwargs["fft_shape"]) == largest[:3]
    assert batch.data.shape == batch.weights.shape == (4, fc.C, 31, 31)
    assert batch.data.dtype == batch.weights.dtype == np.float32
    for i, (r, (h, w)) in enumerate(zip(runs, fc.FRAMES)):
        for padded, own in ((batch.data, r.obs[0]), (batch.weights, r.obs[1])):
            np.testing.assert_array_equal(padded[i, :, :h, :w], own)
            assert not padded[i, :, h:, :].any() and not padded[i, :, :, w:].any()
        assert (batch.weights[i, :, :h, :w] > 0).all()
    assert [len(s) for s in batch.specs] == [len(r.specs) for r in runs]
