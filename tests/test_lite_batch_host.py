"""Host side of scarlet_amd.lite.fit_blends (no GPU): the grouping of blends into device
batches, the FFT shape query and the order of the results."""

import numpy as np
import pytest

from conftest import golden


def _blends(kind):
    import test_gpu_lite_batch as t

    return t._blends(kind)


def test_fft_shape_for_follows_the_batch_rule():
    from scarlet_amd.batch import fft_shape_for

    # fused kernel: smallest-area supported shape >= frame + stamp // 2
    assert fft_shape_for(58, 48, (5, 43, 43)) == (80, 80)
    assert fft_shape_for(52, 40, (5, 43, 43), "fused") == (80, 64)
    # rocFFT: the reference rule fft.py:116-167 (next fast length of frame + stamp + 3, even x)
    assert fft_shape_for(58, 48, (5, 43, 43), "rocfft") == (108, 96)
    # frames the fused kernel cannot take fall back to rocFFT, or fail with "fused"
    assert fft_shape_for(150, 150, (1, 41, 41)) == fft_shape_for(150, 150, (1, 41, 41), "rocfft")
    with pytest.raises(Exception):
        fft_shape_for(150, 150, (1, 41, 41), "fused")
    assert fft_shape_for(33, 17, None) == (33, 17)


@pytest.mark.parametrize("kind", ["fista", "adaprox"])
def test_grouping_is_deterministic_and_keeps_fft_shapes(kind):
    from scarlet_amd.batch import fft_shape_for
    from scarlet_amd.lite.fitting import group_keys

    blends = _blends(kind)
    keys = group_keys(blends, 30, 1e-3)
    assert keys == group_keys(_blends(kind), 30, 1e-3)
    groups = {}
    for b, k in zip(blends, keys):
        groups.setdefault(k, []).append(b)
    assert any(len({b.observation.images.shape for b in g}) > 1 for g in groups.values())
    for key, members in groups.items():
        path, fy, fx, zb = key[-1]
        kshape = key[4]
        H = max(b.observation.images.shape[1] for b in members)
        W = max(b.observation.images.shape[2] for b in members)
        # every member's own frame gets the group's FFT shape and path ...
        for b in members:
            assert fft_shape_for(*b.observation.images.shape[1:], kshape) == (fy, fx)
            assert fft_shape_for(*b.observation.images.shape[1:], kshape, path) == (fy, fx)
        # ... which is alias-free for the padded frame as well, with the same kernel variant
        assert fy >= H + kshape[1] // 2 and fx >= W + kshape[2] // 2
        if path == "fused":
            assert min(fy // 16 - (H + 15) // 16, fx // 16 - (W + 15) // 16, 2) == zb


def test_results_come_back_in_input_order(monkeypatch):
    from scarlet_amd import lite
    from scarlet_amd.lite import fitting

    blends = _blends("adaprox")
    seen = []

    def fake_group(members, key, max_iter, e_rel, min_iter, resize, device):
        seen.append([id(b) for b in members])
        for b in members:
            b.it = max_iter
            b.loss.append(float(id(b) % 1000))
        return set()

    monkeypatch.setattr(fitting, "_fit_group", fake_group)
    out = lite.fit_blends(blends, 30, e_rel=1e-3, reweight=False)
    assert out == [(30, float(id(b) % 1000)) for b in blends]
    assert sorted(i for g in seen for i in g) == sorted(id(b) for b in blends)
    assert len(seen) < len(blends)


def test_refusals_need_no_gpu():
    from scarlet_amd import lite

    blends = _blends("fista")
    blends[1].components[0]._sed.step = 2 * blends[1].components[0]._morph.step
    with pytest.raises(NotImplementedError):
        lite.fit_blends(blends, 10)
    with pytest.raises(ValueError):
        lite.fit_blends(blends[:1], 10, devices="ranks")
    assert golden("hsc_cosmos_35")["images"].shape[0] == 5
