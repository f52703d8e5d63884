"""The links of the proximal chain that follow the sweep (positivity, centre-on, normalisation)
and the AMSGrad step of the register-resident update kernels, flag set by flag set, on boxes of
the size classes 0, 1, 2, 3, 4 and 6 (21^2, 31^2, 41^2 and 30 x 40, 51^2, 61^2, 71^2; classes 5, 7
and 8, the boxes that fill a class, the boundaries of the sweep plans and the general kernel are
in tests/test_gpu_update_classes.py): against the CPU oracle, and bit for bit between
update_kernel_mixed, the per-class update_kernel_reg launches and each component stepped alone.

Null renderer, three bands, a 96 x 96 frame; the boxes of a blend do not overlap, so a component's
gradient does not depend on its neighbours and "alone" has the same bits to compare.  Blend 2
holds the 71^2 box: a four-wavefront class in the batch sends every class through its own
launch, without it the two blends of five one-wavefront classes share update_kernel_mixed.
None of the box sizes is a multiple of 64 pixels (tail slots), 30 x 40 is even in both axes
(level plan), and the last box of blend 1 hangs over the lower right corner of the frame.
Two iterations: the first-iteration body of the AMSGrad pass and the later one.
"""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

C, H, W = 3, 96, 96
# (blend, box shape, origin)
LAYOUT = [(0, (61, 61), (0, 0)), (0, (31, 31), (0, 62)), (0, (21, 21), (32, 62)),
          (1, (51, 51), (0, 0)), (1, (41, 41), (52, 0)), (1, (30, 40), (0, 53)),
          (1, (41, 41), (60, 70)),
          (2, (71, 71), (10, 12))]
N_IT = 2


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd
    from scarlet_amd import _lib

    _lib.load()
    assert _lib.load().smi_device_count() >= 1
    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def scene():
    """Data, weights and the components' starting values (never modified)."""
    rng = np.random.default_rng(20260)
    noise = np.array([0.02, 0.03, 0.025], dtype=np.float32)
    data = (rng.normal(0, 1, (3, C, H, W)) * noise[None, :, None, None]).astype(np.float32)
    seds, morphs, morphs_low = [], [], []
    for b, (h, w), (oy, ox) in LAYOUT:
        yy, xx = np.mgrid[:h, :w]
        cy, cx = h // 2, w // 2
        r2 = ((yy - cy) / (0.17 * h)) ** 2 + ((xx - cx) / (0.22 * w)) ** 2
        # not monotonic, some negative pixels, the maximum away from 1
        m = (np.exp(-0.5 * r2) * (1 + 0.3 * rng.normal(0, 1, (h, w))) - 0.02).astype(np.float32)
        m *= np.float32(0.8)
        sed = (1 + rng.random(C)).astype(np.float32)
        truth = np.exp(-0.5 * r2 * 1.3).astype(np.float32)
        ys, xs = slice(max(oy, 0), min(oy + h, H)), slice(max(ox, 0), min(ox + w, W))
        data[b, :, ys, xs] += (1.2 * sed[:, None, None] * truth[None])[:, ys.start - oy:ys.stop - oy,
                                                                     xs.start - ox:xs.stop - ox]
        seds.append(sed)
        morphs.append(m)
        # the same image with a negative centre pixel: after the sweep and positivity the centre
        # lies below every centre floor, so CenterOnConstraint is what sets it
        low = m.copy()
        low[cy, cx] = np.float32(-0.05)
        morphs_low.append(low)
    weights = np.broadcast_to((1 / noise ** 2)[None, :, None, None], data.shape).astype(np.float32).copy()
    return dict(data=data, weights=weights, seds=seds, morphs=morphs, morphs_low=morphs_low,
                noise=noise)


def _flag_sets(lib):
    """name -> (ComponentSpec keywords, chain of the oracle after the sweep: positivity floor or
    None, centre floor or None, normalisation or None, fixed image)"""
    std = lib.PROX_EXTENDED_SOURCE
    return {
        "standard": (dict(), (0.0, 1e-6, "max", False)),
        "no_positivity": (dict(prox_flags=std & ~lib.PROX_POSITIVE), (None, 1e-6, "max", False)),
        "no_center_on": (dict(prox_flags=std & ~lib.PROX_CENTER_ON), (0.0, None, "max", False)),
        "cfloor_below_pfloor": (dict(pos_floor=1e-3, center_floor=1e-5), (1e-3, 1e-5, "max", False)),
        "cfloor_above_pfloor": (dict(pos_floor=1e-5, center_floor=1e-2), (1e-5, 1e-2, "max", False)),
        "norm_sum": (dict(prox_flags=(std & ~lib.PROX_NORM_MAX) | lib.PROX_NORM_SUM),
                     (0.0, 1e-6, "sum", False)),
        "no_norm": (dict(prox_flags=std & ~lib.PROX_NORM_MAX), (0.0, 1e-6, None, False)),
        "fixed_morph": (dict(prox_flags=std | lib.COMPONENT_FIXED_MORPH), (0.0, 1e-6, "max", True)),
        # the centre floor binds: a centre of about 0.8 between the positivity floor and a
        # centre floor above the maximum of the image ...
        "cfloor_above_max": (dict(pos_floor=1e-3, center_floor=2.0), (1e-3, 2.0, "max", False)),
        # ... and (scene with the negative centre pixel) a centre below both floors
        "low_standard": (dict(), (0.0, 1e-6, "max", False)),
        "low_cfloor_above_pfloor": (dict(pos_floor=1e-3, center_floor=1e-2), (1e-3, 1e-2, "max", False)),
        "low_cfloor_below_pfloor": (dict(pos_floor=1e-2, center_floor=1e-3), (1e-2, 1e-3, "max", False)),
        "low_no_norm": (dict(prox_flags=std & ~lib.PROX_NORM_MAX, center_floor=0.5),
                        (0.0, 0.5, None, False)),
    }


FLAG_SETS = ["standard", "no_positivity", "no_center_on", "cfloor_below_pfloor", "cfloor_above_pfloor",
             "norm_sum", "no_norm", "fixed_morph", "cfloor_above_max", "low_standard",
             "low_cfloor_above_pfloor", "low_cfloor_below_pfloor", "low_no_norm"]


def _run(amd, scene, blends, kw, which=None, lite=False, morphs="morphs"):
    """Step the components `which` (indices into LAYOUT; default: all of `blends`) of the blends
    `blends`; returns {LAYOUT index: (sed, morph, m, v, vhat)} and the batch's loss histories."""
    idx = [i for i, (b, _, _) in enumerate(LAYOUT) if b in blends and (which is None or i in which)]
    comps = []
    for b in blends:
        comps.append([amd.ComponentSpec(scene["seds"][i], scene[morphs][i], LAYOUT[i][2],
                                        sed_min_step=scene["noise"] / (10 if lite else 1), **kw)
                      for i in idx if LAYOUT[i][0] == b])
    extra = dict(log_norm=False) if lite else {}
    batch = amd.BlendBatch(scene["data"][list(blends)], scene["weights"][list(blends)], comps,
                           kernel=None, max_iter=N_IT + 2, **extra)
    batch.set_sub_ranges(1)
    if lite:
        batch.step(0, N_IT, e_rel=1e-6, prox_max_iter=1)
    else:
        batch.step(0, N_IT, e_rel=1e-3)
    sed, morphs = batch.parameters()
    mom = batch.moments()
    loss = batch.loss_history()
    batch.close()
    order = [i for b in blends for i in idx if LAYOUT[i][0] == b]
    out = {i: (sed[n], morphs[n], mom["m_morph"][n], mom["v_morph"][n], mom["vhat_morph"][n])
           for n, i in enumerate(order)}
    return out, loss


def _assert_same_bits(a, b, what):
    for x, y in zip(a, b):
        assert_array_equal(x, y, err_msg=str(what))


def _three_ways(amd, scene, kw, lite=False, morphs="morphs"):
    # (which launch a batch takes: launch_update in csrc/kernels.hip -- several size classes and no
    # four-wavefront class among them -> update_kernel_mixed; with the 71^2 box one launch per class)
    mixed, loss_mixed = _run(amd, scene, (0, 1), kw, lite=lite, morphs=morphs)
    per_class, loss_class = _run(amd, scene, (0, 1, 2), kw, lite=lite, morphs=morphs)
    for i in mixed:
        _assert_same_bits(mixed[i], per_class[i], ("mixed / per class", i))
    for b in (0, 1):
        assert_array_equal(loss_mixed[b], loss_class[b])
    for i, (b, _, _) in enumerate(LAYOUT):
        alone, _ = _run(amd, scene, (b,), kw, which=(i,), lite=lite, morphs=morphs)
        _assert_same_bits(alone[i], per_class[i], ("alone / per class", i))
    return per_class, loss_class


@pytest.mark.parametrize("name", FLAG_SETS)
def test_chain_flag_sets_three_launch_shapes_and_the_oracle(amd, scene, name):
    from oracle import pgm, proxops
    from scarlet_amd import _lib

    kw, (pfloor, cfloor, norm, fixed) = _flag_sets(_lib)[name]
    morphs = "morphs_low" if name.startswith("low_") else "morphs"
    got, loss = _three_ways(amd, scene, kw, morphs=morphs)

    class Comp(pgm.Component):
        def morph_prox(self, x, step):
            x = proxops.prox_monotonic(x, step, "angle", 0.0)
            if pfloor is not None:
                x = proxops.prox_positivity(x, step, np.float32(pfloor))
            if cfloor is not None:
                x = proxops.prox_center_on(x, step, np.float32(cfloor))
            if norm is not None:
                x = proxops.prox_normalization(x, step, norm)
            return x

    for b in (0, 1, 2):
        idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
        sc = pgm.Scene(scene["data"][b].shape, scene["data"][b], scene["weights"][b], None,
                       [Comp(scene["seds"][i].copy(), scene[morphs][i].copy(), LAYOUT[i][2],
                             sed_min_step=scene["noise"], fixed=(False, fixed)) for i in idx])
        for it in range(N_IT):
            sc.step(it, 1e-3)
        a = np.asarray(loss[b], dtype=np.float64) - sc.log_norm
        ref = np.asarray(sc.loss, dtype=np.float64) - sc.log_norm
        assert a.shape == ref.shape and np.all(np.abs(a - ref) <= 1e-5 * np.abs(ref)), (a, ref)
        for i, c in zip(idx, sc.components):
            # the tolerances of test_hsc_steps_vs_oracle
            assert rel_err(got[i][0], c.sed) < 1e-4, (name, i)
            assert np.abs(got[i][1] - c.morph).max() < 1e-4, (name, i)
            assert rel_err(got[i][3], c.v_morph) < 1e-3, (name, i)
            if norm == "max" and pfloor is not None:
                assert got[i][1].max() == 1.0 and got[i][1].min() >= 0.0


def test_lite_chain_three_launch_shapes_and_the_oracle(amd, scene):
    """scarlet.lite's chain (centre-fitted monotonicity, background threshold instead of
    positivity, centre floor 1e-20, maximum normalisation, one application of the prox)."""
    from oracle import lite as olite
    from scarlet_amd import _lib

    flags = _lib.PROX_MONOTONIC | _lib.PROX_FIT_CENTER | _lib.PROX_CENTER_ON | _lib.PROX_NORM_MAX
    noise = scene["noise"]
    kw = dict(prox_flags=flags, neighbor_weight="angle", min_gradient=0.0, center_floor=1e-20,
              bg_level=noise * 0.25, morph_step=1e-2)
    got, loss = _three_ways(amd, scene, kw, lite=True)
    for b in (0, 1, 2):
        idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
        sc = olite.LiteScene(scene["data"][b], scene["weights"][b], None,
                             [olite.LiteComponent(scene["seds"][i].copy(), scene["morphs"][i].copy(),
                                                  LAYOUT[i][2], noise, kind="adaprox",
                                                  sed_min_step=noise / 10) for i in idx])
        sc.fit(N_IT, e_rel=0, resize=None)
        ref = np.array(sc.loss[:N_IT])
        # (the early-iteration bound of test_lite_loop_vs_the_reference_run)
        assert np.abs(-np.array(loss[b])[:N_IT] / ref - 1).max() < 3e-5
        for i, c in zip(idx, sc.components):
            assert rel_err(got[i][0], c.sed) < 1e-4, i
            assert np.abs(got[i][1] - c.morph).max() < 1e-4, i


@pytest.mark.parametrize("blends,victim", [((0, 1, 2), 4), ((0, 1, 2), 7), ((0, 1), 4)],
                         ids=["per_class_41", "team_71", "mixed_41"])
def test_a_nan_in_one_pixel_fails_its_blend_and_leaves_the_others_alone(amd, scene, blends, victim):
    """A NaN in one pixel of one component's image (and so of its gradient): the maximum of the
    fast chain would drop it, so that component's team takes the exact chain, the image comes
    out non-finite and the blend fails in that very iteration -- with the loss of that iteration
    recorded, as test_loss_history_of_a_blend_that_goes_non_finite expects -- while the blends
    beside it get the bits they get in a batch without the NaN.  Victims: a 41^2 box in per-class
    launches, the 71^2 box (a team of four wavefronts: the vote crosses wavefronts; pixel
    (7, 30) belongs to the third of them) and a 41^2 box in update_kernel_mixed."""
    idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] in blends]
    n = idx.index(victim)
    vb = blends.index(LAYOUT[victim][0])

    def batch_of(poison):
        comps = [[amd.ComponentSpec(scene["seds"][i], scene["morphs"][i], LAYOUT[i][2],
                                    sed_min_step=scene["noise"])
                  for i in idx if LAYOUT[i][0] == b] for b in blends]
        batch = amd.BlendBatch(scene["data"][list(blends)], scene["weights"][list(blends)], comps,
                               kernel=None, max_iter=8)
        batch.set_sub_ranges(1)
        batch.step(0, 2, e_rel=1e-3)
        if poison:
            seds, morphs = batch.parameters()
            morphs[n][7, 30] = np.nan  # away from the centre
            batch.set_parameters(seds, morphs)
        batch.step(2, 3, e_rel=1e-3)
        out = batch.status(), batch.states(), batch.loss_history(), batch.parameters()
        batch.close()
        return out

    (n_active, first_bad), states, loss, (sed, morphs) = batch_of(True)
    _, states_ok, loss_ok, (sed_ok, morphs_ok) = batch_of(False)
    nb = len(blends)
    assert list(states_ok) == [0] * nb and [len(h) for h in loss_ok] == [5] * nb
    assert first_bad == vb and n_active == nb - 1
    assert list(states) == [3 if b == vb else 0 for b in range(nb)]
    # iterations 0 and 1, plus iteration 2 whose update failed; the others all five
    assert [len(h) for h in loss] == [3 if b == vb else 5 for b in range(nb)]
    # (the loss of iteration 2 is taken on the model that holds the NaN)
    assert_array_equal(loss[vb][:2], loss_ok[vb][:2])
    assert np.isnan(loss[vb][2])
    for b in range(nb):
        if b != vb:
            assert_array_equal(loss[b], loss_ok[b])
    for m, i in enumerate(idx):
        if LAYOUT[i][0] != LAYOUT[victim][0]:
            assert_array_equal(sed[m], sed_ok[m])
            assert_array_equal(morphs[m], morphs_ok[m])
    assert not np.isfinite(morphs[n]).all()
