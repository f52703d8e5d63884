"""The once-per-iteration part of the register-resident update kernels (upd_step): the tenth of
a blend's first local iteration, taken behind a wave-uniform branch, the square root of the
AMSGrad denominator, and the gather of the gradient (offsets from the workgroup's table for a
box inside its frame, computed lane by lane for a box over an edge).

Layout of tests/test_gpu_update_chain.py: null renderer, three bands, a 96 x 96 frame, boxes of a
blend that do not overlap.  Blend 2 holds the 71^2 box (a team of four wavefronts; with it every
class gets a launch of its own, without it the blends share update_kernel_mixed).
"""

import ctypes

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
N_FIRST, N_SECOND = 2, 2  # iterations before and after the iteration bases are set


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd
    from scarlet_amd import _lib

    assert _lib.load().smi_device_count() >= 1
    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def scene():
    """Data, weights and the components' starting values (never modified)."""
    rng = np.random.default_rng(20261)
    noise = np.array([0.02, 0.03, 0.025], dtype=np.float32)
    data = (rng.normal(0, 1, (3, C, H, W)) * noise[None, :, None, None]).astype(np.float32)
    seds, morphs = [], []
    for b, (h, w), (oy, ox) in LAYOUT:
        yy, xx = np.mgrid[:h, :w]
        r2 = ((yy - h // 2) / (0.17 * h)) ** 2 + ((xx - w // 2) / (0.22 * w)) ** 2
        m = (np.exp(-0.5 * r2) * (1 + 0.3 * rng.normal(0, 1, (h, w))) - 0.02).astype(np.float32)
        m *= np.float32(0.8)
        sed = (1 + rng.random(C)).astype(np.float32)
        truth = np.exp(-0.5 * r2 * 1.3).astype(np.float32)
        ys, xs = slice(max(oy, 0), min(oy + h, H)), slice(max(ox, 0), min(ox + w, W))
        data[b, :, ys, xs] += (1.2 * sed[:, None, None] * truth[None])[:, ys.start - oy:ys.stop - oy,
                                                                     xs.start - ox:xs.stop - ox]
        seds.append(sed)
        morphs.append(m)
    weights = np.broadcast_to((1 / noise ** 2)[None, :, None, None], data.shape).astype(np.float32).copy()
    return dict(data=data, weights=weights, seds=seds, morphs=morphs, noise=noise)


def _batch(amd, scene, blends):
    comps = [[amd.ComponentSpec(scene["seds"][i], scene["morphs"][i], LAYOUT[i][2],
                                sed_min_step=scene["noise"])
              for i in range(len(LAYOUT)) if LAYOUT[i][0] == b] for b in blends]
    batch = amd.BlendBatch(scene["data"][list(blends)], scene["weights"][list(blends)], comps,
                           kernel=None, max_iter=N_FIRST + N_SECOND + 2)
    batch.set_sub_ranges(1)
    return batch


def _results(batch, blends):
    sed, morphs = batch.parameters()
    mom = batch.moments()
    loss = batch.loss_history()
    order = [i for b in blends for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
    out = {i: (sed[n], morphs[n], mom["m_morph"][n], mom["v_morph"][n], mom["vhat_morph"][n])
           for n, i in enumerate(order)}
    return out, {b: np.asarray(loss[n]) for n, b in enumerate(blends)}


def _run_restart(amd, scene, blends, restarted):
    """N_FIRST iterations of every blend, then N_SECOND more in which the blends `restarted`
    count from local iteration 0 again while the others go on."""
    batch = _batch(amd, scene, blends)
    batch.step(0, N_FIRST, e_rel=1e-3)
    batch.set_iteration_base(np.array([N_FIRST if b in restarted else 0 for b in blends]))
    batch.step(N_FIRST, N_SECOND, e_rel=1e-3)
    out = _results(batch, blends)
    batch.close()
    return out


@pytest.fixture(scope="module")
def alone(amd, scene):
    """(blend, restarted) -> that blend stepped in a batch of its own (computed once)."""
    cache = {}

    def get(b, restarted):
        if (b, restarted) not in cache:
            cache[b, restarted] = _run_restart(amd, scene, (b,), (b,) if restarted else ())
        return cache[b, restarted]

    return get


@pytest.fixture(scope="module")
def oracle_runs(scene):
    """(blend, restarted) -> the oracle's scene after the same iterations (computed once)."""
    from oracle import pgm, proxops

    class Comp(pgm.Component):
        def morph_prox(self, x, step):
            x = proxops.prox_monotonic(x, step, "angle", 0.0)
            x = proxops.prox_positivity(x, step, np.float32(0.0))
            x = proxops.prox_center_on(x, step, np.float32(1e-6))
            return proxops.prox_normalization(x, step, "max")

    cache = {}

    def get(b, restarted):
        if (b, restarted) not in cache:
            idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
            sc = pgm.Scene(scene["data"][b].shape, scene["data"][b], scene["weights"][b], None,
                           [Comp(scene["seds"][i].copy(), scene["morphs"][i].copy(), LAYOUT[i][2],
                                 sed_min_step=scene["noise"]) for i in idx])
            for it in range(N_FIRST):
                sc.step(it, 1e-3)
            for it in range(N_SECOND):
                sc.step(it if restarted else N_FIRST + it, 1e-3)
            cache[b, restarted] = sc
        return cache[b, restarted]

    return get


@pytest.mark.parametrize("blends,restarted", [((0, 1, 2), 1), ((0, 1, 2), 2), ((0, 1), 0)],
                         ids=["per_class", "team_71", "mixed"])
def test_first_iteration_tenth_of_one_blend_beside_blends_that_go_on(amd, scene, alone, oracle_runs,
                                                                      blends, restarted):
    """Two or three blends in one launch, one of them at local iteration 0 (the step is a tenth,
    vhat = v) while the others are at iteration 2: every blend gets the bits it gets alone, and
    the oracle's values to the tolerances of tests/test_gpu_update_chain.py."""
    got, loss = _run_restart(amd, scene, blends, (restarted,))
    for b in blends:
        ref, ref_loss = alone(b, b == restarted)
        for i in ref:
            for x, y in zip(got[i], ref[i]):
                assert_array_equal(x, y, err_msg=str(("in the batch / alone", b, i)))
        assert_array_equal(loss[b], ref_loss[b])
        sc = oracle_runs(b, b == restarted)
        idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
        a = np.asarray(loss[b], dtype=np.float64) - sc.log_norm
        want = np.asarray(sc.loss, dtype=np.float64) - sc.log_norm
        print(b, "loss", a, want)
        assert a.shape == want.shape and np.all(np.abs(a - want) <= 1e-5 * np.abs(want)), (a, want)
        for i, c in zip(idx, sc.components):
            print(b, i, rel_err(got[i][0], c.sed), np.abs(got[i][1] - c.morph).max(),
                  rel_err(got[i][3], c.v_morph))
            assert rel_err(got[i][0], c.sed) < 1e-4, i
            assert np.abs(got[i][1] - c.morph).max() < 1e-4, i
            assert rel_err(got[i][3], c.v_morph) < 1e-3, i
    # (the restart is not a no-op: the blend differs from itself going on)
    other, _ = alone(restarted, False)
    assert any(not np.array_equal(got[i][1], other[i][1]) for i in other)


# ---- the square root -------------------------------------------------------------------------

SQRT_MIN = np.float32(2.0 ** -96)  # rounded_math.h: kSqrtNormalMin
EPS = np.float32(1e-8)


def _sqrt_operands():
    f32 = np.float32
    up = lambda x: np.nextafter(f32(x), f32(np.inf))  # noqa: E731
    down = lambda x: np.nextafter(f32(x), f32(0))  # noqa: E731
    x = [EPS, SQRT_MIN, up(SQRT_MIN), down(SQRT_MIN), np.finfo(np.float32).max, f32(np.inf)]
    for k in range(1, 65):
        sq = f32(k * k)
        x += [down(sq), sq, up(sq)]
    x += [f32(2.0) ** e for e in range(-96, 128)]
    rng = np.random.default_rng(808)
    lo, hi = int(EPS.view(np.uint32)), int(np.finfo(np.float32).max.view(np.uint32))
    rnd = rng.integers(lo, hi + 1, size=1 << 16, dtype=np.uint32).view(np.float32)
    return np.concatenate([np.array(x, dtype=np.float32), rnd])


def test_sqrt_rn_normal_is_numpys_float32_sqrt_bit_for_bit(amd):
    from scarlet_amd import _lib

    lib = _lib.load()
    x = _sqrt_operands()
    assert x.dtype == np.float32 and (x[np.arange(x.size) != 3] >= SQRT_MIN).all()
    y = np.full_like(x, np.nan)
    _lib.check(lib.smi_sqrt_rn_normal_test(_lib.ptr(x, ctypes.c_float), _lib.ptr(y, ctypes.c_float),
                                           x.size))
    want = np.sqrt(x)
    assert want.dtype == np.float32 and np.isinf(want[5])
    bad = np.nonzero(y.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, [(float(x[i]), float(y[i]), float(want[i])) for i in bad[:8]]


@pytest.mark.parametrize("blends", [(0, 2), (0,)], ids=["per_class_and_team", "mixed"])
def test_a_batch_with_eps_zero_takes_the_general_sqrt_and_matches_the_oracle(amd, scene, blends):
    """eps = 0 lies below kSqrtNormalMin: the AMSGrad pass takes sqrtf as before.  (Blends whose
    boxes lie inside the frame: with eps = 0 a pixel whose gradient is exactly zero divides
    0 by 0, in the reference as well.)"""
    from oracle import pgm, proxops

    class Comp(pgm.Component):
        def morph_prox(self, x, step):
            x = proxops.prox_monotonic(x, step, "angle", 0.0)
            x = proxops.prox_positivity(x, step, np.float32(0.0))
            x = proxops.prox_center_on(x, step, np.float32(1e-6))
            return proxops.prox_normalization(x, step, "max")

    batch = _batch(amd, scene, blends)
    batch.set_optimizer(eps=0.0)
    batch.step(0, 2, e_rel=1e-3)
    got, loss = _results(batch, blends)
    batch.close()
    for b in blends:
        idx = [i for i in range(len(LAYOUT)) if LAYOUT[i][0] == b]
        sc = pgm.Scene(scene["data"][b].shape, scene["data"][b], scene["weights"][b], None,
                       [Comp(scene["seds"][i].copy(), scene["morphs"][i].copy(), LAYOUT[i][2],
                             sed_min_step=scene["noise"]) for i in idx])
        for it in range(2):
            sc.step(it, 1e-3, eps=0.0)
        a = np.asarray(loss[b], dtype=np.float64) - sc.log_norm
        want = np.asarray(sc.loss, dtype=np.float64) - sc.log_norm
        print(b, "loss", a, want)
        assert a.shape == want.shape and np.all(np.abs(a - want) <= 1e-5 * np.abs(want)), (a, want)
        for i, c in zip(idx, sc.components):
            print(b, i, rel_err(got[i][0], c.sed), np.abs(got[i][1] - c.morph).max(),
                  rel_err(got[i][3], c.v_morph))
            assert np.isfinite(got[i][1]).all()
            assert rel_err(got[i][0], c.sed) < 1e-4, i
            assert np.abs(got[i][1] - c.morph).max() < 1e-4, i
            assert rel_err(got[i][3], c.v_morph) < 1e-3, i


# ---- the gather offsets ----------------------------------------------------------------------

SHAPES = [(21, 21), (41, 41), (61, 61), (30, 40), (71, 71)]


def _placements(h, w, Hb, Wb):
    """inside the frame [0, Hb) x [0, Wb); over its top, bottom, left and right edge; over its
    upper left corner"""
    return [(5, 0), (-(h // 3), 1), (Hb - h + h // 3, 1), (2, -(w // 3)), (2, Wb - w + w // 3),
            (-(h // 2), -(w // 2))]


def _dyadic(Hb, Wb):
    """Six blends (one per placement) of five boxes (one per shape), which may overlap.  Every
    value is a small multiple of 1/4 or a power of two, so the model, w (m - d) and both sums
    of the gradient are exact in float32 in whatever order they are taken: NumPy in float64
    gives the bits every correct evaluation gives."""
    rng = np.random.default_rng(77)
    nb = 6
    data = (rng.integers(-8, 9, (nb, C, H, W)) / 4).astype(np.float32)
    weights = rng.choice([1.0, 2.0], (nb, C, H, W)).astype(np.float32)
    comps = []
    for b in range(nb):
        comps.append([((rng.integers(0, 5, s) / 4).astype(np.float32),
                       rng.choice([1.0, 2.0], C).astype(np.float32), _placements(*s, Hb, Wb)[b])
                      for s in SHAPES])
    return dict(data=data, weights=weights, comps=comps)


def _expected_gradients(dy, weights, Hb, Wb):
    """g_sed, g_morph of every component: the slice of G = w (model - data) into its box, zero
    outside the frame [0, Hb) x [0, Wb) (float64; exact)."""
    out = []
    for b, comps in enumerate(dy["comps"]):
        model = np.zeros((C, H, W))
        boxes = []
        for morph, sed, (oy, ox) in comps:
            h, w = morph.shape
            ys, xs = slice(max(oy, 0), min(oy + h, Hb)), slice(max(ox, 0), min(ox + w, Wb))
            bys, bxs = slice(ys.start - oy, ys.stop - oy), slice(xs.start - ox, xs.stop - ox)
            model[:, ys, xs] += sed[:, None, None].astype(np.float64) * morph[None, bys, bxs]
            boxes.append((ys, xs, bys, bxs))
        G = weights[b].astype(np.float64) * (model - dy["data"][b])
        for (morph, sed, _), (ys, xs, bys, bxs) in zip(comps, boxes):
            boxed = np.zeros((C,) + morph.shape)
            boxed[:, bys, bxs] = G[:, ys, xs]
            out.append(((boxed * morph[None]).sum(axis=(1, 2)),
                        (sed[:, None, None].astype(np.float64) * boxed).sum(axis=0)))
    return out


@pytest.mark.parametrize("extents", [None, (80, 72)], ids=["full_frame", "frame_extents"])
def test_gathered_gradient_of_boxes_inside_and_over_the_edges_bit_for_bit(amd, extents):
    """Boxes of 21^2 (no full slot), 41^2, 61^2, 30 x 40 (even) and 71^2 pixels inside the frame,
    over each edge and over a corner, once in frames smaller than the batch's: g_sed and g_morph
    of the gradient-only path are the exact sums, and so is what the update kernels gathered --
    from the workgroup's table of offsets or lane by lane -- as the first moments they leave
    after one iteration from zero, m = (1 - b1) g and v = (1 - b2) g g, show."""
    Hb, Wb = extents or (H, W)
    dyadic = _dyadic(Hb, Wb)
    weights = dyadic["weights"].copy()
    weights[:, :, Hb:, :] = 0
    weights[:, :, :, Wb:] = 0
    specs = [[amd.ComponentSpec(sed, morph, origin, sed_min_step=0.01) for morph, sed, origin in comps]
             for comps in dyadic["comps"]]
    nb = len(specs)
    batch = amd.BlendBatch(dyadic["data"], weights, specs, kernel=None, max_iter=4,
                           frame_shapes=None if extents is None else [extents] * nb)
    batch.set_sub_ranges(1)
    g_sed, g_morph = batch.gradient()
    want = _expected_gradients(dyadic, weights, Hb, Wb)
    for n, (ws, wm) in enumerate(want):
        assert np.abs(wm).max() > 0 and np.abs(ws).max() < 2 ** 20
        assert_array_equal(g_morph[n], wm.astype(np.float32), err_msg="g_morph %d" % n)
        assert_array_equal(g_sed[n], ws.astype(np.float32), err_msg="g_sed %d" % n)
    batch.step(0, 1, e_rel=1e-3)
    mom = batch.moments()
    batch.close()
    one = np.float32(1)
    c1, c2 = one - np.float32(0.9), one - np.float32(0.999)
    for n, (_, wm) in enumerate(want):
        g = wm.astype(np.float32)
        assert_array_equal(mom["m_morph"][n], c1 * g, err_msg="m_morph %d" % n)
        assert_array_equal(mom["v_morph"][n], c2 * g * g, err_msg="v_morph %d" % n)
