"""The six kernels of scarlet_amd/csrc/shift.hip against float64, shape by shape, on a real
MI355X: the cases of tests/shift_cases.py (white-noise images, every branch of the box shape,
both sides of the LDS / global switch, the 240 px limit), whose power to see a wrong Nyquist
term tests/test_shift_host.py proves on the CPU.

No tolerance here comes from the kernels' output: the forward bound is derived
(``shift_cases.forward_bound``), every other figure is one tests/test_gpu_parity.py already
uses, cited where it stands.  Each test prints its figures before it asserts.
"""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import shift_cases as sc_
from shift_cases import CASES, KERNEL_CASES, RTOL

pytestmark = pytest.mark.gpu

EPS32 = 2.0**-23


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd
    from scarlet_amd import _lib

    _lib.load()
    assert _lib.load().smi_device_count() >= 1
    return scarlet_amd


@pytest.fixture(scope="module")
def cases():
    return {name: sc_.make_case(name) for name in CASES}


@pytest.fixture(scope="module")
def references(cases):
    """Per case and blend, computed once: the oracle scene at the first shifts, its gradients
    and the tolerance scales.  Read only."""
    cache = {}

    def get(name, b):
        if (name, b) not in cache:
            sc = sc_.oracle_scene(cases[name], b)
            _, grads = sc.loss_and_gradients()
            sc.loss.clear()
            cache[name, b] = (sc, grads, sc_.grad_scales(sc))
        return cache[name, b]

    return get


def specs_of(amd, comps, live=None):
    """ComponentSpecs without constraint (``prox_flags=0``); ``live``: the index of the one
    component that keeps its spectrum, the others get zeros."""
    return [amd.ComponentSpec(c["sed"] if live in (None, k) else np.zeros_like(c["sed"]),
                              c["morph"], c["origin"], prox_flags=0, shift=c["shift"])
            for k, c in enumerate(comps)]


def batch_of(amd, case, blends=None, **kw):
    blends = case["blends"] if blends is None else blends
    batch = amd.BlendBatch(case["data"], case["weights"], [specs_of(amd, b, **kw) for b in blends],
                           kernel=case["kernel"], max_iter=4)
    assert batch.conv_path == "fused"
    return batch


def flat(case):
    return [(b, k, c) for b, comps in enumerate(case["blends"]) for k, c in enumerate(comps)]


def check_forward(case, shifted, which, tag):
    """Shifted images against ``ShiftOperator.forward`` of the float32 image in float64,
    elementwise within the derived bound; integer shifts against the zero-filled roll."""
    from oracle import fftconv

    for i, (b, k, c) in enumerate(flat(case)):
        x = c["morph"].astype(np.float64)
        if c[which] is None:
            assert_array_equal(shifted[i], c["morph"])  # not shifting: the parameter itself
            continue
        op = fftconv.ShiftOperator(x.shape, c[which])
        err = np.abs(shifted[i] - op.forward(x))
        ratio = (err / sc_.forward_bound(op, x)).max()
        print("forward %s %s blend %d comp %d %s shift %s: max error / bound = %.3f"
              % (case["name"], tag, b, k, x.shape, tuple(c[which]), ratio))
        assert ratio <= 1.0, (b, k)
        if sc_.is_integer(c[which][0]) and sc_.is_integer(c[which][1]):
            # known answer, independent of the oracle
            assert np.abs(shifted[i] - sc_.zero_filled_roll(x, c[which])).max() <= EPS32 * x.max()


@pytest.mark.parametrize("name", list(CASES))
def test_shift_forward(amd, cases, name):
    """``shift_forward_kernel`` alone (``model_morphologies``): at the shifts of construction,
    after ``set_centers`` to a second set (beyond one pixel, negative integers: the forward
    follows the state), and at zero shift, where it returns the parameter.  The parameters
    stay the unshifted images, bit for bit."""
    case = cases[name]
    batch = batch_of(amd, case)
    comps = flat(case)

    def params_untouched():
        _, params = batch.parameters()
        for i, (b, k, c) in enumerate(comps):
            assert_array_equal(params[i], c["morph"])

    check_forward(case, batch.model_morphologies(), "shift", "first")
    assert_allclose(batch.centers()["center"],
                    [np.zeros(2) if c["shift"] is None else c["shift"] for _, _, c in comps])
    params_untouched()
    batch.set_centers([np.zeros(2) if c["shift2"] is None else c["shift2"] for _, _, c in comps])
    check_forward(case, batch.model_morphologies(), "shift2", "second")
    params_untouched()
    batch.set_centers(np.zeros((len(comps), 2)))
    unshifted = batch.model_morphologies()
    for i, (b, k, c) in enumerate(comps):
        assert np.abs(unshifted[i] - c["morph"]).max() <= EPS32 * c["morph"].max()
    params_untouched()
    batch.close()


def check_gradients(case, references, g_sed, g_morph, g_shift):
    """Tolerances of test_shifting_scene_forward_and_gradient (tests/test_gpu_parity.py):
    2 RTOL x the magnitudes the float32 sums run over; a component without shift keeps the
    plain gathered gradient, to RTOL as in test_hsc_gradient_vs_oracle."""
    i = 0
    for b, comps in enumerate(case["blends"]):
        sc, grads, scales = references(case["name"], b)
        for k, c in enumerate(comps):
            s_sed, s_morph = scales[k]
            e_sed = np.abs(g_sed[i] - grads[k][0]).max() / s_sed
            e_morph = np.abs(g_morph[i] - grads[k][1]).max() / s_morph
            print("gradient %s blend %d comp %d %s: g_sed %.2e g_morph %.2e (x scale)"
                  % (case["name"], b, k, c["morph"].shape, e_sed, e_morph))
            if c["shift"] is None:
                assert e_sed < RTOL and e_morph < RTOL, (b, k)
            else:
                n_pix = c["morph"].size
                e_shift = np.abs(g_shift[i] - grads[k][2]).max() / (s_morph * np.sqrt(n_pix))
                print("    g_shift %.2e (x scale x sqrt(pixels)); device %s oracle %s"
                      % (e_shift, g_shift[i], grads[k][2]))
                assert e_sed < 2 * RTOL and e_morph < 2 * RTOL and e_shift < 2 * RTOL, (b, k)
            i += 1


@pytest.mark.parametrize("name", list(CASES))
def test_shift_gradients(amd, cases, references, name):
    """``shift_backward_kernel`` (``grad_only``): gradients w.r.t. spectra, images (pulled back
    through the shift) and shifts against ``oracle.pgm.Scene.loss_and_gradients`` in float64."""
    case = cases[name]
    batch = batch_of(amd, case)
    if name == "limit":
        # A finding, pinned: the C ABI takes a shifting box of up to 240 x 240 and the shift kernels
        # run it (test_shift_forward), but the update kernel that shares the gradient launch keeps
        # one image of the largest box in the LDS and refuses more than 40956 pixels.  The case
        # ``limit_update`` has the backward kernel at the same FFT lengths.
        with pytest.raises(amd._lib.ScarletAmdError,
                           match="component box too large for the LDS-resident update"):
            batch.gradient()
        batch.close()
        return
    g_sed, g_morph = batch.gradient()
    g_shift = batch.centers()["gradient"]
    batch.close()
    check_gradients(case, references, g_sed, g_morph, g_shift)


@pytest.mark.parametrize("name", ["packed", "pushed"])
def test_a_component_alone_gives_the_same_bits(amd, cases, name):
    """Each shifting component next to its neighbours and in a batch of its own: the shifted
    image and ``g_morph`` are equal bit for bit -- the arithmetic per component is the same
    whether the work arrays are in the LDS or in global memory, so a difference means scratch
    regions that overlap or a path that depends on the neighbours.  For the gradient image of
    the two batches to be the same, the neighbours of the joint batch have zero spectra (they
    add exact zeros to the model and still run both shift kernels on their own images)."""
    case = cases[name]
    comps = case["blends"][0]
    for k, c in enumerate(comps):
        if c["shift"] is None:
            continue
        joint = batch_of(amd, case, live=k)
        alone = batch_of(amd, case, blends=[[c]])
        f_joint, f_alone = joint.model_morphologies()[k], alone.model_morphologies()[0]
        (_, gm_joint), (_, gm_alone) = joint.gradient(), alone.gradient()
        joint.close()
        alone.close()
        print("alone %s comp %d: forward differs at %d pixels, g_morph at %d"
              % (name, k, (f_joint != f_alone).sum(), (gm_joint[k] != gm_alone[0]).sum()))
        assert np.abs(gm_alone[0]).max() > 0
        assert_array_equal(f_joint, f_alone)
        assert_array_equal(gm_joint[k], gm_alone[0])


def assert_loss_close(loss, ref_loss, log_norm, rtol):
    """As in tests/test_gpu_parity.py: the chi2 part of the loss."""
    a = np.asarray(loss, dtype=np.float64) - log_norm
    b = np.asarray(ref_loss, dtype=np.float64) - log_norm
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rtol * np.abs(b)), (a, b)


@pytest.mark.parametrize("name", ["small", "scratch_edge", "two_blends"])
def test_two_steps(amd, cases, name):
    """``step(0, 2)``: the AMSGrad step of the shift inside the backward kernel and the forward
    that follows it run in the right order, on both paths (the second loss is the one of the
    model after the first update).  Tolerances of
    test_free_shift_on_a_box_beyond_the_lds (tests/test_gpu_parity.py)."""
    case = cases[name]
    batch = batch_of(amd, case)
    batch.step(0, 2)
    sed, morphs = batch.parameters()
    center = batch.centers()["center"]
    losses = batch.loss_history()
    batch.close()
    i = 0
    for b, comps in enumerate(case["blends"]):
        sc = sc_.oracle_scene(case, b)
        for it in range(2):
            sc.step(it, 1e-3)
        assert_loss_close(losses[b], sc.loss, sc.log_norm, rtol=2e-4)
        moved = 0.0
        for k, (c, oc) in enumerate(zip(comps, sc.components)):
            e_sed = np.abs(sed[i] - oc.sed).max() / np.abs(oc.sed).max()
            e_morph = np.abs(morphs[i] - oc.morph).max()
            e_shift = np.abs(center[i] - oc.shift).max()
            print("steps %s blend %d comp %d: sed %.2e morph %.2e shift %.2e"
                  % (name, b, k, e_sed, e_morph, e_shift))
            assert e_sed < 1e-3 and e_morph < 2e-3 and e_shift < 2e-3, (b, k)
            moved = max(moved, np.abs(oc.shift - c["shift"]).max())
            i += 1
        assert moved > 1e-2


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_shift(amd, name):
    """``set_kernel_shift`` / ``kernel_shift(kernel=True)`` / ``gradient()``: the stamps at the
    current shift, the rendering with them and d(-logL)/d(shift), with the tolerances of
    test_kernel_shift_on_the_device (tests/test_gpu_parity.py): 2e-7 max|kernel| for the
    stamps, 1e-5 max for the rendering, rtol 2e-4 for the gradient.

    Where the stamp fills the batch's kernel the reference is the oracle scene with
    ``psf_shift``.  For the 9 x 13 stamp inside the 15 x 15 kernel the oracle scene takes the
    shifted stamp, ``fourier_shift(stamp, shift)`` at ``fft_shape(stamp, stamp, padding=10)``
    centred in zeros, as its fixed kernel, and the gradient reference is
    ``ShiftOperator(stamp.shape, shift)`` applied to the central crop of
    ``G_K[u] = sum_x r[x] model[x - (u - p//2)]`` (tests/test_shift_host.py shows that the two
    constructions agree where both exist)."""
    from oracle import fftconv

    kc = sc_.make_kernel_case(name)
    nb, ph, pw = len(kc["shifts"]), kc["ph"], kc["pw"]
    inner = kc["stamps"].shape[-2:] != (ph, pw)
    specs = [[amd.ComponentSpec(c["sed"], c["morph"], c["origin"], prox_flags=0) for c in comps]
             for comps in kc["blends"]]
    start = np.stack([sc_.embed(s, ph, pw) for s in kc["stamps"]])
    batch = amd.BlendBatch(kc["data"], kc["weights"], specs, kernel=start if nb > 1 else start[0],
                           max_iter=4)
    assert batch.conv_path == "fused"
    batch.set_kernel_shift(kc["stamps"] if nb > 1 else kc["stamps"][0], kc["shifts"],
                           kc["fft_shape"], step=1e-2)
    state = batch.kernel_shift(kernel=True)
    assert_array_equal(state["shift"], kc["shifts"])
    _, rendered, _ = batch.forward(model=False)
    batch.gradient()
    gradient = batch.kernel_shift()["gradient"]
    batch.close()
    for b in range(nb):
        stamp = kc["stamps"][b].astype(np.float64)
        want = sc_.embed(fftconv.fourier_shift(stamp, kc["shifts"][b]), ph, pw)
        e_stamp = np.abs(state["kernel"][b] - want).max() / np.abs(stamp).max()
        sc = sc_.kernel_scene(kc, b, free=not inner)
        model = sc.get_model()
        ref = sc.render(model)
        e_render = np.abs(rendered[b] - ref).max() / np.abs(ref).max()
        if inner:
            assert_array_equal(state["kernel"][b][want == 0], 0.0)
            g_ref = sc_.stamp_shift_gradient(kc["stamps"][b], kc["shifts"][b],
                                             sc_.kernel_gradient_image(sc, ph, pw))
        else:
            g_ref = sc.psf_shift_gradient(model, ref)
        print("kernel %s blend %d: stamp %.2e rendering %.2e gradient %s (oracle %s)"
              % (name, b, e_stamp, e_render, gradient[b], g_ref))
        assert e_stamp < 2e-7
        assert e_render < 1e-5
        assert_allclose(gradient[b], g_ref, rtol=2e-4)
        if all(sc_.is_integer(s) for s in kc["shifts"][b]):
            for j in range(kc["bands"]):
                rolled = sc_.zero_filled_roll(stamp[j], kc["shifts"][b])
                assert np.abs(state["kernel"][b][j] - rolled).max() < 2e-7 * np.abs(stamp).max()
