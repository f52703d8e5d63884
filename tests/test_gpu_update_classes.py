"""The proximal chain and whole steps of the update kernels (update_kernel_reg, update_kernel_mixed
and the general update_kernel of csrc/kernels.hip) at the edges of every size class, of every sweep
plan and with every link of the chain: tests/update_class_cases.py holds the boxes (a box that
fills each of the nine classes exactly, one a few pixels into the next, 47^2 / 49^2 / 63^2 / 65^2
at the boundaries of the ring schedule, 123^2 .. 128^2 in the general kernel, four boxes that
overhang their frame), tests/test_update_classes_host.py the CPU preconditions.

Part 1, the chain alone: with all-zero weights every gradient is zero, the AMSGrad (or FISTA)
step leaves the image where it was (m = v = vhat = 0: x - alpha * 0 / sqrt(eps) = x, and the
candidate z - r (z - x) = z), and with prox_max_iter = 1 the iteration's result is the proximal
chain of the starting image, applied once.  The sweep is written in correctly rounded single
operations and the other links are maxima, selections and products with powers of two, so the
device image must equal the oracle's chain (oracle.proxops, oracle.lite) BIT FOR BIT -- which
pins the sweep inside the update kernels the way test_sweep_bit_exact pins the stand-alone
entry.  With a normalisation: the numpy restatement of the kernels' reciprocal, one ulp from the
oracle's division (maximum), the reordered-sum bound (sum).

Part 2, whole steps with a real gradient: three iterations against oracle.pgm.Scene /
oracle.lite.LiteScene at the tolerances the project states for that comparison.

Both parts run every case in several launch shapes and require the same bits from all:
  table    all register-resident boxes in one batch: it holds four-wavefront classes, so every
           class gets its own update_kernel_reg launch (classes 0 .. 8)
  mixed    the one-wavefront boxes in one batch: update_kernel_mixed
  alone    every box in a batch of its own: update_kernel_reg of one class; the general kernel
           for 123^2 and 127 x 128 (slot layout) and 128^2 (level plan, no slots)
  general  the three boxes beyond kMaxRegisterBox in one batch -- and, in part 1, the whole table
           with them: one box beyond the register classes sends every component of a batch
           through the general kernel, 128^2 takes the slot path away from the batch
"""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import update_class_cases as cases

pytestmark = pytest.mark.gpu

REGISTER = cases.register_blends()
GENERAL = cases.general_blends()
MIXED = cases.one_wavefront(REGISTER)


@pytest.fixture(scope="module")
def amd():
    import scarlet_amd
    from scarlet_amd import _lib

    _lib.load()
    assert _lib.load().smi_device_count() >= 1
    return scarlet_amd


def rel_err(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


_OBS = {}


def _observation(blend, zero):
    key = (blend.name, zero)
    if key not in _OBS:
        _OBS[key] = cases.observation(blend, zero)
    return _OBS[key]


def _run(amd, blends, kw, batch_kw, zero, steps):
    """One batch of one-component blends.  `steps`: [(iterations, step keywords), ...]; returns
    {blend name: [state after each entry of `steps`]} with state = dict(sed, morph, m_morph,
    v_morph, vhat_morph, loss)."""
    data = np.stack([_observation(b, zero)[0] for b in blends])
    weights = np.stack([_observation(b, zero)[1] for b in blends])
    comps = [[amd.ComponentSpec(cases.start_spectrum(b), cases.start_image(b), b.origin, **kw)]
             for b in blends]
    frames = [b.frame for b in blends]
    if all(f == (cases.H, cases.W) for f in frames):
        frames = None
    n_total = sum(n for n, _ in steps)
    batch = amd.BlendBatch(data, weights, comps, kernel=None, max_iter=n_total + 2,
                           frame_shapes=frames, **batch_kw)
    batch.set_sub_ranges(1)
    out = {b.name: [] for b in blends}
    it = 0
    for n, step_kw in steps:
        batch.step(it, n, **step_kw)
        it += n
        sed, morphs = batch.parameters()
        mom = batch.moments()
        loss = batch.loss_history()
        assert list(batch.states()) == [0] * len(blends)
        for k, b in enumerate(blends):
            out[b.name].append(dict(sed=sed[k], morph=morphs[k], m_morph=mom["m_morph"][k],
                                    v_morph=mom["v_morph"][k], vhat_morph=mom["vhat_morph"][k],
                                    loss=np.array(loss[k])))
    batch.close()
    return out


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for n, (sa, sb) in enumerate(zip(a, b)):
        for key in sa:
            assert_array_equal(sa[key], sb[key], err_msg="%s: %s after entry %d" % (what, key, n))


def _launch_shapes(amd, kw, batch_kw, zero, steps, with_table_in_general=False):
    """The case in every launch shape (module docstring), the same bits required from all of
    them; returns {blend name: states} for the register blends (from `table`) and the general
    blends (from `general`), and the states of the register blends in the general kernel."""
    table = _run(amd, REGISTER, kw, batch_kw, zero, steps)
    mixed = _run(amd, MIXED, kw, batch_kw, zero, steps)
    for b in MIXED:
        _same_bits(mixed[b.name], table[b.name], "mixed / table " + b.name)
    general = _run(amd, GENERAL, kw, batch_kw, zero, steps)
    for b in REGISTER + GENERAL:
        alone = _run(amd, [b], kw, batch_kw, zero, steps)
        _same_bits(alone[b.name], (table if b in REGISTER else general)[b.name],
                   "alone / batch " + b.name)
    everything = None
    if with_table_in_general:
        everything = _run(amd, REGISTER + GENERAL, kw, batch_kw, zero, steps)
    out = dict(table)
    out.update(general)
    return out, everything


# ------------------------------------------------------------------ part 1: the chain alone
@pytest.mark.parametrize("name", list(cases.CHAINS))
def test_chain_of_the_starting_image_in_every_class_and_launch_shape(amd, name):
    """Zero gradient, one application of the chain (module docstring).  Without a normalisation
    the image is the oracle's chain bit for bit; so is everything else the step leaves: the
    spectrum where it was, zero moments."""
    from scarlet_amd import _lib

    chain = cases.CHAINS[name]
    kw, batch_kw = cases.chain_spec_keywords(_lib, chain)
    steps = [(1, dict(e_rel=1e-3, prox_max_iter=1))]
    got, everything = _launch_shapes(amd, kw, batch_kw, True, steps, with_table_in_general=True)
    for b in REGISTER + GENERAL:
        x0, sed = cases.start_image(b), cases.start_spectrum(b)
        states = [got[b.name][0], everything[b.name][0]]
        for where, state in zip(("own kernel", "general kernel"), states):
            what = "%s %s %s" % (name, b.name, where)
            assert_array_equal(state["sed"], sed, err_msg=what)
            if chain.scheme != "fista":  # (FISTA keeps z in the first moment)
                for key in ("m_morph", "v_morph", "vhat_morph"):
                    assert not state[key].any(), (what, key)
            image = state["morph"]
            assert image.dtype == np.float32
            if chain.norm is None:
                assert_array_equal(image, cases.oracle_chain(x0, chain, sed), err_msg=what)
                continue
            u = cases.oracle_chain(x0, chain, sed, upto_norm=True)
            ref = cases.oracle_chain(x0, chain, sed)
            if chain.norm == "max":
                # one correctly rounded reciprocal, the maximum mapped to exactly 1 ...
                assert_array_equal(image, cases.reciprocal_max_normalisation(u), err_msg=what)
                # ... which the kernels claim to lie within one ulp of the quotient
                ulps = cases.ulp_distance(image, ref).max()
                print(what, "ulps from the oracle's division:", ulps)
                assert ulps <= 1, what
                assert image.max() == 1.0 and image.min() >= 0.0, what
            else:
                # the divisor is a sum in another order: (N - 1) u for the reordered sum of
                # non-negative terms (Higham 4.2, as tests/test_gpu_measure.py), one rounding
                # each for the reciprocal, the product and the oracle's quotient
                bound = (u.size + 2) * 2.0 ** -24
                err = np.abs(image.astype(np.float64) - ref)
                worst = (err / np.maximum(np.abs(ref.astype(np.float64)), 1e-300))[ref != 0].max()
                print(what, "relative error %.3g, bound %.3g" % (worst, bound))
                assert np.all(err <= bound * np.abs(ref.astype(np.float64))), what
                assert_array_equal(image == 0, ref == 0, err_msg=what)


# ------------------------------------------------------------------ part 2: whole steps
@pytest.mark.parametrize("case", cases.STEP_CASES)
def test_three_iterations_in_every_class_and_launch_shape(amd, case):
    """Data = noise + 1.2 x spectrum x a narrower Gaussian, weights 1 / noise^2.  Against the
    oracle: parameters within 1e-5 after the first iteration (test_first_step_exact_structure);
    after three, images and spectra within 1e-4, v_morph within 1e-3, chi^2 = loss - log_norm
    within 1e-5 relative (test_hsc_steps_vs_oracle,
    test_chain_flag_sets_three_launch_shapes_and_the_oracle); lite's loss within 3e-5
    (test_lite_chain_three_launch_shapes_and_the_oracle).  Parameters, moments and loss histories
    bit for bit between the launch shapes."""
    from scarlet_amd import _lib

    kw, batch_kw = cases.step_spec_keywords(_lib, case)
    lite = case.startswith("lite_")
    step_kw = dict(e_rel=1e-6, prox_max_iter=1) if lite else dict(e_rel=1e-3)
    steps = [(1, step_kw), (cases.N_STEPS - 1, step_kw)]
    got, _ = _launch_shapes(amd, kw, batch_kw, False, steps)
    failures = []
    for b in REGISTER + GENERAL:
        ref = cases.oracle_steps(b, case)
        first, last = got[b.name]
        figures = dict(
            first_sed=rel_err(first["sed"], ref["first"][0]),
            first_morph=np.abs(first["morph"] - ref["first"][1]).max(),
            sed=rel_err(last["sed"], ref["last"][0]),
            morph=np.abs(last["morph"] - ref["last"][1]).max())
        bounds = dict(first_sed=1e-5, first_morph=1e-5, sed=1e-4, morph=1e-4)
        assert last["loss"].shape == ref["loss"].shape == (cases.N_STEPS,)
        if lite:
            figures["loss"] = np.abs(-last["loss"] / ref["loss"] - 1).max()
            bounds["loss"] = 3e-5
        else:
            chi2 = last["loss"].astype(np.float64) - ref["log_norm"]
            chi2_ref = ref["loss"] - ref["log_norm"]
            figures["loss"] = (np.abs(chi2 - chi2_ref) / np.abs(chi2_ref)).max()
            bounds["loss"] = 1e-5
            figures["v_morph"] = rel_err(last["v_morph"], ref["last"][2])
            bounds["v_morph"] = 1e-3
            if case == "standard":
                assert last["morph"].max() == 1.0 and last["morph"].min() >= 0.0
        print(case, b.name, " ".join("%s=%.2e" % kv for kv in figures.items()))
        failures += [(b.name, key, figures[key], bounds[key]) for key in figures
                     if not figures[key] < bounds[key]]
    assert not failures, failures
