"""The loss bookkeeping of an iteration (finalize_blend) inside the grid of a persistent
update launch, against the kernel of its own (SMI_FOLD_FINALIZE=0), bit for bit.

The switches are read once per process, so every run is a fresh child process (this file as a
script): six children, started together once per module -- {folded, SMI_FOLD_FINALIZE=0} x
{SMI_PERSIST_BLOCKS=1, =3, no switch} -- each running all cases of its group and writing an .npz.
SMI_PERSIST_BLOCKS makes a launch persistent as soon as it has more full workgroups than that:
more than 12 boxes of 41^2 pixels, more than 3 x 16 boxes of 21^2.  SMI_MIXED_LIMIT=0 keeps a
small batch of two size classes on one launch per class; the group without switches (0) runs
the one launch for all small classes of a range (update_kernel_mixed).

Every case also reads back the plan of the launch that carried the bookkeeping
(smi_update_last_fold_plan_test) and asserts where it travelled: inside the persistent grid,
as trailing workgroups, or as the kernel of its own.

Frame 3 x 56 x 56 under a 5 x 5 kernel (the 64^2 fused convolution), standard monotonic boxes
(their ring plan is staged in LDS, the condition for a persistent launch).
"""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, W = 3, 56, 56
NOISE = 0.02

NONE, TRAILING, IN_GRID, SEPARATE = 0, 1, 2, 3
# name -> (group of the child: SMI_PERSIST_BLOCKS or 0, blends, boxes per blend as a list of
# sides, iterations, options); options["plan"] = (updating workgroups, persistent, bookkeeping)
# of the last launch that had a bookkeeping to place, in the folded child
CASES = {
    # more blends than workgroups: one workgroup does the bookkeeping of all six blends
    "many_blends": (1, 6, [41] * 5, 8, dict(plan=(1, 1, IN_GRID))),
    # two ranges of three blends: the second range's blends start at 3
    "second_range": (1, 6, [41] * 5, 8, dict(sub_ranges=2, plan=(1, 1, IN_GRID))),
    # the stopping rule on: blend 2 (weights near zero: its loss does not move) stops after
    # min_iter, the others go on
    "one_blend_stops": (1, 6, [41] * 5, 10, dict(check=True, min_iter=3, e_rel=1e-7, flat=2,
                                                  plan=(1, 1, IN_GRID))),
    "blend_in_state_2": (1, 6, [41] * 5, 8, dict(states=[0, 2, 0, 0, 0, 0],
                                                   plan=(1, 1, IN_GRID))),
    "blend_pauses": (1, 6, [41] * 5, 8, dict(pause_at=[99, 99, 99, 99, 3, 99], check=True,
                                              min_iter=99, plan=(1, 1, IN_GRID))),
    # ten boxes make one workgroup: not persistent, trailing workgroups as before
    "small_launch": (1, 2, [41] * 5, 8, dict(plan=(1, 0, TRAILING))),
    # two size classes, a launch each on streams of their own: the 41^2 one (16 boxes, first
    # and persistent) carries the bookkeeping, the 21^2 one (16 boxes, one workgroup) does not
    "two_classes": (1, 4, [41] * 4 + [21] * 4, 8, dict(plan=(1, 1, IN_GRID))),
    # more workgroups than blends: 60 boxes of 21^2 in two blends, three workgroups
    "more_workgroups": (3, 2, [21] * 30, 8, dict(plan=(3, 1, IN_GRID))),
    # one launch for two small classes: a range of at most 1024 components gets trailing
    # workgroups, a larger one (here 1030, below the mixed kernel's limit of 3072) the
    # bookkeeping kernel of its own in front, as before
    "mixed_small": (0, 4, [21] * 3 + [31] * 3, 8, dict(plan=(24, 0, TRAILING))),
    "mixed_large": (0, 103, [21] * 5 + [31] * 5, 8, dict(plan=(1030, 0, SEPARATE))),
}
KEYS = ("plan", "n_loss", "loss", "state", "progress_n", "converged", "sed", "morph", "m_sed", "v_sed",
        "vhat_sed", "m_morph", "v_morph", "vhat_morph")


def _scene(name):
    """Data, weights, component specs (seeded by the case's name)."""
    import scarlet_amd as amd

    _, nb, sides, _, opt = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    data = (rng.normal(0, NOISE, (nb, C, H, W))).astype(np.float32)
    weights = np.full(data.shape, 1 / NOISE ** 2, dtype=np.float32)
    if "flat" in opt:
        weights[opt["flat"]] *= np.float32(1e-12)
    comps = []
    for b in range(nb):
        blend = []
        for k, side in enumerate(sides):
            oy, ox = (int(x) for x in rng.integers(0, H - side + 1, 2))
            yy, xx = np.mgrid[:side, :side] - side // 2
            r2 = (yy / (0.15 * side)) ** 2 + (xx / (0.2 * side)) ** 2
            truth = np.exp(-0.5 * r2).astype(np.float32)
            sed = (1 + rng.random(C)).astype(np.float32)
            data[b, :, oy:oy + side, ox:ox + side] += sed[:, None, None] * truth[None]
            start = (np.exp(-0.3 * r2) * (1 + 0.2 * rng.normal(0, 1, r2.shape))).astype(np.float32)
            blend.append(amd.ComponentSpec(0.7 * sed, start, (oy, ox), sed_min_step=NOISE))
        comps.append(blend)
    kernel = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.float32)[None] / 256
    return data, weights, comps, kernel


def _run_case(name):
    import ctypes

    import scarlet_amd as amd
    from scarlet_amd import _lib

    _, nb, _, n_iter, opt = CASES[name]
    data, weights, comps, kernel = _scene(name)
    batch = amd.BlendBatch(data, weights, comps, kernel=kernel, max_iter=n_iter + 2)
    batch.set_sub_ranges(opt.get("sub_ranges", 1))
    if "states" in opt:
        batch.set_states(np.array(opt["states"]))
    # (every case sets the pause counters: the convergence flags exist from then on)
    batch.set_pause_at(np.array(opt.get("pause_at", [99] * nb)))
    batch.step(0, n_iter, e_rel=opt.get("e_rel", 1e-3), min_iter=opt.get("min_iter", 1),
               check_convergence=opt.get("check", False))
    loss = batch.loss_history()
    state, n = batch.progress()
    plan = np.zeros(8, dtype=np.int64)
    _lib.check(_lib.load().smi_update_last_fold_plan_test(_lib.ptr(plan, ctypes.c_int64)))
    out = dict(plan=plan, n_loss=np.array([len(x) for x in loss]), state=state, progress_n=n,
               converged=batch.converged(), loss=np.concatenate(loss))
    sed, morphs = batch.parameters()
    out["sed"] = np.asarray(sed)
    out["morph"] = np.concatenate([np.ravel(m) for m in morphs])
    for key, val in batch.moments().items():
        if key in KEYS:
            out[key] = (np.concatenate([np.ravel(x) for x in val]) if isinstance(val, (list, tuple))
                        else np.asarray(val))
    batch.close()
    return out


def _child_main(grid, path):
    sys.path.insert(0, ROOT)
    out = {}
    for name, case in CASES.items():
        if case[0] == grid:
            for key, val in _run_case(name).items():
                out[name + "/" + key] = val
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(folded, group): arrays of the child's cases}: six child processes side by side."""
    tmp = tmp_path_factory.mktemp("update_fold")
    base = {k: v for k, v in os.environ.items()
            if not k.startswith("SMI_") and k != "SCARLET_AMD_LIB"}
    procs, out = {}, {}
    try:
        for folded in (True, False):
            for grid in (1, 3, 0):
                env = dict(base)
                if grid:
                    env.update(SMI_PERSIST_BLOCKS=str(grid), SMI_MIXED_LIMIT="0")
                if not folded:
                    env["SMI_FOLD_FINALIZE"] = "0"
                path = str(tmp / ("%d_%d.npz" % (folded, grid)))
                procs[folded, grid] = (path, subprocess.Popen(
                    [sys.executable, os.path.abspath(__file__), str(grid), path], env=env,
                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for key, (path, proc) in procs.items():
            # (a child takes a few seconds, most of them the start of the runtime)
            log, _ = proc.communicate(timeout=120)
            assert proc.returncode == 0, (key, log[-3000:])
            out[key] = dict(np.load(path))
    finally:
        for _, proc in procs.values():
            if proc.poll() is None:
                proc.kill()
                proc.communicate()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bookkeeping_in_the_update_grid_gives_the_bits_of_its_own_kernel(runs, name):
    grid, nb, sides, n_iter, opt = CASES[name]
    new, ref = runs[True, grid], runs[False, grid]
    keys = [k for k in new if k.startswith(name + "/")]
    assert sorted(keys) == sorted(name + "/" + k for k in KEYS) == sorted(
        k for k in ref if k.startswith(name + "/"))
    for k in keys:
        if k.endswith("/plan"):
            continue
        assert new[k].dtype == ref[k].dtype and new[k].shape == ref[k].shape, k
        assert new[k].tobytes() == ref[k].tobytes(), k
    # where the bookkeeping travelled: {pack, workgroups, persistent, staged, LDS, LDS with
    # table, table offset, bookkeeping}; the other child never had one to place
    plan = new[name + "/plan"]
    print(name, "plan", plan)
    assert (plan[1], plan[2], plan[7]) == opt["plan"], plan
    assert plan[3] == (1 if grid else 0)  # (a staged ring plan: the condition for persistent)
    assert ref[name + "/plan"][7] == NONE
    n_loss, state = new[name + "/n_loss"], new[name + "/state"]
    conv = new[name + "/converged"]
    print(name, "n_loss", n_loss, "state", state, "converged", conv)
    assert np.array_equal(n_loss, new[name + "/progress_n"])
    assert np.all(np.isfinite(new[name + "/loss"])) and np.all(np.isfinite(new[name + "/morph"]))
    # the bookkeeping ran exactly once per blend and iteration
    expect = np.full(nb, n_iter)
    if name == "one_blend_stops":
        # (the rule fires at the first iteration it may: local iteration min_iter + 1)
        expect[opt["flat"]] = opt["min_iter"] + 2
        assert conv[opt["flat"]] == 1 and conv.sum() == 1
        assert state[opt["flat"]] == 2 and np.all(np.delete(state, opt["flat"]) == 0)
    elif name == "blend_in_state_2":
        expect[1] = 0
        assert state[1] == 2
    elif name == "blend_pauses":
        expect[4] = opt["pause_at"][4] + 1
        assert state[4] == 2 and conv.sum() == 0
    assert np.array_equal(n_loss, expect), (n_loss, expect)


if __name__ == "__main__":
    _child_main(int(sys.argv[1]), sys.argv[2])
