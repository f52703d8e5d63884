"""``fit_blends``: many ``Blend`` objects fitted in one device batch per group of blends whose
own frames get the same convolution (reference: the per-blend loop of
scarlet/testing/api.py:216-224, every blend through ``Blend.fit``, blend.py:85-198).  The batch
stays on the device for the whole call: resize test and resize on the device, every blend at its
own iteration counter and pausing at its own hooks; ``Blend.fit`` takes the same path for one
blend.

``_fit_blends_on`` sorts the blends (``_sort_blends``: ``_classify``, ``_group_key``) into those
``Blend.fit``'s own loop has to fit and groups that share bands, kernel cube shape and the
convolution plan of their own frame, each opened by ``_open_batch``: frames of different sizes
are padded to the largest of the group (``_pad_cubes``) and clipped on the device
(``BlendBatch(frame_shapes=..., frame_kinds="all")``), frames of one size open the batch they
always opened.  ``_fit_group_resident`` is the loop of a group; what it decides is plain NumPy on
plain arrays, tested without a device: how far every blend runs in the next launch
(``_plan_round``, on ``blend._next_round``), which boxes shrink or grow and to which size (``_resize_candidates``, on the rules of ``morphology.py``), the
rows the device resizes by itself (``_device_rows``).  ``_host_visit`` runs ``update()`` of the
sources the device does not stand for, ``_component_table`` holds what the loop tracks per
component and ``_write_back`` brings the device's state to the Python objects."""

import functools
import logging
import os
from types import SimpleNamespace

import numpy as np

from .batch import BlendBatch, _conv_plan
from .blend import (Blend, _adaprox_options, _at_hook, _flatten, _mark_std, _next_round,
                    _update_sources)
from .component import CombinedComponent, FactorizedComponent
from .model import Model, UpdateException
from .morphology import (ImageMorphology, Morphology, _edge_pull, _margin_of_empty,
                         get_minimal_boxsize)
from .parameter import Parameter
from .renderer import ConvolutionRenderer, NullRenderer, ResolutionRenderer

logger = logging.getLogger("scarlet_amd.blend")


def _export_state(blend):
    """What a fit changes on a Blend, as plain picklable data: the loss history and, per
    factorized component, the box of the morphology and both children's Parameters
    (values, m / v / vhat / std, halved steps after a resize)."""
    comps = _flatten(blend.sources)
    return dict(loss=list(blend.loss),
                comps=[(c.children[1].bbox.origin, c.children[1].bbox.shape,
                        c.children[0]._parameters, c.children[1]._parameters) for c in comps])


def _refresh_boxes(node):
    """Boxes of the containers after their morphologies changed (component.py:172-185,
    280-290: only a container below which a box changed gets a new one)."""
    if isinstance(node, FactorizedComponent):
        box = node._joint_box(*node.children)
        changed = box != node.bbox
        if changed:
            node.bbox = box
        return changed
    changed = [_refresh_boxes(c) for c in node.children]
    if any(changed) and isinstance(node, CombinedComponent):
        node.bbox = node._union_box()
    return any(changed)


def _import_state(blend, state):
    """Apply ``_export_state`` of another process' copy of ``blend``."""
    blend.loss[:] = state["loss"]
    for comp, (origin, shape, p_spec, p_morph) in zip(_flatten(blend.sources), state["comps"]):
        spectrum, morphology = comp.children
        morphology.bbox.origin, morphology.bbox.shape = tuple(origin), tuple(shape)
        for mine, theirs in zip(spectrum._parameters, p_spec):
            mine[...] = theirs
            mine.__dict__.update(theirs.__dict__)
        # a resized image is a new Parameter (morphology.py:155-163, 180-193); a parameter
        # the morphology also holds by name (``shift``) keeps its identity
        new = []
        for mine, theirs in zip(morphology._parameters, p_morph):
            if mine.shape == theirs.shape:
                mine[...] = theirs
                mine.__dict__.update(theirs.__dict__)
                new.append(mine)
            else:
                new.append(theirs)
        morphology._parameters = tuple(new)
    for src in blend.sources:
        _refresh_boxes(src)


def fit_blends(blends, max_iter=200, e_rel=1e-3, min_iter=1, devices=None, _report=None,
               **alg_kwargs):
    """Fit many independent ``Blend`` objects together.

    Equivalent to ``[b.fit(max_iter, e_rel, min_iter, **alg_kwargs) for b in blends]``
    -- same per-blend iteration counts, losses, parameter and optimizer-state side
    effects -- but blends that share the number of bands, the shape of the difference-kernel
    cube and the convolution plan of their OWN frame (path, FFT shape and fused-kernel
    variant: ``plan_fit_blends``) run in one device batch, whatever their frame sizes, so
    every kernel launch works on all of them (the batched path the benchmark measures,
    behind the reference's per-blend API).  Frames of different sizes are padded to the
    largest of their group with data 0 and weight 0, and every component -- images, point
    sources, shifting, starlet and profile components -- is clipped to its blend's own
    frame on the device (``BlendBatch(frame_shapes=..., frame_kinds="all")``): a blend gets what
    ``Blend.fit`` gives it alone, whatever list it is in -- bit for bit on the fused
    convolution path; frames too large for it go through rocFFT, where the loss is summed in
    blocks of the padded plane and a padded blend's losses are those of its own fit to the
    rounding of that float64 sum.  Blends without a convolution
    (``NullRenderer``) share a batch when their frames are equal.  Blends with observations on a
    coarser pixel grid (``ResolutionRenderer`` on the spectral path) share a batch when they also
    agree in their exact frame and in the shape classes of these observations; every launch of
    the low-resolution chain then works on all of them, each with its own operators, and every
    blend keeps the bits of its own ``Blend.fit`` (``plan_fit_blends``).  The box-resizing hook
    and the restart it triggers (blend.py:196-198, 284-292) stay per blend: after every
    round the blends are regrouped by their own iteration counter.

    ``devices``: where the blends run (the reference's unit is the per-blend
    loop of ``testing/api.py:216-224``).  ``None`` / an int: one GPU.  A list of GPU
    indices: contiguous shards ``dist.shard_range(len(blends), i, len(devices))``, one
    host thread per GPU.  ``"ranks"``: one process per GPU under ``torch.distributed``
    (every rank holds the same list of blends): rank r fits its shard on GPU LOCAL_RANK
    and the fitted state of every blend is all-gathered, so all ranks return the same
    results and hold the same parameters.  Results do not depend on the partition.

    Returns the list of ``(n_iter, logL)`` tuples; a blend whose parameters turned
    non-finite gets ``(n_iter, nan)`` (and keeps the state of its last iteration), the
    others continue; ``fit_blends.errors`` lists ``(index, ArithmeticError)`` of the last call.

    ``_report``: a dict that receives what the call did -- ``"groups"`` and ``"alone"`` as
    ``plan_fit_blends`` returns them and ``"batches"``, the number of ``BlendBatch`` objects
    the groups opened (with ``devices="ranks"``: of this rank's shard).
    """
    blends = list(blends)
    kw = dict(max_iter=max_iter, e_rel=e_rel, min_iter=min_iter, **alg_kwargs)
    fit_blends.errors = []
    report = dict(groups=[], alone={}, batches=0, operator_bytes=[])
    if _report is not None:
        _report.clear()
        _report.update(report)
        report = _report
    if isinstance(devices, str):
        if devices != "ranks":
            raise ValueError("devices must be None, an int, a list of GPU indices or 'ranks'")
        from . import dist as sdist

        rank, local_rank, world = sdist.env_rank()
        if not sdist._active():
            if world > 1:
                raise RuntimeError("fit_blends(devices='ranks') under WORLD_SIZE={} needs an "
                                   "initialised process group (scarlet_amd.dist."
                                   "init_process_group)".format(world))
            rank, world = 0, 1
        lo, hi = sdist.shard_range(len(blends), rank, world)
        # a rank that fails must still take part in the collective, or the others hang in it:
        # its exception travels as text and every rank raises together
        try:
            part = {}
            mine, errs = _fit_blends_on(blends[lo:hi], local_rank, _report=part, **kw)
            _merge_report(report, part, lo)
            part = dict(lo=lo, results=mine, errors=[(lo + i, str(e)) for i, e in errs],
                        states=[_export_state(b) for b in blends[lo:hi]], failed=None)
            import pickle

            pickle.dumps(part)
        except Exception as e:  # noqa: BLE001 -- re-raised on every rank below
            part = dict(lo=lo, results=[], errors=[], states=[],
                        failed="rank {}: {}: {}".format(rank, type(e).__name__, e))
        parts = sdist.gather_objects(part)
        failed = [p["failed"] for p in parts if p["failed"]]
        if failed:
            raise RuntimeError("fit_blends(devices='ranks') failed: " + "; ".join(failed))
        out = []
        for part in parts:
            out.extend(part["results"])
            fit_blends.errors.extend((i, ArithmeticError(msg)) for i, msg in part["errors"])
            if part["lo"] != lo:
                for blend, state in zip(blends[part["lo"]:], part["states"]):
                    _import_state(blend, state)
                    _mark_std(blend.parameters)
        return out
    if devices is None or np.isscalar(devices) or len(devices) == 1:
        device = 0 if devices is None else int(devices if np.isscalar(devices) else devices[0])
        # A thousand blends are a few million live Python objects, none of them garbage; the
        # cyclic collector would walk them again and again while the loop below allocates
        # its temporaries (measured: a quarter of the call).  Reference counting still frees
        # everything the loop drops.
        # gc.freeze() takes what exists now out of the collector's generations for the duration
        # of the call; the collector itself stays on (other threads, callbacks).  gc.unfreeze()
        # empties the WHOLE permanent generation, so the call keeps its hands off when the
        # application froze objects itself (a pre-fork server) or another fit_blends is running.
        import gc

        with _freeze_lock:
            mine = gc.get_freeze_count() == 0 and not _freeze_users[0]
            if mine:
                gc.freeze()
            if mine or _freeze_users[0]:
                _freeze_users[0] += 1
                mine = True
        try:
            out, fit_blends.errors = _fit_blends_on(blends, device, _report=report, **kw)
        finally:
            if mine:
                with _freeze_lock:
                    _freeze_users[0] -= 1
                    if not _freeze_users[0]:
                        gc.unfreeze()
        return out
    from concurrent.futures import ThreadPoolExecutor
    from .dist import shard_range

    cuts = [shard_range(len(blends), i, len(devices)) for i in range(len(devices))]
    parts = [{} for _ in cuts]
    with ThreadPoolExecutor(len(devices)) as pool:
        jobs = [pool.submit(_fit_blends_on, blends[lo:hi], int(dev), _report=rep, **kw)
                for (lo, hi), dev, rep in zip(cuts, devices, parts)]
        out = []
        for (lo, _), job, rep in zip(cuts, jobs, parts):
            part, errs = job.result()
            _merge_report(report, rep, lo)
            out.extend(part)
            fit_blends.errors.extend((lo + i, e) for i, e in errs)
    return out


fit_blends.errors = []


def _merge_report(report, part, lo):
    """The report of the shard that starts at blend ``lo`` into the report of the call."""
    report["groups"].extend((key, [lo + i for i in idx]) for key, idx in part.get("groups", []))
    report.setdefault("operator_bytes", []).extend(part.get("operator_bytes", []))
    report["alone"].update((lo + i, why) for i, why in part.get("alone", {}).items())
    report["batches"] += part.get("batches", 0)


def plan_fit_blends(blends, max_iter=200, e_rel=1e-3, min_iter=1, devices=None, details=False,
                    **alg_kwargs):
    """``(groups, alone)`` of ``fit_blends(blends, ...)`` with the same arguments, without a
    GPU: ``groups``, a list of ``(key, positions)`` -- the blends of every device batch, in the
    order the batches are opened and in list order inside a group -- and ``alone``,
    ``{position: reason}`` of the blends ``Blend.fit``'s own loop fits one at a time.
    ``key = (bands, kernel cube shape, (conv_path, Fy, Fx, zb))``: the convolution plan is
    that of the blend's own frame (``_conv_plan``), so the frames of a group may differ;
    without a kernel (``NullRenderer``) the plan is ``(None, h, w, 0)``, the frame itself.
    A blend with observations on coarser grids (``ResolutionRenderer``, all on the spectral
    path) has three more entries in its key: its exact frame ``(h, w)`` -- such a group is never
    padded --, the shape classes ``(C, n_a, n_b, Fy, Fx)`` of these observations in order and
    their number.  Such a group is cut so that the transformed operators of one batch stay
    within ``LOWRES_OPERATOR_CAP`` bytes: every part is an entry of ``groups`` (a batch) under
    the same key.  ``details=True`` returns a third item, the bytes of these operators per
    entry of ``groups`` (0 without such observations).
    With a list of ``devices`` every shard (``dist.shard_range``) has groups of its own.
    Like the fit, the call prepares the blends' device descriptions and drops what an earlier
    ``fit`` left of its scheme on them."""
    blends = list(blends)
    if isinstance(devices, str) and devices != "ranks":
        raise ValueError("devices must be None, an int, a list of GPU indices or 'ranks'")
    if isinstance(devices, str):
        from . import dist as sdist

        rank, _, world = sdist.env_rank()
        if not sdist._active():
            rank, world = 0, 1
        cuts = [sdist.shard_range(len(blends), rank, world)]
    elif devices is None or np.isscalar(devices) or len(devices) == 1:
        cuts = [(0, len(blends))]
    else:
        from .dist import shard_range

        cuts = [shard_range(len(blends), i, len(devices)) for i in range(len(devices))]
    report = dict(groups=[], alone={}, batches=0, operator_bytes=[])
    for lo, hi in cuts:
        part = {}
        _sort_blends(blends[lo:hi], dict(alg_kwargs), part)
        _merge_report(report, part, lo)
    if details:
        return report["groups"], report["alone"], report["operator_bytes"]
    return report["groups"], report["alone"]


def _device_hook_covers(node):
    """True when everything ``node.update()`` can do is an ``ImageMorphology.update`` of a
    factorized component (no shift, no point source) below it -- what the device's resize test
    stands for.  Any other ``update`` in the tree (a user subclass) keeps the blend on the path
    that calls every hook on the host."""
    if isinstance(node, FactorizedComponent):
        spectrum, morphology = node.children
        return (type(node).update is FactorizedComponent.update
                and type(spectrum).update is Model.update
                and type(morphology).update is ImageMorphology.update
                and not getattr(morphology, "shifting", False))
    if isinstance(node, CombinedComponent):
        return (type(node).update is CombinedComponent.update
                and all(_device_hook_covers(c) for c in node.children))
    return False


def _pad_cubes(cubes):
    """``(n, C, H, W)`` float32: the ``(C, h, w)`` cubes in the top left corners of planes of
    the largest ``h`` and the largest ``w``, zeros beyond."""
    H, W = max(c.shape[1] for c in cubes), max(c.shape[2] for c in cubes)
    out = np.zeros((len(cubes), cubes[0].shape[0], H, W), dtype=np.float32)
    for i, c in enumerate(cubes):
        out[i, :, :c.shape[1], :c.shape[2]] = c
    return out


def _open_batch(runs, specs, flat, capacity, device, opt, report=None):
    """The device batch of a group of blends (``_group_key``): their observation cubes stacked,
    the components ``flat`` described by ``specs`` (per blend), room for ``capacity`` losses
    per blend, the blends' loss constants, the state stored on the Parameters and the
    optimizer constants ``opt``.  Frames of different sizes are padded to the largest (data 0,
    weight 0) and become the batch's frame extents; the convolution is the one every member's
    own frame gets (the padded frame might pick another).  ``report["batches"]`` counts."""
    data, weights, kernel = zip(*(r.obs for r in runs))
    frames = [tuple(d.shape[1:]) for d in data]
    ragged = {}
    if len(set(frames)) > 1:
        path, fy, fx, _ = _conv_plan(*frames[0], kernel[0].shape)
        ragged = dict(fft_shape=(fy, fx), conv_path=path, frame_shapes=frames,
                      frame_kinds="all")
        data, weights = _pad_cubes(data), _pad_cubes(weights)
    else:
        data, weights = np.stack(data), np.stack(weights)
    batch = BlendBatch(data, weights, specs,
                       kernel=None if kernel[0] is None else np.stack(kernel),
                       max_iter=capacity, device=device, **ragged)
    if report is not None:
        report["batches"] = report.get("batches", 0) + 1
    try:
        # observations on coarser pixel grids: terms of their own blend, evaluated together per
        # shape class (the group shares frame and classes: _group_key)
        for i, r in enumerate(runs):
            for obs, idx in r.lowres:
                batch.attach_lowres(obs.renderer._operators(), idx, obs.data, obs.weights,
                                    obs.log_norm, blend=i)
        if any(r.blend._loss_constant for r in runs):
            batch.add_loss_constant([r.blend._loss_constant for r in runs])
        Blend._upload_state(batch, flat)
        batch.set_optimizer(**opt)
    except BaseException:
        batch.close()
        raise
    return batch


def _fit_group_rebuilt(group, device, max_iter, opt, step_kw, report=None):
    """Blends of one group (``_group_key``), with components the resident path does not cover
    (point sources, free shifts, starlet and profile components): a device batch per round and
    iteration counter, state over the host in between."""
    while True:
        todo = [r for r in group if r.result is None and r.total < max_iter]
        if not todo:
            return
        by_local = {}
        for r in todo:
            by_local.setdefault(r.local, []).append(r)
        for local, part in by_local.items():
            comps = [_flatten(r.blend.sources) for r in part]
            flat = [c for cs in comps for c in cs]
            n = _next_round(local, min(max_iter - r.total for r in part))
            batch = _open_batch(part, [r.blend._specs(c) for r, c in zip(part, comps)], flat, n,
                                device, opt, report)
            try:
                if local > 0:  # the stopping rule compares with the loss before this round
                    batch.set_previous_loss(np.array([r.blend.loss[-1] for r in part]))
                batch.step(local, n, check_convergence=True, **step_kw)
                states = batch.states()
                losses = batch.loss_history()
                Blend._download_all(batch, flat)
            finally:
                batch.close()
            for r, state, loss in zip(part, states, losses):
                blend = r.blend
                blend.loss.extend(loss)
                done = len(loss)
                if state == 3:
                    r.result = ArithmeticError("parameters of the blend are not finite")
                    continue
                r.local = local + done
                restart = done == n and _at_hook(r.local) and _update_sources(blend.sources)
                if restart:
                    r.base, r.local = len(blend.loss), 0
                elif state == 2 or r.total >= max_iter:
                    r.result = True


# fit_blends calls that share the gc.freeze() of the first of them (see there)
_freeze_lock = __import__("threading").Lock()
_freeze_users = [0]


def _device_resize_covers(blend, flat=None):
    """True when the device can also carry out every resize below ``blend``
    (``smi_batch_update_components`` with keep = 2 / 3): stock ``shrink_box``, odd square boxes,
    a constant step on float32 / float64 images.  ``flat``: the blend's components, if the
    caller has them already."""
    for c in (_flatten(blend.sources) if flat is None else flat):
        morphology = c.children[1]
        image = morphology._parameters[0]
        h, w = morphology.bbox.shape[-2:]
        if (type(morphology).shrink_box is not Morphology.shrink_box or h != w or h % 2 == 0
                or h > 1000 or image.dtype not in (np.float32, np.float64)):
            return False
        if morphology.resizing and not image.fixed and not isinstance(image.step, (int, float)):
            return False
    return True


def _component_table(group, comps, host_resize=False):
    """What the resident loop tracks per component of a group, built once from the Python
    objects (``comps``: the components of every blend).  ``first``: index of each blend's first
    component (and the total behind them); ``blend_of`` / ``source_of``: the blend and the
    source (counted through the group) above a component -- ``update()`` of a source stops at
    its first child that resizes (component.py:172-185); ``resizable``: may ``update()`` act;
    ``on_device`` (per blend): the device resizes its boxes by itself (``host_resize``: none
    does, the development switch).  What the host follows for those: ``origin``, the constant
    ``step`` of the image (nan for a step rule of its own), ``wide`` (a float64 host image) and
    ``moved``, set once the device has resized the box."""
    flat = [c for cs in comps for c in cs]
    images = [c.children[1]._parameters[0] for c in flat]
    first = np.concatenate([[0], np.cumsum([len(c) for c in comps])]).astype(np.int64)
    # (a source is one factorized component or a combined one: no second walk through the tree
    # for the common case)
    below = np.array([1 if isinstance(src, FactorizedComponent) else len(_flatten([src]))
                      for r in group for src in r.blend.sources], dtype=np.int64)
    return SimpleNamespace(
        first=first,
        blend_of=np.repeat(np.arange(len(group)), np.diff(first)),
        source_of=np.repeat(np.arange(len(below)), below),
        on_device=np.array([not host_resize and _device_resize_covers(r.blend, cs)
                            for r, cs in zip(group, comps)], dtype=bool),
        resizable=np.array([bool(c.children[1].resizing) and not image.fixed
                            for c, image in zip(flat, images)], dtype=bool),
        origin=np.array([c.children[1].bbox.origin[-2:] for c in flat],
                        dtype=np.int64).reshape(-1, 2),
        step=np.array([float(image.step) if isinstance(image.step, (int, float)) else np.nan
                       for image in images]),
        wide=np.array([image.dtype == np.float64 for image in images], dtype=bool),
        moved=np.zeros(len(flat), dtype=bool))


def _plan_round(state, left, local, g, lockstep=False):
    """The next launch of the resident batch, whose iteration counter stands at ``g``, from
    what is known per blend: ``state`` (0 iterating, 2 finished, 3 failed), the iterations
    ``left`` of its budget and the ``local`` counter of its adaprox call.  None when no blend
    is live.  Otherwise ``live``; ``quota``: every live blend runs up to ITS next resize hook
    or to the end of its budget (``_next_round``) -- the device pauses it there, after counter
    ``pause_at``, while its batch mates go on in the same ``n`` iterations of the launch;
    ``states`` (a blend out of budget counts as finished) and counter ``base`` for the device.
    ``lockstep`` (development switch): all blends to the nearest hook of any of them."""
    live = (state == 0) & (left > 0)
    if not live.any():
        return None
    quota = _next_round(local, left)
    if lockstep:
        quota = np.full(len(local), int(quota[live].min()))
    return SimpleNamespace(
        live=live, quota=quota, n=int(quota[live].max()),
        states=np.where((state == 0) & ~live, 2, state).astype(np.int32),
        base=np.where(live, g - local, 0), pause_at=np.where(live, g + quota - 1, -1))


_NO_PIXEL = np.iinfo(np.int32).max  # margin of an image without a pixel > 0 (scarlet_amd.h)


def _resize_candidates(margin, pull, shapes, step, at_hook):
    """What ``ImageMorphology.update`` (morphology.py:132-207) would do to the components
    ``at_hook``, from the device's two reductions (``BlendBatch.resize_test``: the empty
    ``margin`` and the largest ``pull`` over an edge), the box ``shapes`` and the constant
    ``step`` of every image: ``(shrink, grow, standard, close)``.  ``standard``: the standard
    size that holds the occupied pixels, the new size of a box that shrinks.  An image with a
    step rule of its own (``step`` nan) always counts as growing: the device's pull is taken
    with the constant step, so the host's ``update()`` has to see it.  ``close``: indices of
    growing components whose pull lies within 1e-6 (relative) of the threshold 0.1; the
    host's own ``_edge_pull`` has the last word on these."""
    size = shapes.max(axis=1)
    margin = np.where(margin == _NO_PIXEL, _margin_of_empty(shapes.min(axis=1)), margin)
    standard = get_minimal_boxsize(size - 2 * margin)
    shrink = at_hook & (standard < size)
    grow = at_hook & ~shrink & ((pull > 0.1 * (1 - 1e-6)) | np.isnan(step))
    return shrink, grow, standard, np.flatnonzero(grow & (pull < 0.1 * (1 + 1e-6)))


def _device_rows(dev, shrink, standard, size, source_of, wide, origin, step):
    """The rows the device resizes by itself, of the candidates ``dev``: exactly one per
    source, its first (``CombinedComponent.update`` stops at the first child that resizes).
    ``(resized, keep)``: what ``BlendBatch.update_components`` takes for them -- ``rows`` with
    the new ``size`` (``standard`` for a box that shrinks, the next standard size for one
    that grows), the origin moved by the inset (< 0: the pad of a growing box) and the halved
    step -- and their ``keep`` codes, 2 for a float32 host image, 3 for a float64 one."""
    rows = np.flatnonzero(dev)
    rows = rows[np.unique(source_of[rows], return_index=True)[1]]
    new_size = np.where(shrink[rows], standard[rows], get_minimal_boxsize(size[rows] + 1))
    new_origin = origin[rows] + ((size[rows] - new_size) // 2)[:, None]
    return (dict(rows=rows, origin_y=new_origin[:, 0], origin_x=new_origin[:, 1], size=new_size,
                 morph_step=step[rows] / 2), np.where(wide[rows], 3, 2))


def _host_visit(batch, group, flat, specs, t, wanted, hook):
    """The blends at a ``hook`` that the device does not resize: the sources with a
    ``wanted`` component below them get their records from the device and have ``update()``
    run (``update()`` of the others is a no-op by the device's test; a source is visited as a
    whole, the reference stops at its first child that resizes) -- the host keeps the last
    word.  Returns the blends that restart, the rows of the component table that take their
    state from the host (a component whose image Parameter was replaced: sliced or padded,
    step halved; ``flat`` and ``specs`` are brought up to date) and their state records."""
    visit = [i for i in np.flatnonzero(hook & ~t.on_device).tolist()
             if wanted[t.first[i]:t.first[i + 1]].any()]
    calls = []  # (blend, source, indices of the components below it)
    for i in visit:
        k = int(t.first[i])
        for src in group[i].blend.sources:
            n = len(_flatten([src]))
            if wanted[k:k + n].any():
                calls.append((i, src, np.arange(k, k + n)))
            k += n
    rows, states = [], []
    if not calls:
        return rows, rows, states
    idx = np.concatenate([below for _, _, below in calls])
    for k, rec in zip(idx, batch.component_states(idx)):
        _record_to_parameters(flat[k], rec)
    before = {i: [c.children[1]._parameters[0] for c in flat[t.first[i]:t.first[i + 1]]]
              for i in visit}
    changed = set()
    for i, src, _ in calls:
        try:
            src.update()
        except UpdateException:
            changed.add(i)
    for i in sorted(changed):
        lo = int(t.first[i])
        flat[lo:t.first[i + 1]] = _flatten(group[i].blend.sources)
        for j, image in enumerate(before[i]):
            c = flat[lo + j]
            if c.children[1]._parameters[0] is not image:
                specs[i][j] = _resized_spec(specs[i][j], c)
                rows.append(lo + j)
                states.append(_parameters_to_record(c))
    return sorted(changed), rows, states


def _write_back(batch, group, flat, t):
    """Device -> Python objects: new image Parameters (morphology.py:155-163, 180-193) and
    boxes of the components the device has resized, then all values, moments and the losses
    recorded since the fit began."""
    for k in np.flatnonzero(t.moved):
        morphology = flat[k].children[1]
        image = morphology._parameters[0]
        shape = tuple(batch._shapes[k])
        morphology._parameters = (
            Parameter(np.zeros(shape, dtype=image.dtype), name=image.name, prior=image.prior,
                      constraint=image.constraint, step=float(t.step[k]), fixed=image.fixed),
        ) + morphology._parameters[1:]
        morphology.bbox.origin = tuple(int(o) for o in t.origin[k])
        morphology.bbox.shape = shape
    if t.moved.any():
        sources = [src for r in group for src in r.blend.sources]
        for j in np.unique(t.source_of[t.moved]):
            _refresh_boxes(sources[j])
    Blend._download_all(batch, flat)
    history = batch.loss_history()
    n_loss = batch.progress()[1]
    for i, r in enumerate(group):
        r.blend.loss.extend(history[i][:n_loss[i]])


def _fit_group_resident(group, device, max_iter, opt, step_kw, mode=None, report=None):
    """Blends of one group (``_group_key``), factorized image components only: ONE
    device batch for the whole fit, and every launch steps ALL blends that are still
    iterating.  The observation is uploaded once.  A blend whose boxes change starts its
    adaprox call anew (blend.py:276-302) while its batch mates go on: the device keeps the
    counter at which each blend's call began (``smi_batch_set_iteration_base``), and blends
    whose calls restarted at different times do not stop each other at every hook of any of
    them (``_plan_round``; 1024 benchmark blends: 12 rounds instead of 32).  At a resize
    hook the device evaluates the two reductions ``ImageMorphology.update`` decides on for
    every component (``smi_batch_resize_test``, ``_resize_candidates``); for blends made of the
    stock classes the resize itself -- centred slice, or zero-padded moments and a
    ``linear_ramp``-padded image, step halved (morphology.py:132-207) -- also happens on the
    device (``_device_rows``, ``smi_batch_update_components`` with keep = 2 / 3) and the Python
    objects learn their new boxes when the fit is over (``_write_back``).  Other blends in
    which a box may change come to the host and go back as new rows of the component table
    (``_host_visit``, keep = 0).  ``mode``: the development switch of ``_fit_blends_on``.

    When a launch or a host hook raises, what the device holds -- boxes it resized,
    parameters, moments, the losses of the iterations that ran -- still reaches the Python
    objects, so that no blend is left with a box its Parameters do not fit."""
    nb = len(group)
    comps = [_flatten(r.blend.sources) for r in group]
    flat = [c for cs in comps for c in cs]
    specs = [r.specs for r in group]
    t = _component_table(group, comps, host_resize=mode == "host-resize")
    prior = np.array([len(r.blend.loss) for r in group])  # losses of earlier fits
    base = np.zeros(nb, dtype=np.int64)
    local = np.zeros(nb, dtype=np.int64)
    count = np.zeros(nb, dtype=np.int64)  # losses recorded on the device so far
    state = np.zeros(nb, dtype=np.int32)  # 0 iterating, 2 finished, 3 failed
    g = 0  # the batch's iteration counter: blend i is at g - (its counter base) = local[i]
    pushed = (None, None)  # what the device holds as per-blend states / counter bases
    batch = _open_batch(group, specs, flat, max(max_iter, 1), device, opt, report)
    try:
        while True:
            plan = _plan_round(state, max_iter - base - local, local, g, mode == "lockstep")
            if plan is None:
                break
            live = plan.live
            batch.set_round(*[new if old is None or not np.array_equal(old, new) else None
                              for old, new in zip(pushed, (plan.states, plan.base))],
                            plan.pause_at)
            batch.step(g, plan.n, check_convergence=True, **step_kw)
            g += plan.n
            now, cnt, stopped = batch.round()
            done = cnt - count
            count = cnt.astype(np.int64)
            local[live] += done[live]
            # failed / stopped by its own rule / paused: goes on
            state[live] = np.where(now[live] == 3, 3, np.where(stopped[live] != 0, 2, 0))
            pushed = (now.astype(np.int32), plan.base)
            hook = live & (now != 3) & (done == plan.quota) & _at_hook(local)
            if not hook.any() or not t.resizable.any():
                continue
            margin, pull = batch.resize_test()
            shapes = np.array(batch._shapes)
            shrink, grow, standard, close = _resize_candidates(
                margin, pull, shapes, t.step, hook[t.blend_of] & t.resizable)
            # -- blends of the stock classes: the device resizes
            dev = (shrink | grow) & t.on_device[t.blend_of]
            close = close[dev[close]]
            if close.size:  # the host's own arithmetic on the edges of these few
                for k, rec in zip(close, batch.component_states(close)):
                    edges = _edge_pull(rec["morph"], rec["m_morph"].astype(np.float64),
                                       rec["v_morph"].astype(np.float64), t.step[k])
                    grow[k] = dev[k] = bool(np.any(edges > 0.1))
            if not (shrink | grow).any():
                continue
            resized, codes = _device_rows(dev, shrink, standard, shapes.max(axis=1),
                                          t.source_of, t.wide, t.origin, t.step)
            rows = resized["rows"]
            t.origin[rows, 0], t.origin[rows, 1] = resized["origin_y"], resized["origin_x"]
            t.step[rows], t.moved[rows] = resized["morph_step"], True
            # -- the others: over the host
            changed, from_host, states = _host_visit(
                batch, group, flat, specs, t, (shrink | grow) & ~t.on_device[t.blend_of], hook)
            restart = np.zeros(nb, dtype=bool)
            restart[t.blend_of[rows]] = restart[changed] = True
            if not restart.any():
                continue
            keep = np.ones(len(flat), dtype=np.int32)
            keep[rows], keep[from_host] = codes, 0
            batch.update_components(specs, keep, states, resized=resized if rows.size else None)
            # adaprox starts anew (a restarted blend that was about to stop goes on)
            base[restart] = prior[restart] + count[restart]
            local[restart] = 0
            state[restart & (state == 2)] = 0
        _write_back(batch, group, flat, t)
    except BaseException:
        # (an error of the regular write-back itself included: it is tried once more)
        try:
            _write_back(batch, group, flat, t)
        except Exception:
            pass
        raise
    finally:
        batch.close()
    for i, r in enumerate(group):
        r.base, r.local = int(base[i]), int(local[i])
        r.result = (ArithmeticError("parameters of the blend are not finite")
                    if state[i] == 3 else True)


def _resized_spec(spec, comp):
    """The device description of a component whose box ``ImageMorphology.update`` has just
    changed: the update replaces the image Parameter by its slice or padded copy in a new box
    and halves its (constant) step (morphology.py:146-193); spectrum, constraints and everything
    else of the description stay.  Same as ``Blend._specs`` would make from scratch
    (tests/test_host_logic.py), without walking through the constraint chain again."""
    import copy

    morphology = comp.children[1]
    image = morphology._parameters[0]
    new = copy.copy(spec)
    new.morph = np.asarray(image, dtype=np.float32)
    new.origin = tuple(int(o) for o in morphology.bbox.origin[-2:])
    new.morph_step = float(image.step)
    return new


def _record_to_parameters(comp, rec):
    """A state record of the device (``BlendBatch.component_states``) into the Parameters of
    a factorized component: values in place, moments as float64 arrays."""
    sed = comp.children[0]._parameters[0]
    image = comp.children[1]._parameters[0]
    sed[...] = rec["sed"]
    sed.m, sed.v, sed.vhat = (rec[n].astype(np.float64) for n in ("m_sed", "v_sed", "vhat_sed"))
    image[...] = rec["morph"]
    image.m, image.v, image.vhat = (rec[n].astype(np.float64)
                                    for n in ("m_morph", "v_morph", "vhat_morph"))


def _parameters_to_record(comp):
    sed = comp.children[0]._parameters[0]
    image = comp.children[1]._parameters[0]
    return dict(sed=np.asarray(sed), m_sed=sed.m, v_sed=sed.v, vhat_sed=sed.vhat,
                morph=np.asarray(image), m_morph=image.m, v_morph=image.v, vhat_morph=image.vhat)


class _Run:
    """A blend in a device batch: its observation cubes, the device description of its
    components, and where its fit stands."""

    def __init__(self, blend, obs, specs, lowres=()):
        # `base + local` is the reference's `it`: 0 at the start of fit(), the length
        # of the whole loss history after a restart (blend.py:101, 198)
        self.blend, self.obs, self.specs = blend, obs, specs
        # (observation, model channels of its bands) of every ResolutionRenderer observation
        self.lowres = tuple(lowres)
        self.base, self.local, self.result = 0, 0, None

    @property
    def total(self):
        return self.base + self.local


def _classify(blend):
    """``(why, run)`` of a blend of ``fit_blends``: ``why`` it has to be fitted by itself, in
    ``Blend.fit``'s own loop -- like ``[b.fit() for b in blends]`` would
    (scarlet/testing/api.py:216-224) -- or None and its ``_Run`` in a device batch."""
    blend._psf, blend._scheme = None, ("amsgrad", 0.25)  # nothing left over from an earlier fit()
    if any(not p.fixed for obs in blend.observations for p in obs.parameters):
        return "free renderer parameters (psf_shift)", None
    if any(type(obs.renderer) not in (NullRenderer, ConvolutionRenderer, ResolutionRenderer)
           for obs in blend.observations):
        return "a user-defined renderer: Blend.fit's host-rendered mode", None
    obs = blend._observation()  # (built once: the data, weight and kernel cubes)
    if blend._extra_layers:
        # further cubes on the model's grid are terms of ONE blend's loss on the device
        # (smi_batch_add_observation)
        return "several observations of one channel", None
    if any(o.renderer.isrot for o, _ in blend._lowres):
        # its resampler evaluates the 2-D shifts in Fourier space under the dense path's
        # contract: a batch of one blend (Blend.fit attaches the renderer's own handle)
        return "a low-resolution observation on a rotated grid", None
    if any(not o.renderer.on_spectral_path() for o, _ in blend._lowres):
        # the dense products keep Fy Fx Fx n_b floats per band: a batch of one blend
        return "a low-resolution observation on the dense path", None
    specs = blend._specs(_flatten(blend.sources))  # (once: 15 us per component)
    if blend._host:  # (hoststep.py: one iteration per device call)
        return "parameters the host updates", None
    return None, _Run(blend, obs, specs, blend._lowres)


def _group_key(run):
    """What the blends of one device batch share: the number of bands, the shape of the
    difference-kernel cube (one stamp for all bands or one per band) and the convolution plan
    of the blend's OWN frame -- ``(conv_path, Fy, Fx, zb)``, ``_conv_plan`` -- so that padding
    to a batch mate's frame never changes the convolution a blend sees.  Without a kernel
    (``NullRenderer``) the plan is the frame shape itself."""
    data, _, kernel = run.obs
    key = _key_of(data.shape, None if kernel is None else kernel.shape)
    if run.lowres:
        # Observations on coarser grids (ResolutionRenderer) are terms of their blend's loss
        # that the device evaluates per shape class, and they do not combine with frame
        # extents: such a group shares the exact frame (it is never padded), the number of
        # these observations and, one by one, their classes (C, n_a, n_b, Fy, Fx).
        key += (tuple(int(n) for n in data.shape[1:]),
                tuple(obs.renderer.shape_class() for obs, _ in run.lowres), len(run.lowres))
    return key


@functools.lru_cache(maxsize=4096)
def _key_of(shape, kshape):
    # (a catalogue of equal frames asks the library once, not once per blend)
    C, h, w = (int(n) for n in shape)
    kshape = None if kshape is None else tuple(int(n) for n in kshape)
    return C, kshape, _conv_plan(h, w, kshape)


def _sort_blends(blends, alg_kwargs, report):
    """Every blend by itself (and why), or in a group: ``(prox_max_iter, opt, sorted_out,
    groups)`` -- the adaprox options parsed from ``alg_kwargs`` (which is emptied),
    ``_classify`` of every blend and ``[(key, positions)]`` in order of first appearance.
    ``report`` receives ``groups`` and ``alone`` (``plan_fit_blends``)."""
    report.update(groups=[], alone={}, batches=0, operator_bytes=[])
    if alg_kwargs.get("callback") is not None or alg_kwargs.get("scheme", "amsgrad") != "amsgrad":
        why = ("a callback" if alg_kwargs.get("callback") is not None else
               "scheme {!r}".format(alg_kwargs.get("scheme"))) + ": Blend.fit's host-stepped mode"
        report["alone"] = {i: why for i in range(len(blends))}
        return None, None, None, None
    alg_kwargs.pop("scheme", None)
    alg_kwargs.pop("callback", None)
    prox_max_iter, opt = _adaprox_options(alg_kwargs)
    sorted_out = [_classify(b) for b in blends]
    groups = {}
    for i, (why, run) in enumerate(sorted_out):
        if why is not None:
            report["alone"][i] = why
        else:
            groups.setdefault(_group_key(run), []).append(i)
    # a group with low-resolution observations is cut into batches whose pooled operators stay
    # under the cap; a blend has the same bits on either side of a cut
    report["groups"], report["operator_bytes"] = [], []
    for key, idx in groups.items():
        each = [sum(obs.renderer.operator_bytes() for obs, _ in sorted_out[i][1].lowres)
                for i in idx]
        for lo, hi in _cut_by_bytes(each, LOWRES_OPERATOR_CAP):
            report["groups"].append((key, idx[lo:hi]))
            report["operator_bytes"].append(int(sum(each[lo:hi])))
    return prox_max_iter, opt, sorted_out, report["groups"]


# Device memory the transformed operators E of ONE batch may take (bytes): per low-resolution
# observation C n_a Fy Kx complex float32 (ResolutionRenderer.operator_bytes; 0.3 MB for an
# 11 x 11 observation of two bands on a 54 x 60 grid, 10.5 MB for 36 x 36 pixels of five bands
# on 120 x 120).  An MI355X has 288 GB of HBM; a fit that shards over threads or shares its card
# with other jobs should not take more than a sixteenth of it, 18 GB, of which the batch's
# other arrays (cubes, the work arrays of the pool: about a tenth of E), the upload buffers and
# the runtime need their part -- 12 GiB for E: 1 200 tutorial-sized blends or 40 000
# catalogue-sized ones in one batch, far beyond where a larger batch still gains anything.
LOWRES_OPERATOR_CAP = 12 << 30


def _cut_by_bytes(each, cap):
    """``[(lo, hi)]``: consecutive runs of a list of sizes ``each`` whose sums stay within
    ``cap`` (a single entry beyond the cap is a run of its own)."""
    cuts, lo, total = [], 0, 0
    for i, n in enumerate(each):
        if i > lo and total + n > cap:
            cuts.append((lo, i))
            lo, total = i, 0
        total += n
    if len(each) > lo:
        cuts.append((lo, len(each)))
    return cuts


def _fit_alone(blend, device, *args, **kwargs):
    """``Blend.fit`` on GPU ``device``; an ArithmeticError is returned instead of raised."""
    blend.device = device
    try:
        return blend.fit(*args, **kwargs)
    except ArithmeticError as e:
        return e


def _assemble(blends, fitted):
    """(results, [(index, error)]) of ``fit_blends`` from what is there per blend: what its own
    ``Blend.fit`` returned, the ArithmeticError that ended its fit, or its ``_Run``."""
    out, errors = [], []
    for i, (blend, res) in enumerate(zip(blends, fitted)):
        if isinstance(res, _Run):
            res = res.result
            if not isinstance(res, Exception):
                _mark_std(blend.parameters)
                res = (len(blend.loss), -blend.loss[-1])
        if isinstance(res, Exception):
            errors.append((i, res))
            res = (len(blend.loss), float("nan"))
        out.append(res)
    return out, errors


def _fit_blends_on(blends, device, max_iter=200, e_rel=1e-3, min_iter=1, _from_fit=False,
                   _report=None, **alg_kwargs):
    """``fit_blends`` of ``blends`` on GPU ``device``: (results, [(index, error)]).
    ``_from_fit``: the call comes from ``Blend.fit`` itself, which keeps a blend that has to be
    fitted by its own loop (``None, None`` is returned then).  ``_report``: the dict of
    ``fit_blends``.  The environment variable ``SCARLET_AMD_FIT_BLENDS`` is a development
    switch for A/B runs, read here once per call: ``rebuild`` (a batch per round instead of
    the resident one), ``host-resize`` (every resize over the host), ``lockstep`` (all blends
    stop at the nearest hook of any of them)."""
    args = (max_iter, e_rel, min_iter)
    report = {} if _report is None else _report
    host_stepped = dict(alg_kwargs)
    prox_max_iter, opt, sorted_out, groups = _sort_blends(blends, alg_kwargs, report)
    if sorted_out is None:
        # a callback sees every blend's parameters after every iteration, another scheme of
        # proxmin.adaprox steps on the host from the device's gradients: both are Blend.fit's
        # host-stepped modes, one blend at a time -- which is what this call stands for
        # (scarlet/testing/api.py:216-224)
        return _assemble(blends, [_fit_alone(b, device, *args, **host_stepped) for b in blends])
    mode = os.environ.get("SCARLET_AMD_FIT_BLENDS")
    # -- every blend: by itself (and why), or in a batch
    if _from_fit and any(why is not None for why, _ in sorted_out):
        return None, None
    fitted = []
    for i, (why, run) in enumerate(sorted_out):
        if why is not None:
            logger.debug("fit_blends: blend %d is fitted by itself: %s", i, why)
            run = _fit_alone(blends[i], device, *args, prox_max_iter=prox_max_iter, **opt)
        fitted.append(run)
    # -- the groups: bands, kernel cube shape and the convolution plan of the own frame
    step_kw = dict(e_rel=e_rel, min_iter=min_iter, prox_max_iter=prox_max_iter)
    for _, idx in groups:
        group = [fitted[i] for i in idx]
        if mode != "rebuild" and all(_device_hook_covers(src) for r in group
                                     for src in r.blend.sources):
            _fit_group_resident(group, device, max_iter, opt, step_kw, mode, report)
        else:
            _fit_group_rebuilt(group, device, max_iter, opt, step_kw, report)
    return _assemble(blends, fitted)
