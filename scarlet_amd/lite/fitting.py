"""``fit_blends`` for ``scarlet.lite``: many ``LiteBlend`` objects fitted together.

A catalogue of parent blends rarely has two parents with the same footprint, so blends are
batched with ragged frames: a group of blends is padded to its largest frame (data 0,
weight 0) and every blend's components are clipped to its own frame on the device
(``BlendBatch(frame_shapes=...)``, ``smi_batch_set_frame_extents``).  A group shares
everything a batch holds for all its blends -- update rule and optimizer constants, bands,
difference-kernel stamp shape, iteration counter -- and the FFT shape and convolution path
its blends' own frames would get (and, on the fused path, the kernel variant), so padding never
changes the convolution a blend sees.
"""

import threading

import numpy as np

from ..batch import BlendBatch, _conv_plan

# rocFFT batches of transposed complex shapes must not be alive on one device at the same
# time (smi_batch_create, plans_enter): with several host threads on one device, the
# rocFFT-path groups of that device run one after the other
_rocfft_locks = {}
_rocfft_locks_guard = threading.Lock()


def _rocfft_lock(device):
    with _rocfft_locks_guard:
        return _rocfft_locks.setdefault(device, threading.Lock())


def _check(blend, max_iter, e_rel):
    """The refusals of ``LiteBlend.fit`` for one blend, before any GPU work.  Returns the group
    key of a blend that runs, or None when there is nothing to run (no components, or the
    counter is at ``max_iter``)."""
    if not blend.components:
        return None
    kind = blend._kind()
    if blend.it >= max_iter:
        return None
    settings, opt = blend._optimizer(kind)
    if settings["prox_max_iter"] != 1 and settings["prox_e_rel"] != e_rel:
        raise NotImplementedError("more than one proximal sub-iteration needs prox_e_rel == e_rel")
    for c in blend.components:
        blend._spec(c, kind)
    obs = blend.observation
    kernel = obs.diff_kernel
    if kernel is not None and any(s % 2 == 0 for s in kernel.image.shape[1:]):
        raise NotImplementedError("difference kernels need odd stamps (the flipped kernel "
                                  "of an even stamp is not the transposed convolution)")
    C, h, w = obs.images.shape
    kshape = None if kernel is None else tuple(kernel.image.shape)
    return (kind, tuple(sorted(settings.items())),
            None if opt is None else tuple(sorted(opt.items())),
            C, kshape, blend.it, bool(blend.loss), _conv_plan(h, w, kshape))


def _upload(blends, kind, key, capacity, device):
    """One BlendBatch of the group's blends, padded to the largest frame (frame extents only
    when their frames differ), with their parameters, optimizer state and previous losses."""
    _, settings, opt, C, kshape, _, _, (path, fy, fx, _) = key
    shapes = [b.observation.images.shape[1:] for b in blends]
    H, W = max(s[0] for s in shapes), max(s[1] for s in shapes)
    data = np.zeros((len(blends), C, H, W), dtype=np.float32)
    weights = np.zeros_like(data)
    for i, b in enumerate(blends):
        h, w = shapes[i]
        data[i, :, :h, :w] = b.observation.images
        weights[i, :, :h, :w] = b.observation.weights
    kw = {}
    if kshape is not None:
        kw = dict(kernel=np.stack([np.asarray(b.observation.diff_kernel.image, np.float32)
                                   for b in blends]),
                  fft_shape=(fy, fx), conv_path=path)
    comps = [c for b in blends for c in b.components]
    batch = BlendBatch(
        data, weights, [[b._spec(c, kind) for c in b.components] for b in blends],
        max_iter=max(capacity, 1), scheme="fista" if kind == "fista" else "amsgrad",
        log_norm=False, device=device,
        frame_shapes=shapes if len(set(shapes)) > 1 else None, **kw)
    try:
        if kind == "fista":
            batch.set_fista_state(z_sed=np.stack([c._sed.z for c in comps]),
                                  z_morph=[c._morph.z for c in comps],
                                  t=[(c._sed.t, c._morph.t) for c in comps])
        else:
            def finite(a):  # vhat starts at -inf (lite/parameters.py:267-269): any value
                return np.where(np.isfinite(a), a, 0)  # below v is equivalent

            batch.set_moments(
                m_sed=np.stack([c._sed.m for c in comps]), v_sed=np.stack([c._sed.v for c in comps]),
                vhat_sed=np.stack([finite(c._sed.vhat) for c in comps]),
                m_morph=[c._morph.m for c in comps], v_morph=[c._morph.v for c in comps],
                vhat_morph=[finite(c._morph.vhat) for c in comps])
            batch.set_optimizer(**dict(opt))
        if blends[0].loss:  # (all of a group or none: the key holds bool(loss))
            batch.set_previous_loss([-b.loss[-1] for b in blends])
    except BaseException:
        batch.close()
        raise
    return batch


def _download(batch, blends, members, kind, offsets):
    """Parameters and FISTA / AMSGrad state of the blends at positions ``members`` of the
    batch, from the device."""
    seds, morphs = batch.parameters()
    st = batch.fista_state() if kind == "fista" else batch.moments()
    for j in members:
        for k, c in enumerate(blends[j].components, offsets[j]):
            c._sed.x = seds[k].astype(c._sed.x.dtype)
            c._morph.x = morphs[k].astype(c._morph.x.dtype)
            if kind == "fista":
                c._sed.z, c._morph.z = st["z_sed"][k].copy(), st["z_morph"][k].copy()
                c._sed.t, c._morph.t = float(st["t"][k][0]), float(st["t"][k][1])
            else:
                c._sed.m, c._sed.v, c._sed.vhat = (st[n][k].copy() for n in ("m_sed", "v_sed", "vhat_sed"))
                c._morph.m, c._morph.v, c._morph.vhat = (
                    st[n][k].copy() for n in ("m_morph", "v_morph", "vhat_morph"))


def _fit_group(blends, key, max_iter, e_rel, min_iter, resize, device):
    """LiteBlend.fit of every blend of one group (all at the same counter), round by round.
    Returns the set of positions whose parameters turned non-finite."""
    kind = key[0]
    settings = dict(key[1])
    it = blends[0].it
    active = list(range(len(blends)))
    failed = set()
    while it < max_iter and active:
        members = [blends[i] for i in active]
        counts = [len(b.components) for b in members]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        batch = _upload(members, kind, key, max_iter - it, device)
        running = list(range(len(members)))  # positions in the batch still iterating
        ended_at = {}                         # position -> final counter of a blend that stopped
        resized = set()
        try:
            while it < max_iter and running and not resized:
                if resize is None:
                    last = max_iter - 1
                else:
                    last = min(max(-(-it // resize), 1) * resize, max_iter - 1)
                n = last - it + 1
                _, before = batch.progress()
                batch.step(it, n, e_rel=e_rel, min_iter=min_iter,
                           prox_max_iter=settings["prox_max_iter"], check_convergence=True)
                states, after = batch.progress()
                hooks = []
                for j in list(running):
                    if states[j] >= 3:
                        failed.add(active[j])
                        running.remove(j)
                        continue
                    converged = states[j] == 2
                    if converged:
                        # the stopping rule fired in iteration it + n_done - 1; the
                        # reference breaks before incrementing the counter
                        ended_at[j] = it + int(after[j] - before[j]) - 1
                        running.remove(j)
                        ended = ended_at[j]
                    else:
                        ended = it + n - 1
                    if resize is not None and ended > 0 and ended % resize == 0:
                        hooks.append(j)
                it += n
                if hooks:
                    _download(batch, members, hooks, kind, offsets)
                    for j in hooks:
                        b = members[j]
                        if any([c.resize() for c in b.components if hasattr(c, "resize")]):
                            resized.add(j)
            losses = batch.loss_history()
            done = [j for j in range(len(members)) if active[j] not in failed]
            for j in done:
                members[j].loss += [-float(v) for v in losses[j]]
                members[j].it = ended_at.get(j, it)
            _download(batch, members, [j for j in done if j not in resized], kind, offsets)
        finally:
            batch.close()
        # (a blend that failed keeps the counter, losses and parameters of the last batch
        # that ended well for it)
        active = [active[j] for j in running]
    return failed


def _fit_on(blends, keys, device, max_iter, e_rel, min_iter, resize, reweight=False):
    """Groups the blends of one shard and fits every group on ``device``; with ``reweight``
    the blends that did not fail -- those with nothing to fit included -- are then reweighted
    there (``weight_blends``).  Returns the positions (within the shard) of the blends that
    failed."""
    groups = {}
    for i, key in enumerate(keys):
        if key is not None:
            groups.setdefault(key, []).append(i)
    failed = set()
    for key, idx in groups.items():
        lock = _rocfft_lock(device) if key[-1][0] == "rocfft" else None
        if lock is not None:
            lock.acquire()
        try:
            bad = _fit_group([blends[i] for i in idx], key, max_iter, e_rel, min_iter, resize,
                             device)
        finally:
            if lock is not None:
                lock.release()
        failed.update(idx[j] for j in bad)
    if reweight:
        from .measure import weight_blends

        weight_blends([b for i, b in enumerate(blends) if i not in failed], device=device)
    return failed


def group_keys(blends, max_iter, e_rel=1e-4):
    """The device group of every blend (None: nothing to fit), in input order: what
    ``fit_blends`` batches together.  Raises the refusals ``fit_blends`` raises."""
    keys = []
    for b in blends:
        key = _check(b, max_iter, e_rel)
        if key is not None and any(int(o) != 0 for o in tuple(b.observation.bbox.origin)[1:]):
            raise NotImplementedError("observations whose bbox has a non-zero spatial origin are "
                                      "not supported by lite.fit_blends")
        keys.append(key)
    return keys


def fit_blends(blends, max_iter, e_rel=1e-4, min_iter=1, resize=10, reweight=True, devices=None):
    """Fit many ``LiteBlend`` objects together.

    Equivalent to ``[b.fit(max_iter, e_rel, min_iter, resize, reweight) for b in blends]``
    -- the same iteration counters (``b.it``), appended losses, boxes, parameters and
    optimizer state -- but blends that agree on the update rule and its constants, the
    number of bands, the difference-kernel stamp shape, the iteration counter and the FFT
    shape of their own frame run in one device batch, whatever their frame sizes (ragged
    frames: ``BlendBatch(frame_shapes=...)``).  Box resizing stays per blend, every
    ``resize`` iterations, on the host.  With ``reweight`` the blends are then reweighted
    together (``weight_blends``: what ``weight_sources`` sets, one device batch per group).

    ``devices``: ``None`` / an int: one GPU; a list of GPU indices: contiguous shards
    (``dist.shard_range``), one host thread each.  Results do not depend on the partition.

    Every blend is checked before any GPU work: the ``NotImplementedError``s of
    ``LiteBlend.fit``, and observations whose bbox has a non-zero spatial origin.  A blend
    whose parameters turn non-finite gets ``(it, nan)`` and is listed in
    ``fit_blends.errors`` as ``(index, ArithmeticError)``; the others go on.

    Returns the list of ``(it, loss[-1])`` in input order.
    """
    blends = list(blends)
    fit_blends.errors = []
    if isinstance(devices, str):
        raise ValueError("devices must be None, an int or a list of GPU indices")
    keys = group_keys(blends, max_iter, e_rel)
    if devices is None or np.isscalar(devices):
        devices = [0 if devices is None else int(devices)]
    devices = [int(d) for d in devices]
    failed = set()
    if len(devices) == 1:
        failed = _fit_on(blends, keys, devices[0], max_iter, e_rel, min_iter, resize, reweight)
    elif blends:
        from concurrent.futures import ThreadPoolExecutor

        from ..dist import shard_range

        cuts = [shard_range(len(blends), i, len(devices)) for i in range(len(devices))]
        with ThreadPoolExecutor(len(devices)) as pool:
            jobs = [pool.submit(_fit_on, blends[lo:hi], keys[lo:hi], dev, max_iter, e_rel,
                                min_iter, resize, reweight)
                    for (lo, hi), dev in zip(cuts, devices)]
            for (lo, _), job in zip(cuts, jobs):
                failed.update(lo + i for i in job.result())
    out = []
    for i, (b, key) in enumerate(zip(blends, keys)):
        if i in failed:
            fit_blends.errors.append(
                (i, ArithmeticError("parameters of the blend are not finite")))
            out.append((b.it, float("nan")))
        elif key is None:
            # nothing to run on the device (no components, or the counter is at max_iter):
            # LiteBlend.fit only reports then (the reweighting is done, with its shard)
            out.append(b.fit(max_iter, e_rel, min_iter, resize, reweight=False))
        else:
            out.append((b.it, b.loss[-1]))
    return out


fit_blends.errors = []
