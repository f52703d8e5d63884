"""Source initialisation (reference scarlet/initialization.py): runs once per
blend on the host before the fit.  The monotonicity sweep used here goes through
the C ABI (seam 1) to the GPU; rendering for the spectrum solve uses the device
renderer."""

import logging

import numpy as np

from ._catalog import Launcher, chunks, defaults, offsets
from .bbox import Box
from .morphology import get_minimal_boxsize  # noqa: F401  (reference exports it here)
from .renderer import ConvolutionRenderer, NullRenderer

logger = logging.getLogger("scarlet_amd.initialization")


def _as_tuple(observations):
    return observations if hasattr(observations, "__iter__") else (observations,)


def _warn_nonpositive(spectrum, sky_coord):
    if np.any(spectrum <= 0):
        msg = f"Zero or negative spectrum {spectrum} at {sky_coord}"
        (logger.warning if np.all(spectrum <= 0) else logger.info)(msg)


def get_pixel_spectrum(sky_coord, observations, correct_psf=False, models=None, concat=True):
    """Data values at the pixel of ``sky_coord`` in every channel; divided by
    the PSF peak (``correct_psf``) or by a model's value there (``models``)."""
    if models is not None:
        assert correct_psf is False
    if not hasattr(observations, "__iter__"):
        observations, models = (observations,), (models,)
    elif models is None:
        models = (None,) * len(observations)
    else:
        assert len(models) == len(observations)
    spectra = []
    for obs, model in zip(observations, models):
        iy, ix = np.round(obs.get_pixel(sky_coord)).astype("int")
        spectrum = obs.data[:, iy, ix].copy()
        if correct_psf and obs.psf is not None:
            spectrum /= obs.psf.get_model().max(axis=(1, 2))
        elif model is not None:
            spectrum /= model[:, iy, ix].copy()
        spectra.append(spectrum)
        _warn_nonpositive(spectrum, sky_coord)
    return np.concatenate(spectra).reshape(-1) if concat else spectra


def get_psf_spectrum(sky_coord, observations, compute_snr=False, concat=True):
    """PSF-weighted (matched-filter) flux per channel at ``sky_coord`` and,
    optionally, the signal-to-noise ratio of a point source there."""
    observations = _as_tuple(observations)
    spectra, num, den = [], [], []
    for obs in observations:
        index = np.round(obs.get_pixel(sky_coord)).astype("int")
        psf = obs.psf.get_model()
        bbox = obs.psf.bbox + (0, *index)
        img = bbox.extract_from(obs.data)
        noise = bbox.extract_from(obs.noise_rms)
        masked = bbox.extract_from(obs.noise_rms.mask)
        spec = []
        for c in range(obs.C):
            ok = ~masked[c]
            p, d = psf[c, ok], img[c, ok]
            flux = d @ p
            spec.append(flux / (p @ p))
            if compute_snr:
                num.append(flux)
                den.append((p * noise[c, ok] ** 2) @ p)
        spec = np.array(spec)
        spectra.append(spec)
        _warn_nonpositive(spec, sky_coord)
    if concat:
        spectra = np.concatenate(spectra).reshape(-1)
    if compute_snr:
        return spectra, np.sum(num) / np.sqrt(np.sum(den))
    return spectra


def trim_morphology(center_index, morph, bg_thresh=0, boxsize=None):
    """Zero the pixels at or below ``bg_thresh`` and cut a square box of
    standard size around ``center_index`` that holds what is left."""
    morph[~(morph > bg_thresh)] = 0
    bbox = Box.from_data(morph, min_value=0)
    if bbox.contains(center_index):
        size = 2 * max(
            center_index[0] - bbox.start[-2], bbox.stop[0] - center_index[-2],
            center_index[1] - bbox.start[-1], bbox.stop[1] - center_index[-1],
        )
    else:
        size = 0
    if boxsize is None:
        boxsize = get_minimal_boxsize(size)
    half = boxsize // 2
    bbox = Box.from_bounds(
        (center_index[0] - half, center_index[0] + half + 1),
        (center_index[1] - half, center_index[1] + half + 1),
    )
    return bbox.extract_from(morph), bbox


def build_initialization_image(observations, spectra=None):
    """Inverse-variance, spectrum-weighted coadd of all channels and its noise
    level: the detection image morphologies are initialised from."""
    if not hasattr(observations, "__iter__"):
        observations, spectra = (observations,), (spectra,)
    assert len(observations) == len(spectra)
    frame = observations[0].model_frame
    usable = [isinstance(o.renderer, (NullRenderer, ConvolutionRenderer)) for o in observations]
    if not hasattr(observations[0], "_detect"):
        detect, var = [], []
        for obs, ok in zip(observations, usable):
            if not ok:
                continue
            d = np.zeros(frame.shape, dtype=frame.dtype)
            v = np.zeros(frame.shape, dtype=frame.dtype)
            data_sl, model_sl = obs.renderer.slices
            obs.renderer.map_channels(d)[model_sl] += obs.data[data_sl]
            obs.renderer.map_channels(v)[model_sl] += obs.noise_rms[data_sl] ** 2
            detect.append(d)
            var.append(v)
        observations[0]._detect = (np.array(detect), np.array(var))
    detect, var = observations[0]._detect
    weights_c = []
    for obs, ok, spec in zip(observations, usable, spectra):
        if not ok:
            continue
        s = np.zeros(frame.C)
        obs.renderer.map_channels(s)[:] = 1 if spec is None else spec
        weights_c.append(s)
    spectrum = np.stack(weights_c, axis=0)[:, :, None, None]
    weight = np.zeros(var.shape)
    positive = var > 0
    weight[positive] = 1 / var[positive]
    weight *= spectrum
    return (weight * detect).sum(axis=(0, 1)), np.sqrt((spectrum * weight).sum(axis=(0, 1)))


def init_source(frame, center, observations, thresh=1, max_components=1, min_components=1,
                min_snr=50, shifting=False, resizing=True, boxsize=None, fallback=True):
    """One source at ``center`` with up to ``max_components`` components; with
    ``fallback`` the count is limited by the point-source SNR and reduced (down
    to a compact source) while initialisation yields non-finite parameters."""
    from .source import ExtendedSource

    observations = _as_tuple(observations)
    if fallback:
        _, snr = get_psf_spectrum(center, observations, compute_snr=True)
        by_snr = np.floor(snr / min_snr).astype("int")
        max_components = np.min([max_components, np.max([min_components, by_snr])])
    while max_components >= 0:
        try:
            if max_components > 0:
                source = ExtendedSource(frame, center, observations, thresh=thresh,
                                        shifting=shifting, resizing=resizing, boxsize=boxsize,
                                        K=max_components)
            else:
                source = ExtendedSource(frame, center, observations, shifting=shifting,
                                        resizing=resizing, boxsize=boxsize, compact=True)
            source.check_parameters()
        except ArithmeticError as exc:
            if not fallback:
                raise exc
            logger.info(f"Could not initialize source at {center} with {max_components} "
                        f"components: {exc}")
            max_components -= 1
            continue
        return source


# Detection images of a scene's sources, swept in one launch ahead of the loop over the sources
# (``prepare_detection_sweeps``): key -> (pixel spectra, coadd, coadd rms, symmetrised
# profile, the same profile made monotonic about the source's pixel, the trimming threshold the
# swept profile is good for -- None: any).  ``SingleExtendedSource`` looks its centre up here
# before it computes them itself.
_prepared = {}


def _prepared_key(sky_coord, observations):
    try:
        coord = tuple(float(v) for v in np.asarray(sky_coord, dtype=float).reshape(-1))
    except (TypeError, ValueError):
        return None
    return coord + tuple(id(obs) for obs in observations)


# Half-width of the window about a source's pixel in which its detection image is swept first
# (prepare_detection_sweeps); frames that are not much larger are swept whole.
SWEEP_WINDOW = 32


def _window(pixel, shape):
    R = SWEEP_WINDOW
    py, px = int(pixel[0]), int(pixel[1])
    return max(py - R, 0), min(py + R + 1, shape[0]), max(px - R, 0), min(px + R + 1, shape[1])


def _window_pays(shape, thresh):
    R = SWEEP_WINDOW
    return thresh is not None and thresh >= 0 and max(shape) > 2 * R + 1 + R // 2


def _rim_below(win, cut, shape, floor):
    """The largest value on the sides of the window that have frame beyond them is at or
    below ``floor`` (NaNs: no)."""
    y0, y1, x0, x1 = cut
    rim = [edge for beyond, edge in ((y0 > 0, win[0]), (y1 < shape[0], win[-1]),
                                     (x0 > 0, win[:, 0]), (x1 < shape[1], win[:, -1])) if beyond]
    return not rim or max(float(np.max(e)) for e in rim) <= floor


def sweep_in_window(profile, pixel, thresh, detect_std):
    """One image through the windowed sweep of ``prepare_detection_sweeps`` ('flat' weights,
    no minimal gradient): the swept profile with zeros outside the window, or None where the
    window does not pay or its rim is brighter than the smallest trimming threshold."""
    from . import operator

    if not _window_pays(profile.shape, thresh):
        return None
    if not (0 <= pixel[0] < profile.shape[0] and 0 <= pixel[1] < profile.shape[1]):
        return None
    cut = y0, y1, x0, x1 = _window(pixel, profile.shape)
    win = np.ascontiguousarray(profile[y0:y1, x0:x1])[None]
    operator.prox_weighted_monotonic_many(win, [(int(pixel[0]) - y0, int(pixel[1]) - x0)],
                                          neighbor_weight="flat", min_gradient=0)
    if not _rim_below(win[0], cut, profile.shape, thresh * float(np.min(detect_std))):
        return None
    full = np.zeros_like(profile)
    full[y0:y1, x0:x1] = win[0]
    return full


def prepare_detection_sweeps(frame, centers, observations, thresh=None):
    """What every ``SingleExtendedSource`` of the scene starts from -- the spectrum-weighted
    coadd about its centre, symmetrised and made monotonic (source.py:312-333) -- for ALL
    centres at once: the host part per centre, then ONE launch of the monotonic sweep for all
    of them (``operator.prox_weighted_monotonic_many``) instead of a host -> GPU -> host round
    trip per source.  Same arithmetic, same bits as the per-source path; centres the
    preparation cannot serve (outside the frame, a failing pixel spectrum) are left to it.

    With ``thresh`` (the caller's trimming threshold) the sweep runs in a window of
    ``2 SWEEP_WINDOW + 1`` pixels about the centre first.  The sweep bounds a pixel by the mean
    of its neighbours CLOSER to the centre ('flat' weights, no minimal gradient), and every
    closer neighbour of a pixel of a centred square lies in the square: inside the window the
    result is the full frame's, bit for bit, and every pixel outside is at most the largest
    value on the window's rim.  If that is at or below the smallest trimming threshold of the
    frame, ``trim_morphology`` zeroes everything outside whatever its value: the window's sweep
    IS the source's profile (tables of 65^2 instead of the frame's pixels, the same for every
    centre away from the border).  Otherwise the centre is swept on the whole frame."""
    from . import operator

    observations = _as_tuple(observations)
    _prepared.clear()
    rows = []
    for center in centers:
        key = _prepared_key(center, observations)
        if key is None or key in _prepared:
            continue
        try:
            per_obs = get_pixel_spectrum(center, observations, concat=False)
            coadd, coadd_rms = build_initialization_image(observations, spectra=per_obs)
            pixel = np.round(frame.get_pixel(center)).astype("int")
            if not (0 <= pixel[0] < coadd.shape[0] and 0 <= pixel[1] < coadd.shape[1]):
                continue
            profile = operator.prox_uncentered_symmetry(coadd.copy(), 0, center=pixel, algorithm="sdss")
        except Exception:  # the per-source path reports it
            continue
        rows.append((key, per_obs, coadd, coadd_rms, pixel, np.ascontiguousarray(profile)))
    if not rows:
        return 0

    def sweep(images_and_centres):
        """[(image, centre)] -> the swept images, one launch per image shape"""
        out = [None] * len(images_and_centres)
        by_shape = {}
        for n, (image, _) in enumerate(images_and_centres):
            by_shape.setdefault((image.shape, image.dtype.str), []).append(n)
        for group in by_shape.values():
            swept = np.stack([images_and_centres[n][0] for n in group])
            operator.prox_weighted_monotonic_many(
                swept, [tuple(int(v) for v in images_and_centres[n][1]) for n in group],
                neighbor_weight="flat", min_gradient=0)
            for n, image in zip(group, swept):
                out[n] = image
        return out

    shape = rows[0][5].shape
    whole = list(range(len(rows)))
    if _window_pays(shape, thresh):
        cuts = [_window(r[4], shape) for r in rows]
        swept = sweep([(np.ascontiguousarray(r[5][y0:y1, x0:x1]), (r[4][0] - y0, r[4][1] - x0))
                       for r, (y0, y1, x0, x1) in zip(rows, cuts)])
        whole = []
        for n, (r, cut, win) in enumerate(zip(rows, cuts, swept)):
            # (floor: the smallest trimming threshold of the frame)
            if not _rim_below(win, cut, shape, thresh * float(np.min(r[3]))):
                whole.append(n)
                continue
            full = np.zeros_like(r[5])
            full[cut[0]:cut[1], cut[2]:cut[3]] = win
            _prepared[r[0]] = (r[1], r[2], r[3], r[5], full, thresh)
    if whole:
        swept = sweep([(rows[n][5].copy(), rows[n][4]) for n in whole])
        for n, out in zip(whole, swept):
            r = rows[n]
            _prepared[r[0]] = (r[1], r[2], r[3], r[5], out, None)
    return len(rows)


def prepared_detection(sky_coord, observations):
    """The prepared images of a centre, or None."""
    if not _prepared:
        return None
    return _prepared.get(_prepared_key(sky_coord, _as_tuple(observations)))


def init_all_sources(frame, centers, observations, thresh=1, max_components=1,
                     min_components=1, min_snr=50, shifting=False, resizing=True, boxsize=None,
                     fallback=True, silent=False, set_spectra=True):
    """Initialise a source at every centre; returns ``(sources, skipped)``."""
    observations = _as_tuple(observations)
    sources, skipped = [], []
    centers = list(centers)
    try:
        # (all sources' detection images through the monotonic sweep in one launch)
        if max_components > 0 and len(centers) > 1:
            prepare_detection_sweeps(frame, centers, observations, thresh=thresh)
        return _init_all_sources(frame, centers, observations, thresh, max_components,
                                 min_components, min_snr, shifting, resizing, boxsize, fallback,
                                 silent, set_spectra)
    finally:
        _prepared.clear()


def _init_all_sources(frame, centers, observations, thresh, max_components, min_components,
                      min_snr, shifting, resizing, boxsize, fallback, silent, set_spectra):
    sources, skipped = [], []
    for k, center in enumerate(centers):
        try:
            sources.append(
                init_source(frame, center, observations, thresh=thresh,
                            max_components=max_components, min_components=min_components,
                            min_snr=min_snr, shifting=shifting, resizing=resizing,
                            boxsize=boxsize, fallback=fallback)
            )
        except Exception as exc:
            logger.warning(f"Failed to initialize source {k}")
            if not silent:
                raise exc
            skipped.append(k)
    if set_spectra:
        set_spectra_to_match(sources, observations)
    return sources, skipped


def set_spectra_to_match(sources, observations):
    """Best-fit amplitude of every component in every channel: weighted linear
    least squares of the rendered unit-spectrum component models against the data."""
    from .component import CombinedComponent

    observations = _as_tuple(observations)
    frame = observations[0].model_frame
    parameters, update_of, models, sums = [], [], [], []
    for i, src in enumerate(sources):
        comps = src.children if isinstance(src, CombinedComponent) else (src,)
        for j, comp in enumerate(comps):
            p = comp.get_parameter("spectrum")
            parameters.append(p)
            if p is not None and not p.fixed:
                p[:] = 1
            model = comp.get_model(frame=frame)
            target = len(models)
            # (np.allclose(a, b) implies |sum a - sum b| <= N atol + rtol sum |b|: most pairs are
            # told apart by two numbers instead of a pass over both cubes)
            total, bound = float(np.sum(model)), 1e-8 * model.size
            for prev, other in enumerate(models):
                gap = bound + 1e-5 * sums[prev][1]
                if abs(total - sums[prev][0]) > 2 * gap + 1e-9 * (abs(total) + abs(sums[prev][0])):
                    continue
                if np.allclose(model, other):
                    target = prev
                    logger.warning(
                        f"Source {i}, Component {j} has a model identical to another component.\n"
                        "This is likely not intended, and the source/component should be deleted. "
                        "Spectra will be identical.")
            update_of.append(target)
            if target == len(models):
                models.append(model)
                sums.append((total, float(np.sum(np.abs(model)))))
    models = np.array(models)
    n_models = len(models)
    for obs in observations:
        # The reference hands float64 unit-spectrum models to the renderer and solves the
        # normal equations in double (initialization.py:493-588); their condition numbers
        # are several hundred (250 .. 700 on the quickstart scene), so float32 convolutions
        # of the device would show up as 1e-4 in the spectra.  This one-off solve therefore
        # renders on the host in double where the renderer is a plain convolution.
        # (a subclass that overrides the rendering inherits render_float64 without meaning it)
        from .renderer import ConvolutionRenderer, NullRenderer

        precise = (obs.renderer.render_float64
                   if type(obs.renderer) in (ConvolutionRenderer, NullRenderer)
                   and hasattr(obs.renderer, "render_float64") else None)
        if precise is not None and not obs.parameters:
            rendered = np.stack([precise(m) for m in models], axis=0)
        else:
            rendered = np.stack([obs.render(m) for m in models], axis=0).astype(np.float64)
        spectra = np.zeros((n_models, obs.C))
        for c in range(obs.C):
            im = obs.data[c].reshape(-1).astype(np.float64)
            w = obs.weights[c].reshape(-1).astype(np.float64)
            m = rendered[:, c].reshape(n_models, -1)
            mw = m * w[None, :]
            seen = np.flatnonzero(np.sum(mw, axis=1) / np.sum(m, axis=1) / np.mean(w) > 0.1)
            if len(seen) == n_models:
                spectra[:, c] = np.linalg.inv(mw @ m.T) @ m @ (im * w)
            else:
                spectra[seen, c] = np.linalg.inv(mw[seen] @ m[seen].T) @ m[seen] @ (im * w)
        for k, p in enumerate(parameters):
            if p is not None and not p.fixed:
                obs.renderer.map_channels(p)[:] = spectra[update_of[k]]
    for p in parameters:
        if p is not None and p.constraint is not None:
            p[:] = p.constraint(p, 0)


# ---------------------------------------------------------------------------------------------
# init_blends: init_all_sources for a catalogue of blends.  The morphologies of all sources of
# a chunk of blends come from three launches of csrc/init_sources.hip (psf_snr, sweep, crop);
# the source objects are assembled on the host through the existing classes, and the float64
# normal equations of ``set_spectra=True`` come from two more (spectra_tiles, spectra_reduce);
# the host solves them, K x K per blend and band.
# ---------------------------------------------------------------------------------------------
_i4, _i8 = np.int32, np.int64
_PSF_SNR_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4), ("ph", _i4),
                          ("pw", _i4), ("bands", _i4), ("reserved", _i4), ("cube_off", _i8),
                          ("psf_off", _i8), ("out_off", _i8)], align=True)
_SWEEP_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4), ("bands", _i4),
                        ("reserved", _i4), ("cube_off", _i8), ("spec_off", _i8), ("out_off", _i8),
                        ("thresh", "f8")], align=True)
_CROP_DESC = np.dtype([("h", _i4), ("w", _i4), ("y0", _i4), ("x0", _i4), ("side", _i4),
                       ("layers", _i4), ("plane_off", _i8), ("floor_off", _i8), ("out_off", _i8),
                       ("percentile", "f8")], align=True)
_SPECTRA_BLEND = np.dtype([("h", _i4), ("w", _i4), ("y0", _i4), ("x0", _i4), ("fh", _i4),
                           ("fw", _i4), ("bands", _i4), ("kh", _i4), ("kw", _i4), ("n_comp", _i4),
                           ("comp0", _i4), ("reserved", _i4), ("cube_off", _i8), ("stamp_off", _i8),
                           ("part_off", _i8), ("out_off", _i8)], align=True)
_SPECTRA_COMPONENT = np.dtype([("y0", _i4), ("x0", _i4), ("h", _i4), ("w", _i4),
                               ("morph_off", _i8)], align=True)
SPECTRA_TILE = 16
MAX_COMPONENTS = 64       # of a blend
MAX_PRESENT = 32          # components whose convolved model reaches one tile
# |seen ratio - 0.1| <= NEAR_SEEN: the band is the loop's to decide
NEAR_SEEN = 1e-6
# the float64 plane of a source lives in the LDS of a CU: 160 KiB less 1 KiB of scratch
MAX_SWEEP_PIXELS = (160 * 1024 - 1024) // 8
MAX_STAMP = 63
MAX_BOX_SIDE = 1 << 12
# |snr / min_snr - k| <= NEAR_INTEGER * k: the loop forms the S/N with float32 dots in no fixed
# order, the device in float64; a count that close to the edge is the loop's to decide
NEAR_INTEGER = 1e-4
_OPTION_DEFAULTS = dict(thresh=1, max_components=1, min_components=1, min_snr=50, shifting=False,
                        resizing=True, boxsize=None, fallback=True, silent=False, set_spectra=True)


def _covers(slices, shape):
    return all(isinstance(s, slice) and range(*s.indices(n)) == range(n)
               for s, n in zip(slices, shape))


def _box_side(boxsize):
    """Side of the box ``trim_morphology`` cuts for ``boxsize``."""
    return 2 * (int(boxsize) // 2) + 1


def _refusal(frame, centers, observations, opts):
    """Why the device path of ``init_blends`` does not take a blend, or None."""
    from .frame import Frame

    if not isinstance(frame, Frame):
        return "frame is not a Frame"
    observations = tuple(_as_tuple(observations))
    if len(observations) != 1:
        return "{} observations: the device path takes one".format(len(observations))
    obs = observations[0]
    renderer = getattr(obs, "renderer", None)
    if getattr(obs, "model_frame", None) is not frame or renderer is None:
        return "the observation is not matched to the frame"
    if type(renderer) is ConvolutionRenderer:
        if renderer._convolution_type != "fft" or renderer.parameters:
            return "ConvolutionRenderer with a real-space convolution or a free psf_shift"
    elif type(renderer) is not NullRenderer:
        return "renderer {} is neither ConvolutionRenderer nor NullRenderer".format(
            type(renderer).__name__)
    if np.dtype(frame.dtype) != np.float32:
        return "frame dtype {} is not float32".format(np.dtype(frame.dtype).name)
    data, weights = obs.data, obs.weights
    if (type(data) is not np.ndarray or type(weights) is not np.ndarray
            or data.dtype != np.float32 or weights.dtype != np.float32):
        return "data or weights are not plain float32 arrays"
    shape = tuple(frame.shape)
    if (tuple(data.shape) != shape or renderer.channel_map is not None
            or not all(_covers(sl, shape) for sl in renderer.slices)):
        return "the observation does not cover exactly the model frame"
    if frame.psf is None:
        return "no frame PSF"
    if obs.psf is None:
        return "no observation PSF"
    if type(renderer) is ConvolutionRenderer:
        stamp = np.shape(renderer.diff_kernel.image)
        if len(stamp) != 3 or stamp[1] % 2 == 0 or stamp[2] % 2 == 0:
            return "even difference-kernel stamp"
        if max(stamp[1:]) > MAX_STAMP:
            return "difference-kernel stamp beyond {0} x {0}".format(MAX_STAMP)
    pshape = tuple(obs.psf.bbox.shape)
    if len(pshape) != 3 or pshape[0] != shape[0] or max(pshape[1:]) > MAX_STAMP:
        return "observation PSF is not one stamp per band of at most {0} x {0}".format(MAX_STAMP)
    if shape[1] * shape[2] > MAX_SWEEP_PIXELS:
        return "frame of {} pixels beyond the {} float64 pixels of the sweep kernel's LDS image".format(
            shape[1] * shape[2], MAX_SWEEP_PIXELS)
    if not 0 <= opts["max_components"] <= 2:
        return "max_components outside 0 .. 2"
    if not (np.isfinite(opts["thresh"]) and opts["thresh"] >= 0):
        return "thresh is negative or not finite"
    if opts["boxsize"] is not None and not 1 <= _box_side(opts["boxsize"]) <= MAX_BOX_SIDE:
        return "boxsize beyond the crop kernel's limits"
    if opts["fallback"] and not (np.isfinite(opts["min_snr"]) and opts["min_snr"] > 0):
        return "min_snr is not a positive number"
    centers = list(centers)
    if not centers:
        return "no centres"
    for center in centers:
        try:
            pixel = np.round(frame.get_pixel(center)).astype("int")
            same = np.array_equal(pixel, np.round(obs.get_pixel(center)).astype("int"))
        except Exception:
            return "a centre that is no coordinate"
        if not same:
            return "a centre on another pixel of the observation than of the frame"
        if not (0 <= pixel[0] < shape[1] and 0 <= pixel[1] < shape[2]):
            return "centre {} rounds to a pixel outside the frame".format(tuple(np.ravel(center)))
    return None


def _options(kwargs):
    unknown = set(kwargs) - set(_OPTION_DEFAULTS)
    if unknown:
        raise TypeError("unexpected arguments: {}".format(sorted(unknown)))
    return dict(_OPTION_DEFAULTS, **kwargs)


def _group_key(frame, observations):
    """Blends of one device group share dtype, bands and the shape of the PSF stamp."""
    obs = tuple(_as_tuple(observations))[0]
    return (np.dtype(frame.dtype).str, int(frame.C)) + tuple(int(n) for n in obs.psf.bbox.shape[1:])


def plan_init_blends(frames, centers, observations, **options):
    """``(groups, fallback)`` of ``init_blends``, without touching the GPU or the library: the
    positions of the blends of every device group, keyed by ``(dtype, bands, PSF stamp height,
    width)`` in order of first appearance and in list order inside a group, and ``(position,
    reason)`` of the blends that go through ``init_all_sources``."""
    opts = _options(options)
    frames, centers, observations = list(frames), [list(c) for c in centers], list(observations)
    if not len(frames) == len(centers) == len(observations):
        raise ValueError("frames, centers and observations must have one entry per blend, got "
                         "{}, {} and {}".format(len(frames), len(centers), len(observations)))
    groups, fallback = {}, []
    for i, (frame, cs, obs) in enumerate(zip(frames, centers, observations)):
        reason = _refusal(frame, cs, obs, opts)
        if reason is None:
            groups.setdefault(_group_key(frame, obs), []).append(i)
        else:
            fallback.append((i, reason))
    return groups, fallback


def _blend_bytes(frame, n_sources, boxsize=None):
    """Upper bound of the bytes of the device working set of one blend: data, variance and
    weight cubes; per source the swept float64 plane and two float64 layers of its box, twice
    (the cut-outs and the morphologies of the normal equations) -- the box of ``boxsize``, or,
    where the trim decides, the largest standard box a frame of this size can ask for --; the
    sums of the normal equations of two components per source, tile by tile."""
    C, h, w = frame.shape
    n = h * w
    side = (_box_side(boxsize) if boxsize is not None
            else _box_side(get_minimal_boxsize(2 * max(h, w))))
    K = 2 * n_sources
    tiles = -(-h // SPECTRA_TILE) * -(-w // SPECTRA_TILE)
    return (3 * 4 * C * n + n_sources * 8 * (n + 4 * side * side)
            + 8 * (tiles + 1) * C * (K * K + 3 * K))


def _detect_cubes(obs):
    """``observations[0]._detect`` as ``build_initialization_image`` makes and keeps it: the
    data and the variance on the model frame."""
    if not hasattr(obs, "_detect"):
        frame = obs.model_frame
        d = np.zeros(frame.shape, dtype=frame.dtype)
        v = np.zeros(frame.shape, dtype=frame.dtype)
        data_sl, model_sl = obs.renderer.slices
        obs.renderer.map_channels(d)[model_sl] += obs.data[data_sl]
        obs.renderer.map_channels(v)[model_sl] += obs.noise_rms[data_sl] ** 2
        obs._detect = (np.array([d]), np.array([v]))
    return obs._detect


def component_count(snr_sums, opts):
    """Components ``init_source`` starts a source with, from the ``(bands, 3)`` float64 sums of
    the psf_snr kernel; None where the loop has to decide (a non-finite S/N, or ``snr /
    min_snr`` within ``NEAR_INTEGER`` of a count it would change)."""
    lo, hi = int(opts["min_components"]), int(opts["max_components"])
    if not opts["fallback"]:
        return hi
    with np.errstate(all="ignore"):
        ratio = float(np.sum(snr_sums[:, 0]) / np.sqrt(np.sum(snr_sums[:, 2])) / opts["min_snr"])
    if not np.isfinite(ratio):
        return None
    for k in range(min(lo, hi), max(lo, hi) + 2):
        if abs(ratio - k) <= NEAR_INTEGER * max(abs(k), 1):
            return None
    count = min(hi, max(lo, int(np.floor(ratio))))
    return count if count >= 0 else None


def trim_box(bounds, pixel, boxsize=None):
    """``(origin, side)`` of the box ``trim_morphology`` cuts around ``pixel`` for a morphology
    whose pixels ``> 0`` have the inclusive ``bounds`` (min row, max row, min col, max col;
    max < min: none)."""
    if boxsize is None:
        b0, b1, l0, l1 = (int(v) for v in bounds)
        cy, cx = int(pixel[0]), int(pixel[1])
        size = 0
        if b1 >= b0 and b0 <= cy <= b1 and l0 <= cx <= l1:
            size = 2 * max(cy - b0, b1 + 1 - cy, cx - l0, l1 + 1 - cx)
        boxsize = get_minimal_boxsize(size)
    half = int(boxsize) // 2
    return (int(pixel[0]) - half, int(pixel[1]) - half), 2 * half + 1


def _call(dv, step, table, *args):
    """One smi_init_sources_<step>_f32 launch through the chunk's ``Launcher``."""
    dv.call("smi_init_sources_%s_f32" % step, table, *args, tag=step)


def pack_chunk(blends, opts):
    """Host tables and buffers of the first two launches of a chunk.  ``blends``: a list of
    ``(frame, centers, observation)``.  Returns a dict with the packed ``data``, ``var``
    (float32), ``psfs`` and ``spectra`` (float64), the ``psf_snr`` and ``sweep`` tables, per source
    its blend, pixel and pixel spectra, and ``loop``: the blends of the chunk (by position in it)
    that a look at their values sends through ``init_all_sources``, with the reason -- non-finite
    data, or a variance that is not positive."""
    n_pix = [b[0].shape[1] * b[0].shape[2] for b in blends]
    cube_off, n_cube = offsets([b[0].C * n for b, n in zip(blends, n_pix)])
    psfs = [np.asarray(b[2].psf.get_model(), np.float64) for b in blends]
    psf_off, n_psf = offsets([p.size for p in psfs])
    data, var, loop = [], [], {}
    src_blend, src_pixel, src_spec = [], [], []
    for k, (frame, centers, obs) in enumerate(blends):
        d, v = _detect_cubes(obs)
        d, v = np.asarray(d[0]), np.ma.getdata(v[0])
        data.append(d)
        # (the coadd reads the variance as it stands, also under the mask of noise_rms, where
        # get_psf_spectrum leaves the pixel out: those pixels go up negated)
        var.append(np.where(obs.weights != 0, v, -v))
        if not (np.isfinite(d).all() and np.isfinite(v).all() and (v > 0).all()
                and psfs[k].shape[0] == frame.C):
            loop[k] = "data or variance not finite, or a variance that is not positive"
            continue
        for center in centers:
            src_blend.append(k)
            src_pixel.append(tuple(int(p) for p in np.round(frame.get_pixel(center)).astype("int")))
            src_spec.append(get_pixel_spectrum(center, (obs,), concat=False))
    ns = len(src_blend)
    spec_off, n_spec = offsets([blends[k][0].C for k in src_blend])
    snr_off, n_snr = offsets([3 * blends[k][0].C for k in src_blend])
    plane_off, n_plane = offsets([n_pix[k] for k in src_blend])
    snr_t, sweep_t = np.zeros(ns, _PSF_SNR_DESC), np.zeros(ns, _SWEEP_DESC)
    spectra = np.zeros(n_spec, np.float64)
    for s, k in enumerate(src_blend):
        C, h, w = blends[k][0].shape
        (cy, cx), (_, ph, pw) = src_pixel[s], psfs[k].shape
        snr_t[s] = (h, w, cy, cx, ph, pw, C, 0, cube_off[k], psf_off[k], snr_off[s])
        sweep_t[s] = (h, w, cy, cx, C, 0, cube_off[k], spec_off[s], plane_off[s], opts["thresh"])
        # (the loop writes the float32 pixel spectrum into a float64 vector of the frame's bands)
        spectra[spec_off[s]:spec_off[s] + C] = src_spec[s][0]
    return dict(data=data, var=var, n_cube=n_cube, cube_off=cube_off, psfs=psfs, n_psf=n_psf, spectra=spectra,
                psf_snr=snr_t, sweep=sweep_t, n_snr=n_snr, n_plane=n_plane, snr_off=snr_off,
                plane_off=plane_off, src_blend=src_blend, src_pixel=src_pixel, src_spec=src_spec,
                loop=loop)


def _floor_image(cache, frame, center, side):
    """The peak-normalised band-mean model PSF in a box of ``side``: what
    ``SingleExtendedSource.init_morph`` takes the maximum with; once per frame and side."""
    from .source import CompactExtendedSource

    key = (id(frame), side)
    if key not in cache:
        cache[key] = CompactExtendedSource.init_morph(frame, center, boxsize=side)[0]
    return cache[key]


def _components(sources):
    from .component import CombinedComponent

    return [c for s in sources for c in (s.children if isinstance(s, CombinedComponent) else (s,))]


def _identical_pair(frame_shape, morphs, boxes):
    """Does ``set_spectra_to_match`` meet two components with identical models?  Its own cheap
    screen (the sum and the sum of absolute values within the ``np.allclose`` bound, a little
    wider here for the other order of the sums), then ``np.allclose`` of the two planes."""
    C, H, W = frame_shape
    placed, sums = [], []
    for m, (y0, x0) in zip(morphs, boxes):
        h, w = m.shape
        ys, ye, xs, xe = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        cut = m[ys - y0:ye - y0, xs - x0:xe - x0]
        placed.append((ys, xs, cut))
        sums.append((C * float(np.sum(cut)), C * float(np.sum(np.abs(cut)))))
    bound = 1e-8 * C * H * W
    for k in range(len(morphs)):
        for prev in range(k):
            gap = bound + 1e-5 * sums[prev][1]
            if abs(sums[k][0] - sums[prev][0]) > 2 * gap + 1e-8 * (abs(sums[k][0]) + abs(sums[prev][0])):
                continue
            planes = np.zeros((2, H, W))
            for plane, (ys, xs, cut) in zip(planes, (placed[k], placed[prev])):
                plane[ys:ys + cut.shape[0], xs:xs + cut.shape[1]] = cut
            if np.allclose(planes[0], planes[1]):
                return True
    return False


def _most_present(region, boxes, shapes, kh, kw):
    """The largest number of components whose box, grown by the stamp's half, meets one tile of
    ``region`` = (y0, x0, fh, fw)."""
    y0, x0, fh, fw = region
    most = 0
    for ty in range(0, fh, SPECTRA_TILE):
        for tx in range(0, fw, SPECTRA_TILE):
            th, tw = min(SPECTRA_TILE, fh - ty), min(SPECTRA_TILE, fw - tx)
            n = 0
            for (by, bx), (h, w) in zip(boxes, shapes):
                cy, cx = by - y0, bx - x0
                n += (cy - kh // 2 < ty + th and cy + h + kh // 2 > ty
                      and cx - kw // 2 < tx + tw and cx + w + kw // 2 > tx)
            most = max(most, n)
    return most


def pack_spectra(items, cube_off):
    """Host tables and buffers of the two spectra launches.  ``items``: ``(k, frame, observation,
    sources)`` of the blends of a chunk that have their sources, ``k`` the position in the chunk;
    ``cube_off[k]``: where the blend's data cube lies.  Sets every free spectrum to 1, as
    ``set_spectra_to_match`` does first.  Returns a dict with the ``blends``, ``components`` and
    ``work`` tables, the packed float64 ``morphs`` and ``stamps``, ``n_part`` and ``n_out``,
    ``taken``: per packed blend ``(k, parameters, bands, components, out_off)``, and ``loop``:
    the reason per blend the loop has to take."""
    from .component import FactorizedComponent

    rows, comp_rows, work, morph_parts, stamp_parts, taken, loop = [], [], [], [], [], [], {}
    n_morph = n_stamp = n_part = n_out = 0
    for k, frame, obs, sources in items:
        C, H, W = frame.shape
        comps = _components(sources)
        parameters, morphs, boxes = [], [], []
        for comp in comps:
            p = comp.get_parameter("spectrum")
            if (not isinstance(comp, FactorizedComponent) or p is None or p.fixed
                    or p.shape != (C,)):
                loop[k] = "a component without a free spectrum of the frame's bands"
                break
            p[:] = 1
            m = np.asarray(comp.get_models_of_children()[1], np.float64)
            if m.ndim != 2 or not m.size:
                loop[k] = "a morphology that is no image"
                break
            parameters.append(p)
            morphs.append(m)
            boxes.append(tuple(int(o) for o in comp.bbox.origin[-2:]))
        if k in loop:
            continue
        K = len(morphs)
        if not 1 <= K <= MAX_COMPONENTS:
            loop[k] = "{} components: the device takes 1 .. {}".format(K, MAX_COMPONENTS)
            continue
        if type(obs.renderer) is ConvolutionRenderer:
            stamps = np.asarray(obs.renderer.kernel_image(), np.float64)
        else:
            stamps = np.ones((C, 1, 1))
        if stamps.ndim != 3 or stamps.shape[0] != C:
            loop[k] = "difference kernel without one stamp per band"
            continue
        kh, kw = stamps.shape[1:]
        # the region: what the convolved models reach inside the frame
        lo_y = lo_x = 1 << 30
        hi_y = hi_x = -(1 << 30)
        for m, (y0, x0) in zip(morphs, boxes):
            ys, ye, xs, xe = max(y0, 0), min(y0 + m.shape[0], H), max(x0, 0), min(x0 + m.shape[1], W)
            if ys < ye and xs < xe:
                lo_y, hi_y = min(lo_y, ys - kh // 2), max(hi_y, ye + kh // 2)
                lo_x, hi_x = min(lo_x, xs - kw // 2), max(hi_x, xe + kw // 2)
        lo_y, hi_y, lo_x, hi_x = max(lo_y, 0), min(hi_y, H), max(lo_x, 0), min(hi_x, W)
        if lo_y >= hi_y or lo_x >= hi_x:
            loop[k] = "no component inside the frame"
            continue
        region = (lo_y, lo_x, hi_y - lo_y, hi_x - lo_x)
        if K > MAX_PRESENT and _most_present(region, boxes, [m.shape for m in morphs], kh,
                                             kw) > MAX_PRESENT:
            loop[k] = "more than {} components reach one tile".format(MAX_PRESENT)
            continue
        if _identical_pair(frame.shape, morphs, boxes):
            loop[k] = "two components with identical models"
            continue
        tiles = -(-region[2] // SPECTRA_TILE) * -(-region[3] // SPECTRA_TILE)
        E = K * K + 3 * K
        b = len(rows)
        rows.append((H, W) + region + (C, kh, kw, K, len(comp_rows), 0, cube_off[k], n_stamp,
                                       n_part, n_out))
        for m, (y0, x0) in zip(morphs, boxes):
            comp_rows.append((y0, x0, m.shape[0], m.shape[1], n_morph))
            morph_parts.append(m)
            n_morph += m.size
        work += [(b, t) for t in range(tiles)]
        stamp_parts.append(stamps)
        taken.append((k, parameters, C, K, n_out))
        n_stamp += stamps.size
        n_part += tiles * C * E
        n_out += C * E
    return dict(blends=np.array(rows, _SPECTRA_BLEND) if rows else np.zeros(0, _SPECTRA_BLEND),
                components=(np.array(comp_rows, _SPECTRA_COMPONENT) if comp_rows
                            else np.zeros(0, _SPECTRA_COMPONENT)),
                work=np.array(work, np.int32).reshape(-1, 2), morphs=morph_parts, n_morph=n_morph,
                stamps=stamp_parts, n_stamp=n_stamp, n_part=n_part, n_out=n_out, taken=taken,
                loop=loop)


def seen_components(sum_mw, sum_m, mean_w):
    """The components ``set_spectra_to_match`` solves a band for: those whose ``seen`` ratio
    ``sum m w / sum m / mean(w)`` exceeds 0.1; None where the loop has to decide (a ratio that
    is not finite, or within ``NEAR_SEEN`` of 0.1)."""
    with np.errstate(all="ignore"):
        ratio = np.asarray(sum_mw, np.float64) / np.asarray(sum_m, np.float64) / mean_w
    if not np.isfinite(ratio).all() or (np.abs(ratio - 0.1) <= NEAR_SEEN).any():
        return None
    return np.flatnonzero(ratio > 0.1)


def solve_spectra(sums, K, weights):
    """``(K, bands)`` spectra from the ``(bands, K K + 3 K)`` sums of the device -- G, r, sum m w
    and sum m per band -- and the observation's ``weights``, as ``set_spectra_to_match`` ends; or
    the reason (a string) why the loop has to take the blend."""
    C = sums.shape[0]
    spectra = np.zeros((K, C))
    for c in range(C):
        G, rest = sums[c, :K * K].reshape(K, K), sums[c, K * K:].reshape(3, K)
        mean_w = np.mean(weights[c].reshape(-1).astype(np.float64))
        seen = seen_components(rest[1], rest[2], mean_w)
        if seen is None:
            return "a band whose seen ratio is not finite or within {} of 0.1".format(NEAR_SEEN)
        try:
            spectra[seen, c] = np.linalg.inv(G[np.ix_(seen, seen)]) @ rest[0][seen]
        except np.linalg.LinAlgError:
            return "a singular normal matrix"
    if not np.isfinite(spectra).all():
        return "a spectrum that is not finite"
    return spectra


def _run_chunk(blends, opts, device, report):
    """``init_all_sources`` of the blends of one chunk, ``(frame, centers, observation)`` each:
    the list of their ``(sources, skipped)``, or the reason (a string) why the loop has to take
    the blend."""
    import time

    t0 = time.perf_counter()
    pk = pack_chunk(blends, opts)
    src_blend, src_pixel = pk["src_blend"], pk["src_pixel"]
    ns = len(src_blend)
    loop = dict(pk["loop"])
    dv = Launcher(device, pad=1)
    torch = dv.torch
    t1 = time.perf_counter()
    with torch.cuda.device(dv.dev):
        d_data, d_var = dv.cat(pk["data"], np.float32), dv.cat(pk["var"], np.float32)
        d_psfs, d_spec = dv.cat(pk["psfs"], np.float64), dv.up(pk["spectra"] if ns else np.zeros(1))
        d_snr = dv.empty(pk["n_snr"], np.float64)
        d_planes = dv.empty(pk["n_plane"], np.float64)
        d_bounds, d_peaks = dv.empty(4 * ns, np.int32), dv.empty(ns, np.float64)
        if opts["fallback"]:
            _call(dv, "psf_snr", pk["psf_snr"], d_data, d_var, pk["n_cube"], d_psfs, pk["n_psf"],
                  d_snr, pk["n_snr"])
        _call(dv, "sweep", pk["sweep"], d_data, d_var, pk["n_cube"], d_spec, len(pk["spectra"]),
              d_planes, pk["n_plane"], d_bounds, d_peaks, ns)
        snr = d_snr.cpu().numpy()
        bounds = d_bounds.cpu().numpy()[:4 * ns].reshape(ns, 4)
        t2 = time.perf_counter()
        # ---- between the launches: component count and box of every source
        counts, boxes, floors = [], [], {}
        for s, k in enumerate(src_blend):
            C = blends[k][0].C
            count = component_count(snr[pk["snr_off"][s]:pk["snr_off"][s] + 3 * C].reshape(C, 3),
                                    opts)
            if count is None:
                loop.setdefault(k, "a source whose snr / min_snr is not finite or within {} of a "
                                   "component count".format(NEAR_INTEGER))
            counts.append(count)
            boxes.append(trim_box(bounds[s], src_pixel[s], opts["boxsize"]))
        cropped = [s for s in range(ns) if src_blend[s] not in loop and counts[s] > 0]
        sizes = [counts[s] * boxes[s][1] ** 2 for s in cropped]
        out_off, n_out = offsets(sizes)
        floor_parts, floor_at, n_floor = [], {}, 0
        crop_t = np.zeros(len(cropped), _CROP_DESC)
        for j, s in enumerate(cropped):
            k = src_blend[s]
            frame, centers, _ = blends[k]
            (y0, x0), side = boxes[s]
            key = (id(frame), side)
            if key not in floor_at:
                floor_at[key] = n_floor
                floor_parts.append(_floor_image(floors, frame, centers[0], side))
                n_floor += side * side
            crop_t[j] = (frame.shape[1], frame.shape[2], y0, x0, side, counts[s],
                         pk["plane_off"][s], floor_at[key], out_off[j], 25.0)
        d_floors = dv.cat(floor_parts, np.float64)
        d_out, d_flags = dv.empty(n_out, np.float64), dv.empty(len(cropped), np.int32)
        _call(dv, "crop", crop_t, d_planes, pk["n_plane"], d_floors, n_floor, d_out, n_out,
              d_flags, len(cropped))
        morphs = d_out.cpu().numpy()
        flags = d_flags.cpu().numpy()[:len(cropped)]
    t3 = time.perf_counter()
    at, empty = {}, set()
    for j, s in enumerate(cropped):
        if flags[j] & 1:
            loop.setdefault(src_blend[s], "a morphology that is not finite")
        if flags[j] & 2:  # (the cut-out held no pixel > 0: what the loop warns about)
            empty.add(s)
        at[s] = int(out_off[j])
    # ---- the source objects
    results = [None if k in loop else ([], []) for k in range(len(blends))]
    noise = {}
    for s, k in enumerate(src_blend):
        if k in loop:
            continue
        frame, centers, obs = blends[k]
        center = centers[len(results[k][0])]
        if k not in noise:
            from .source import _noise_rms
            noise[k] = _noise_rms((obs,))
        if s in empty:
            logger.warning(f"No flux in morphology model for source at {center}")
        try:
            (y0, x0), side = boxes[s]
            layers = [morphs[at[s] + i * side * side:at[s] + (i + 1) * side * side]
                      .reshape(side, side).copy() for i in range(counts[s])]
            source = _assemble(frame, center, obs, counts[s], pk["src_spec"][s], layers,
                               Box((side, side), origin=(y0, x0)), noise[k], opts)
            source.check_parameters()
        except Exception as exc:  # (whatever it is, the loop meets and reports it)
            loop[k] = "{} while assembling a source".format(type(exc).__name__)
            results[k] = None
            continue
        results[k][0].append(source)
    t4 = time.perf_counter()
    # ---- the spectra: normal equations on the device, K x K solves on the host
    if opts["set_spectra"]:
        items = [(k, blends[k][0], blends[k][2], r[0]) for k, r in enumerate(results)
                 if r is not None and r[0]]
        sp = pack_spectra(items, pk["cube_off"])
        for k, why in sp["loop"].items():
            loop[k], results[k] = why, None
        if sp["taken"]:
            with torch.cuda.device(dv.dev):
                d_weights = dv.cat([b[2].weights for b in blends], np.float32)
                d_morphs, d_stamps = dv.cat(sp["morphs"], np.float64), dv.cat(sp["stamps"], np.float64)
                d_part, d_sums = dv.empty(sp["n_part"], np.float64), dv.empty(sp["n_out"], np.float64)
                _call(dv, "spectra_tiles", sp["blends"], sp["components"], sp["work"], d_data,
                      d_weights, pk["n_cube"], d_stamps, sp["n_stamp"], d_morphs, sp["n_morph"],
                      d_part, sp["n_part"], sp["n_out"])
                _call(dv, "spectra_reduce", sp["blends"], d_part, sp["n_part"], d_sums, sp["n_out"])
                sums = d_sums.cpu().numpy()
            for k, parameters, C, K, off in sp["taken"]:
                E = K * K + 3 * K
                spectra = solve_spectra(sums[off:off + C * E].reshape(C, E), K, blends[k][2].weights)
                if isinstance(spectra, str):
                    loop[k], results[k] = spectra, None
                    continue
                for p, row in zip(parameters, spectra):
                    p[:] = row
                for p in parameters:
                    if p.constraint is not None:
                        p[:] = p.constraint(p, 0)
    t5 = time.perf_counter()
    if report is not None:
        report["launches"] = list(dv.launches)  # (of the last chunk)
        times = report.setdefault("times", {})
        for name, dt in (("pack", t1 - t0), ("device", t2 - t1), ("crop", t3 - t2),
                         ("assemble", t4 - t3), ("spectra", t5 - t4)):
            times[name] = times.get(name, 0.0) + dt
    return [loop[k] if r is None else r for k, r in enumerate(results)]


def _assemble(frame, center, obs, count, per_obs, layers, bbox, noise, opts):
    """The source ``ExtendedSource(..., K=count)`` builds at ``center``, from the morphology
    layers of the device: the same classes, parameters, steps and constraint chains, through the
    classes' own parts."""
    from .component import CombinedComponent, FactorizedComponent
    from .source import (CompactExtendedSource, MultiExtendedSource, SingleExtendedSource,
                         _fitted_morphology)
    from .spectrum import TabulatedSpectrum

    shifting, resizing = opts["shifting"], opts["resizing"]
    if count == 0:
        return CompactExtendedSource(frame, center, (obs,), shifting=shifting, resizing=resizing,
                                     boxsize=opts["boxsize"])
    amplitudes = np.concatenate(per_obs).reshape(-1)
    if count == 1:
        source = SingleExtendedSource.__new__(SingleExtendedSource)
        spectrum = TabulatedSpectrum(frame, amplitudes, min_step=noise.copy())
        morphology = _fitted_morphology(frame, center, layers[0], bbox, shifting, resizing)
        FactorizedComponent.__init__(source, frame, spectrum, morphology)
        source.center = morphology.center
        return source
    source = MultiExtendedSource.__new__(MultiExtendedSource)
    # (what the single source's spectrum parameter holds)
    amplitudes = TabulatedSpectrum(frame, amplitudes, min_step=noise.copy()).get_parameter(0)._data
    min_step = noise / 10
    components = []
    for layer in layers:
        morphology = _fitted_morphology(frame, center, layer, bbox.copy(), shifting, resizing)
        components.append(FactorizedComponent(
            frame, TabulatedSpectrum(frame, amplitudes.copy(), min_step=min_step), morphology))
        source.center = morphology.center
    CombinedComponent.__init__(source, components)
    return source


def init_blends(frames, centers, observations, device=None, _working_set_bytes=None,
                _report=None, **options):
    """``init_all_sources`` for a catalogue: ``results[i]`` is what ``init_all_sources(frames[i],
    centers[i], observations[i], **options)`` returns, ``(sources, skipped)`` -- the same source
    classes, boxes, centres, steps, constraint chains and flags, the morphology images and the
    pixel spectra bit for bit -- with at most five launches of csrc/init_sources.hip per chunk
    of blends, whatever their frames, stamps and source counts: the point-source S/N that decides
    the component count, the spectrum-weighted coadd with symmetry, monotonic sweep and trim of
    every source, the normalised cut-outs with their bulge / disk split and, for
    ``set_spectra=True``, the float64 weighted normal equations of ``set_spectra_to_match`` tile
    by tile and their sum.  The host solves them (K x K per blend and band); these spectra agree
    with the loop's within the rounding of the two ways to form the sums (catalogue initialisation), and do
    not depend on the list a blend is in.

    ``observations[i]``: one ``Observation`` matched to ``frames[i]``, or a sequence holding one.
    The options are those of ``init_all_sources``.  Blends the device path does not take go
    through ``init_all_sources`` after the device groups, in list order; ``plan_init_blends``
    names them and says why.  So does a blend whose values leave a decision to the loop:
    non-finite data, a non-finite morphology or spectrum, a source whose ``snr / min_snr`` lies
    within 1e-4 (relative) of a component count, a band whose ``seen`` ratio lies within 1e-6 of
    0.1, two components with identical models, a singular normal matrix, more than 64
    components or more than 32 on one 16 x 16 tile.  ``device``: GPU index (default 0).
    ``_report``: a dict that receives ``fallback`` -- ``(position, reason)`` of the blends the
    loop took --, ``launches`` of the last chunk and the seconds by step in ``times``."""
    import time

    opts = _options(options)
    frames, centers, observations = list(frames), [list(c) for c in centers], list(observations)
    groups, fallback = plan_init_blends(frames, centers, observations, **options)
    budget, device = defaults(_working_set_bytes, device)
    results = [None] * len(frames)
    for idx in groups.values():
        items = [(i, _blend_bytes(frames[i], len(centers[i]), opts["boxsize"])) for i in idx]
        for chunk in chunks(items, budget):
            blends = [(frames[i], centers[i], tuple(_as_tuple(observations[i]))[0]) for i in chunk]
            for i, result in zip(chunk, _run_chunk(blends, opts, device, _report)):
                if isinstance(result, str):
                    fallback.append((i, "at run time: " + result))
                else:
                    results[i] = result
    t0 = time.perf_counter()
    for i, result in enumerate(results):
        if result is None:
            results[i] = init_all_sources(frames[i], centers[i], observations[i], **opts)
    if _report is not None:
        _report.setdefault("times", {})["loop"] = time.perf_counter() - t0
        _report["fallback"] = sorted(fallback)
    return results
