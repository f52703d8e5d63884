"""Parameterisation of ``scarlet.lite`` components and the joint spectrum fit
(reference scarlet/lite/initialization.py:140-186, 250-318, 608-645).

``init_all_sources_main`` (lite/initialization.py:321-419) is provided with both
monotonicity variants (weighted sweep, or ``use_mask=True``: the monotonic mask operators);
``init_all_sources_wavelets`` (lite/initialization.py:422-605) starts from the detection
coefficients of ``scarlet_amd.detect.get_detect_wavelets`` (starlet transform on the GPU);
``init_blends`` is the same initialisation for a catalogue of blends, as device batches
(csrc/lite_init.hip); ``init_blends_main`` is ``init_all_sources_main`` (weighted sweep) for a
catalogue of blends: coadd, symmetry, sweep and trim of every source on the device
(csrc/lite_init_main.hip), with one table of relative cosines per chunk in the place of a weight
table and a radial sort per source.
"""

from functools import partial

import numpy as np

from .._catalog import Launcher, chunks, defaults, offsets
from ..bbox import Box, overlapped_slices
from ..detect import get_detect_wavelets, get_detect_wavelets_batch
from ..initialization import get_minimal_boxsize, trim_morphology
from ..operator import (NEIGHBOR_COORDS, prox_monotonic_mask, prox_uncentered_symmetry,
                        prox_weighted_monotonic)
from ..parameter import relative_step
from .measure import calculate_snr
from .models import LiteComponent, LiteFactorizedComponent, LiteSource
from .parameters import AdaproxParameter, FistaParameter
from .spectra import _solve_spectra
from .utils import bounds_to_bbox, insert_image, project_morph_to_center


def get_min_psf(psfs, thresh=0.01):
    """Central part of a (bands, h, w) PSF cube outside of which no two bands differ by
    more than ``thresh`` relative to their overall maximum (lite/initialization.py:19-80)."""
    py, px = psfs.shape[1] // 2, psfs.shape[2] // 2
    xx, yy = np.meshgrid(np.arange(psfs.shape[-1]), np.arange(psfs.shape[-2]))
    R = np.sqrt((xx - px) ** 2 + (yy - py) ** 2)
    max_radius = 0
    for p1 in range(len(psfs) - 1):
        for p2 in range(p1 + 1, len(psfs)):
            diff = (psfs[p1] - psfs[p2]) / np.max([psfs[p1], psfs[p2]])
            max_radius = max(max_radius, int(np.max(R * (np.abs(diff) > thresh))))
    dy, dx = py - max_radius, px - max_radius
    sy = slice(dy, -dy) if dy > 0 else slice(None)
    sx = slice(dx, -dx) if dx > 0 else slice(None)
    return psfs[:, sy, sx].copy()


def init_monotonic_morph(detect, center, full_box, grow=0, normalize=True, use_mask=True,
                         thresh=0):
    """Morphology of a monotonic source cut out of the 2-D detection image ``detect``:
    the radial monotonicity operator ('angle' weights, sweep on the GPU) centred on
    ``center``, trimmed at ``thresh`` (lite/initialization.py:83-138).  Returns
    ``(bbox, morph)``; ``morph`` is None when nothing is left."""
    if use_mask:
        _, morph, bounds = prox_monotonic_mask(detect, 0, center, max_iter=0)
        bbox = bounds_to_bbox(bounds)
        if bbox.shape == (1, 1) and morph[bbox.slices][0, 0] == 0:
            return bbox, None
        if grow is not None and grow > 0:
            bbox = bbox.grow(grow)
        morph, bbox = project_morph_to_center(morph, center, bbox, full_box)
    else:
        prox = prox_weighted_monotonic(detect.shape, neighbor_weight="angle", center=center,
                                       min_gradient=0)
        morph = prox(detect, 0).reshape(detect.shape)
        morph, bbox = trim_morphology(center, morph, bg_thresh=thresh)
        if np.max(morph) == 0:
            return Box((0, 0, 0)), None
    if normalize:
        morph /= np.max(morph)
    return bbox, morph


def init_main_parameters(detect, center, observation, convolved=None, use_mask=False, thresh=0.5):
    """Box, morphology and spectrum of one source the way scarlet main initialises an
    ExtendedSource (lite/initialization.py:188-247): symmetrised detection image ->
    monotonic morphology trimmed at ``thresh * mean(noise_rms)``; spectrum = data over
    convolved morphology at the centre pixel."""
    symmetric = prox_uncentered_symmetry(detect.copy(), 0, center, "sdss")
    bbox, morph = init_monotonic_morph(symmetric, center, observation.bbox[1:], grow=0,
                                       normalize=False, use_mask=use_mask,
                                       thresh=np.mean(observation.noise_rms) * thresh)
    if morph is None:
        return bbox, None, None
    images = observation.images
    at_center = (slice(None), center[0], center[1])
    if convolved is None:
        full = insert_image(observation.bbox[1:], bbox, morph)
        convolved = observation.convolve(np.repeat(full[None], images.shape[0], axis=0), mode="real")
    sed = images[at_center] / convolved[at_center]
    sed[sed < 0] = 0
    peak = np.max(morph)
    return bbox, morph / peak, sed * peak


def init_all_sources_main(observation, centers, detect=None, min_snr=50, use_mask=False,
                          percentile=25, thresh=0.5):
    """One ``LiteSource`` of plain ``LiteComponent``s per centre
    (lite/initialization.py:321-419): PSF-shaped if nothing monotonic is found, two
    components (bulge above / disk below ``percentile`` % of the peak, spectra by a joint
    fit) when the PSF-weighted SNR allows ``2 * min_snr``, otherwise one.  Wrap the
    result with ``parameterize_sources``."""
    if detect is None:
        detect = np.sum(observation.images / (observation.noise_rms**2)[:, None, None], axis=0)
    bands = observation.shape[0]
    convolved = observation.convolve(np.repeat(detect[None], bands, axis=0), mode="real")
    model_psf = observation.model_psf[0]
    py, px = model_psf.shape[0] // 2, model_psf.shape[1] // 2
    psf_sed = observation.convolve(np.repeat(observation.model_psf, bands, axis=0),
                                   mode="real")[:, py, px]
    spec_box = observation.bbox[0]
    sources = []
    for center in centers:
        snr = np.floor(calculate_snr(observation.images, observation.variance, observation.psfs,
                                     center))
        bbox, morph, sed = init_main_parameters(detect, center, observation, convolved, use_mask,
                                                thresh)
        if morph is None:
            sed = observation.images[:, center[0], center[1]] / psf_sed
            sed[sed < 0] = 0
            bbox = Box(model_psf.shape, origin=(center[0] - py, center[1] - px))
            comps = [LiteComponent(center, spec_box @ bbox, sed, model_psf / np.max(model_psf))]
        elif snr / min_snr >= 2:
            level = percentile / 100
            bulge = np.maximum(morph - level, 0)
            disk = np.minimum(morph, level)
            bulge /= np.max(bulge)
            disk /= np.max(disk)
            bulge_sed, disk_sed = multifit_seds(observation, [bulge, disk], [bbox, bbox])
            comps = [LiteComponent(center, spec_box @ bbox, bulge_sed, bulge),
                     LiteComponent(center, spec_box @ bbox, disk_sed, disk)]
        else:
            comps = [LiteComponent(center, spec_box @ bbox, sed, morph)]
        sources.append(LiteSource(comps, observation.dtype))
    return sources


def multifit_seds(observation, morphs, boxes):
    """Least-squares spectra of all components at once, band by band: the convolved
    morphologies are the columns of the design matrix."""
    if len(morphs) != len(boxes):
        raise ValueError("morphs and boxes should have the same number of parameters, "
                         "got {} and {} respectively".format(len(morphs), len(boxes)))
    bands = observation.images.shape[0]
    dtype = observation.images.dtype
    spec_box = observation.bbox[0]
    full_box = boxes[0]
    for box in boxes[1:]:
        full_box = full_box | box
    full_box = spec_box @ full_box
    img = insert_image(full_box, observation.bbox, observation.images)
    design = np.zeros((bands, len(morphs), img[0].size), dtype=dtype)
    for k, (morph, bbox) in enumerate(zip(morphs, boxes)):
        # one broadcast copy of the morphology per band, convolved with that band's kernel
        cube = np.repeat(insert_image(full_box[1:], bbox, morph)[None], bands, axis=0)
        design[:, k] = observation.convolve(cube).reshape(bands, -1)
    seds = np.zeros((len(morphs), bands), dtype=dtype)
    for b in range(bands):
        seds[:, b] = np.linalg.lstsq(design[b].T, img[b].reshape(-1), rcond=None)[0]
    seds[seds < 0] = 0
    return seds


def init_adaprox_component(center, bbox, sed, morph, observation, factor=10, bg_thresh=None,
                           max_prox_iter=1):
    """Component whose parameters follow proximal AMSGrad: spectrum step 1 % of its mean
    but at least ``noise_rms / factor``, morphology step 1e-2."""
    sed = AdaproxParameter(
        sed, step=partial(relative_step, factor=1e-2, minimum=observation.noise_rms / factor),
        max_prox_iter=max_prox_iter)
    morph = AdaproxParameter(morph, step=1e-2, max_prox_iter=max_prox_iter)
    return LiteFactorizedComponent(sed, morph, center, bbox, observation.bbox,
                                   observation.noise_rms, bg_thresh=bg_thresh)


def init_fista_component(center, bbox, sed, morph, observation, bg_thresh=None):
    """Component whose parameters follow FISTA with step 1 / (2 <w>), <w> the mean
    positive weight inside the box."""
    _, in_obs = overlapped_slices(bbox, observation.bbox)
    w = observation.weights[in_obs]
    step = 1 / (2 * np.mean(w[w > 0]))
    return LiteFactorizedComponent(FistaParameter(sed, step=step), FistaParameter(morph, step=step),
                                   center, bbox, observation.bbox, observation.noise_rms,
                                   bg_thresh=bg_thresh)


class WaveletInitParameters:
    """What every source of one wavelet initialisation shares: the positive detection
    coefficients summed over all scales but the last (``detectlets``), over ``bulge_slice``
    and over ``disk_slice``, the observation convolved with ``detectlets`` and the spectrum of
    the model PSF.  See ``init_all_sources_wavelets`` for the parameters."""

    def __init__(self, observation, bulge_slice=slice(None, 2), disk_slice=slice(2, -1),
                 bulge_grow=5, disk_grow=5, use_psf=True, scales=5, wavelets=None):
        if wavelets is None:
            wavelets = get_detect_wavelets(observation.images, observation.variance,
                                           scales=scales)
        wavelets[wavelets < 0] = 0
        self.detectlets = np.sum(wavelets[:-1], axis=0)
        self.bulgelets = np.sum(wavelets[bulge_slice], axis=0)
        self.disklets = np.sum(wavelets[disk_slice], axis=0)
        bands = observation.shape[0]
        model_psf = observation.model_psf[0]
        self.convolved = observation.convolve(np.repeat(self.detectlets[None], bands, axis=0),
                                              mode="real")
        self.py = observation.model_psf.shape[1] // 2
        self.px = observation.model_psf.shape[2] // 2
        self.psf_sed = observation.convolve(np.repeat(model_psf[None], bands, axis=0),
                                            mode="real")[:, self.py, self.px]
        self.observation = observation
        self.images = observation.images
        self.bulge_grow = bulge_grow
        self.disk_grow = disk_grow
        self.use_psf = use_psf


def init_wavelet_source(center, nbr_components, init):
    """One ``LiteSource`` at ``center`` from the wavelet coefficients in ``init``
    (``WaveletInitParameters``): the model PSF when ``nbr_components < 1`` (and
    ``init.use_psf``) or when nothing is detected at the centre; one monotonic component for
    ``nbr_components < 2``; otherwise a bulge and a disk component, falling back to one
    component if either is empty.  As in the reference, the result is an empty source when the
    single component vanishes and None when neither bulge nor disk is found."""
    obs = init.observation
    spec_box = obs.bbox[0]
    at_center = (slice(None), center[0], center[1])
    if (nbr_components < 1 and init.use_psf) or init.detectlets[center[0], center[1]] <= 0:
        model_psf = obs.model_psf[0]
        sed = init.images[at_center] / init.psf_sed
        sed[sed < 0] = 0
        bbox = Box(model_psf.shape, origin=(center[0] - init.py, center[1] - init.px))
        return LiteSource([LiteComponent(center, spec_box @ bbox, sed,
                                         model_psf / np.max(model_psf))], obs.dtype)
    if nbr_components < 2:
        bbox, morph = init_monotonic_morph(init.detectlets, center, obs.bbox[1:],
                                           init.disk_grow)
        if morph is None or np.max(morph) <= 0:
            return LiteSource([], obs.dtype)
        sed = init.images[at_center] / init.convolved[at_center]
        sed[sed < 0] = 0
        return LiteSource([LiteComponent(center, spec_box @ bbox, sed, morph / np.max(morph))],
                          obs.dtype)
    bulge_box, bulge = init_monotonic_morph(init.bulgelets, center, obs.bbox[1:],
                                            init.bulge_grow)
    disk_box, disk = init_monotonic_morph(init.disklets, center, obs.bbox[1:], init.disk_grow)
    if bulge is None and disk is None:
        return None
    if bulge is None or disk is None:
        return init_wavelet_source(center, 1, init)
    bulge_sed, disk_sed = multifit_seds(obs, [bulge, disk], [bulge_box, disk_box])
    comps = []
    # (the reference tests the bulge by its count of non-zero entries, the disk by its sum)
    if np.count_nonzero(bulge_sed):
        comps.append(LiteComponent(center, spec_box @ bulge_box, bulge_sed, bulge))
    if np.sum(disk_sed) != 0:
        comps.append(LiteComponent(center, spec_box @ disk_box, disk_sed, disk))
    return LiteSource(comps, obs.dtype)


def init_all_sources_wavelets(observation, centers, min_snr=50, bulge_grow=5, disk_grow=5,
                              use_psf=True, bulge_slice=slice(None, 2), disk_slice=slice(2, -1),
                              scales=5, wavelets=None):
    """One source per centre from wavelet detection images (lite/initialization.py:568-605):
    the number of components is ``floor(SNR) / min_snr`` (PSF below 1, one component below 2,
    bulge and disk above).  ``wavelets``: detection coefficients ``(scales+1, Ny, Nx)``,
    default ``get_detect_wavelets(images, variance, scales)``.  Wrap the result with
    ``parameterize_sources`` before fitting."""
    init = WaveletInitParameters(observation, bulge_slice, disk_slice, bulge_grow, disk_grow,
                                 use_psf, scales, wavelets)
    sources = []
    for center in centers:
        snr = np.floor(calculate_snr(observation.images, observation.variance, observation.psfs,
                                     center))
        sources.append(init_wavelet_source(center, snr / min_snr, init))
    return sources


def parameterize_sources(sources, observation, parameterization):
    """Re-wrap the spectra / morphologies of ``sources`` with ``parameterization``
    (e.g. ``init_adaprox_component``); inputs are copied."""
    out = []
    for src in sources:
        comps = [parameterization(center=tuple(c.center), sed=c.sed.copy(), morph=c.morph.copy(),
                                  bbox=c.bbox.copy(), observation=observation)
                 for c in src.components]
        out.append(LiteSource(comps, src.dtype))
    return out


# ---------------------------------------------------------------------------
# init_blends: init_all_sources_wavelets for a catalogue, device batches per group
# ---------------------------------------------------------------------------
# lite_init.hip: frame sides, pixels of a frame (one workgroup fills a mask), stamp sides,
# wavelet planes; a blend beyond them takes init_all_sources_wavelets
_MAX_EXTENT = 1 << 14
_MAX_PIXELS = 1 << 22
_MAX_STAMP = 255
_MAX_PLANES = 64

_i4, _i8 = "i4", "i8"
_COADD_DESC = np.dtype([("n_planes", _i4), ("first", _i4, 3), ("count", _i4, 3), ("step", _i4, 3),
                        ("reserved", _i4, 2), ("n_pix", _i8), ("wavelet_off", _i8),
                        ("coadd_off", _i8)], align=True)
_SNR_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4), ("ph", _i4), ("pw", _i4),
                      ("image_off", _i8), ("psf_off", _i8)], align=True)
_TAPS_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4), ("kh", _i4), ("kw", _i4),
                       ("plane_off", _i8), ("stamp_off", _i8), ("out_off", _i8)], align=True)
_MASK_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4), ("plane_off", _i8),
                       ("pix_off", _i8), ("valid_off", _i8)], align=True)
_CROP_DESC = np.dtype([("h", _i4), ("w", _i4), ("y0", _i4), ("x0", _i4), ("bh", _i4), ("bw", _i4),
                       ("plane_off", _i8), ("valid_off", _i8), ("out_off", _i8)], align=True)
_FIT_DESC = np.dtype([("h", _i4), ("w", _i4), ("y0", _i4), ("x0", _i4), ("fh", _i4), ("fw", _i4),
                      ("a_y0", _i4), ("a_x0", _i4), ("a_h", _i4), ("a_w", _i4),
                      ("b_y0", _i4), ("b_x0", _i4), ("b_h", _i4), ("b_w", _i4),
                      ("kh", _i4), ("kw", _i4), ("image_off", _i8), ("stamp_off", _i8),
                      ("a_off", _i8), ("b_off", _i8)], align=True)
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _np_dtype(a):
    """NumPy dtype of a host array or a torch tensor (None for what NumPy does not have)."""
    if _is_tensor(a):
        name = str(a.dtype).split(".")[-1]
        try:
            return np.dtype(name)
        except TypeError:
            return None
    return np.asarray(a).dtype


def _plane_selection(sl, n_planes):
    """``(first, count, step)`` of the planes ``wavelets[sl]`` holds, in its order."""
    r = range(*sl.indices(n_planes))
    return (r.start if len(r) else 0), len(r), r.step


def _init_key(obs, wavelets, bulge_slice, disk_slice, scales):
    """``(key, reason)``: the group ``(wavelet dtype, image dtype, model PSF dtype, bands)`` of
    a blend the device batch takes, or None and why it goes through
    ``init_all_sources_wavelets``."""
    images = obs.images
    if not isinstance(images, np.ndarray) or images.ndim != 3:
        return None, "images.ndim != 3"
    if images.dtype not in _FLOATS:
        return None, "images are neither float32 nor float64"
    C, h, w = images.shape
    if min(C, h, w) < 1 or max(h, w) > _MAX_EXTENT or h * w > _MAX_PIXELS or C > 65535:
        return None, "frame beyond the kernel's limits"
    if tuple(obs.bbox.shape) != images.shape or any(obs.bbox.origin):
        return None, "the observation's box is not its image at the origin"
    variance = obs.variance
    if (not isinstance(variance, np.ndarray) or variance.shape != images.shape
            or variance.dtype != images.dtype):
        return None, "variance differs from the images in shape or dtype"
    if obs.model_psf is None or obs.diff_kernel is None:
        return None, "no model PSF"
    model_psf = np.asarray(obs.model_psf)
    if model_psf.ndim != 3 or model_psf.dtype not in _FLOATS:
        return None, "model PSF is not a float32 / float64 cube"
    psfs = np.asarray(obs.psfs)
    if psfs.ndim != 3 or psfs.shape[0] != C or psfs.dtype != images.dtype:
        return None, "PSFs differ from the images in bands or dtype"
    stamp = np.asarray(obs.diff_kernel.image)
    if stamp.ndim != 3 or stamp.shape[0] not in (1, C):
        return None, "difference kernel is not a stamp per band"
    if stamp.shape[1] % 2 == 0 or stamp.shape[2] % 2 == 0:
        return None, "even difference-kernel stamp"
    if (max(stamp.shape[1:]) > _MAX_STAMP or max(psfs.shape[1:]) > _MAX_STAMP
            or max(model_psf.shape[1:]) > _MAX_STAMP):
        return None, "stamp beyond the kernel's limits"
    if not (isinstance(bulge_slice, slice) and isinstance(disk_slice, slice)):
        return None, "plane selection is not a slice"
    if wavelets is None:
        wdtype = np.dtype(np.float64)  # get_detect_wavelets
        if min(h, w) < 2:
            return None, "frame too small for the starlet transform"
    else:
        wdtype = _np_dtype(wavelets)
        if wdtype not in _FLOATS:
            return None, "wavelets are neither float32 nor float64"
        shape = tuple(wavelets.shape)
        if len(shape) != 3 or shape[1:] != (h, w) or not 1 <= shape[0] <= _MAX_PLANES:
            return None, "wavelets are not (planes, Ny, Nx) of the frame"
    return (wdtype, images.dtype, model_psf.dtype, C), None


def plan_init_blends(observations, centers, wavelets=None, bulge_slice=slice(None, 2),
                     disk_slice=slice(2, -1), scales=5):
    """``(groups, fallback)`` of ``init_blends``, without touching the GPU: the positions of
    the blends of every device group, keyed by ``(wavelet dtype, image dtype, model PSF dtype,
    bands)`` in order of first appearance and in input order inside a group, and
    ``(position, reason)`` of the blends that go through ``init_all_sources_wavelets``.
    Raises ``ValueError`` for a centre outside its frame, or a catalogue whose arguments
    differ in length."""
    observations, centers = list(observations), list(centers)
    wavelets = [None] * len(observations) if wavelets is None else list(wavelets)
    if not len(observations) == len(centers) == len(wavelets):
        raise ValueError("observations, centers and wavelets must have one entry per blend, got "
                         "{}, {} and {}".format(len(observations), len(centers), len(wavelets)))
    groups, fallback = {}, []
    for i, (obs, cs, wav) in enumerate(zip(observations, centers, wavelets)):
        shape = np.shape(obs.images)
        if len(shape) == 3:
            for c in cs:
                if not (len(c) == 2 and 0 <= c[0] < shape[1] and 0 <= c[1] < shape[2]):
                    raise ValueError("blend {}: centre {} lies outside its {} x {} frame".format(
                        i, tuple(c), shape[1], shape[2]))
        key, reason = _init_key(obs, wav, bulge_slice, disk_slice, scales)
        if key is None:
            fallback.append((i, reason))
        else:
            groups.setdefault(key, []).append(i)
    return groups, fallback


def _n_planes(obs, wavelets, scales):
    """Planes of a blend's detection coefficients: the passed ones, or those
    ``get_detect_wavelets`` will make."""
    if wavelets is not None:
        return int(wavelets.shape[0])
    from ..wavelet import _checked_scales

    return _checked_scales(obs.images.shape, scales) + 1


def _init_bytes(obs, n_sources, n_planes, key):
    """Bytes of the device working set of one blend: wavelets (written straight into the
    chunk's buffer) and coadds, images and variance, the stamps in the wavelets' type and in
    float64, and per source the state of up to three mask tasks (visited, two flag maps,
    valid map)."""
    wdtype, idtype, _, C = key
    n = obs.images.shape[1] * obs.images.shape[2]
    stamp = C * int(np.prod(np.shape(obs.diff_kernel.image)[1:]))
    return ((n_planes + 3) * n * wdtype.itemsize + 2 * C * n * idtype.itemsize
            + stamp * (wdtype.itemsize + 8) + n_sources * 3 * 7 * n)


def _monotonic_box(bounds, seed_value, center, grow):
    """The box ``init_monotonic_morph(use_mask=True)`` cuts around ``center`` for a mask with
    ``bounds`` whose seed holds ``seed_value``; None when nothing is left.  (The size rule is
    that of ``project_morph_to_center``, which needs the full-frame morphology.)"""
    bbox = bounds_to_bbox(bounds)
    if bbox.shape == (1, 1) and seed_value == 0:
        return None
    if grow is not None and grow > 0:
        bbox = bbox.grow(grow)
    if bbox.contains(center):
        size = 2 * max(center[0] - bbox.start[-2], bbox.stop[0] - center[-2],
                       center[1] - bbox.start[-1], bbox.stop[1] - center[-1])
    else:
        size = 0
    half = get_minimal_boxsize(size) // 2
    return Box.from_bounds((center[0] - half, center[0] + half + 1),
                           (center[1] - half, center[1] + half + 1))


def _solve_pairs(sums, dtype):
    """Spectra ``(n, 2, C)`` of ``dtype`` from the sums ``(n, C, 5)`` of the normal equations
    (a.a, a.b, b.b, a.img, b.img): the minimum-norm solution of every 2 x 2 system, then the
    ``< 0`` clip of ``multifit_seds``."""
    n, C = sums.shape[:2]
    seds = np.zeros((n, 2, C), dtype=dtype)
    if n == 0:
        return seds
    gram = np.empty((n, C, 2, 2))
    gram[..., 0, 0], gram[..., 1, 1] = sums[..., 0], sums[..., 2]
    gram[..., 0, 1] = gram[..., 1, 0] = sums[..., 1]
    seds[:] = np.moveaxis(_solve_spectra(gram, sums[..., 3:], dtype), 1, 2)
    return seds


def _call(ch, C, step, dtype, table, *args):
    """One smi_lite_init_<step>_<dtype> launch through the chunk's ``Launcher``; the entries
    whose kernels loop over the bands take ``C`` first."""
    entry = "smi_lite_init_%s_%s" % (step, "f64" if dtype == np.float64 else "f32")
    ch.call(entry, table, *args, head=(C,) if step in ("snr", "taps", "fit") else (), tag=step)


def _run_init_chunk(blends, key, opts, device):
    """``init_all_sources_wavelets`` of the blends of one chunk: ``blends`` is a list of
    ``(observation, centers, wavelets)``; returns the list of their source lists.  Three
    steps: the detection coefficients in one device buffer, the launches with the host
    decisions between them, the assembly of the sources on the host."""
    ch = Launcher(device)
    with ch.torch.cuda.device(ch.dev):
        d_wavelets, n_planes = _chunk_wavelets(ch, key, blends, opts)
        state = _chunk_launches(ch, key, blends, opts, d_wavelets, n_planes)
    return _chunk_assemble(blends, state)


def _chunk_wavelets(ch, key, blends, opts):
    """The detection coefficients of the chunk's blends, one after another in one device
    buffer (those not passed in come from one ``get_detect_wavelets_batch`` call for all of
    them and never visit the host), and the number of planes of every blend.  Passed arrays
    and tensors are only read."""
    n_planes = [_n_planes(obs, wav, opts["scales"]) for obs, _, wav in blends]
    sizes = [p * obs.images.shape[1] * obs.images.shape[2]
             for p, (obs, _, _) in zip(n_planes, blends)]
    off, total = offsets(sizes)
    d_wavelets = ch.empty(total, key[0])
    missing = [obs for obs, _, wav in blends if wav is None]
    computed = iter(get_detect_wavelets_batch([obs.images for obs in missing],
                                              [obs.variance for obs in missing],
                                              scales=opts["scales"], device=True))
    for (obs, _, wav), at, n in zip(blends, off, sizes):
        if wav is None:
            wav = next(computed)
        elif not _is_tensor(wav):
            wav = ch.torch.from_numpy(np.ascontiguousarray(wav))
        d_wavelets[at:at + n].copy_(wav.reshape(-1))
    return d_wavelets, n_planes


_PSF, _ONE, _TWO, _NONE = 0, 1, 2, 3  # component classes; _NONE: neither bulge nor disk


def _chunk_launches(ch, key, blends, opts, d_wavelets, n_planes):
    """Everything of a chunk that touches the device: packs and uploads the inputs, runs the
    seven (eight with 2 -> 1 fallbacks) launches of lite_init.hip and decides on the host, as
    ``init_wavelet_source`` does, what follows from each.  Returns what the assembly needs,
    all of it in host memory."""
    from types import SimpleNamespace

    wdtype, idtype, mdtype, C = key
    call = partial(_call, ch, C)
    nb = len(blends)
    # ---- the three coadds
    n_pix = np.array([b[0].images.shape[1] * b[0].images.shape[2] for b in blends], np.int64)
    wav_off, n_wav = offsets(np.array(n_planes, np.int64) * n_pix)
    coadd_off, n_coadd = offsets(3 * n_pix)
    image_off, n_image = offsets(C * n_pix)
    coadds = np.zeros(nb, _COADD_DESC)
    for b in range(nb):
        sel = [_plane_selection(sl, n_planes[b])
               for sl in (slice(None, -1), opts["bulge_slice"], opts["disk_slice"])]
        coadds[b] = (n_planes[b], [s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel],
                     (0, 0), n_pix[b], wav_off[b], coadd_off[b])
    d_coadds = ch.empty(n_coadd, wdtype)
    call("coadd", wdtype, coadds, d_wavelets, n_wav, d_coadds, n_coadd)
    # ---- per source: SNR sums, centre taps; per blend: the spectrum of the model PSF
    d_images = ch.cat([b[0].images for b in blends], idtype)
    d_variance = ch.cat([b[0].variance for b in blends], idtype)
    psf_off, n_psf = offsets([b[0].psfs.size for b in blends])
    d_psfs = ch.cat([b[0].psfs for b in blends], idtype)
    stamps = [np.broadcast_to(np.asarray(b[0].diff_kernel.image),
                              (C,) + np.shape(b[0].diff_kernel.image)[1:]) for b in blends]
    stamp_off, n_stamp = offsets([s.size for s in stamps])
    d_stamps_w = ch.cat(stamps, wdtype)
    d_stamps_m = d_stamps_w if mdtype == wdtype else ch.cat(stamps, mdtype)
    model_psfs = [np.asarray(b[0].model_psf)[0] for b in blends]
    mpsf_off, n_mpsf = offsets([m.size for m in model_psfs])
    d_model_psfs = ch.cat(model_psfs, mdtype)

    src_blend = np.array([b for b in range(nb) for _ in blends[b][1]], np.int64)
    src_center = [c for b in blends for c in b[1]]
    ns = len(src_center)
    snr_t, taps_t = np.zeros(ns, _SNR_DESC), np.zeros(ns, _TAPS_DESC)
    ptaps_t = np.zeros(nb, _TAPS_DESC)
    for s in range(ns):
        b = src_blend[s]
        _, h, w = blends[b][0].images.shape
        cy, cx = int(src_center[s][0]), int(src_center[s][1])
        _, ph, pw = blends[b][0].psfs.shape
        _, kh, kw = stamps[b].shape
        snr_t[s] = (h, w, cy, cx, ph, pw, image_off[b], psf_off[b])
        taps_t[s] = (h, w, cy, cx, kh, kw, coadd_off[b], stamp_off[b], s * (C + 1))
    for b in range(nb):
        mh, mw = model_psfs[b].shape
        _, kh, kw = stamps[b].shape
        ptaps_t[b] = (mh, mw, mh // 2, mw // 2, kh, kw, mpsf_off[b], stamp_off[b], b * (C + 1))
    d_snr = ch.empty(2 * ns, np.float64)
    d_taps = ch.empty(ns * (C + 1), wdtype)
    d_ptaps = ch.empty(nb * (C + 1), mdtype)
    call("snr", idtype, snr_t, d_images, d_variance, n_image, d_psfs, n_psf, d_snr, 2 * ns)
    call("taps", wdtype, taps_t, d_coadds, n_coadd, d_stamps_w, n_stamp, d_taps, ns * (C + 1))
    call("taps", mdtype, ptaps_t, d_model_psfs, n_mpsf, d_stamps_m, n_stamp, d_ptaps,
         nb * (C + 1))
    snr = d_snr.cpu().numpy()[:2 * ns].reshape(ns, 2)
    taps = d_taps.cpu().numpy()[:ns * (C + 1)].reshape(ns, C + 1)
    ptaps = d_ptaps.cpu().numpy()[:nb * (C + 1)].reshape(nb, C + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_comp = np.floor(snr[:, 0] / np.sqrt(snr[:, 1])) / opts["min_snr"]
    # ---- the component class of every source, as init_wavelet_source decides it
    kind = np.full(ns, _TWO)
    kind[n_comp < 2] = _ONE
    if opts["use_psf"]:
        kind[n_comp < 1] = _PSF
    kind[taps[:, C] <= 0] = _PSF
    grows = (opts["disk_grow"], opts["bulge_grow"], opts["disk_grow"])  # of planes 0, 1, 2

    # ---- monotonic masks: (source, plane) tasks, one more launch for the 2 -> 1 fallbacks
    n_valid = int(sum(n_pix[src_blend[s]] * (3 if kind[s] == _TWO else 1)
                      for s in range(ns) if kind[s] != _PSF))
    d_valid = ch.empty(n_valid, np.uint8)
    valid_used = [0]

    def run_masks(tasks):
        """Boxes (None: nothing left) and valid-map offsets of the ``(source, plane)`` tasks."""
        table = np.zeros(len(tasks), _MASK_DESC)
        pix = 0
        for k, (s, plane) in enumerate(tasks):
            b = src_blend[s]
            _, h, w = blends[b][0].images.shape
            table[k] = (h, w, int(src_center[s][0]), int(src_center[s][1]),
                        coadd_off[b] + plane * n_pix[b], pix, valid_used[0])
            pix += n_pix[b]
            valid_used[0] += n_pix[b]
        d_visited, d_unchecked = ch.empty(pix, np.int32), ch.empty(pix, np.uint8)
        d_orphans = ch.empty(pix, np.uint8)
        d_bounds, d_seeds = ch.empty(4 * len(tasks), np.int32), ch.empty(len(tasks), wdtype)
        call("masks", wdtype, table, d_coadds, n_coadd, d_visited, d_unchecked, d_orphans, pix,
             d_valid, n_valid, d_bounds, d_seeds, len(tasks))
        bounds = d_bounds.cpu().numpy()[:4 * len(tasks)].reshape(-1, 4)
        seeds = d_seeds.cpu().numpy()
        return [(_monotonic_box(bounds[k], seeds[k], src_center[s], grows[plane]),
                 int(table[k]["valid_off"])) for k, (s, plane) in enumerate(tasks)]

    tasks = []
    for s in range(ns):
        if kind[s] == _ONE:
            tasks.append((s, 0))
        elif kind[s] == _TWO:
            tasks += [(s, 1), (s, 2)]
    found = dict(zip(tasks, run_masks(tasks))) if tasks else {}
    again = []
    for s in range(ns):
        if kind[s] != _TWO:
            continue
        bulge, disk = found[(s, 1)][0], found[(s, 2)][0]
        if bulge is None and disk is None:
            kind[s] = _NONE
        elif bulge is None or disk is None:
            kind[s] = _ONE  # init_wavelet_source(center, 1, init); detectlets[center] > 0 holds
            again.append((s, 0))
    if again:
        found.update(zip(again, run_masks(again)))

    # ---- crop and normalise every component, then the joint fits
    comps = []  # (source, plane, box, valid_off)
    for s in range(ns):
        for plane in {_ONE: (0,), _TWO: (1, 2)}.get(int(kind[s]), ()):
            box, valid_off = found[(s, plane)]
            if box is not None:
                comps.append((s, plane, box, valid_off))
    out_off, n_out = offsets([c[2].shape[0] * c[2].shape[1] for c in comps])
    crop_t = np.zeros(len(comps), _CROP_DESC)
    comp_at = {}
    for k, (s, plane, box, valid_off) in enumerate(comps):
        b = src_blend[s]
        _, h, w = blends[b][0].images.shape
        crop_t[k] = (h, w, box.origin[0], box.origin[1], box.shape[0], box.shape[1],
                     coadd_off[b] + plane * n_pix[b], valid_off, out_off[k])
        comp_at[(s, plane)] = k
    d_out = ch.empty(n_out, wdtype)
    call("crop", wdtype, crop_t, d_coadds, n_coadd, d_valid, n_valid, d_out, n_out)
    pairs = [s for s in range(ns) if kind[s] == _TWO]
    fit_t = np.zeros(len(pairs), _FIT_DESC)
    for k, s in enumerate(pairs):
        b = src_blend[s]
        _, h, w = blends[b][0].images.shape
        _, kh, kw = stamps[b].shape
        ka, kb = comp_at[(s, 1)], comp_at[(s, 2)]
        a, bb = comps[ka][2], comps[kb][2]
        full = a | bb
        fit_t[k] = (h, w, full.origin[0], full.origin[1], full.shape[0], full.shape[1],
                    a.origin[0], a.origin[1], a.shape[0], a.shape[1],
                    bb.origin[0], bb.origin[1], bb.shape[0], bb.shape[1], kh, kw,
                    image_off[b], stamp_off[b], out_off[ka], out_off[kb])
    d_sums = ch.empty(len(pairs) * C * 5, np.float64)
    if len(pairs):
        d_stamps_fit = ch.cat(stamps, np.float64)
        call("fit", wdtype, fit_t, d_out, n_out, d_images, int(idtype == np.float64), n_image,
             d_stamps_fit, n_stamp, d_sums, len(pairs) * C * 5)
    morphs = d_out.cpu().numpy()
    sums = d_sums.cpu().numpy()[:len(pairs) * C * 5].reshape(len(pairs), C, 5)
    boxes = {key: comps[k][2] for key, k in comp_at.items()}
    offs = {key: int(out_off[k]) for key, k in comp_at.items()}
    return SimpleNamespace(C=C, idtype=idtype, src_blend=src_blend, src_center=src_center,
                           kind=kind, taps=taps, ptaps=ptaps, boxes=boxes, offs=offs,
                           morphs=morphs, pairs=pairs, sums=sums)


def _chunk_assemble(blends, st):
    """The sources of a chunk from what ``_chunk_launches`` brought back, source by source as
    ``init_wavelet_source`` builds them."""
    C = st.C
    pair_seds = dict(zip(st.pairs, _solve_pairs(st.sums, st.idtype)))
    results = [[] for _ in blends]
    for s, center in enumerate(st.src_center):
        b = st.src_blend[s]
        obs = blends[b][0]
        spec_box = obs.bbox[0]
        at_center = (slice(None), center[0], center[1])

        def morph_of(plane):
            box, at = st.boxes[(s, plane)], st.offs[(s, plane)]
            return box, st.morphs[at:at + box.shape[0] * box.shape[1]].reshape(box.shape).copy()

        kind = st.kind[s]
        if kind == _PSF:
            model_psf = obs.model_psf[0]
            py, px = obs.model_psf.shape[1] // 2, obs.model_psf.shape[2] // 2
            sed = obs.images[at_center] / st.ptaps[b, :C]
            sed[sed < 0] = 0
            bbox = Box(model_psf.shape, origin=(center[0] - py, center[1] - px))
            src = LiteSource([LiteComponent(center, spec_box @ bbox, sed,
                                            model_psf / np.max(model_psf))], obs.dtype)
        elif kind == _NONE:
            src = None
        elif kind == _ONE:
            if (s, 0) not in st.boxes:
                src = LiteSource([], obs.dtype)
            else:
                bbox, morph = morph_of(0)
                if np.max(morph) <= 0:
                    src = LiteSource([], obs.dtype)
                else:
                    sed = obs.images[at_center] / st.taps[s, :C]
                    sed[sed < 0] = 0
                    src = LiteSource([LiteComponent(center, spec_box @ bbox, sed,
                                                    morph / np.max(morph))], obs.dtype)
        else:
            (bulge_box, bulge), (disk_box, disk) = morph_of(1), morph_of(2)
            bulge_sed, disk_sed = pair_seds[s]
            cs = []
            # (the reference tests the bulge by its count of non-zero entries, the disk by its sum)
            if np.count_nonzero(bulge_sed):
                cs.append(LiteComponent(center, spec_box @ bulge_box, bulge_sed, bulge))
            if np.sum(disk_sed) != 0:
                cs.append(LiteComponent(center, spec_box @ disk_box, disk_sed, disk))
            src = LiteSource(cs, obs.dtype)
        results[b].append(src)
    return results


def init_blends(observations, centers, min_snr=50, bulge_grow=5, disk_grow=5, use_psf=True,
                bulge_slice=slice(None, 2), disk_slice=slice(2, -1), scales=5, wavelets=None,
                device=None, _working_set_bytes=None):
    """``init_all_sources_wavelets`` for many blends: ``sources[i]`` is what
    ``init_all_sources_wavelets(observations[i], centers[i], ..., wavelets=wavelets[i])``
    returns -- boxes, morphologies, the spectra of PSF and single-component sources bit for
    bit; the spectra of two-component sources from float64 normal equations instead of a
    float32 FFT convolution and ``lstsq`` -- with a fixed number of launches of
    csrc/lite_init.hip per group of blends that share dtypes and bands; frames, stamps and
    source counts may differ.

    ``centers``: one list of integer ``(y, x)`` per observation; a centre outside its frame
    raises ``ValueError``.  ``wavelets``: None, or per blend None, a host array
    ``(S, Ny, Nx)`` or the device tensor of ``get_detect_wavelets(..., device=True)``; neither
    is modified.  Blends the device path does not take (an even difference-kernel stamp,
    other dtypes, ``images.ndim != 3``, a frame or stamp beyond the kernels' limits) go
    through ``init_all_sources_wavelets``, with a host copy of their wavelets.  ``device``:
    GPU index of the batches (default 0).  Wrap every list of the result with
    ``parameterize_sources`` before fitting."""
    observations, centers = list(observations), [list(c) for c in centers]
    wavelets = [None] * len(observations) if wavelets is None else list(wavelets)
    budget, device = defaults(_working_set_bytes, device)
    groups, fallback = plan_init_blends(observations, centers, wavelets, bulge_slice, disk_slice,
                                        scales)
    opts = dict(min_snr=min_snr, bulge_grow=bulge_grow, disk_grow=disk_grow, use_psf=use_psf,
                bulge_slice=bulge_slice, disk_slice=disk_slice, scales=scales)
    sources = [None] * len(observations)
    for key, idx in groups.items():
        items = []
        for i in idx:
            if not centers[i]:
                sources[i] = []
                continue
            planes = _n_planes(observations[i], wavelets[i], scales)
            items.append((i, _init_bytes(observations[i], len(centers[i]), planes, key)))
        for chunk in chunks(items, budget):
            blends = [(observations[i], centers[i], wavelets[i]) for i in chunk]
            for i, result in zip(chunk, _run_init_chunk(blends, key, opts, device)):
                sources[i] = result
    for i, _ in fallback:
        wav = wavelets[i]
        if wav is not None:  # (the loop clips its argument in place)
            wav = wav.detach().cpu().numpy().copy() if _is_tensor(wav) else np.array(wav)
        sources[i] = init_all_sources_wavelets(observations[i], centers[i], min_snr, bulge_grow,
                                               disk_grow, use_psf, bulge_slice, disk_slice,
                                               scales, wav)
    return sources


# ---------------------------------------------------------------------------
# init_blends_main: init_all_sources_main (weighted sweep) for a catalogue, device batches
# ---------------------------------------------------------------------------
# lite_init_main.hip: one workgroup sweeps a source with its frame in LDS.  A CU has 160 KiB,
# all of which one workgroup may take; the kernel keeps 1 KiB of it for its reductions.
_LDS_BYTES = 160 * 1024
_LDS_RESERVE = 1024

_MAIN_COADD_DESC = np.dtype([("bands", _i4), ("reserved", _i4), ("n_pix", _i8),
                             ("image_off", _i8), ("nr2_off", _i8), ("detect_off", _i8)],
                            align=True)
_MAIN_SWEEP_DESC = np.dtype([("h", _i4), ("w", _i4), ("cy", _i4), ("cx", _i4),
                             ("plane_off", _i8), ("out_off", _i8), ("thresh", "f8")], align=True)
_MAIN_SPLIT_DESC = np.dtype([("bh", _i4), ("bw", _i4), ("morph_off", _i8), ("bulge_off", _i8),
                             ("disk_off", _i8)], align=True)


def _max_sweep_pixels(dtype):
    """Pixels of the largest frame the sweep kernel holds in LDS."""
    return (_LDS_BYTES - _LDS_RESERVE) // np.dtype(dtype).itemsize


_COSINES = {}


def _relative_cosines(ry, rx):
    """``cos(arctan2(-Y, -X) - arctan2(dy, dx))`` for every offset ``|Y| <= ry``, ``|X| <= rx``
    of a pixel from its centre and every neighbour ``(dy, dx)``, ``(2 ry + 1, 2 rx + 1, 8)``
    float64: the expression of ``getRadialMonotonicWeights``, evaluated by NumPy on contiguous
    arrays as there, so the bits are the same.  It depends on neither the centre nor the
    frame.  (The last table is kept: the chunks of a catalogue share their largest frame.)"""
    key = (int(ry), int(rx))
    if key not in _COSINES:
        Y = np.repeat(np.arange(-key[0], key[0] + 1), 2 * key[1] + 1)
        X = np.tile(np.arange(-key[1], key[1] + 1), 2 * key[0] + 1)
        to_peak = np.arctan2(-Y, -X)
        table = np.empty((Y.size, 8))
        for i, (dy, dx) in enumerate(NEIGHBOR_COORDS):
            table[:, i] = np.cos(to_peak - np.arctan2(float(dy), float(dx)))
        _COSINES.clear()
        _COSINES[key] = table.reshape(2 * key[0] + 1, 2 * key[1] + 1, 8)
    return _COSINES[key]


def _sweep_level(Y, X):
    """Level of the pixel at offset ``(Y, X)`` from the centre in the sweep of
    lite_init_main.hip: ``2 M + m - 1`` with ``M = max(|Y|, |X|)``, ``m = min(|Y|, |X|)``
    (-1 for the centre itself).  Every 8-neighbour strictly nearer the centre has a strictly
    smaller level: on the same ``M`` its ``m`` is one less, on ``M - 1`` its ``m`` is at most
    one more, and no pixel of ``M + 1`` is nearer."""
    Y, X = np.abs(Y), np.abs(X)
    return 2 * np.maximum(Y, X) + np.minimum(Y, X) - 1


def _main_key(obs, detect, use_mask, percentile):
    """``(key, reason)``: the group ``(image dtype, model PSF dtype, bands)`` of a blend the
    device batch of ``init_blends_main`` takes, or None and why it goes through
    ``init_all_sources_main``."""
    if use_mask:
        return None, "use_mask=True: the mask operators run on the GPU blend by blend"
    if not 0 < percentile < 100:
        return None, "percentile outside (0, 100)"
    shape = np.shape(obs.images)
    planes = (np.broadcast_to(np.zeros((), np.float64), (1,) + tuple(shape[1:]))
              if len(shape) == 3 else None)
    key, reason = _init_key(obs, planes, slice(None), slice(None), 0)
    if key is None:
        return None, reason
    _, idtype, mdtype, C = key
    h, w = shape[1:]
    if h * w > _max_sweep_pixels(idtype):
        return None, ("frame of {} pixels beyond the {} {} pixels of the sweep kernel's LDS image "
                      "({} KiB per CU less {} KiB)".format(
                          h * w, _max_sweep_pixels(idtype), idtype.name, _LDS_BYTES // 1024,
                          _LDS_RESERVE // 1024))
    if detect is None:
        noise_rms = np.asarray(obs.noise_rms)
        if (noise_rms.shape != (C,) or noise_rms.dtype.kind != "f"
                or np.result_type(idtype, (noise_rms ** 2).dtype) != idtype):
            return None, "noise_rms would make the coadd another dtype than the images"
    else:
        if not isinstance(detect, np.ndarray) or detect.shape != (h, w):
            return None, "detect is not a 2-D array of the frame's shape"
        if detect.dtype != idtype:
            return None, "detect differs from the images in dtype"
    return (idtype, mdtype, C), None


def plan_init_blends_main(observations, centers, detect=None, use_mask=False, percentile=25):
    """``(groups, fallback)`` of ``init_blends_main``, without touching the GPU: the positions
    of the blends of every device group, keyed by ``(image dtype, model PSF dtype, bands)`` in
    order of first appearance and in input order inside a group, and ``(position, reason)`` of
    the blends that go through ``init_all_sources_main``.  Raises ``ValueError`` for a centre
    outside its frame, or a catalogue whose arguments differ in length."""
    observations, centers = list(observations), list(centers)
    detect = [None] * len(observations) if detect is None else list(detect)
    if not len(observations) == len(centers) == len(detect):
        raise ValueError("observations, centers and detect must have one entry per blend, got "
                         "{}, {} and {}".format(len(observations), len(centers), len(detect)))
    groups, fallback = {}, []
    for i, (obs, cs, det) in enumerate(zip(observations, centers, detect)):
        shape = np.shape(obs.images)
        if len(shape) == 3:
            for c in cs:
                if not (len(c) == 2 and 0 <= c[0] < shape[1] and 0 <= c[1] < shape[2]):
                    raise ValueError("blend {}: centre {} lies outside its {} x {} frame".format(
                        i, tuple(c), shape[1], shape[2]))
        key, reason = _main_key(obs, det, use_mask, percentile)
        if key is None:
            fallback.append((i, reason))
        else:
            groups.setdefault(key, []).append(i)
    return groups, fallback


def _main_bytes(obs, n_sources, key):
    """Bytes of the device working set of one blend of ``init_blends_main``: detection image,
    images and variance; per source the swept plane and up to three cut-outs, counted as a
    frame each; the stamps in the data type, the model PSF's type and float64; and the table
    of relative cosines its frame needs, 64 bytes for each of ``(2 h - 1) (2 w - 1)`` offsets
    (a chunk holds one table, that of its largest frame: this counts it per blend)."""
    idtype, mdtype, C = key
    h, w = obs.images.shape[1:]
    n = h * w
    stamp = C * int(np.prod(np.shape(obs.diff_kernel.image)[1:]))
    return ((1 + 2 * C + 4 * n_sources) * n * idtype.itemsize
            + stamp * (idtype.itemsize + mdtype.itemsize + 8) + 64 * (2 * h - 1) * (2 * w - 1))


def _trim_box(bounds, center):
    """The box ``trim_morphology`` cuts around ``center`` for a morphology whose pixels
    ``> 0`` have the inclusive ``bounds`` (min row, max row, min col, max col; max < min:
    none)."""
    b0, b1, l0, l1 = (int(v) for v in bounds)
    bbox = Box.from_bounds((b0, b1 + 1), (l0, l1 + 1)) if b1 >= b0 else Box.from_bounds((0, 0), (0, 0))
    if bbox.contains(center):
        size = 2 * max(center[0] - bbox.start[-2], bbox.stop[0] - center[-2],
                       center[1] - bbox.start[-1], bbox.stop[1] - center[-1])
    else:
        size = 0
    half = get_minimal_boxsize(size) // 2
    return Box.from_bounds((center[0] - half, center[0] + half + 1),
                           (center[1] - half, center[1] + half + 1))


def _run_main_chunk(blends, key, opts, device):
    """``init_all_sources_main`` of the blends of one chunk: ``blends`` is a list of
    ``(observation, centers, detect)``; returns the list of their source lists."""
    ch = Launcher(device)
    with ch.torch.cuda.device(ch.dev):
        state = _main_launches(ch, key, blends, opts)
    return _main_assemble(blends, state)


def _main_launches(ch, key, blends, opts):
    """Everything of a chunk that touches the device: packs and uploads the inputs, runs the
    (at most) eight launches -- main_coadd, snr, taps twice, main_sweep, then after the host
    has decided class and box of every source crop, main_split and fit -- and returns what the
    assembly needs, all of it in host memory."""
    from types import SimpleNamespace

    idtype, mdtype, C = key
    call = partial(_call, ch, C)
    nb = len(blends)
    shapes = [b[0].images.shape[1:] for b in blends]
    n_pix = np.array([h * w for h, w in shapes], np.int64)
    image_off, n_image = offsets(C * n_pix)
    detect_off, n_detect = offsets(n_pix)
    d_images = ch.cat([b[0].images for b in blends], idtype)
    d_variance = ch.cat([b[0].variance for b in blends], idtype)
    # ---- the detection images: the passed ones, the coadds of the others
    host_detect = np.zeros(n_detect, idtype)
    missing = [b for b in range(nb) if blends[b][2] is None]
    for b in range(nb):
        if blends[b][2] is not None:
            host_detect[detect_off[b]:detect_off[b] + n_pix[b]] = blends[b][2].reshape(-1)
    d_detect = ch.up(host_detect) if len(missing) < nb else ch.empty(n_detect, idtype)
    coadds = np.zeros(len(missing), _MAIN_COADD_DESC)
    for k, b in enumerate(missing):
        coadds[k] = (C, 0, n_pix[b], image_off[b], k * C, detect_off[b])
    d_nr2 = ch.cat([np.asarray(blends[b][0].noise_rms) ** 2 for b in missing], idtype)
    call("main_coadd", idtype, coadds, d_images, n_image, d_nr2, len(missing) * C, d_detect,
         n_detect)
    # ---- per source: SNR sums, centre taps of the convolved detection image; per blend: the
    # spectrum of the model PSF
    psf_off, n_psf = offsets([b[0].psfs.size for b in blends])
    d_psfs = ch.cat([b[0].psfs for b in blends], idtype)
    stamps = [np.broadcast_to(np.asarray(b[0].diff_kernel.image),
                              (C,) + np.shape(b[0].diff_kernel.image)[1:]) for b in blends]
    stamp_off, n_stamp = offsets([s.size for s in stamps])
    d_stamps_i = ch.cat(stamps, idtype)
    d_stamps_m = d_stamps_i if mdtype == idtype else ch.cat(stamps, mdtype)
    model_psfs = [np.asarray(b[0].model_psf)[0] for b in blends]
    mpsf_off, n_mpsf = offsets([m.size for m in model_psfs])
    d_model_psfs = ch.cat(model_psfs, mdtype)

    src_blend = np.array([b for b in range(nb) for _ in blends[b][1]], np.int64)
    src_center = [c for b in blends for c in b[1]]
    ns = len(src_center)
    swept_off, n_swept = offsets(n_pix[src_blend])
    thresh = [float(np.mean(b[0].noise_rms) * opts["thresh"]) for b in blends]
    snr_t, taps_t = np.zeros(ns, _SNR_DESC), np.zeros(ns, _TAPS_DESC)
    sweep_t = np.zeros(ns, _MAIN_SWEEP_DESC)
    ptaps_t = np.zeros(nb, _TAPS_DESC)
    for s in range(ns):
        b = src_blend[s]
        h, w = shapes[b]
        cy, cx = int(src_center[s][0]), int(src_center[s][1])
        _, ph, pw = blends[b][0].psfs.shape
        _, kh, kw = stamps[b].shape
        snr_t[s] = (h, w, cy, cx, ph, pw, image_off[b], psf_off[b])
        taps_t[s] = (h, w, cy, cx, kh, kw, detect_off[b], stamp_off[b], s * (C + 1))
        sweep_t[s] = (h, w, cy, cx, detect_off[b], swept_off[s], thresh[b])
    for b in range(nb):
        mh, mw = model_psfs[b].shape
        _, kh, kw = stamps[b].shape
        ptaps_t[b] = (mh, mw, mh // 2, mw // 2, kh, kw, mpsf_off[b], stamp_off[b], b * (C + 1))
    d_snr = ch.empty(2 * ns, np.float64)
    d_taps = ch.empty(ns * (C + 1), idtype)
    d_ptaps = ch.empty(nb * (C + 1), mdtype)
    call("snr", idtype, snr_t, d_images, d_variance, n_image, d_psfs, n_psf, d_snr, 2 * ns)
    call("taps", idtype, taps_t, d_detect, n_detect, d_stamps_i, n_stamp, d_taps, ns * (C + 1))
    call("taps", mdtype, ptaps_t, d_model_psfs, n_mpsf, d_stamps_m, n_stamp, d_ptaps,
         nb * (C + 1))
    # ---- symmetry, sweep and trim of every source
    ry, rx = max(h for h, _ in shapes) - 1, max(w for _, w in shapes) - 1
    cosines = _relative_cosines(ry, rx)
    d_cos = ch.up(cosines.reshape(-1))
    d_swept = ch.empty(n_swept, idtype)
    d_bounds, d_peaks = ch.empty(4 * ns, np.int32), ch.empty(ns, idtype)
    call("main_sweep", idtype, sweep_t, d_detect, n_detect, d_cos, cosines.size, ry, rx, d_swept,
         n_swept, d_bounds, d_peaks, ns)
    snr = d_snr.cpu().numpy()[:2 * ns].reshape(ns, 2)
    taps = d_taps.cpu().numpy()[:ns * (C + 1)].reshape(ns, C + 1)
    ptaps = d_ptaps.cpu().numpy()[:nb * (C + 1)].reshape(nb, C + 1)
    bounds = d_bounds.cpu().numpy()[:4 * ns].reshape(ns, 4)
    peaks = d_peaks.cpu().numpy()[:ns]
    # ---- the class and the box of every source, as init_all_sources_main decides them.  (A
    # swept plane is nowhere above its centre pixel, so what is left of it after the trim holds
    # the centre, the box holds all of it, and the maximum of the box is that of the plane.)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_comp = np.floor(snr[:, 0] / np.sqrt(snr[:, 1])) / opts["min_snr"]
    kind = np.where(n_comp >= 2, _TWO, _ONE)
    kind[peaks == 0] = _PSF
    boxes = {s: _trim_box(bounds[s], src_center[s]) for s in range(ns) if kind[s] != _PSF}
    # ---- cut-outs divided by their maximum; bulge and disk of the two-component sources
    sizes = [boxes[s].shape[0] * boxes[s].shape[1] * (3 if kind[s] == _TWO else 1)
             for s in boxes]
    out_off, n_out = offsets(sizes)
    offs = dict(zip(boxes, (int(o) for o in out_off)))
    crop_t = np.zeros(len(boxes), _CROP_DESC)
    for k, (s, box) in enumerate(boxes.items()):
        h, w = shapes[src_blend[s]]
        crop_t[k] = (h, w, box.origin[0], box.origin[1], box.shape[0], box.shape[1],
                     swept_off[s], 0, offs[s])
    d_out = ch.empty(n_out, idtype)
    d_all = ch.torch.ones(int(n_pix.max()), dtype=ch.torch.uint8, device=ch.dev)
    call("crop", idtype, crop_t, d_swept, n_swept, d_all, int(n_pix.max()), d_out, n_out)
    pairs = [s for s in boxes if kind[s] == _TWO]
    split_t, fit_t = np.zeros(len(pairs), _MAIN_SPLIT_DESC), np.zeros(len(pairs), _FIT_DESC)
    for k, s in enumerate(pairs):
        b = src_blend[s]
        h, w = shapes[b]
        _, kh, kw = stamps[b].shape
        box = boxes[s]
        (y0, x0), (bh, bw) = box.origin, box.shape
        split_t[k] = (bh, bw, offs[s], offs[s] + bh * bw, offs[s] + 2 * bh * bw)
        fit_t[k] = (h, w, y0, x0, bh, bw, y0, x0, bh, bw, y0, x0, bh, bw, kh, kw,
                    image_off[b], stamp_off[b], offs[s] + bh * bw, offs[s] + 2 * bh * bw)
    call("main_split", idtype, split_t, d_out, n_out, float(opts["percentile"] / 100))
    d_sums = ch.empty(len(pairs) * C * 5, np.float64)
    if len(pairs):
        d_stamps_fit = ch.cat(stamps, np.float64)
        call("fit", idtype, fit_t, d_out, n_out, d_images, int(idtype == np.float64), n_image,
             d_stamps_fit, n_stamp, d_sums, len(pairs) * C * 5)
    morphs = d_out.cpu().numpy()
    sums = d_sums.cpu().numpy()[:len(pairs) * C * 5].reshape(len(pairs), C, 5)
    return SimpleNamespace(C=C, idtype=idtype, src_blend=src_blend, src_center=src_center,
                           kind=kind, taps=taps, ptaps=ptaps, peaks=peaks, boxes=boxes, offs=offs,
                           morphs=morphs, pairs=pairs, sums=sums)


def _main_assemble(blends, st):
    """The sources of a chunk from what ``_main_launches`` brought back, source by source as
    ``init_all_sources_main`` builds them."""
    C = st.C
    pair_seds = dict(zip(st.pairs, _solve_pairs(st.sums, st.idtype)))
    results = [[] for _ in blends]
    for s, center in enumerate(st.src_center):
        b = st.src_blend[s]
        obs = blends[b][0]
        spec_box = obs.bbox[0]
        at_center = (slice(None), center[0], center[1])
        kind = st.kind[s]
        if kind == _PSF:
            model_psf = obs.model_psf[0]
            py, px = model_psf.shape[0] // 2, model_psf.shape[1] // 2
            sed = obs.images[at_center] / st.ptaps[b, :C]
            sed[sed < 0] = 0
            bbox = Box(model_psf.shape, origin=(center[0] - py, center[1] - px))
            comps = [LiteComponent(center, spec_box @ bbox, sed, model_psf / np.max(model_psf))]
        else:
            bbox, at = st.boxes[s], st.offs[s]
            n = bbox.shape[0] * bbox.shape[1]
            cut = [st.morphs[at + k * n:at + (k + 1) * n].reshape(bbox.shape).copy()
                   for k in range(3 if kind == _TWO else 1)]
            if kind == _TWO:
                bulge_sed, disk_sed = pair_seds[s]
                comps = [LiteComponent(center, spec_box @ bbox, bulge_sed, cut[1]),
                         LiteComponent(center, spec_box @ bbox, disk_sed, cut[2])]
            else:
                sed = obs.images[at_center] / st.taps[s, :C]
                sed[sed < 0] = 0
                comps = [LiteComponent(center, spec_box @ bbox, sed * st.peaks[s], cut[0])]
        results[b].append(LiteSource(comps, obs.dtype))
    return results


def init_blends_main(observations, centers, detect=None, min_snr=50, use_mask=False,
                     percentile=25, thresh=0.5, device=None, _working_set_bytes=None):
    """``init_all_sources_main`` for many blends: ``sources[i]`` is what
    ``init_all_sources_main(observations[i], centers[i], detect=detect[i], min_snr=min_snr,
    percentile=percentile, thresh=thresh)`` returns -- number and class of the sources, centres,
    boxes, morphologies, dtypes and the spectra of PSF and single-component sources bit for bit;
    the spectra of bulge + disk sources from float64 normal equations instead of a float32 FFT
    convolution and ``lstsq`` -- with at most eight launches of csrc/lite_init_main.hip and
    csrc/lite_init.hip per chunk of blends that share dtypes and bands; frames, stamps and
    source counts may differ.  The contract is for finite data (images, variance, PSFs and
    detection images without NaN or infinity).

    ``centers``: one list of integer ``(y, x)`` per observation; a centre outside its frame
    raises ``ValueError``.  ``detect``: None, or per blend None (the coadd
    ``sum(images / noise_rms**2)``) or a 2-D array of the frame's shape, which is only read.
    Blends the device path does not take -- ``use_mask=True``, a ``percentile`` outside
    (0, 100), a ``detect`` or ``noise_rms`` of another dtype than the images, everything
    ``init_blends`` refuses, a frame beyond the sweep kernel's LDS image (40704 float32 or
    20352 float64 pixels) -- go through ``init_all_sources_main``; ``plan_init_blends_main``
    names them.  ``device``: GPU index of the batches (default 0).  Wrap every list of the
    result with ``parameterize_sources`` before fitting."""
    observations, centers = list(observations), [list(c) for c in centers]
    detect = [None] * len(observations) if detect is None else list(detect)
    budget, device = defaults(_working_set_bytes, device)
    groups, fallback = plan_init_blends_main(observations, centers, detect, use_mask, percentile)
    opts = dict(min_snr=min_snr, percentile=percentile, thresh=thresh)
    sources = [None] * len(observations)
    for key, idx in groups.items():
        items = []
        for i in idx:
            if not centers[i]:
                sources[i] = []
                continue
            items.append((i, _main_bytes(observations[i], len(centers[i]), key)))
        for chunk in chunks(items, budget):
            blends = [(observations[i], centers[i], detect[i]) for i in chunk]
            for i, result in zip(chunk, _run_main_chunk(blends, key, opts, device)):
                sources[i] = result
    for i, _ in fallback:
        sources[i] = init_all_sources_main(observations[i], centers[i], detect[i], min_snr,
                                           use_mask, percentile, thresh)
    return sources
