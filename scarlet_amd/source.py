"""Extended-source models (reference scarlet/source.py:249-522, 615-807):
``ExtendedSource`` factory -> ``SingleExtendedSource`` / ``MultiExtendedSource`` /
``CompactExtendedSource``, ``PointSource`` (source.py:92-128), ``RandomSource``
(source.py:61-89), ``StarletSource`` (source.py:525-612), ``GaussianSource`` and
``SpergelSource`` (source.py:131-246)."""

import logging
from functools import partial

import numpy as np

from . import initialization as init
from . import operator
from .bbox import Box, overlapped_slices
from .component import CombinedComponent, Component, FactorizedComponent
from .constraint import CenterOnConstraint, PositivityConstraint
from .morphology import (ExtendedSourceMorphology, GaussianMorphology, ImageMorphology,
                         PointSourceMorphology, SpergelMorphology, StarletMorphology)
from .parameter import Parameter, relative_step
from .spectrum import TabulatedSpectrum

logger = logging.getLogger("scarlet_amd.source")


def _as_sequence(observations):
    return observations if hasattr(observations, "__iter__") else (observations,)


def _noise_rms(observations):
    """Mean noise rms per channel, channels of all observations in a row."""
    per_obs = [np.array(np.mean(obs.noise_rms, axis=(1, 2))) for obs in observations]
    return np.concatenate(per_obs).reshape(-1)


def _nearest_pixel(frame, sky_coord):
    return np.round(frame.get_pixel(sky_coord)).astype("int")


def _box_around(pixel, shape):
    """2-D box of ``shape`` whose middle pixel (shape // 2) is ``pixel``."""
    return Box(shape, origin=tuple(int(p) - n // 2 for p, n in zip(pixel, shape)))


def _fitted_morphology(frame, sky_coord, image, bbox, shifting, resizing):
    """The morphology every extended source is FITTED with, however it was initialised:
    monotonic with 'angle' weights and no minimal gradient, not symmetric
    (source.py:289-300, 480-496, 632-643)."""
    return ExtendedSourceMorphology(
        frame, frame.get_pixel(sky_coord), image, bbox=bbox, monotonic="angle",
        symmetric=False, min_grad=0, shifting=shifting, resizing=resizing)


class NullSource(Component):
    """A source without components (source.py:24-58): its model is zero over the whole frame.
    It keeps a place in a list of sources; it has no parameters and is not fitted."""

    def __init__(self, model_frame):
        super().__init__(model_frame)

    def get_model(self, *parameters, frame=None):
        return self._in_frame(np.zeros(self.frame.shape), frame)


class RandomSource(FactorizedComponent):
    """A source without a shape of its own: uniform random numbers over the whole model
    frame as image, then as spectrum (drawn from ``np.random`` in that order).  The spectrum
    moves in steps of a tenth of its mean and is kept non-negative."""

    def __init__(self, model_frame, observations=None):
        n_channels, height, width = model_frame.bbox.shape
        morphology = ImageMorphology(model_frame, np.random.rand(height, width))
        amplitudes = Parameter(np.random.rand(n_channels), name="spectrum",
                               step=partial(relative_step, factor=1e-1),
                               constraint=PositivityConstraint())
        super().__init__(model_frame, TabulatedSpectrum(model_frame, amplitudes), morphology)


class PointSource(FactorizedComponent):
    """Point source: the model PSF at a free centre times a spectrum taken from the
    peak pixel of the observations, corrected for the PSF (source.py:92-128)."""

    def __init__(self, model_frame, sky_coord, observations):
        observations = _as_sequence(observations)
        position = np.array(model_frame.get_pixel(sky_coord), dtype=float)
        morphology = PointSourceMorphology(
            model_frame, Parameter(position, name="center", step=3e-2))
        amplitudes = init.get_pixel_spectrum(sky_coord, observations, correct_psf=True)
        super().__init__(
            model_frame,
            TabulatedSpectrum(model_frame, amplitudes, min_step=_noise_rms(observations)),
            morphology)
        self.center = morphology.center


def _ellipticity_parameter(ellipticity):
    """The free "ellipticity" of a profile source.  Like the reference, only an ndarray is
    taken; ``None`` and a tuple -- a ``TypeError`` and an ``AttributeError`` from deep inside
    the reference -- are named here."""
    if ellipticity is None:
        raise TypeError("ellipticity=None: pass the two components (e1, e2) as an ndarray, "
                        "np.zeros(2) for a round source")
    if not isinstance(ellipticity, np.ndarray):
        raise TypeError("ellipticity must be an ndarray of two floats, got {}".format(
            type(ellipticity).__name__))
    if ellipticity.shape != (2,):
        raise ValueError("ellipticity must have shape (2,), got {}".format(ellipticity.shape))
    return Parameter(ellipticity, name="ellipticity", step=0.01)


class _ProfileSource(FactorizedComponent):
    """What ``GaussianSource`` and ``SpergelSource`` share: the spectrum of the pixel under
    the centre, not corrected for the PSF, over the peak value of the (unnormalised) profile,
    with the noise level scaled alike as smallest step (source.py:166-185, 227-246)."""

    def _finish(self, model_frame, sky_coord, observations, morphology):
        peak = morphology.f(0)
        amplitudes = init.get_pixel_spectrum(sky_coord, observations, correct_psf=False)
        amplitudes /= peak
        noise = _noise_rms(observations)
        noise /= peak
        super().__init__(model_frame, TabulatedSpectrum(model_frame, amplitudes, min_step=noise),
                         morphology)
        self.center = morphology.center


class GaussianSource(_ProfileSource):
    """An elliptical Gaussian of standard deviation ``sigma`` pixels at ``sky_coord``; centre
    (step 0.01), sigma (a tenth of itself) and ``ellipticity`` (an ndarray (e1, e2), step
    0.01) are fitted in float64."""

    def __init__(self, model_frame, sky_coord, sigma, ellipticity, observations):
        observations = _as_sequence(observations)
        center = Parameter(np.array(model_frame.get_pixel(sky_coord), dtype=float),
                           name="center", step=0.01)
        radius = Parameter(np.array((sigma,), dtype=float), name="radius", step=relative_step)
        morphology = GaussianMorphology(model_frame, center, radius,
                                        ellipticity=_ellipticity_parameter(ellipticity))
        self._finish(model_frame, sky_coord, observations, morphology)


class SpergelSource(_ProfileSource):
    """A Spergel (2010) profile of index ``nu`` and half-light radius ``rhalf`` pixels at
    ``sky_coord``; centre, nu and ``ellipticity`` move in steps of 0.01, the radius in steps
    of a hundredth of itself."""

    def __init__(self, model_frame, sky_coord, nu, rhalf, ellipticity, observations):
        observations = _as_sequence(observations)
        center = Parameter(np.array(model_frame.get_pixel(sky_coord), dtype=float),
                           name="center", step=0.01)
        nu = Parameter(np.array((nu,), dtype=float), name="nu", step=0.01)
        radius = Parameter(np.array((rhalf,), dtype=float), name="radius",
                           step=partial(relative_step, factor=0.01))
        morphology = SpergelMorphology(model_frame, center, nu, radius,
                                       ellipticity=_ellipticity_parameter(ellipticity))
        self._finish(model_frame, sky_coord, observations, morphology)


class CompactExtendedSource(FactorizedComponent):
    """Source initialised with the model PSF as morphology."""

    def __init__(self, model_frame, sky_coord, observations, shifting=False, resizing=True,
                 boxsize=None):
        assert model_frame.psf is not None
        observations = _as_sequence(observations)
        image, bbox = self.init_morph(model_frame, sky_coord, boxsize=boxsize)
        morphology = _fitted_morphology(model_frame, sky_coord, image, bbox, shifting, resizing)
        # the PSF-corrected peak amplitude belongs to a unit-sum profile; the
        # morphology is peak-normalised instead
        amplitudes = init.get_pixel_spectrum(sky_coord, observations, correct_psf=True)
        amplitudes /= image.sum()
        super().__init__(
            model_frame,
            TabulatedSpectrum(model_frame, amplitudes, min_step=_noise_rms(observations)),
            morphology)
        self.center = morphology.center

    @staticmethod
    def init_morph(frame, sky_coord, boxsize=None):
        """Band-averaged model PSF, peak-normalised, in a standard-size box."""
        pixel = _nearest_pixel(frame, sky_coord)
        psf = frame.psf.get_model().mean(axis=0)
        side = init.get_minimal_boxsize(max(psf.shape)) if boxsize is None else boxsize
        bbox = _box_around(pixel, (side, side))
        into, out_of = overlapped_slices(bbox, _box_around(pixel, psf.shape))
        image = np.zeros(bbox.shape)
        image[into] = psf[out_of]
        image /= image.max()
        return image, bbox


class SingleExtendedSource(FactorizedComponent):
    """One spectrum x one monotonic morphology, initialised from the
    signal-to-noise weighted coadd of the observations."""

    def __init__(self, model_frame, sky_coord, observations, thresh=1.0, shifting=False,
                 resizing=True, boxsize=None):
        observations = _as_sequence(observations)
        # (init_all_sources sweeps the detection images of all its sources in one launch)
        ready = init.prepared_detection(sky_coord, observations)
        if ready is not None:
            per_obs, coadd, coadd_rms, symmetrised, swept, good_for = ready
            if good_for is not None and not thresh >= good_for:
                swept = None  # (swept in a window that a lower threshold may look beyond)
        else:
            per_obs = init.get_pixel_spectrum(sky_coord, observations, concat=False)
            coadd, coadd_rms = init.build_initialization_image(observations, spectra=per_obs)
            symmetrised = swept = None
        spectrum = TabulatedSpectrum(model_frame, np.concatenate(per_obs).reshape(-1),
                                     min_step=_noise_rms(observations))
        image, bbox = self.init_morph(model_frame, sky_coord, coadd, coadd_rms, thresh=thresh,
                                      symmetric=True, monotonic="flat", min_grad=0,
                                      boxsize=boxsize, _swept=swept)
        morphology = _fitted_morphology(model_frame, sky_coord, image, bbox, shifting, resizing)
        super().__init__(model_frame, spectrum, morphology)
        self.center = morphology.center

    @staticmethod
    def init_morph(frame, sky_coord, detect, detect_std, thresh=1, symmetric=True,
                   monotonic="flat", min_grad=0, boxsize=None, _swept=None):
        """Cut-out of the detection image around the source: symmetrised and made
        monotonic about the nearest pixel, trimmed at ``thresh * detect_std``,
        peak-normalised and never narrower than the model PSF.  ``_swept``: the symmetrised,
        monotonic profile when ``init_all_sources`` has prepared it (symmetric, 'flat'
        weights, no minimal gradient)."""
        pixel = _nearest_pixel(frame, sky_coord)
        if _swept is not None and symmetric and monotonic == "flat" and min_grad == 0:
            profile = _swept.copy()
        else:
            profile = detect.copy()
            if symmetric:
                profile = operator.prox_uncentered_symmetry(profile, 0, center=pixel,
                                                            algorithm="sdss")
            if monotonic:
                weights = "angle" if monotonic is True else monotonic
                windowed = None
                if weights == "flat" and min_grad == 0:
                    # (a window about the pixel where its rim proves the rest lies below the
                    # trimming threshold: initialization.prepare_detection_sweeps)
                    windowed = init.sweep_in_window(profile, pixel, thresh, detect_std)
                if windowed is not None:
                    profile = windowed
                else:
                    sweep = operator.prox_weighted_monotonic(profile.shape, neighbor_weight=weights,
                                                             center=pixel, min_gradient=min_grad)
                    profile = sweep(np.ascontiguousarray(profile), 0).reshape(profile.shape)
        image, bbox = init.trim_morphology(pixel, profile, bg_thresh=detect_std * thresh,
                                           boxsize=boxsize)
        if image.sum() > 0:
            image /= image.max()
        else:
            # nothing above the threshold: a single lit pixel at the centre
            logger.warning(f"No flux in morphology model for source at {sky_coord}")
            image = CenterOnConstraint(tiny=1)(image, 0)
        if frame.psf is not None:
            # noisy initialisations leave a few pixels only: never narrower than the PSF
            floor, _ = CompactExtendedSource.init_morph(frame, sky_coord, boxsize=max(bbox.shape))
            image = np.maximum(image, floor)
        return image, bbox


class StarletSource(FactorizedComponent):
    """A source whose morphology is a stack of starlet coefficients (``StarletMorphology``).

    With ``sky_coord`` it starts from the ``ExtendedSource`` at that position, without one
    from a ``RandomSource`` over the whole frame: diffuse light that is neither monotonic nor
    symmetric.  ``spectrum`` replaces the initial spectrum (a ``Parameter`` named "spectrum",
    or an array, which then takes the noise of ``observations`` as its minimal step).
    ``starlet_thresh`` is the hard threshold of all but the coarsest plane in units of the
    norm of every scale's wavelet; ``monotonic`` asks for monotonic planes instead."""

    def __init__(self, model_frame, sky_coord=None, observations=None, spectrum=None, thresh=1.0,
                 monotonic=False, starlet_thresh=5e-3, boxsize=None):
        if sky_coord is None:
            seed = RandomSource(model_frame)
        else:
            seed = ExtendedSource(model_frame, sky_coord, observations, thresh=thresh,
                                  boxsize=boxsize)
        converted = StarletSource.from_source(seed, monotonic=monotonic,
                                              starlet_thresh=starlet_thresh)
        own_spectrum, morphology = converted.children
        if spectrum is not None:
            if isinstance(spectrum, Parameter):
                assert spectrum.name == "spectrum"
                own_spectrum = spectrum
            else:
                own_spectrum = TabulatedSpectrum(
                    model_frame, spectrum, min_step=_noise_rms(_as_sequence(observations)))
        super().__init__(converted.frame, own_spectrum, morphology)

    @classmethod
    def from_source(cls, source, monotonic=False, starlet_thresh=5e-3):
        """The factorized ``source`` with its morphology turned into starlet coefficients
        of the image it models now; the spectrum object is shared."""
        assert isinstance(source, FactorizedComponent)
        spectrum, morphology = source.children
        starlets = StarletMorphology(source.frame, morphology.get_model(), bbox=morphology.bbox,
                                     monotonic=monotonic, threshold=starlet_thresh)
        made = cls.__new__(cls)
        FactorizedComponent.__init__(made, source.frame, spectrum, starlets)
        return made


class MultiExtendedSource(CombinedComponent):
    """K components stacked vertically: the single-source morphology is cut at
    flux percentiles into an outer plateau and inner remainders."""

    def __init__(self, model_frame, sky_coord, observations, K=2, flux_percentiles=None,
                 thresh=1.0, shifting=False, resizing=True, boxsize=None):
        flux_percentiles = (25,) if flux_percentiles is None else flux_percentiles
        assert K == len(flux_percentiles) + 1
        observations = _as_sequence(observations)
        single = ExtendedSource(model_frame, sky_coord, observations, thresh=thresh,
                                boxsize=boxsize)
        single_spectrum, single_morphology = single.children
        amplitudes = single_spectrum.get_parameter(0)._data
        layers, boxes = self.init_morphs(single_morphology, flux_percentiles)
        # every layer starts from the full spectrum, with ten times finer steps
        min_step = _noise_rms(observations) / 10
        components = []
        for layer, bbox in zip(layers, boxes):
            morphology = _fitted_morphology(model_frame, sky_coord, layer, bbox, shifting,
                                            resizing)
            components.append(FactorizedComponent(
                model_frame,
                TabulatedSpectrum(model_frame, amplitudes.copy(), min_step=min_step),
                morphology))
            self.center = morphology.center
        super().__init__(components)

    @staticmethod
    def init_morphs(morphology, flux_percentiles):
        morph = morphology.get_model()
        K = len(flux_percentiles) + 1
        layers = np.zeros((K,) + morph.shape, dtype=morph.dtype)
        layers[0] = morph
        peak = morph.max()
        below = 0
        for k, perc in enumerate(np.sort(flux_percentiles), start=1):
            cut = perc * peak / 100
            inside = morph > cut
            layers[k - 1][inside] = cut - below
            layers[k][inside] = morph[inside] - cut
            below = cut
        for k in range(K):
            if np.all(layers[k] <= 0):
                logger.warning(f"Zero or negative morphology for component {k}")
            layers[k] /= layers[k].max()
        return layers, tuple(morphology.bbox.copy() for _ in range(K))


def ExtendedSource(model_frame, sky_coord, observations, K=1, flux_percentiles=None, thresh=1.0,
                   compact=False, shifting=False, resizing=True, boxsize=None):
    """Factory: ``CompactExtendedSource`` if ``compact``, ``SingleExtendedSource`` for
    ``K == 1``, else ``MultiExtendedSource`` with ``K`` components."""
    if compact:
        return CompactExtendedSource(model_frame, sky_coord, observations, shifting=shifting,
                                     resizing=resizing, boxsize=boxsize)
    if K == 1:
        return SingleExtendedSource(model_frame, sky_coord, observations, thresh=thresh,
                                    shifting=shifting, resizing=resizing, boxsize=boxsize)
    return MultiExtendedSource(model_frame, sky_coord, observations, K=K,
                               flux_percentiles=flux_percentiles, thresh=thresh,
                               shifting=shifting, resizing=resizing, boxsize=boxsize)
