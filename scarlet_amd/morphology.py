"""Image, starlet and profile (Gaussian, Spergel) morphologies of factorized components
(reference scarlet/morphology.py:26-688)."""

import numpy as np
import numpy.ma as ma

from .bbox import Box, overlapped_slices
from .constraint import (
    CenterOnConstraint,
    Constraint,
    ConstraintChain,
    L0Constraint,
    MonotonicMaskConstraint,
    MonotonicityConstraint,
    NormalizationConstraint,
    PositivityConstraint,
    SymmetryConstraint,
)
from .frame import Frame
from .model import Model, UpdateException
from .parameter import prepare_param, Parameter, relative_step


def get_minimal_boxsize(size, min_size=21, increment=10):
    """Smallest odd box size ``min_size + k * increment`` that holds ``size``
    pixels (reference initialization.py:173-177); ``size`` is a number or an array."""
    steps = np.ceil(np.maximum(np.asarray(size) - min_size, 0) / increment).astype(np.int64)
    boxsize = min_size + increment * steps
    return boxsize if boxsize.ndim else int(boxsize)


def _margin_of_empty(short_side):
    """``_empty_margin`` of an image (or an array of images) that holds no pixel above the
    threshold, from the shorter side of its box: all of it is margin."""
    return (short_side + 1) // 2


def _empty_margin(image, thresh):
    """Width of the frame of pixels <= ``thresh`` around ``image``: the largest ``d`` such
    that the d outermost rows and columns on every side hold nothing above ``thresh``
    (the whole image counts as margin when it is empty)."""
    mask = np.asarray(image) > thresh
    rows = mask.any(axis=1)
    if not rows.any():
        return _margin_of_empty(min(image.shape))
    cols = mask.any(axis=0)
    # first and last occupied row / column, counted from the nearer edge
    return int(min(rows.argmax(), cols.argmax(), rows[::-1].argmax(), cols[::-1].argmax()))


def _edge_pull(image, m, v, step):
    """Mean pull of the next Adam step over each of the four edges of the box
    (morphology.py:166-176): ``-m / sqrt(sqrt(v)) * step * (image > 0)`` averaged over the
    edge pixels with ``v != 0``.  The reference evaluates the whole image as a masked array
    and takes the means of four slices; this is the same arithmetic on the four edges only --
    the masked mean is the sum of the zero-filled slice over the count of unmasked entries --
    bit for bit (tests/test_host_logic.py), at a tenth of the cost.  An edge without an
    unmasked pixel gives nan, as the masked constant does when it is put into an array."""
    out = np.empty(4)
    for e, sl in enumerate(((slice(None), 0), (slice(None), -1), (0, slice(None)), (-1, slice(None)))):
        vv = v[sl]
        seen = vv != 0
        count = int(seen.sum())
        if count == 0:
            out[e] = np.nan
            continue
        gu = -m[sl] / np.sqrt(np.sqrt(np.where(seen, vv, 1.0))) * step
        pull = gu * (image[sl] > 0)
        out[e] = np.where(seen, pull, 0.0).sum() * 1.0 / count
    return out


class Morphology(Model):
    """Spatial part of a factorized component inside ``bbox`` (default: the box of
    ``frame``)."""

    def __init__(self, frame, *parameters, bbox=None):
        assert isinstance(frame, Frame)
        assert bbox is None or isinstance(bbox, Box)
        self.frame = frame
        self.bbox = frame.bbox if bbox is None else bbox
        super().__init__(*parameters)

    def shrink_box(self, image, thresh=0):
        """Peel off empty borders; adopt the next smaller standard box size
        (morphology.py:50-67)."""
        size = max(image.shape)
        newsize = get_minimal_boxsize(size - 2 * _empty_margin(image, thresh))
        if newsize < size:
            inset = (size - newsize) // 2
            self.bbox.origin = tuple(o + inset for o in self.bbox.origin)
            self.bbox.shape = (newsize, newsize)


class ImageMorphology(Morphology):
    """Free-form image morphology inside ``bbox``."""

    def __init__(self, frame, image, bbox=None, shifting=False, shift=None, resizing=True):
        if isinstance(image, Parameter):
            assert image.name == "image"
        else:
            image = Parameter(image, name="image", step=relative_step,
                              constraint=PositivityConstraint())
        # without a box the image must cover the frame's spatial extent
        assert image.shape == (frame.bbox[1:].shape if bbox is None else bbox.shape)
        bbox = Box(image.shape) if bbox is None else bbox
        self.resizing = resizing
        self.shifting = shifting
        if shift is None:
            # kept for parameter-order compatibility with the reference, which creates
            # this unused 2-vector for every image morphology (morphology.py:113)
            shift = Parameter(np.zeros(2), name="shift", step=1e-2, fixed=self.shifting)
        else:
            assert shift.shape == (2,)
            if not isinstance(shift, Parameter):
                shift = Parameter(shift, name="shift", step=1e-2)
        super().__init__(frame, image, shift, bbox=bbox)

    def get_model(self, *parameters):
        image = self.get_parameter(0, *parameters)
        if self.shifting:
            # Fourier sub-pixel shift (morphology.py:124-130).  The reference creates
            # the shift with ``fixed=self.shifting`` (morphology.py:113), so with
            # shifting=True and no explicit ``shift`` it stays at zero and this is the
            # identity up to FFT round-off.
            from . import fft

            image = fft.shift(image, self.get_parameter(1, *parameters), return_Fourier=False)
        return image

    def update(self):
        """Every 10 iterations: shrink the box when all edges are empty, grow it
        when the next Adam step pulls flux over an edge; the optimizer state is
        sliced / padded along and the step halved (reference morphology.py:132-207)."""
        image = self._parameters[0]
        if not self.resizing or image.fixed:
            return
        bbox = self.bbox.copy()
        self.shrink_box(image)
        if bbox != self.bbox:
            # the new box sits `inset` pixels inside the old one on every side (shrink_box)
            inset = self.bbox.origin[-1] - bbox.origin[-1]
            sl = tuple(slice(inset, inset + n) for n in self.bbox.shape)

            def cut(a):
                return a[sl] if a is not None else None

            image = Parameter(image[sl], name=image.name, prior=image.prior,
                              constraint=image.constraint, step=image.step / 2,
                              fixed=image.fixed, m=cut(image.m), v=cut(image.v),
                              vhat=cut(image.vhat))
            self._parameters = (image,) + self._parameters[1:]
            raise UpdateException
        if image.m is not None:
            edge_pull = _edge_pull(np.asarray(image), image.m, image.v, image.step)
            if np.any(edge_pull > 0.1):
                size = max(bbox.shape)
                newsize = get_minimal_boxsize(size + 1)
                pad = (newsize - size) // 2

                def grow(a):
                    return np.pad(a, pad, mode="constant") if a is not None else None

                image = Parameter(np.pad(image, pad, mode="linear_ramp"), name=image.name,
                                  prior=image.prior, constraint=image.constraint,
                                  step=image.step / 2, fixed=image.fixed, m=grow(image.m),
                                  v=grow(image.v), vhat=grow(image.vhat))
                self._parameters = (image,) + self._parameters[1:]
                self.bbox.origin = tuple(o - pad for o in self.bbox.origin)
                self.bbox.shape = (newsize, newsize)
                raise UpdateException


class ExtendedSourceMorphology(ImageMorphology):
    """Image morphology for galaxies: monotonic from the centre (``monotonic`` in
    'flat' / 'angle' / 'nearest' or None), optionally symmetric, positive, centre
    pixel kept on, normalised to unit maximum; step 1e-2."""

    def __init__(self, frame, center, image, bbox=None, monotonic="angle", symmetric=False,
                 min_grad=0, shifting=False, resizing=True):
        # booleans are the old spelling of the monotonicity argument
        weighting = {True: "angle", False: None}.get(monotonic, monotonic) \
            if isinstance(monotonic, bool) else monotonic
        shape_terms = []
        if weighting is not None:
            shape_terms.append(MonotonicityConstraint(neighbor_weight=weighting,
                                                      min_gradient=min_grad))
        if symmetric:
            shape_terms.append(SymmetryConstraint())
        # the order of the fused device chain (constraint._DEVICE_ORDER)
        constraints = shape_terms + [PositivityConstraint(), CenterOnConstraint(),
                                     NormalizationConstraint("max")]
        image = Parameter(image, name="image", step=1e-2, constraint=ConstraintChain(*constraints))
        self.pixel_center = np.round(center).astype("int")
        # with shifting the sub-pixel offset of the centre becomes a free parameter
        # (morphology.py:673-676); Blend.fit refuses it: free Fourier shifts do not run
        # on the device yet
        self.shift = (Parameter(np.asarray(center, dtype=float) - self.pixel_center,
                                name="shift", step=1e-1) if shifting else None)
        super().__init__(frame, image, bbox=bbox, shifting=shifting, shift=self.shift,
                         resizing=resizing)

    @property
    def center(self):
        if self.shift is not None:
            return self.pixel_center + self.shift
        return self.pixel_center


class PointSourceMorphology(Morphology):
    """The model PSF (``frame.psf``) evaluated at a free sub-pixel ``center``
    (reference morphology.py:476-513).  The box is the PSF box moved to the rounded
    initial centre and never changes; the only parameter is the centre."""

    def __init__(self, frame, center):
        from .psf import PSF

        assert frame.psf is not None and isinstance(frame.psf, PSF)
        self.psf = frame.psf
        # the PSF box, centred on the origin, moves to the pixel nearest the centre
        cy, cx = (int(c) for c in np.rint(np.asarray(center, dtype=float)))
        self.center = prepare_param(center, name="center")
        super().__init__(frame, self.center, bbox=self.psf.bbox + (0, cy, cx))

    def get_model(self, *parameters):
        """Model-frame PSF image evaluated at the sub-pixel offset of the centre from
        the middle of the box."""
        (y_lo, y_hi), (x_lo, x_hi) = self.bbox.bounds[1:]
        middle = np.array([(y_lo + y_hi) / 2, (x_lo + x_hi) / 2])
        return self.psf.get_model(offset=np.asarray(self.get_parameter(0, *parameters)) - middle)

    @property
    def integral(self):
        return self.psf.get_model().sum()


def starlet_thresholds(norm, threshold):
    """Absolute hard threshold of every coefficient plane of a ``StarletMorphology``:
    ``threshold`` times the norm of that scale's wavelet, and no threshold on the last
    (coarse) plane (morphology.py:549-556).  ``norm``: ``Starlet.norm``, one entry per plane."""
    per_plane = np.zeros(len(norm)) + threshold
    per_plane *= np.asarray(norm, dtype=np.float64)
    per_plane[-1] = 0
    return per_plane


def shrink_slices(old_origin, old_shape, new_origin, new_shape):
    """Slices that cut the last two axes of an array over the box ``(old_origin, old_shape)``
    down to its overlap with the box ``(new_origin, new_shape)``: what a shrink applies to
    coefficients and moments (morphology.py:582-598)."""
    return tuple(slice(max(n - o, 0), min(n - o + size, extent))
                 for o, extent, n, size in zip(old_origin[-2:], old_shape[-2:],
                                               new_origin[-2:], new_shape[-2:]))


def plane_thresholds(constraint):
    """``(positivity floor, threshold per plane)`` of the constraint a non-monotonic
    ``StarletMorphology`` puts on its coefficients -- ``ConstraintChain(PositivityConstraint,
    L0Constraint(absolute))``, applied once, with a threshold that is constant over every
    plane -- or ``None`` for anything else (which the device loop does not run)."""
    if not isinstance(constraint, ConstraintChain) or constraint.repeat != 1:
        return None
    if len(constraint.constraints) != 2:
        return None
    positive, hard = constraint.constraints
    if type(positive) is not PositivityConstraint or type(hard) is not L0Constraint:
        return None
    if hard.type != "absolute":
        return None
    thresh = np.asarray(hard.thresh, dtype=np.float64)
    if thresh.ndim == 3:
        flat = thresh.reshape(len(thresh), -1)
        if not np.all(flat == flat[:, :1]):
            return None
        thresh = flat[:, 0]
    if thresh.ndim != 1:
        return None
    return float(positive.zero), thresh


class StarletMorphology(Morphology):
    """Morphology whose parameter ``coeffs`` is the stack of generation-2 starlet
    coefficients of an image, all scales the box admits; the model is their reconstruction.

    Not monotonic (the default): the coefficients are kept positive and every plane but the
    last is hard-thresholded at ``threshold`` times the norm of its wavelet.  ``monotonic``:
    a ``MonotonicMaskConstraint`` about the middle of the box instead, which ``Blend.fit`` runs
    plane by plane in the device loop and which a shrink re-centres on the new box.  The transform runs on the device, so the coefficients
    are the reference's bit for bit.

    Unlike the reference, a shrink keeps the thresholds per plane: the reference's
    ``L0Constraint`` holds an array of the old box's shape and fails at the next proximal
    step."""

    def __init__(self, frame, image, bbox=None, monotonic=False, threshold=0):
        from .wavelet import Starlet

        if bbox is None:
            assert frame.bbox[1:].shape == image.shape
            bbox = Box(image.shape)
        self.monotonic = monotonic
        self.transform = Starlet.from_image(image)
        coeffs = self.transform.coefficients
        if monotonic:
            middle = tuple(n // 2 for n in bbox.shape)
            constraint = MonotonicMaskConstraint(middle, center_radius=1)
        else:
            per_plane = starlet_thresholds(self.transform.norm, threshold)
            constraint = ConstraintChain(
                PositivityConstraint(0),
                L0Constraint(np.broadcast_to(per_plane[:, None, None], coeffs.shape).copy()))
        super().__init__(frame, Parameter(coeffs, name="coeffs", step=1e-2, constraint=constraint),
                         bbox=bbox)

    def get_model(self, *parameters):
        from .wavelet import starlet_reconstruction

        return starlet_reconstruction(np.asarray(self.get_parameter(0, *parameters)))

    def update(self):
        """Every 10 iterations: peel off borders the reconstruction leaves empty (below
        1e-8).  Coefficients and moments are cut to the new box, planes and step stay
        (morphology.py:572-604)."""
        coeffs = self.get_parameter(0)
        if coeffs.fixed:
            return
        before = self.bbox.copy()
        self.shrink_box(self.get_model(), thresh=1e-8)
        if before == self.bbox:
            return
        cut = (slice(None),) + shrink_slices(before.origin, before.shape, self.bbox.origin,
                                             self.bbox.shape)

        def sliced(a):
            return None if a is None else np.asarray(a)[cut]

        constraint = coeffs.constraint
        if self.monotonic:
            constraint = MonotonicMaskConstraint(tuple(n // 2 for n in self.bbox.shape),
                                                 center_radius=1)
        else:
            rule = plane_thresholds(constraint)
            if rule is not None:  # the thresholds never depended on the pixel
                floor, per_plane = rule
                constraint = ConstraintChain(
                    PositivityConstraint(floor),
                    L0Constraint(np.broadcast_to(
                        per_plane[:, None, None], (len(per_plane),) + tuple(self.bbox.shape)).copy()))
        shrunk = Parameter(np.asarray(coeffs)[cut].copy(), name=coeffs.name, prior=coeffs.prior,
                           constraint=constraint, step=coeffs.step, fixed=coeffs.fixed,
                           m=sliced(coeffs.m), v=sliced(coeffs.v), vhat=sliced(coeffs.vhat))
        self._parameters = (shrunk,) + self._parameters[1:]
        raise UpdateException


class ProfileProx(Constraint):
    """The proximal operator a ``ProfileMorphology`` puts on one of its parameters
    (morphology.py:319-326, 472-473); ``kind`` names it, so that ``Blend.fit`` can tell the
    stock rule -- which the device applies -- from a user's."""

    def __init__(self, kind, f):
        super().__init__(f)
        self.kind = kind


class ProfileMorphology(Morphology):
    """Morphology from a radial profile ``func(R2, *parameters)`` of the squared elliptical
    radius in units of the parameter "radius", about the parameter "center", sheared by the
    parameter "ellipticity" (morphology.py:210-326).  The model is evaluated on the integer
    pixel grid of the box in float64 and is not normalised.

    The box is square: ``boxsize`` a side at construction, afterwards -- ``update()``, every
    10 iterations of a fit -- the smallest standard size that holds ten radii, around the
    pixel nearest to the centre.  It may overhang the frame.

    ``Blend.fit`` runs ``GaussianMorphology`` and ``SpergelMorphology``; a subclass with a
    profile function of its own has no gradient there and is refused."""

    def __init__(self, frame, func, *parameters, boxsize=None, resize=True):
        self.f = func
        self.center = self.get_parameter("center", *parameters)
        bbox = self.get_box(*parameters, boxsize=boxsize)
        self.resizing = resize
        self._set_grid(bbox)
        self.get_parameter("radius", *parameters).constraint = ProfileProx("radius", self._radius_prox)
        self.get_parameter("ellipticity", *parameters).constraint = ProfileProx(
            "ellipticity", self._eps_prox)
        super().__init__(frame, *parameters, bbox=bbox)

    def _set_grid(self, bbox):
        self._Y = np.arange(bbox.shape[-2], dtype="float") + bbox.origin[-2]
        self._X = np.arange(bbox.shape[-1], dtype="float") + bbox.origin[-1]

    def elliptical_radius2(self, *parameters):
        """``R2`` of every pixel of the box: squared sheared distance over radius squared."""
        center = self.get_parameter("center", *parameters)
        y = (self._Y - center[-2])[:, None]
        x = (self._X - center[-1])[None, :]
        e1, e2 = self.get_parameter("ellipticity", *parameters)
        shear = np.sqrt(1 - (e1 ** 2 + e2 ** 2))
        xs = ((1 - e1) * x - e2 * y) / shear
        ys = (-e2 * x + (1 + e1) * y) / shear
        R2 = ys ** 2 + xs ** 2
        radius = self.get_parameter("radius", *parameters)
        return R2 / radius ** 2

    def get_model(self, *parameters):
        return self.f(self.elliptical_radius2(*parameters), *parameters)

    def update(self):
        """Move the box to ``get_box()`` if that differs (morphology.py:288-300); parameters
        and their moments keep their shapes."""
        if not self.resizing:
            return
        bbox = self.get_box()
        if bbox != self.bbox:
            self.bbox.origin = bbox.origin
            self.bbox.shape = bbox.shape
            self._set_grid(bbox)
            raise UpdateException

    def get_box(self, *parameters, boxsize=None):
        if boxsize is None:
            radius = np.asarray(self.get_parameter("radius", *parameters), dtype=float)
            boxsize = get_minimal_boxsize(10 * float(radius.reshape(-1)[0]))
        center = self.get_parameter("center", *parameters)
        assert center is not None and len(center) >= 2
        origin = (int(round(center[-2])) - (boxsize // 2), int(round(center[-1])) - (boxsize // 2))
        return Box((boxsize, boxsize), origin=origin)

    @staticmethod
    def _radius_prox(x, step):
        return np.maximum(x, 1e-2)

    @staticmethod
    def _eps_prox(x, step):
        norm2 = (x ** 2).sum()
        if norm2 > 1:
            x /= np.sqrt(norm2) * 1.1  # back inside the unit circle
        return x


def _first_side(radius):
    """``ceil(10 radius)`` of a number or a one-element array, as a plain int."""
    return int(np.ceil(10 * float(np.asarray(radius, dtype=float).reshape(-1)[0])))


class GaussianMorphology(ProfileMorphology):
    """``exp(-R2 / 2)``: an elliptical Gaussian of standard deviation ``sigma`` pixels
    (morphology.py:329-369).  Plain numbers become fixed parameters; pass ``Parameter``s named
    "center", "radius" and "ellipticity" for what is to be fitted."""

    def __init__(self, frame, center, sigma, ellipticity=(0, 0), boxsize=None):
        assert len(center) == 2
        self.center = prepare_param(center, name="center")
        radius = prepare_param(sigma, name="radius")
        assert len(ellipticity) == 2
        ellipticity = prepare_param(ellipticity, name="ellipticity")
        if boxsize is None:
            boxsize = _first_side(sigma)
        super().__init__(frame, self._f, self.center, radius, ellipticity, boxsize=boxsize)

    def _f(self, R2, *parameters):
        return np.exp(-R2 / 2)

    @property
    def integral(self):
        return 2 * np.pi * self.get_parameter("radius") ** 2


class SpergelMorphology(ProfileMorphology):
    """The profile of Spergel (2010), ``f_nu(c_nu sqrt(R2 + 1e-4))`` with ``f_nu(u) = (u / 2)^nu
    K_nu(u) / Gamma(nu + 1)``, half-light radius ``rhalf`` pixels and ``nu`` kept within
    [-0.85, 4] (morphology.py:384-473).  ``c_nu`` is the reference's stored quartic fit."""

    _minimum_nu, _maximum_nu = -0.85, 4.00
    _z = np.array([-0.00788962, 0.0735303, -0.27770785, 0.99483285, 1.25227402])

    def __init__(self, frame, center, nu, rhalf, ellipticity=(0, 0), boxsize=None):
        assert len(center) == 2
        self.center = prepare_param(center, name="center")
        nu = prepare_param(nu, name="nu")
        assert self._minimum_nu <= nu[0] <= self._maximum_nu
        nu.constraint = ProfileProx("nu", self._nu_prox)
        radius = prepare_param(rhalf, name="radius")
        assert len(ellipticity) == 2
        ellipticity = prepare_param(ellipticity, name="ellipticity")
        if boxsize is None:
            boxsize = _first_side(rhalf)
        super().__init__(frame, self._f, self.center, nu, radius, ellipticity, boxsize=boxsize)

    def _f(self, R2, *parameters):
        nu = self.get_parameter("nu", *parameters)
        return self._f_nu(np.sqrt(R2 + 1e-4) * self._cnu(nu), nu)

    @property
    def integral(self):
        cnu = self._cnu(self.get_parameter("nu"))
        return 2 * np.pi * self.get_parameter("radius") ** 2 / cnu ** 2

    @staticmethod
    def _f_nu(x, nu):
        from scipy.special import gamma, kv

        return (x / 2) ** nu * kv(nu, x) / gamma(nu + 1)

    def _cnu(self, nu):
        z = self._z
        return z[0] * nu ** 4 + z[1] * nu ** 3 + z[2] * nu ** 2 + z[3] * nu + z[4]

    def _nu_prox(self, x, step):
        return np.maximum(np.minimum(self._maximum_nu, x), self._minimum_nu)
