"""Starlet wavelets (reference scarlet/wavelet.py) on the GPU.

The transform, its inverse and the multiresolution support run as HIP kernels
(``csrc/starlet.hip``); the coefficients are the reference's bit for bit (float64, the
B-spline sums in the reference's order, no FMA).  A user's own ``convolve2D`` callable runs
on the host in NumPy, with the reference's loop around it.

Where the reference crashes this module does what was meant instead:

- the ``Starlet.image`` / ``generation`` / ``convolve2D`` setters pass ``generation`` as
  ``scales`` to ``starlet_transform`` (the reference then fails an assertion); here they
  recompute the coefficients with the same number of scales;
- ``multiband_starlet_reconstruction`` raises ``TypeError`` in the reference (it iterates
  over an int); here it inverts ``multiband_starlet_transform``;
- ``get_multiresolution_support(image_type="space")`` calls ``starlet_transform`` with a
  shape tuple as the image in the reference; here it raises ``NotImplementedError``.
"""

import ctypes

import numpy as np

from . import _lib


class InputError(Exception):
    """Exception raised for errors in the input."""

    def __init__(self, message):
        self.message = message


def get_scales(image_shape, scales=None):
    """Number of starlet scales for an image of shape ``image_shape``: at most
    ``log2(min(height, width)) - 1``, the maximum when ``scales`` is None."""
    max_scale = int(np.log2(np.min(image_shape[-2:]))) - 1
    if scales is None or scales > max_scale:
        scales = max_scale
    return int(scales)


def _checked_scales(image_shape, scales=None):
    """``get_scales``, refusing what leaves no coefficient plane: an image one pixel high or
    wide (``get_scales`` gives -1) or a negative ``scales``.  The reference fails there too
    (``np.zeros`` of a negative or empty first axis); this raises before any device call."""
    scales = get_scales(image_shape, scales)
    if scales < 0:
        raise ValueError(
            "starlet transform needs scales >= 0, got %d for an image of shape %s (an image "
            "must be at least 2 pixels high and wide)" % (scales, tuple(image_shape[-2:])))
    return scales


# ---------------------------------------------------------------------------
# device plumbing: torch tensors hold the device buffers, the library does the work
# ---------------------------------------------------------------------------
def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _lib.ScarletAmdError("the starlet transform needs a GPU (there is no CPU fallback)")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _upload(a):
    """A float32 / float64 device copy of ``a`` (other types become float64, as the
    reference's products with float64 taps do)."""
    torch = _torch()
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def transform_device(d_images, scales, generation=2):
    """Starlet coefficients ``(scales+1, n, H, W)`` (float64 device tensor) of the
    ``(n, H, W)`` device tensor ``d_images``; ``scales`` is used as given."""
    torch = _torch()
    lib = _lib.load()
    n, H, W = d_images.shape
    out = torch.empty((scales + 1, n, H, W), dtype=torch.float64, device=d_images.device)
    work = torch.empty((n, H, W), dtype=torch.float64, device=d_images.device)
    fn = lib.smi_starlet_transform_f32 if d_images.dtype == torch.float32 else \
        lib.smi_starlet_transform_f64
    _lib.check(fn(_vp(d_images), n, H, W, scales, generation, _vp(out), _vp(work), _stream(torch)))
    return out


def reconstruction_device(d_coeffs, generation=2):
    """Inverse of :func:`transform_device`: ``(n, H, W)`` float64 device tensor."""
    torch = _torch()
    lib = _lib.load()
    d_coeffs = d_coeffs.to(torch.float64).contiguous()
    P, n, H, W = d_coeffs.shape
    out = torch.empty((n, H, W), dtype=torch.float64, device=d_coeffs.device)
    work = torch.empty((n, H, W), dtype=torch.float64, device=d_coeffs.device)
    _lib.check(lib.smi_starlet_reconstruction_f64(_vp(d_coeffs), n, H, W, P - 1, generation,
                                                  _vp(out), _vp(work), _stream(torch)))
    return out


def support_device(d_coeffs, sigma0, thresh0, K=3, epsilon=1e-1, max_iter=20, masked=True):
    """Multiresolution support ("ground") of the ``(planes, n, H, W)`` float64 device tensor
    for ``n`` independent images; ``sigma0`` / ``thresh0``: ``(n, planes)`` initial
    ``sigma_j`` and ``K * sigma_j`` as the caller's dtype rounded them.
    Returns ``(M, M * w, iterations)``: int32 and float64 device tensors, int array."""
    torch = _torch()
    lib = _lib.load()
    P, n, H, W = d_coeffs.shape
    sigma0 = np.ascontiguousarray(np.broadcast_to(sigma0, (n, P)), dtype=np.float64)
    thresh0 = np.ascontiguousarray(np.broadcast_to(thresh0, (n, P)), dtype=np.float64)
    M = torch.empty((P, n, H, W), dtype=torch.int32, device=d_coeffs.device)
    Mw = torch.empty((P, n, H, W), dtype=torch.float64, device=d_coeffs.device) if masked else None
    iters = np.zeros(n, dtype=np.int32)
    _lib.check(lib.smi_multiresolution_support_f64(
        _vp(d_coeffs), n, P, H, W, n * H * W, H * W, _lib.ptr(sigma0, ctypes.c_double),
        _lib.ptr(thresh0, ctypes.c_double), float(K), float(epsilon), int(max_iter), _vp(M),
        _vp(Mw) if masked else None, _lib.ptr(iters, ctypes.c_int32), _stream(torch)))
    return M, Mw, iters


def coadd_device(d_images):
    """``np.sum(images, axis=0)`` of a ``(bands, H, W)`` float32 / float64 device tensor,
    summed band after band in the images' type."""
    torch = _torch()
    lib = _lib.load()
    bands, H, W = d_images.shape
    out = torch.empty((H, W), dtype=d_images.dtype, device=d_images.device)
    fn = lib.smi_coadd_f32 if d_images.dtype == torch.float32 else lib.smi_coadd_f64
    _lib.check(fn(_vp(d_images), bands, H, W, _vp(out), _stream(torch)))
    return out


def initial_sigma(dtype, planes, sigma, K):
    """``sigma_j`` and ``K * sigma_j`` of the first support iteration, in the dtypes the
    reference's NumPy expressions give them (wavelet.py:394-396)."""
    sigma_j = np.ones((planes,), dtype=dtype) * sigma
    return sigma_j.astype(np.float64), np.asarray(K * sigma_j).astype(np.float64)


# ---------------------------------------------------------------------------
# the detection chain of a ragged catalogue (csrc/detect_batch.hip)
# ---------------------------------------------------------------------------
# smi_detect_task: one blend of smi_detect_wavelets_*
DETECT_TASK = np.dtype([("bands", "i4"), ("h", "i4"), ("w", "i4"), ("scales", "i4"),
                        ("image_off", "i8"), ("coeff_off", "i8"), ("work_off", "i8"),
                        ("sigma0", "f8"), ("thresh0", "f8")], align=True)
# limits of detect_batch.hip: pixels of a frame one workgroup takes through its support
# iterations, tasks of one call
DETECT_BATCH_MAX_PIXELS = 1 << 16
DETECT_BATCH_MAX_TASKS = 65535


def detect_task_table(shapes, scales, sigma0, thresh0):
    """The task table of ``detect_wavelets_batch_device`` for blends of ``shapes``
    ``(bands, H, W)`` packed one after another: images, coefficients ``(scales_i + 1, H, W)``
    and work planes each in their own buffer, in input order.  ``scales``: as given to the
    transform, per blend; ``sigma0`` / ``thresh0``: per blend, as ``initial_sigma`` rounds
    them (all planes of a blend start equal)."""
    table = np.zeros(len(shapes), DETECT_TASK)
    image_off = coeff_off = work_off = 0
    for k, ((bands, h, w), s) in enumerate(zip(shapes, scales)):
        table[k] = (bands, h, w, s, image_off, coeff_off, work_off, sigma0[k], thresh0[k])
        image_off += bands * h * w
        coeff_off += (s + 1) * h * w
        work_off += h * w
    return table


def detect_table_sizes(table):
    """Elements of the image, coefficient and work buffers the tasks of ``table`` reach."""
    if not len(table):
        return 0, 0, 0
    npix = table["h"].astype(np.int64) * table["w"]
    return (int((table["image_off"] + table["bands"] * npix).max()),
            int((table["coeff_off"] + (table["scales"] + 1) * npix).max()),
            int((table["work_off"] + npix).max()))


def detect_wavelets_batch_device(d_images, table, K=3, epsilon=1e-1, max_iter=20, generation=2,
                                 support=False):
    """Coadd, starlet transform and multiresolution support of every blend of ``table``
    (``DETECT_TASK`` records, see ``detect_task_table``) whose images lie packed in the flat
    float32 / float64 device tensor ``d_images``: a fixed number of launches whatever the
    number of blends, nothing waited for.  Returns ``(masked, support, iterations)``: the flat
    float64 device tensor of ``M * w`` (blend ``i`` holds ``(scales_i + 1, H_i, W_i)`` at
    ``table["coeff_off"][i]``), ``M`` as int32 in the same layout (None unless ``support``)
    and the int32 device tensor of the iterations every blend's support took."""
    torch = _torch()
    lib = _lib.load()
    table = np.ascontiguousarray(table, DETECT_TASK)
    n = len(table)
    n_images, n_coeffs, n_work = detect_table_sizes(table)
    dev = d_images.device
    if d_images.dtype not in (torch.float32, torch.float64) or d_images.dim() != 1:
        raise ValueError("d_images must be a flat float32 or float64 device tensor")
    if d_images.numel() < n_images:
        raise ValueError("the tasks reach beyond the packed images")
    masked = torch.empty(max(n_coeffs, 1), dtype=torch.float64, device=dev)
    iters = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)[:n]
    M = torch.empty(max(n_coeffs, 1), dtype=torch.int32, device=dev) if support else None
    if n == 0:
        return masked, M, iters
    coeffs = torch.empty(max(n_coeffs, 1), dtype=torch.float64, device=dev)
    work = torch.empty(max(n_work, 1), dtype=torch.float64, device=dev)
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.smi_detect_wavelets_scratch_bytes(n, ctypes.byref(nbytes)))
    scratch = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    fn = lib.smi_detect_wavelets_f32 if d_images.dtype == torch.float32 else \
        lib.smi_detect_wavelets_f64
    with torch.cuda.device(dev):
        _lib.check(fn(n, table.ctypes.data, _vp(d_table), float(K), float(epsilon),
                      int(max_iter), int(generation), _vp(d_images), d_images.numel(),
                      _vp(coeffs), coeffs.numel(), _vp(work), work.numel(), _vp(masked),
                      _vp(M) if support else None, _vp(iters), _vp(scratch), scratch.numel(),
                      _stream(torch)))
    return masked, M, iters


# ---------------------------------------------------------------------------
# the reference's interface
# ---------------------------------------------------------------------------
def bspline_convolve(image, scale):
    """Convolve a 2-D image with the B-spline (1/16, 1/4, 3/8, 1/4, 1/16) at spacing
    ``2**scale``, zeros outside the image (wavelet.py:154-191).  On the host, in NumPy: this
    is the building block users combine with their own code; the transforms below run the
    same arithmetic on the device."""
    taps = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])

    def along(x, axis):
        d = 2 ** scale
        n = x.shape[axis]
        out = x * taps[2]
        for tap, shift in ((taps[0], -2 * d), (taps[1], -d), (taps[3], d), (taps[4], 2 * d)):
            if abs(shift) >= n:
                continue
            dst = [slice(None)] * 2
            src = [slice(None)] * 2
            if shift < 0:  # out[i] += x[i + shift] for i >= -shift
                dst[axis], src[axis] = slice(-shift, None), slice(None, n + shift)
            else:
                dst[axis], src[axis] = slice(None, n - shift), slice(shift, None)
            out[tuple(dst)] += x[tuple(src)] * tap
        return out

    return along(along(image, 0), 1)


def _host_transform(image, scales, generation, convolve2D):
    starlet = np.zeros((scales + 1,) + image.shape)
    c = image
    for j in range(scales):
        smooth = convolve2D(c, j)
        starlet[j] = c - (convolve2D(smooth, j) if generation == 2 else smooth)
        c = smooth
    starlet[-1] = c
    return starlet


def starlet_transform(image, scales=None, generation=2, convolve2D=None):
    """Starlet coefficients ``(scales+1, Ny, Nx)`` (float64) of a 2-D image
    (wavelet.py:220-266): ``w_j = c_j - B_j(c_j)`` (generation 1) or
    ``c_j - B_j(B_j(c_j))`` (generation 2), ``c_{j+1} = B_j(c_j)``, last plane
    ``c_scales``.  ``convolve2D=None``: the B-spline on the device."""
    assert len(image.shape) == 2, f"Image should be 2D, got {len(image.shape)}"
    assert generation in (1, 2), f"generation should be 1 or 2, got {generation}"
    scales = _checked_scales(image.shape, scales)
    if convolve2D is not None:
        return _host_transform(image, scales, generation, convolve2D)
    d = _upload(image)
    return transform_device(d[None], scales, generation)[:, 0].cpu().numpy()


def multiband_starlet_transform(image, scales=None, generation=2, convolve2D=None):
    """Starlet transform of every band of a ``(bands, Ny, Nx)`` cube:
    ``(scales+1, bands, Ny, Nx)`` in the cube's dtype (wavelet.py:269-281).  The bands
    are transformed in one batch on the device."""
    assert len(image.shape) == 3, \
        f"Image should be 3D (bands, height, width), got shape {len(image.shape)}"
    assert generation in (1, 2), f"generation should be 1 or 2, got {generation}"
    scales = _checked_scales(image.shape, scales)
    if convolve2D is not None:
        out = np.empty((scales + 1,) + image.shape, dtype=image.dtype)
        for b, band in enumerate(image):
            out[:, b] = _host_transform(band, scales, generation, convolve2D)
        return out
    coeffs = transform_device(_upload(image), scales, generation).cpu().numpy()
    return coeffs.astype(image.dtype, copy=False)


def starlet_reconstruction(starlets, generation=2, convolve2D=None):
    """Image from starlet coefficients ``(scales+1, Ny, Nx)`` (wavelet.py:284-311):
    the sum of the planes (generation 1) or ``c <- B_j(c) + w_j`` from the last scale
    down (generation 2).  Float64; ``convolve2D=None`` on the device."""
    if convolve2D is not None:
        if generation == 1:
            return np.sum(starlets, axis=0)
        scales = len(starlets) - 1
        c = starlets[-1]
        for j in range(scales - 1, -1, -1):
            c = convolve2D(c, j) + starlets[j]
        return c
    d = _upload(np.asarray(starlets, dtype=np.float64))
    return reconstruction_device(d[:, None], generation)[0].cpu().numpy()


def multiband_starlet_reconstruction(starlets, generation=2, convolve2D=None):
    """Inverse of :func:`multiband_starlet_transform`: ``(scales+1, bands, Ny, Nx)`` ->
    ``(bands, Ny, Nx)`` in float64.  (The reference raises ``TypeError`` here.)"""
    if convolve2D is not None:
        return np.stack([starlet_reconstruction(starlets[:, b], generation, convolve2D)
                         for b in range(starlets.shape[1])])
    d = _upload(np.asarray(starlets, dtype=np.float64))
    return reconstruction_device(d, generation).cpu().numpy()


def get_multiresolution_support(image, starlets, sigma, K=3, epsilon=1e-1, max_iter=20,
                                image_type="ground"):
    """Mask (int) of the significant coefficients of ``starlets`` (wavelet.py:314-408),
    "ground" branch: per scale, ``|w| > K sigma_j`` with ``sigma_j`` re-estimated from the
    insignificant coefficients until it changes by less than ``epsilon``.  The standard
    deviations are float64 reductions on the device.  ``image_type="space"`` raises
    ``NotImplementedError``: the reference's branch passes a shape tuple as the image to
    ``starlet_transform`` and cannot run."""
    assert image_type in ("ground", "space")
    if image_type == "space":
        raise NotImplementedError(
            "get_multiresolution_support(image_type='space'): the reference calls "
            "starlet_transform(shape, noise_img, generation=1) with a shape tuple as the image "
            "and fails; only the 'ground' branch is provided")
    d = _upload(np.asarray(starlets, dtype=np.float64))
    sigma0, thresh0 = initial_sigma(np.asarray(image).dtype, len(starlets), sigma, K)
    M, _, _ = support_device(d[:, None], sigma0, thresh0, K, epsilon, max_iter, masked=False)
    return M[:, 0].cpu().numpy().astype(int)


def apply_wavelet_denoising(image, sigma=None, k=3, epsilon=1e-1, max_iter=20,
                            image_type="ground", positive=True):
    """Wavelet denoising of Starck et al. 2011, section 4.1 (wavelet.py:424-465)."""
    image_coeffs = starlet_transform(image)
    if sigma is None:
        sigma = np.median(np.absolute(image - np.median(image)))
    coeffs = image_coeffs.copy()
    support = get_multiresolution_support(image, coeffs, sigma, k, epsilon, max_iter, image_type)
    x = starlet_reconstruction(coeffs)
    for _ in range(max_iter):
        coeffs = starlet_transform(x)
        x = x + starlet_reconstruction(support * (image_coeffs - coeffs))
        if positive:
            x[x < 0] = 0
    return x


class Starlet:
    """Starlet transform of an image (wavelet.py:5-151): the image, its coefficients and the
    generation / filter that relate them.

    Unlike the reference, the ``image``, ``generation`` and ``convolve2D`` setters keep the
    number of scales when they recompute the coefficients (the reference passes
    ``generation`` as ``scales`` and fails)."""

    def __init__(self, image, coefficients, generation, convolve2D):
        self._image = image
        self._coeffs = coefficients
        self._generation = generation
        self._convolve2D = convolve2D
        self._norm = None

    @staticmethod
    def from_image(image, scales=None, generation=2, convolve2D=None):
        """Transform ``image`` (all scales when ``scales`` is None)."""
        return Starlet(image, starlet_transform(image, get_scales(image.shape, scales),
                                                generation, convolve2D), generation, convolve2D)

    @staticmethod
    def from_coefficients(coefficients, generation=2, convolve2D=None):
        """Reconstruct the image of ``coefficients``."""
        return Starlet(starlet_reconstruction(coefficients, generation, convolve2D),
                       coefficients, generation, convolve2D)

    def _retransform(self):
        self._coeffs = starlet_transform(self._image, self.scales, self._generation,
                                         self._convolve2D)

    @property
    def image(self):
        """The real-space image"""
        return self._image

    @image.setter
    def image(self, image):
        self._image = image
        self._retransform()

    @property
    def coefficients(self):
        """Starlet coefficients"""
        return self._coeffs

    @coefficients.setter
    def coefficients(self, coeffs):
        self._coeffs = coeffs
        self._image = starlet_reconstruction(coeffs, self._generation, self._convolve2D)

    @property
    def scales(self):
        """Number of starlet scales"""
        return len(self._coeffs) - 1

    @property
    def generation(self):
        """Generation (1 or 2) of the transform"""
        return self._generation

    @generation.setter
    def generation(self, value):
        if value != self._generation:
            self._generation = value
            self._retransform()
            self._norm = None

    @property
    def convolve2D(self):
        """Filter of the transform (None: the B-spline)"""
        return self._convolve2D

    @convolve2D.setter
    def convolve2D(self, value):
        if value != self._convolve2D:
            self._convolve2D = value
            self._retransform()
            self._norm = None

    @property
    def norm(self):
        """Norm of the transform of a centred Dirac at every scale"""
        if self._norm is None:
            shape = self._image.shape[-2:]
            dirac = np.zeros(shape)
            dirac[shape[0] // 2, shape[1] // 2] = 1
            seed = starlet_transform(dirac, generation=self._generation,
                                     convolve2D=self._convolve2D)
            self._norm = np.sqrt(np.sum(seed ** 2, axis=(-2, -1)))
        return self._norm
