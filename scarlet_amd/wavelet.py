"""Starlet wavelets (reference scarlet/wavelet.py) on the GPU.

The transform, its inverse and the multiresolution support run as HIP kernels
(``csrc/starlet.hip``); the coefficients are the reference's bit for bit (float64, the
B-spline sums in the reference's order, no FMA).  A user's own ``convolve2D`` callable runs
on the host in NumPy, with the reference's loop around it.  ``apply_wavelet_denoising`` and its
list form ``apply_wavelet_denoising_batch`` keep set-up and loop on the device
(``csrc/denoise_batch.hip``), with the same numbers as the loop over the functions above.

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


# ---------------------------------------------------------------------------
# wavelet denoising of a ragged list of images (csrc/denoise_batch.hip)
# ---------------------------------------------------------------------------
# smi_denoise_task: one image of smi_denoise_*
DENOISE_TASK = np.dtype([("h", "i4"), ("w", "i4"), ("scales", "i4"), ("reserved", "i4"),
                         ("image_off", "i8"), ("coeff_off", "i8"), ("plane_off", "i8"),
                         ("sigma0", "f8"), ("thresh0", "f8")], align=True)
# stages of smi_denoise_*
DENOISE_TRANSFORM, DENOISE_SUPPORT, DENOISE_ITERATE = 1, 2, 4
DENOISE_ALL = DENOISE_TRANSFORM | DENOISE_SUPPORT | DENOISE_ITERATE
# limits of denoise_batch.hip: pixels of an image one workgroup takes through its support
# iterations (the limit of detect_batch.hip), tasks of one call; device bytes of one chunk
DENOISE_BATCH_MAX_PIXELS = DETECT_BATCH_MAX_PIXELS
DENOISE_BATCH_MAX_TASKS = 65535
DENOISE_BATCH_BYTES = 1 << 30


def denoise_launches(top_scales, max_iter, stages=DENOISE_ALL):
    """Launches one ``smi_denoise_*`` call enqueues: ``(1 + 4 S) + 2 + (2 S + max_iter *
    max(6 S, 1))`` for the three stages, ``S = top_scales`` the largest scale count of the
    table -- whatever the number of images.  Asked of the library; no GPU needed."""
    n = ctypes.c_int32(0)
    _lib.check(_lib.load().smi_denoise_launches(int(top_scales), int(max_iter), int(stages),
                                                ctypes.byref(n)))
    return n.value


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _denoise_dtype(image):
    """dtype of the device copy of ``image``: float32, or float64 for everything else."""
    name = str(image.dtype).replace("torch.", "")
    return np.dtype(np.float32 if name == "float32" else np.float64)


def plan_wavelet_denoising_batch(images, max_iter=20, _max_tasks=None, _max_bytes=None):
    """``(groups, one_by_one)`` of ``apply_wavelet_denoising_batch``, without touching the GPU.
    ``groups``: one dict per device call -- ``dtype`` (float32, or float64 for everything else,
    as ``_upload`` converts), ``images`` (input positions, in input order; at most 65535 and
    ``DENOISE_BATCH_BYTES`` of device buffers), ``scales`` (the largest scale count among them)
    and ``launches`` (``denoise_launches(scales, max_iter)``: a function of those two alone).
    ``one_by_one``: ``(position, reason)`` of the images that do not join a group: more than
    ``DENOISE_BATCH_MAX_PIXELS`` = 65536 pixels (one workgroup runs all support iterations of an
    image; such an image keeps the per-image support between the same device-resident stages),
    fewer than 2 pixels along an axis or not 2-D (the per-image function raises), and every
    image when ``max_iter < 1`` (the per-image function's own behaviour)."""
    max_tasks = DENOISE_BATCH_MAX_TASKS if _max_tasks is None else _max_tasks
    max_bytes = DENOISE_BATCH_BYTES if _max_bytes is None else _max_bytes
    groups, one_by_one, open_group, used = [], [], {}, {}
    for i, im in enumerate(images):
        if not _is_tensor(im):
            im = np.asarray(im)
        shape = tuple(im.shape)
        if max_iter < 1:
            one_by_one.append((i, "max_iter < 1"))
            continue
        if len(shape) != 2:
            one_by_one.append((i, "not a 2-D image"))
            continue
        if min(shape) < 2:
            one_by_one.append((i, "fewer than 2 pixels along an axis"))
            continue
        h, w = shape
        if h * w > DENOISE_BATCH_MAX_PIXELS:
            one_by_one.append((i, "more than %d pixels" % DENOISE_BATCH_MAX_PIXELS))
            continue
        dtype = _denoise_dtype(im)
        scales = get_scales(shape)
        # image, then image_coeffs (float64), M (int32), current coefficients (float64), x, work
        need = h * w * (dtype.itemsize + (scales + 1) * 20 + 16)
        g = open_group.get(dtype)
        if g is None or len(g["images"]) >= max_tasks or used[dtype] + need > max_bytes:
            g = open_group[dtype] = {"dtype": dtype, "images": [], "scales": 0}
            groups.append(g)
            used[dtype] = 0
        g["images"].append(i)
        g["scales"] = max(g["scales"], scales)
        used[dtype] += need
    for g in groups:
        g["launches"] = denoise_launches(g["scales"], max_iter)
    return groups, one_by_one


def denoise_task_table(shapes, sigma0, thresh0):
    """The task table of ``denoise_device`` for images of ``shapes`` ``(H, W)`` packed one after
    another, each with all its scales: images, coefficient-shaped and plane-shaped buffers in
    input order.  ``sigma0`` / ``thresh0``: per image, as ``initial_sigma`` rounds them."""
    table = np.zeros(len(shapes), DENOISE_TASK)
    plane_off = coeff_off = 0
    for i, (h, w) in enumerate(shapes):
        s = _checked_scales((h, w))
        table[i] = (h, w, s, 0, plane_off, coeff_off, plane_off, sigma0[i], thresh0[i])
        plane_off += h * w
        coeff_off += (s + 1) * h * w
    return table


class _DenoiseBuffers:
    """Device buffers of one ``smi_denoise_*`` table, allocated once before the calls."""

    def __init__(self, torch, table, dev):
        npix = table["h"].astype(np.int64) * table["w"]
        n_coeffs = int(((table["scales"] + 1) * npix).sum())
        n_planes = int(npix.sum())
        self.n = len(table)
        self.coeffs = torch.empty(n_coeffs, dtype=torch.float64, device=dev)
        self.support = torch.empty(n_coeffs, dtype=torch.int32, device=dev)
        self.current = torch.empty(n_coeffs, dtype=torch.float64, device=dev)
        self.x = torch.empty(n_planes, dtype=torch.float64, device=dev)
        self.work = torch.empty(n_planes, dtype=torch.float64, device=dev)
        self.iterations = torch.zeros(self.n, dtype=torch.int32, device=dev)
        nbytes = ctypes.c_int64(0)
        _lib.check(_lib.load().smi_denoise_scratch_bytes(self.n, ctypes.byref(nbytes)))
        self.scratch = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
        self.table = table
        self.d_table = torch.from_numpy(table.view(np.uint8)).to(dev)


def denoise_device(d_images, buffers, stages, K=3, epsilon=1e-1, max_iter=20, positive=True):
    """Enqueue the ``stages`` of ``smi_denoise_*`` for the images packed in the flat float32 /
    float64 device tensor ``d_images`` (``buffers``: ``_DenoiseBuffers`` of their table);
    ``buffers.x`` holds the result after ``DENOISE_ITERATE``.  Nothing is waited for."""
    torch = _torch()
    lib = _lib.load()
    if d_images.dtype not in (torch.float32, torch.float64) or d_images.dim() != 1:
        raise ValueError("d_images must be a flat float32 or float64 device tensor")
    b = buffers
    fn = lib.smi_denoise_f32 if d_images.dtype == torch.float32 else lib.smi_denoise_f64
    with torch.cuda.device(d_images.device):
        _lib.check(fn(b.n, b.table.ctypes.data, _vp(b.d_table), int(stages), float(K),
                      float(epsilon), int(max_iter), int(bool(positive)), _vp(d_images),
                      d_images.numel(), _vp(b.coeffs), _vp(b.support), _vp(b.current),
                      b.coeffs.numel(), _vp(b.x), _vp(b.work), b.x.numel(), _vp(b.iterations),
                      _vp(b.scratch), b.scratch.numel(), _stream(torch)))


def _denoise_device_image(image):
    """The float32 / float64 device tensor of ``image`` (array or tensor)."""
    torch = _torch()
    if not _is_tensor(image):
        return _upload(image)
    if image.dtype not in (torch.float32, torch.float64):
        image = image.to(torch.float64)
    return image.to("cuda").contiguous()


def _denoise_sigma(image, sigma):
    """``sigma`` of one image: as given, or the host median of the reference."""
    if sigma is not None:
        return sigma
    if _is_tensor(image):
        image = image.cpu().numpy()
    return np.median(np.absolute(image - np.median(image)))


def _denoise_pack(torch, images):
    """The images of one group (one device dtype), packed one after another: one copy to the
    device when they are all host arrays."""
    if not any(_is_tensor(im) for im in images):
        packed = np.empty(sum(im.size for im in images), images[0].dtype)
        at = 0
        for im in images:
            packed[at:at + im.size] = im.reshape(-1)
            at += im.size
        return torch.from_numpy(packed).to("cuda")
    return torch.cat([_denoise_device_image(im).reshape(-1) for im in images])


def _denoise_tables(images, sigmas, k):
    """Task table of a group's images with their first thresholds: ``sigma`` (None: the host
    median) and ``initial_sigma`` in the dtype of the image AS GIVEN -- an int16 or float16 image
    is transformed in float64, but its ``sigma_j`` start as ``get_multiresolution_support``
    rounds them for the caller's array."""
    first = []
    for im, s in zip(images, sigmas):
        dtype = _denoise_dtype(im).type if _is_tensor(im) else im.dtype.type
        first.append(initial_sigma(dtype, 1, _denoise_sigma(im, s), k))
    return denoise_task_table([tuple(im.shape) for im in images], [s0[0] for s0, _ in first],
                              [t0[0] for _, t0 in first])


def _denoise_one(image, sigma, k, epsilon, max_iter, positive, device):
    """An image outside the groups.  Beyond the support stage's pixels: the transform and the
    loop of denoise_batch.hip, resident on the device, around the per-image support.  Anything
    else: the reference's loop over the public functions, with whatever it raises."""
    shape = tuple(image.shape)
    if max_iter < 1 or len(shape) != 2 or min(shape) < 2:
        if _is_tensor(image):
            image = image.cpu().numpy()
        x = _denoise_host_loop(image, sigma, k, epsilon, max_iter, positive)
        return _upload(x) if device else x
    torch = _torch()
    table = _denoise_tables([image], [sigma], k)
    d_image = _denoise_device_image(image).reshape(-1)
    buf = _DenoiseBuffers(torch, table, d_image.device)
    denoise_device(d_image, buf, DENOISE_TRANSFORM, k, epsilon, max_iter, positive)
    planes = int(table["scales"][0]) + 1
    M, _, _ = support_device(buf.coeffs.reshape(planes, 1, *shape), table["sigma0"][0],
                             table["thresh0"][0], k, epsilon, max_iter, masked=False)
    buf.support.copy_(M.reshape(-1))
    denoise_device(d_image, buf, DENOISE_ITERATE, k, epsilon, max_iter, positive)
    x = buf.x.reshape(shape)
    return x if device else x.cpu().numpy()


def apply_wavelet_denoising_batch(images, sigma=None, k=3, epsilon=1e-1, max_iter=20,
                                  image_type="ground", positive=True, device=False):
    """``[apply_wavelet_denoising(im, ...) for im in images]`` for 2-D images of any shapes,
    float32 and float64 mixed (other dtypes become float64), host arrays or device tensors, bit
    for bit: per group of ``plan_wavelet_denoising_batch`` one packed upload and one device chain
    (csrc/denoise_batch.hip) that holds set-up and loop and whose number of launches depends on
    the largest scale count and ``max_iter`` only.  ``sigma``: None (the host median of every
    image, taken before anything is enqueued), a scalar, or one entry per image.  Returns the
    list of float64 ``(Ny_i, Nx_i)`` arrays -- with ``device=True`` float64 device tensors,
    views into their group's buffer, without the copy to the host."""
    assert image_type in ("ground", "space")
    if image_type == "space":
        raise NotImplementedError(
            "apply_wavelet_denoising(image_type='space'): get_multiresolution_support provides "
            "only the 'ground' branch (the reference's 'space' branch cannot run)")
    given = [im if _is_tensor(im) else np.asarray(im) for im in images]
    images = [im if _is_tensor(im) or im.dtype in (np.float32, np.float64)
              else im.astype(np.float64) for im in given]
    if sigma is None or np.ndim(sigma) == 0:
        sigmas = [sigma] * len(images)
    else:
        sigmas = list(sigma)
        if len(sigmas) != len(images):
            raise ValueError("sigma must be None, a scalar or one entry per image, got {} for "
                             "{} images".format(len(sigmas), len(images)))
    groups, one_by_one = plan_wavelet_denoising_batch(images, max_iter)
    out = [None] * len(images)
    runs = []
    if groups:
        torch = _torch()
    for g in groups:
        ims = [images[i] for i in g["images"]]
        table = _denoise_tables([given[i] for i in g["images"]],
                                [sigmas[i] for i in g["images"]], k)
        d_images = _denoise_pack(torch, ims)
        buf = _DenoiseBuffers(torch, table, d_images.device)
        denoise_device(d_images, buf, DENOISE_ALL, k, epsilon, max_iter, positive)
        # only the result outlives the call: the stream keeps the order, and the caching
        # allocator hands the other buffers to the next group once the work before is done
        runs.append((g, buf.x, table))
        del buf, d_images
    for g, x, table in runs:
        flat = x if device else x.cpu().numpy()
        for i, t in zip(g["images"], table):
            at, h, w = int(t["plane_off"]), int(t["h"]), int(t["w"])
            out[i] = flat[at:at + h * w].reshape(h, w)
    for i, _ in one_by_one:
        out[i] = _denoise_one(given[i], sigmas[i], k, epsilon, max_iter, positive, device)
    return out


def apply_wavelet_denoising(image, sigma=None, k=3, epsilon=1e-1, max_iter=20,
                            image_type="ground", positive=True):
    """Wavelet denoising of Starck et al. 2011, section 4.1 (wavelet.py:424-465): the batch of
    one image of ``apply_wavelet_denoising_batch``, set-up and loop resident on the device."""
    return apply_wavelet_denoising_batch([image], None if sigma is None else [sigma], k, epsilon,
                                         max_iter, image_type, positive)[0]


def _denoise_host_loop(image, sigma, k, epsilon, max_iter, positive):
    """The reference's loop over the public functions, one device call per step: what
    ``max_iter < 1`` and images without a transform get (it raises as those calls do)."""
    image_coeffs = starlet_transform(image)
    if sigma is None:
        sigma = np.median(np.absolute(image - np.median(image)))
    coeffs = image_coeffs.copy()
    support = get_multiresolution_support(image, coeffs, sigma, k, epsilon, max_iter, "ground")
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
