"""Resampling helpers for multi-resolution rendering (reference
scarlet/interpolation.py:341-560, 708-739): WCS geometry, sinc interpolation of a PSF onto
a finer grid, the Fourier shift ramps.  Host-side set-up; nothing here runs per iteration.

``interpolate_observation`` (interpolation.py:563-599) sinc-interpolates the bands of an
observation onto the grid of a frame -- the detection image of the multi-resolution tutorial --
as two dense products per band on the GPU (``csrc/sinc_resample.hip``), for one observation or
for a catalogue of them; with ``wave_filter=True`` the bands first go through
``wavelet.apply_wavelet_denoising_batch`` and are resampled where they lie on the device.
Where the reference does something else than was meant, this module does what was meant:

- axis pairing: the reference converts the *diagonal* pixels ``(i, i)``, multiplies
  ``image.T`` and transposes the result, which pairs the x offset with the rows and the y
  offset with the columns (a unit pixel at low-resolution ``(2, 5)``, scale 2, offsets
  ``(3, 7)``, peaks at ``(11, 13)`` instead of ``(7, 17)``).  Here the row coordinates come
  from the pixels ``(i, 0)``, the column coordinates from ``(0, j)``, and the result is
  ``Sy @ X @ Sx.T``; with equal offsets the two agree in every bit;
- non-square observations: the reference stacks ``arange(Ho)`` and ``arange(Wo)`` into one
  array, which NumPy refuses when ``Ho != Wo``; they work here;
- rotated grids: the reference passes ``angle=None`` whatever the grids are; here grids
  rotated against each other raise ``NotImplementedError`` (``ResolutionRenderer`` decides
  rotation the same way, and renders between rotated grids).
"""

import numpy as np

from . import _lib, fft, wavelet
from .fft import mk_shifter  # noqa: F401  (same name as in the reference module)


def get_affine(wcs):
    """Linear part of the WCS."""
    try:
        return wcs.wcs.pc
    except AttributeError:
        return wcs.cd


def get_pixel_size(model_affine):
    """Pixel scale of an affine transformation (interpolation.py:387-394)."""
    return np.sqrt(np.abs(model_affine[0, 0])
                   * np.abs(model_affine[1, 1] - model_affine[0, 1] * model_affine[1, 0]))


def get_angles(frame_wcs, model_wcs):
    """``([cos, sin], h)``: rotation between the two pixel grids and the ratio of their
    pixel scales (interpolation.py:397-424)."""
    model_affine, frame_affine = get_affine(model_wcs), get_affine(frame_wcs)
    model_pix, frame_pix = get_pixel_size(model_affine), get_pixel_size(frame_affine)
    h = frame_pix / model_pix
    u = np.sum(frame_affine, axis=0)[:2] / frame_pix
    w = np.sum(model_affine, axis=0)[:2] / model_pix
    u = u / np.sum(u**2) ** 0.5
    w = w / np.sum(w**2) ** 0.5
    return [np.dot(u, w), np.array(u[0] * w[1] - u[1] * w[0])], h


def get_psf_size(psf):
    """Rough 3-sigma radius in pixels from the area above half maximum
    (interpolation.py:708-739)."""
    above = psf / np.max(psf) > 0.5
    d = 2 * (np.sum(above) / np.pi) ** 0.5
    return 3 * d / (2 * (2 * np.log(2)) ** 0.5)


def sinc_interp(images, coord_hr, coord_lr, angle=None, padding=3):
    """Whittaker-Shannon interpolation of ``images`` sampled at ``coord_lr`` onto
    ``coord_hr`` (interpolation.py:427-502)."""
    y_hr, x_hr = coord_hr
    y_lr, x_lr = coord_lr
    hy, hx = np.abs(y_lr[1] - y_lr[0]), np.abs(x_lr[1] - x_lr[0])
    assert hy != 0 and hx != 0
    if (angle is None) or (1 - angle[0] < np.finfo(float).eps):
        sy = np.sinc((y_lr[np.newaxis, :] - y_hr[:, np.newaxis]) / hy)
        sx = np.sinc((x_lr[:, np.newaxis] - x_hr[np.newaxis, :]) / hx)
        return np.array([np.dot(np.dot(sy, image.T), sx) for image in images])
    # general case: every output row is read off a copy of the image that has been
    # Fourier-shifted by the rotated row offset, then sinc-interpolated along both axes
    # (interpolation.py:469-502; also taken for cos = 1 - 2e-16 from unrotated grids)
    cos, sin = angle
    fft_shape = fft._get_fft_shape(images, images, padding=padding, axes=[1, 2])
    X = fft.Fourier(images)
    X_fft = X.fft(fft_shape, (-2, -1))
    ramp_y, ramp_x = mk_shifter(fft_shape)
    shift_y = np.exp(ramp_y[np.newaxis, :] * (-(y_hr[:, np.newaxis]) * cos))
    shift_x = np.exp(ramp_x[np.newaxis, :] * (-(y_hr[:, np.newaxis]) * sin))
    result_fft = X_fft[:, np.newaxis, :, :] * shift_y[np.newaxis, :, :, np.newaxis]
    result_fft = result_fft * shift_x[np.newaxis, :, np.newaxis, :]
    result_shape = np.array([result_fft.shape[0], result_fft.shape[1], X.image.shape[1],
                             X.image.shape[2]])
    shifted = fft.Fourier.from_fft(result_fft, fft_shape, result_shape, [2, 3]).image
    shy = np.sinc((y_lr[np.newaxis, :] + x_hr[:, np.newaxis] * sin) / hy)
    shx = np.sinc((x_lr[np.newaxis, :] - x_hr[:, np.newaxis] * cos) / hx)
    result_y = (shifted[:, :, np.newaxis, :, :]
                * shy[np.newaxis, np.newaxis, :, :, np.newaxis]).sum(axis=-2)
    return (result_y * shx[np.newaxis, np.newaxis, :, :]).sum(axis=-1)


def sinc_interp_inplace(image, h_image, h_target, angle, pad_shape=None):
    """Interpolate a cube from pixel scale ``h_image`` to ``h_target`` over the same
    physical area, odd output size (interpolation.py:505-560)."""
    assert len(image.shape) == 3, "images should be provided as a cube"
    if pad_shape is not None:
        image = fft._pad(image, pad_shape, axes=[-2, -1])
    ny_lr, nx_lr = image.shape[-2:]
    coord_lr = np.array([np.arange(ny_lr) - (ny_lr - 1) / 2, np.arange(nx_lr) - (nx_lr - 1) / 2])
    ny_hr = int(np.round(image.shape[-2] * h_image / h_target))
    nx_hr = int(np.round(image.shape[-1] * h_image / h_target))
    ny_hr += ny_hr % 2 == 0
    nx_hr += nx_hr % 2 == 0
    coord_hr = np.array([np.arange(ny_hr) - (ny_hr - 1) / 2,
                         np.arange(nx_hr) - (nx_hr - 1) / 2]) / h_image * h_target
    return sinc_interp(image, coord_hr, coord_lr, angle=angle)


# ---------------------------------------------------------------------------
# interpolate_observation: sinc matrices on the host, the two products on the device
# (csrc/sinc_resample.hip)
# ---------------------------------------------------------------------------
# smi_sinc_task: one band of one blend of smi_sinc_resample_*
SINC_TASK = np.dtype([("ho", "i4"), ("wo", "i4"), ("hf", "i4"), ("wf", "i4"), ("x_off", "i8"),
                      ("sy_off", "i8"), ("sx_off", "i8"), ("tmp_off", "i8"), ("out_off", "i8")],
                     align=True)
SINC_TILE = 16           # side of the kernel's square LDS tiles (SMI_SINC_TILE)
SINC_MAX_TASKS = 65535   # tasks of one call


def observation_grid(observation, frame):
    """``(y_lr, x_lr)``: the row and the column coordinates of ``observation``'s pixels in the
    pixel grid of ``frame`` (a ``Frame``, an ``Observation`` or anything ``convert_pixel_to``
    accepts), from the pixels ``(i, 0)`` and ``(0, j)``.  Raises ``ValueError`` for an
    observation with fewer than 2 pixels along an axis (there is no spacing to read off) and
    ``NotImplementedError`` for grids rotated against each other.  When both sides carry a
    WCS that is ``ResolutionRenderer``'s own test, ``sin**2 > eps`` of
    ``get_angles(observation.wcs, frame.wcs)``: the linear parts of the two WCS decide, so the
    curvature of a sky projection, which bends the converted pixels by a fraction of a pixel
    over a frame, is no rotation.  Without a WCS on both sides the converted pixels are all
    there is, and they are what the objects say exactly: the same ``sin**2 > eps``, with
    ``sin`` the drift across a line of pixels over its length."""
    Ho, Wo = (int(v) for v in tuple(observation.shape)[-2:])
    if Ho < 2 or Wo < 2:
        raise ValueError("interpolate_observation needs an observation of at least 2 x 2 pixels, "
                         "got %d x %d" % (Ho, Wo))
    rows = np.stack((np.arange(Ho, dtype=np.float64), np.zeros(Ho)), axis=1)
    cols = np.stack((np.zeros(Wo), np.arange(Wo, dtype=np.float64)), axis=1)
    rows = np.asarray(observation.convert_pixel_to(frame, pixel=rows), np.float64).reshape(-1, 2)
    cols = np.asarray(observation.convert_pixel_to(frame, pixel=cols), np.float64).reshape(-1, 2)
    eps = np.finfo(float).eps
    wcs_lr, wcs_hr = getattr(observation, "wcs", None), getattr(frame, "wcs", None)
    if wcs_lr is not None and wcs_hr is not None:
        angle, _ = get_angles(wcs_lr, wcs_hr)
        rotated = np.abs(angle[1]) ** 2 > eps
    else:
        rotated = any(across ** 2 > eps * (along ** 2 + across ** 2) for along, across in (
            (rows[-1, 0] - rows[0, 0], rows[-1, 1] - rows[0, 1]),
            (cols[-1, 1] - cols[0, 1], cols[-1, 0] - cols[0, 0])))
    if rotated:
        raise NotImplementedError("interpolate_observation between rotated pixel grids")
    return rows[:, 0].copy(), cols[:, 1].copy()


def sinc_matrices(y_lr, x_lr, shape):
    """``(Sy, Sx)`` of ``observation_grid``'s coordinates for a frame of ``shape`` ``(Hf, Wf)``:
    the reference's expression ``np.sinc((lr[None, :] - hr[:, None]) / h)`` with ``h`` the first
    spacing of ``lr``, as in ``sinc_interp``.  Float64 ``(Hf, Ho)`` and ``(Wf, Wo)``."""
    y_lr, x_lr = np.asarray(y_lr, np.float64), np.asarray(x_lr, np.float64)
    hy, hx = np.abs(y_lr[1] - y_lr[0]), np.abs(x_lr[1] - x_lr[0])
    assert hy != 0 and hx != 0
    y_hr, x_hr = np.arange(shape[0]), np.arange(shape[1])
    return (np.sinc((y_lr[np.newaxis, :] - y_hr[:, np.newaxis]) / hy),
            np.sinc((x_lr[np.newaxis, :] - x_hr[:, np.newaxis]) / hx))


def _band_views(torch, cubes):
    """Per blend the list of its bands as contiguous 2-D float32 / float64 device tensors.  Host
    cubes are packed per dtype and uploaded in one copy each; device tensors and lists of device
    bands stay where they lie."""
    out = [None] * len(cubes)
    host = {}
    for i, cube in enumerate(cubes):
        if isinstance(cube, (list, tuple)) or wavelet._is_tensor(cube):
            out[i] = [wavelet._denoise_device_image(band) for band in cube]
            ok = all(band.dim() == 2 for band in out[i])
        else:
            cube = np.asarray(cube)
            if cube.dtype not in (np.float32, np.float64):
                cube = cube.astype(np.float64)
            host.setdefault(cube.dtype, []).append((i, cube))
            ok = cube.ndim == 3
        if not ok:
            raise ValueError("the images of a blend must be a (bands, Ny, Nx) cube")
    for dtype, items in host.items():
        packed = np.empty(sum(cube.size for _, cube in items), dtype)
        at = 0
        for _, cube in items:
            packed[at:at + cube.size] = cube.reshape(-1)
            at += cube.size
        flat = torch.from_numpy(packed).to("cuda")
        at = 0
        for i, cube in items:
            C, h, w = cube.shape
            out[i] = [flat[at + c * h * w:at + (c + 1) * h * w].reshape(h, w) for c in range(C)]
            at += cube.size
    return out


def resample_bands(cubes, sy, sx, device=False):
    """``[np.stack([Sy @ X @ Sx.T for X in cube]) for cube, Sy, Sx in zip(cubes, sy, sx)]`` on
    the GPU (csrc/sinc_resample.hip): per blend a float32 / float64 ``(bands, Ho, Wo)`` cube (host
    array, device tensor or list of device bands; other dtypes become float64) and float64
    matrices ``(Hf, Ho)``, ``(Wf, Wo)``; the result float64 ``(bands, Hf, Wf)``.  Bands are read
    where they lie: one call of two launches per dtype and device buffer they lie in, whatever
    the number of blends (65535 bands per call).  Every output element is one chain of fused
    multiply-adds in ascending inner index, so its bits do not depend on the list.
    ``device=True`` returns device tensors, views into one buffer."""
    torch = wavelet._torch()
    lib = _lib.load()
    cubes, sy, sx = list(cubes), list(sy), list(sx)
    if not len(cubes) == len(sy) == len(sx):
        raise ValueError("one cube, one Sy and one Sx per blend")
    bands = _band_views(torch, cubes)
    mats, calls, shapes = [], {}, []
    mat_off = tmp_off = out_off = 0
    for i, (views, a, b) in enumerate(zip(bands, sy, sx)):
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        if a.ndim != 2 or b.ndim != 2:
            raise ValueError("Sy and Sx must be matrices")
        (hf, ho), (wf, wo) = a.shape, b.shape
        mats += [a.reshape(-1), b.reshape(-1)]
        shapes.append((out_off, len(views), hf, wf))
        for v in views:
            if tuple(v.shape) != (ho, wo):
                raise ValueError("blend %d: a band of shape %s does not match Sy %s and Sx %s"
                                 % (i, tuple(v.shape), a.shape, b.shape))
            storage = v.untyped_storage()
            key = (v.dtype, storage.data_ptr())
            if key not in calls:
                calls[key] = (torch.empty(0, dtype=v.dtype, device=v.device).set_(storage), [])
            calls[key][1].append((ho, wo, hf, wf, v.storage_offset(), mat_off, mat_off + a.size,
                                  tmp_off, out_off))
            tmp_off += hf * wo
            out_off += hf * wf
        mat_off += a.size + b.size
    d_out = torch.empty(max(out_off, 1), dtype=torch.float64, device="cuda")
    if out_off:
        d_mats = torch.from_numpy(np.concatenate(mats)).to("cuda")
        d_tmp = torch.empty(max(tmp_off, 1), dtype=torch.float64, device="cuda")
        for base, tasks in calls.values():
            fn = lib.smi_sinc_resample_f32 if base.dtype == torch.float32 else \
                lib.smi_sinc_resample_f64
            for at in range(0, len(tasks), SINC_MAX_TASKS):
                table = np.array(tasks[at:at + SINC_MAX_TASKS], SINC_TASK)
                d_table = torch.from_numpy(table.view(np.uint8)).to("cuda")
                _lib.check(fn(len(table), table.ctypes.data, wavelet._vp(d_table),
                              wavelet._vp(base), base.numel(), wavelet._vp(d_mats), d_mats.numel(),
                              wavelet._vp(d_tmp), d_tmp.numel(), wavelet._vp(d_out), d_out.numel(),
                              wavelet._stream(torch)))
    flat = d_out if device else d_out.cpu().numpy()
    return [flat[at:at + C * hf * wf].reshape(C, hf, wf) for at, C, hf, wf in shapes]


def plan_interpolate_observations(observations, frames, wave_filter=False):
    """What ``interpolate_observations`` will do, without touching the GPU: a dict with
    ``grids`` (per blend ``(y_lr, x_lr)`` of ``observation_grid``), ``shapes`` (per blend the
    result's ``(C, Hf, Wf)``), ``bands`` (the number of tasks of the resampling kernel) and
    ``denoise`` (``wavelet.plan_wavelet_denoising_batch`` of all bands of all observations, or
    None without ``wave_filter``).  Raises ``ValueError`` for lists of different lengths, an
    observation whose data is not a ``(C, Ho, Wo)`` cube and one with fewer than 2 pixels along
    an axis, ``NotImplementedError`` for rotated grids."""
    observations, frames = list(observations), list(frames)
    if len(observations) != len(frames):
        raise ValueError("one frame per observation, got {} observations and {} frames"
                         .format(len(observations), len(frames)))
    grids, shapes, images = [], [], []
    for k, (obs, frame) in enumerate(zip(observations, frames)):
        if len(tuple(obs.shape)) != 3 or len(tuple(frame.shape)) != 3:
            raise ValueError("blend %d: observation and frame must have (C, Ny, Nx) shapes" % k)
        if tuple(obs.data.shape) != tuple(obs.shape):
            raise ValueError("blend %d: data of shape %s in an observation of shape %s"
                             % (k, tuple(obs.data.shape), tuple(obs.shape)))
        grids.append(observation_grid(obs, frame))
        shapes.append((int(obs.shape[0]), int(frame.shape[1]), int(frame.shape[2])))
        images += list(obs.data)
    denoise = wavelet.plan_wavelet_denoising_batch(images) if wave_filter else None
    return {"grids": grids, "shapes": shapes, "bands": len(images), "denoise": denoise}


def interpolate_observations(observations, frames, wave_filter=False, device=False):
    """``[interpolate_observation(o, f, wave_filter) for o, f in zip(observations, frames)]``
    for a catalogue, bit for bit: the sinc matrices of every blend on the host, then the two
    products of all bands of all blends on the GPU (``resample_bands``).  With ``wave_filter``
    all bands of all observations go through one
    ``wavelet.apply_wavelet_denoising_batch(..., device=True)`` call first and are resampled
    where they lie, with no download in between.  Returns one float64 ``(C, Hf, Wf)`` array per
    blend -- device tensors with ``device=True``."""
    observations, frames = list(observations), list(frames)
    plan = plan_interpolate_observations(observations, frames, wave_filter)
    mats = [sinc_matrices(y, x, shape[1:]) for (y, x), shape in zip(plan["grids"], plan["shapes"])]
    cubes = [obs.data for obs in observations]
    if wave_filter:
        counts = [len(cube) for cube in cubes]
        flat = wavelet.apply_wavelet_denoising_batch([band for cube in cubes for band in cube],
                                                     device=True)
        starts = np.concatenate(([0], np.cumsum(counts)))
        cubes = [flat[starts[k]:starts[k + 1]] for k in range(len(counts))]
    return resample_bands(cubes, [m[0] for m in mats], [m[1] for m in mats], device)


def interpolate_observation(observation, frame, wave_filter=False, device=False):
    """Sinc-interpolate the bands of ``observation`` onto the pixel grid of ``frame`` (a
    ``Frame`` or an ``Observation``): float64 ``(C, frame.shape[1], frame.shape[2])``
    (interpolation.py:563-599, with the differences of the module docstring).
    ``wave_filter=True`` denoises the bands with ``wavelet.apply_wavelet_denoising_batch``
    first; ``device=True`` returns the device tensor."""
    return interpolate_observations([observation], [frame], wave_filter, device)[0]
