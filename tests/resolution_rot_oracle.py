"""TEST INFRASTRUCTURE -- float64 restatement of the reference's ``ResolutionRenderer`` between
ROTATED pixel grids (scarlet/renderer.py:319-363, 414-476, 498-524; ``small_axis``, the branch
a square observation takes).

As in ``oracle.resample`` the set-up quantities that depend on WCS and PSF interpolation -- the
padded difference kernel, ``shifts`` (2, n_a), ``other_shifts`` (2, n_b), the FFT shape and the
pixel-scale ratio ``h`` -- are inputs; tests/golden/resolution_rotated.npz holds the reference's
own values.  Restated is the arithmetic:

* ``op[c, a] = h^2 *`` (kernel Fourier-shifted in 2-D by ``shifts[:, a]``);
* per call the centred, padded model Fourier-shifted in 2-D by ``-other_shifts[:, b]`` for every
  ``b``, and ``out[c, a, b] = sum_yx op[c, a, y, x] * shifted[c, b, y, x]``.

A 2-D Fourier shift as the reference does it: ``rfftn`` over (y, x) of the ``ifftshift``ed image
(``Fourier.fft``), times ``exp(-2 pi i (f_y s_y + f_x s_x))`` with ``f_y = fftfreq(Fy)`` and
``f_x = rfftfreq(Fx)`` (``mk_shifter``, interpolation.py:363-371), ``irfftn`` to (Fy, Fx) and
``fftshift`` (``Fourier.from_fft``).  It is a real circular convolution, so its transpose is the
shift by the opposite vector; ``RotatedLowResObservation.adjoint`` uses that through the dense
operator ``d out[c, a, b] / d padded[c, y, x]``, and test_resolution_rot_host.py checks the
pair ``render`` / ``adjoint`` with the inner-product identity.

``render_fourier`` is the same map evaluated in Fourier space, the way the device does it
(scarlet_amd/csrc/resample_rot.hip).
"""

import numpy as np

from oracle import resample


def phase_table(fft_shape, shifts):
    """``exp(-2 pi i (f_y s_y + f_x s_x))``, (n, Fy, Kx), for ``shifts`` (2, n)."""
    Fy, Fx = fft_shape
    fy, fx = np.fft.fftfreq(Fy), np.fft.rfftfreq(Fx)
    sy, sx = np.asarray(shifts, dtype=np.float64)
    return np.exp(-2j * np.pi * (fy[None, :, None] * sy[:, None, None]
                                 + fx[None, None, :] * sx[:, None, None]))


def fourier_shift_2d(images, shifts):
    """``images`` (..., Fy, Fx) Fourier-shifted by every column of ``shifts`` (2, n):
    (..., n, Fy, Fx)."""
    images = np.asarray(images, dtype=np.float64)
    shape = images.shape[-2:]
    spectrum = np.fft.rfftn(np.fft.ifftshift(images, axes=(-2, -1)), axes=(-2, -1))
    shifted = spectrum[..., None, :, :] * phase_table(shape, shifts)
    return np.fft.fftshift(np.fft.irfftn(shifted, shape, axes=(-2, -1)), axes=(-2, -1))


def project_edge_columns(table, Fx):
    """What ``irfftn`` keeps of a spectrum (n, Fy, Kx) on the two self-conjugate columns
    (``kx = 0`` and, for even ``Fx``, ``kx = Fx / 2``): its Hermitian part along y,
    ``(t[ky] + conj(t[-ky mod Fy])) / 2``."""
    out = np.array(table)
    mirror = (-np.arange(table.shape[-2])) % table.shape[-2]
    for kx in ([0] + ([Fx // 2] if Fx % 2 == 0 else [])):
        out[..., kx] = 0.5 * (table[..., kx] + np.conj(table[..., mirror, kx]))
    return out


class RotatedLowResObservation(resample.LowResObservation):
    """``oracle.resample.LowResObservation`` on a rotated grid: ``shifts`` (2, n_a) and
    ``other_shifts`` (2, n_b) as the renderer has them."""

    def __init__(self, kernel, shifts, other_shifts, h, channels, frame_hw, data, weights):
        kernel = np.asarray(kernel, dtype=np.float64)
        self.C, self.Fy, self.Fx = kernel.shape
        self.channels = list(channels)
        self.frame_hw = tuple(frame_hw)
        self.data = np.asarray(data, dtype=np.float64)
        self.weights = np.asarray(weights, dtype=np.float64)
        self.shifts = np.asarray(shifts, dtype=np.float64)
        self.other_shifts = np.asarray(other_shifts, dtype=np.float64)
        # renderer.py:353-354: the kernel shifted in 2-D to every low-resolution row
        self.kernel, self.h2 = kernel, float(h) ** 2
        self.op = self.h2 * fourier_shift_2d(kernel, self.shifts)  # (C, n_a, Fy, Fx)
        H, W = self.frame_hw
        self.y0, self.x0 = (self.Fy - H + 1) // 2, (self.Fx - W + 1) // 2
        self._dense = None

    def render_padded(self, padded):
        """(C, Fy, Fx) -> (C, n_a, n_b) (renderer.py:498-516)."""
        shifted = fourier_shift_2d(padded, -self.other_shifts)  # (C, n_b, Fy, Fx)
        return np.einsum("cayx,cbyx->cab", self.op, shifted)

    def render(self, model):
        return self.render_padded(self._pad(np.asarray(model, dtype=np.float64)[self.channels]))

    @property
    def dense(self):
        """``d out[c, a, b] / d padded[c, y, x]``, (C, n_a, n_b, Fy, Fx): the transpose of the
        shift by ``-other_shifts[:, b]`` is the shift by ``+other_shifts[:, b]``."""
        if self._dense is None:
            self._dense = fourier_shift_2d(self.op, self.other_shifts)
        return self._dense

    def adjoint_padded(self, upstream):
        """(C, n_a, n_b) -> (C, Fy, Fx)."""
        return np.einsum("cabyx,cab->cyx", self.dense, np.asarray(upstream, dtype=np.float64))

    def adjoint(self, upstream, n_model_channels):
        padded = self.adjoint_padded(upstream)
        H, W = self.frame_hw
        out = np.zeros((n_model_channels, H, W))
        out[self.channels] = padded[:, self.y0:self.y0 + H, self.x0:self.x0 + W]
        return out

    def render_fourier(self, padded, project=True):
        """The map of ``render_padded`` in Fourier space:

            out[c, a, b] = 1 / (Fy Fx) sum_k w_kx Re(Ehat[c, a, k] conj(Mhat[c, k] beta[b, k]))

        with ``Ehat[c, a] = h^2 rfftn(kernel[c]) alpha[a]``, ``Mhat = rfftn(padded)``, ``alpha[a]``
        and ``beta[b]`` the phase tables of ``shifts[:, a]`` and ``-other_shifts[:, b]`` and
        ``w = 1`` for ``kx = 0`` and the x-Nyquist term, else 2.  ``irfftn`` returns a real
        image, i.e. it drops the non-Hermitian part of a shifted spectrum on the two
        self-conjugate columns; the kernel's and the model's transforms are Hermitian there, so
        the projection falls on the tables (``project_edge_columns``).  ``project=False``
        leaves both tables pure phases everywhere -- not what ``irfftn`` computes.  (The
        ``ifftshift`` of both images is a common phase factor of ``Ehat`` and ``Mhat`` and
        cancels in the product.)"""
        Fy, Fx = self.Fy, self.Fx
        alpha = phase_table((Fy, Fx), self.shifts)
        beta = phase_table((Fy, Fx), -self.other_shifts)
        if project:
            alpha, beta = project_edge_columns(alpha, Fx), project_edge_columns(beta, Fx)
        Ehat = self.h2 * np.fft.rfftn(self.kernel, axes=(-2, -1))[:, None] * alpha[None]
        Mhat = np.fft.rfftn(np.asarray(padded, dtype=np.float64), axes=(-2, -1))
        w = np.full(Fx // 2 + 1, 2.0)
        w[0] = 1.0
        if Fx % 2 == 0:
            w[-1] = 1.0
        return np.einsum("cayk,cbyk,k->cab", Ehat, np.conj(Mhat[:, None] * beta[None]),
                         w).real / (Fy * Fx)


def build_scene(name, g, n_components=2):
    """``(scene, lowres)``: the oracle's ``pgm.Scene`` of a case of resolution_rot_cases.py -- the
    high-resolution observation embedded in the frame with the facade's difference kernel
    (``ConvolutionRenderer``: pinned elsewhere), the low-resolution term from the REFERENCE's
    set-up quantities (golden ``g``) and the components of ``cases.components``."""
    import resolution_rot_cases as cases
    from oracle import pgm

    frame, obs_hr, obs_lr = cases.scene(name)
    C, H, W = frame.shape
    data_sl, model_sl = obs_hr.renderer.slices
    data, weights = np.zeros((C, H, W)), np.zeros((C, H, W))
    data[0][tuple(model_sl[1:])] = obs_hr.data[0][tuple(data_sl[1:])]
    weights[0][tuple(model_sl[1:])] = obs_hr.weights[0][tuple(data_sl[1:])]
    stamp = np.asarray(obs_hr.renderer.diff_kernel.image, dtype=np.float64)
    kernel = np.zeros((C,) + stamp.shape[1:])
    kernel[0] = stamp[0]
    kernel[1:, stamp.shape[1] // 2, stamp.shape[2] // 2] = 1  # unobserved there: weight zero
    channels = [list(frame.channels).index(c) for c in obs_lr.channels]
    lowres = RotatedLowResObservation(
        g[name + "_kernel"], g[name + "_shifts"], g[name + "_other_shifts"], float(g[name + "_h"]),
        channels, (H, W), obs_lr.data, obs_lr.weights)
    comps = [pgm.Component(sed.astype(np.float64), stamp.astype(np.float64), origin)
             for sed, stamp, origin in cases.components(name, n_components)]
    scene = pgm.Scene((C, H, W), data, weights, kernel, comps, dtype=np.float64,
                      extra_observations=[lowres])
    return scene, lowres
