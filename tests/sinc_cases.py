"""NumPy restatement of ``interpolation.interpolate_observation`` as this project specifies it,
and the scenes of its tests.

The row coordinates of the observation in the frame come from the pixels ``(i, 0)``, the column
coordinates from ``(0, j)``; ``hy`` and ``hx`` are the first spacing of each;
``Sy = sinc((y_lr[None, :] - arange(Hf)[:, None]) / hy)``, ``Sx`` likewise, and every band is
``Sy @ X @ Sx.T`` in float64.  tests/test_interpolate_host.py pins this to the reference's own
result on a scene where the reference's axis pairing is harmless; the same products in
``longdouble`` are the yardstick of the GPU kernel.

Error bounds, per output pixel, with ``B = |Sy| @ |X| @ |Sx|.T``: a float64 evaluation of the
two chained dot products of lengths ``Ho`` and ``Wo`` -- one rounding per multiply and per add,
any order -- is within ``(Ho + Wo) 2**-53 B`` of the exact value (``kernel_bound``), so two of
them differ by at most twice that (``pair_bound``)."""

import numpy as np


class Grid:
    """a duck-typed frame: a ``(C, Ny, Nx)`` shape"""

    def __init__(self, shape):
        self.shape = tuple(shape)


class Scene(Grid):
    """a duck-typed observation: ``data`` on a grid whose pixel ``(i, j)`` lies at
    ``(sy * i + oy, sx * j + ox)`` of the frame, rotated by ``angle`` radians"""

    def __init__(self, data, scale=(2.0, 2.0), offset=(3.0, 3.0), angle=0.0):
        super().__init__(data.shape)
        self.data, self.scale, self.offset, self.angle = data, scale, offset, angle

    def convert_pixel_to(self, target, pixel=None):
        p = np.asarray(pixel, dtype=np.float64).reshape(-1, 2)
        c, s = np.cos(self.angle), np.sin(self.angle)
        y, x = c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]
        return np.stack((y * self.scale[0] + self.offset[0],
                         x * self.scale[1] + self.offset[1]), axis=1)


def matrices(obs, frame):
    """float64 ``(Sy, Sx)`` of the specification"""
    Ho, Wo = obs.shape[1:]
    y_lr = obs.convert_pixel_to(frame, pixel=[(i, 0) for i in range(Ho)])[:, 0]
    x_lr = obs.convert_pixel_to(frame, pixel=[(0, j) for j in range(Wo)])[:, 1]
    hy, hx = np.abs(y_lr[1] - y_lr[0]), np.abs(x_lr[1] - x_lr[0])
    return (np.sinc((y_lr[None, :] - np.arange(frame.shape[1])[:, None]) / hy),
            np.sinc((x_lr[None, :] - np.arange(frame.shape[2])[:, None]) / hx))


def products(sy, cube, sx, dtype=np.float64):
    """``Sy @ X @ Sx.T`` of every band, computed in ``dtype``"""
    sy, sx = np.asarray(sy, dtype), np.asarray(sx, dtype)
    return np.stack([sy @ np.asarray(band, dtype) @ sx.T for band in cube])


def restate(obs, frame, dtype=np.float64, bands=None):
    """``interpolate_observation(obs, frame)``; ``bands``: images in the place of ``obs.data``
    (the denoised ones)"""
    sy, sx = matrices(obs, frame)
    return products(sy, obs.data if bands is None else bands, sx, dtype)


def magnitude(sy, cube, sx):
    """``|Sy| @ |X| @ |Sx|.T`` per band, float64"""
    return products(np.abs(sy), np.abs(np.asarray(cube, np.float64)), np.abs(sx))


def kernel_bound(sy, cube, sx):
    ho, wo = np.shape(cube)[-2:]
    return (ho + wo) * 2.0 ** -53 * magnitude(sy, cube, sx)


def pair_bound(sy, cube, sx):
    return 2 * kernel_bound(sy, cube, sx)


def carried(sy, cube, sx, rel=1e-12):
    """an error of ``rel`` of the cube's largest value in every pixel, carried through
    ``|Sy| @ . @ |Sx|.T``"""
    worst = rel * np.abs(np.asarray(cube, np.float64)).max()
    return magnitude(sy, np.full(np.shape(cube), worst), sx)


def peak_scene():
    """the 24 x 24 scene of the axis-pairing test: scale 2, offsets (3, 7), a unit pixel at
    low-resolution (2, 5), which belongs at (2 * 2 + 3, 2 * 5 + 7) = (7, 17)"""
    data = np.zeros((1, 8, 8))
    data[0, 2, 5] = 1.0
    return Scene(data, (2.0, 2.0), (3.0, 7.0)), Grid((1, 24, 24))


def blobs(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[-2], :shape[-1]]
    out = rng.normal(0.0, 0.3, shape)
    for band in out.reshape((-1,) + tuple(shape[-2:])):
        cy, cx = rng.uniform(1, shape[-2] - 1), rng.uniform(1, shape[-1] - 1)
        band += 6 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / 4.0)
    return out.astype(dtype)


def unusual_scenes():
    """``(observation, frame)`` pairs: non-square into non-square, unequal y and x scales, a
    float32 and a float64 observation"""
    return [
        (Scene(blobs((2, 9, 14), 1, np.float32), (2.0, 2.0), (1.0, 4.0)), Grid((2, 21, 37))),
        (Scene(blobs((3, 12, 12), 2, np.float64), (3.0, 1.5), (0.5, 2.25)), Grid((3, 40, 20))),
        (Scene(blobs((1, 17, 5), 3, np.float64), (1.0, 4.0), (-2.0, 0.0)), Grid((1, 16, 33))),
        (Scene(blobs((2, 6, 7), 4, np.float32), (2.5, 2.5), (3.0, 3.0)), Grid((2, 18, 19))),
    ]


def tutorial_observations():
    """the two observations of the reference's multi-resolution tutorial with their TAN WCS
    (tests/golden/multires_tutorial.npz): ``(low resolution, high resolution)``.  Pixels
    converted through the sky are not exactly affine there: the projection bends a line of 274
    pixels by a few hundredths of a pixel, which is no rotation"""
    import os

    import scarlet_amd as scarlet

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "multires_tutorial.npz"))

    def observation(tag, n):
        wcs = scarlet.TanWCS(g["crpix_" + tag], g["crval_" + tag], g["pc_" + tag],
                             g["cdelt_" + tag], array_shape=(n, n))
        return scarlet.Observation(g["data_" + tag].copy(), wcs=wcs,
                                   psf=scarlet.ImagePSF(g["psf_" + tag].copy()),
                                   channels=[str(c) for c in g["channels_" + tag]])

    return observation("hsc", 50), observation("hst", 250)
