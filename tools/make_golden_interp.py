"""Golden vectors of ``interpolate_observation``: ``tests/golden/interpolate_observation.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present):

    python tools/make_golden_interp.py

The reference is imported through ``oracle.refshim.load_reference``, and its own
``interpolate_observation`` runs on a duck-typed observation and frame: objects with ``.shape``,
``.data`` and an affine ``convert_pixel_to``.  The observation is square, the frame is square
and the y and x offsets and scales are equal, so the reference's pairing of the x offset with
the rows (scarlet_amd/interpolation.py, module docstring) is harmless.  Recorded with and
without ``wave_filter``, together with the reference's ``apply_wavelet_denoising`` of two small
images.  The file holds data only and is written without time stamps.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_golden_detect import save_deterministic  # noqa: E402
from oracle.refshim import load_reference  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "interpolate_observation.npz")
SCALE, OFFSET = 2.0, 3.0
OBS_SHAPE, FRAME_SHAPE = (3, 8, 8), (3, 24, 24)


class Grid:
    """the duck-typed frame: a shape"""

    def __init__(self, shape):
        self.shape = shape


class Scene(Grid):
    """the duck-typed observation: data on a grid ``SCALE`` times coarser than the frame's,
    shifted by ``OFFSET`` along both axes"""

    def __init__(self, data):
        super().__init__(data.shape)
        self.data = data

    def convert_pixel_to(self, target, pixel=None):
        return np.asarray(pixel, dtype=np.float64) * SCALE + OFFSET


def blobs(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[-2], :shape[-1]]
    out = rng.normal(0.0, 0.3, shape)
    for band in out.reshape((-1,) + tuple(shape[-2:])):
        cy, cx = rng.uniform(1, shape[-2] - 1), rng.uniform(1, shape[-1] - 1)
        band += 6 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / 4.0)
    return out.astype(dtype)


def main():
    so = os.path.join(REPO, "oracle", "liboracle.so")
    had_so = os.path.exists(so)
    load_reference.load()
    import scarlet.interpolation as rinterp
    import scarlet.wavelet as rwave

    data = blobs(OBS_SHAPE, 5, np.float32)
    obs, frame = Scene(data), Grid(FRAME_SHAPE)
    out = dict(data=data, scale=np.float64(SCALE), offset=np.float64(OFFSET),
               frame_shape=np.array(FRAME_SHAPE),
               interp=rinterp.interpolate_observation(obs, frame),
               interp_wave=rinterp.interpolate_observation(obs, frame, wave_filter=True))
    for tag, shape, dtype in (("a", (16, 16), np.float32), ("b", (21, 13), np.float64)):
        image = blobs(shape, 7 + len(out), dtype)
        out["denoise_img_" + tag] = image
        out["denoise_" + tag] = rwave.apply_wavelet_denoising(image)
    save_deterministic(OUT, out)
    print("interpolate_observation.npz: %d bytes, interp %s %s" %
          (os.path.getsize(OUT), out["interp"].shape, out["interp"].dtype))
    if not had_so and os.path.exists(so):  # built in the tree by the shims on first use
        os.remove(so)


if __name__ == "__main__":
    main()
