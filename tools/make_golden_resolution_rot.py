"""Golden vectors of ``ResolutionRenderer`` between rotated pixel grids:
``tests/golden/resolution_rotated.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present), run with the interpreter that
has astropy, the one ``oracle/refshim/conda_reference.py`` serves:

    python tools/make_golden_resolution_rot.py

The reference is imported through ``oracle/refshim/conda_reference.py``.  Its rotated branch
(renderer.py:319-363, 498-524) does ``np.array(mk_shifter(shape))`` on the pair of frequency
ramps, which have different lengths (``Fy`` and ``Fx / 2 + 1``): NumPy before 1.24 made a 1-D
object array of the two, NumPy from 1.24 on raises.  This tool therefore WRAPS
``scarlet.interpolation.mk_shifter`` so that it returns the same two arrays in a 1-D object
array -- what the old NumPy made of them; nothing else of the reference is touched.

The scenes are those of ``tests/resolution_rot_cases.py`` with ``astropy.wcs.WCS`` objects of the
same ``crpix``, ``crval`` and ``pc`` (TAN projection, the pixel scale in ``pc``, ``cdelt`` 1).
Per case the file holds the reference's set-up quantities (``angle``, ``h``, ``fft_shape``,
``shifts``, ``other_shifts``, ``diff_kernel.image``, the frame's shape and ``crpix``), the model
of ``cases.model`` and the reference's ``obs.render(model)``.  Data only, written without time
stamps.
"""

import io
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "refshim"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import conda_reference  # noqa: E402
import resolution_rot_cases as cases  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "resolution_rotated.npz")


def save_deterministic(path, arrays):
    """np.savez_compressed without the time stamps: the same inputs give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def astropy_wcs(crpix, crval, pc, shape):
    from astropy.wcs import WCS

    w = WCS(naxis=2)
    w.wcs.ctype = ["RA---TAN", "DEC--TAN"]
    w.wcs.crpix = crpix
    w.wcs.crval = crval
    w.wcs.pc = pc
    w.wcs.cdelt = [1.0, 1.0]
    w.array_shape = tuple(shape)
    return w


def main():
    scarlet = conda_reference.load()
    import scarlet.interpolation as rinterp

    plain = rinterp.mk_shifter

    def mk_shifter(shape, real=False):
        pair = plain(shape, real=real)
        out = np.empty(len(pair), dtype=object)
        for i, ramp in enumerate(pair):
            out[i] = ramp
        return out

    rinterp.mk_shifter = mk_shifter

    out = dict(cases=np.array(sorted(cases.CASES)))
    for name in sorted(cases.CASES):
        case = cases.CASES[name]
        obs = cases.observations(name, scarlet, astropy_wcs)
        frame = scarlet.Frame.from_observations(obs, coverage="union",
                                                model_psf=scarlet.GaussianPSF(sigma=0.8))
        obs_lr = obs[1]
        r = obs_lr.renderer
        assert type(r).__name__ == "ResolutionRenderer" and r.isrot and r.small_axis, name
        assert tuple(frame.shape) == tuple(case["frame"]), (name, frame.shape)
        assert tuple(r._fft_shape) == tuple(case["fft"]), (name, r._fft_shape)
        model = cases.model(name)
        rendered = obs_lr.render(model)
        out[name + "_angle"] = np.array([float(r.angle[0]), float(r.angle[1])])
        out[name + "_h"] = np.float64(r.h)
        out[name + "_fft_shape"] = np.array(r._fft_shape)
        out[name + "_frame_shape"] = np.array(frame.shape)
        out[name + "_frame_crpix"] = np.array(frame.wcs.wcs.crpix)
        out[name + "_shifts"] = np.asarray(r.shifts, dtype=np.float64)
        out[name + "_other_shifts"] = np.asarray(r.other_shifts, dtype=np.float64)
        out[name + "_kernel"] = np.asarray(r.diff_kernel.image)
        out[name + "_model"] = model
        out[name + "_rendered"] = np.asarray(rendered)
        print("%-5s frame %s fft %s angle %+.6f h %.4f rendered %s %s peak %.4g" % (
            name, tuple(frame.shape), tuple(r._fft_shape), float(r.angle[1]), float(r.h),
            rendered.shape, rendered.dtype, np.abs(rendered).max()))
    save_deterministic(OUT, out)
    print("resolution_rotated.npz: %d bytes" % os.path.getsize(OUT))


if __name__ == "__main__":
    main()
