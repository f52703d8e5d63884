"""Golden vectors of the detection chain: ``tests/golden/detect.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present):

    python tools/make_golden_detect.py

The reference is imported through ``oracle.refshim.load_reference``.  That module puts a
placeholder ``scarlet.detect_pybind11`` (no functions) into ``sys.modules`` unless one is
there already, so the pure-Python restatement ``tests/detect_oracle.py`` is registered first:
the reference's own ``detect`` / ``wavelet`` / ``lite`` code then runs on top of it.

Inputs are the reference's MIT-licensed sample data, reduced to the arrays used:
``hsc_cosmos_35`` through the committed fixture ``tests/golden/hsc_cosmos_35.npz`` (the lite
tests build their observation from it), and the bands of ``testdata_3_0`` with its mask.
``get_detect_wavelets`` reads ``variance`` only through ``median(sqrt(variance))``, so the
testdata variance is recorded as its two middle values (``tvar_lo``, ``tvar_hi``): half the
pixels at each gives the same median bit for bit.

Supports and detection masks are stored as packed bits; where a stage's output is ``M * w``
the tests combine the mask with coefficients that are checked bit for bit elsewhere.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import detect_oracle  # noqa: E402

sys.modules["scarlet.detect_pybind11"] = detect_oracle.as_module()
from oracle.refshim import load_reference  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "detect.npz")
TESTDATA = os.path.join(load_reference.REFERENCE, "data", "testdata_3_0.npz")


def save_deterministic(path, arrays):
    """np.savez_compressed without the time stamps: the same inputs give the same bytes"""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def packed(mask):
    return np.packbits(np.asarray(mask, dtype=bool).ravel())


def footprint_arrays(prefix, footprints, out):
    """bounds [n,4], masks concatenated, peaks (y, x, flux) with per-footprint starts"""
    out[prefix + "bounds"] = np.array([fp.bounds for fp in footprints], dtype=np.int32).reshape(-1, 4)
    out[prefix + "masks"] = packed(np.concatenate([fp.footprint.ravel() for fp in footprints])
                                   if footprints else np.zeros(0, bool))
    starts, yx, flux = [0], [], []
    for fp in footprints:
        for p in fp.peaks:
            yx.append((p.y, p.x))
            flux.append(p.flux)
        starts.append(len(yx))
    out[prefix + "peak_start"] = np.array(starts, dtype=np.int32)
    out[prefix + "peak_yx"] = np.array(yx, dtype=np.int32).reshape(-1, 2)
    out[prefix + "peak_flux"] = np.array(flux, dtype=np.float64)


def main():
    so = os.path.join(REPO, "oracle", "liboracle.so")
    had_so = os.path.exists(so)
    scarlet = load_reference.load()
    import scarlet.detect as rdetect
    import scarlet.wavelet as rwave
    from scarlet.lite import models as lm
    import importlib

    li = importlib.import_module("scarlet.lite.initialization")

    hsc = np.load(os.path.join(REPO, "tests", "golden", "hsc_cosmos_35.npz"))
    images = hsc["images"].astype(np.float32)
    weights = hsc["weights"].astype(np.float32)
    variance = (1 / weights).astype(np.float32)
    td = np.load(TESTDATA)
    timages = td["images"].astype(np.float32)
    tmask = td["footprint"].astype(bool)
    svar = np.sort(np.sqrt(td["variance"]).ravel())
    n = svar.size
    assert n % 2 == 0
    # the variance values whose square roots are the two middle order statistics
    flat = td["variance"].ravel()
    order = np.argsort(np.sqrt(flat), kind="stable")
    lo, hi = flat[order[n // 2 - 1]], flat[order[n // 2]]
    tvar = np.where(np.arange(n) < n // 2, lo, hi).astype(np.float32).reshape(td["variance"].shape)
    assert np.median(np.sqrt(tvar)) == np.median(np.sqrt(td["variance"]))

    out = dict(timages=timages, tmask=packed(tmask), tvar_lo=np.float32(lo), tvar_hi=np.float32(hi))

    # -- transforms: a non-square float32 crop and an odd-sized float64 crop -------------
    cases = {"a": images[2, 10:42, 4:44].copy(),                        # 32 x 40 float32
             "b": timages[1, 30:51, 50:77].astype(np.float64).copy()}   # 21 x 27 float64
    for tag, img in cases.items():
        out["img_" + tag] = img
        for gen in (1, 2):
            for scales in (None, 0, 1, 3, 5):
                key = "%s_g%d_s%s" % (tag, gen, "N" if scales is None else scales)
                coeffs = rwave.starlet_transform(img, scales=scales, generation=gen)
                out["w_" + key] = coeffs
                out["rec_" + key] = rwave.starlet_reconstruction(coeffs, generation=gen)
            st = rwave.Starlet.from_image(img, generation=gen)
            out["norm_%s_g%d" % (tag, gen)] = st.norm
    # -- multiresolution support of one band ---------------------------------------------
    band = images[2]
    coeffs = rwave.starlet_transform(band, scales=3)
    sigma = np.median(np.sqrt(variance[2]))
    out["support_hsc2_s3"] = packed(rwave.get_multiresolution_support(band, coeffs, sigma))
    # -- denoising ------------------------------------------------------------------------
    out["denoise_img"] = images[1, 13:45, 8:40].copy()
    out["denoise"] = rwave.apply_wavelet_denoising(out["denoise_img"])
    # -- detection coefficients ----------------------------------------------------------
    for scales in (3, 5):
        det = rdetect.get_detect_wavelets(images, variance, scales=scales)
        out["detect_mask_s%d" % scales] = packed(det != 0)
        out["detect_shape_s%d" % scales] = np.array(det.shape)
        wav = rdetect.get_wavelets(images, variance, scales=scales)
        out["wavelets_mask_s%d" % scales] = packed(wav != 0)
        out["wavelets_shape_s%d" % scales] = np.array(wav.shape)
    detect = rdetect.get_detect_wavelets(images, variance, scales=3)
    out["detect_s3"] = detect
    # -- footprints per scale and the structures -----------------------------------------
    for s, plane in enumerate(detect[:-1]):
        footprint_arrays("fp%d_" % s, detect_oracle.get_footprints(plane, 0, 4, 0), out)
    structures, middle_tree = rdetect.get_blend_structures(detect)
    out["n_structures"] = len(structures)
    for k, st in enumerate(structures):
        for scale in (0, 1, 2):
            out["struct%d_peaks%d" % (k, scale)] = np.array(
                [(p.y, p.x) for p in st.peaks.get(scale, [])], dtype=np.int32).reshape(-1, 2)
    query = list(middle_tree.query())
    out["middle_query_bounds"] = np.array([(b.origin[0], b.origin[1], b.shape[0], b.shape[1])
                                           for b in query], dtype=np.int32).reshape(-1, 4)
    centers = [(p.y, p.x) for box in middle_tree.query(scarlet.Box(images.shape)[1:])
               for p in box.footprint.peaks]
    out["lite_centers"] = np.array(centers, dtype=np.int32)
    # -- multiscale tutorial: peaks of detect * ~mask -------------------------------------
    tdetect = rdetect.get_detect_wavelets(timages, tvar, scales=5)
    out["tutorial_peaks"] = np.array(rdetect.get_peaks(tdetect * ~tmask[None]), dtype=np.int32)
    # -- lite.init_all_sources_wavelets on hsc_cosmos_35 ---------------------------------
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    obs = lm.LiteObservation(images, variance, weights, hsc["psfs"].astype(np.float32),
                             model_psf=model_psf[0][None], convolution_mode="fft")
    init_centers = [tuple(int(v) for v in c) for c in hsc["centers"]]
    sources = li.init_all_sources_wavelets(obs, init_centers, min_snr=50)
    out["init_centers"] = np.array(init_centers, dtype=np.int32)
    out["init_n_comp_of"] = np.array([len(s.components) for s in sources])
    for i, src in enumerate(sources):
        for j, c in enumerate(src.components):
            out["init_sed_%d_%d" % (i, j)] = np.array(c.sed)
            out["init_morph_%d_%d" % (i, j)] = np.array(c.morph)
            out["init_box_%d_%d" % (i, j)] = np.array(c.bbox.origin + c.bbox.shape)
    save_deterministic(OUT, out)
    print("detect.npz: %d bytes, %d structures, %d lite centres, components per source %s"
          % (os.path.getsize(OUT), len(structures), len(centers), list(out["init_n_comp_of"])))
    if not had_so and os.path.exists(so):  # built in the tree by the shims on first use
        os.remove(so)


if __name__ == "__main__":
    main()
