"""The reference's wavelet-model tutorial (docs/tutorials/wavelet_model.ipynb) through the
facade, from the committed fixture: wavelet detection, one ``ExtendedSource`` per peak, one
``StarletSource`` over the whole frame for the diffuse light, and the fit.

    python tools/wavelet_tutorial.py [iterations]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import scarlet_amd as scarlet  # noqa: E402
from scarlet_amd.detect_pybind11 import get_footprints  # noqa: E402


def build(with_starlet=True):
    """(blend, observation) of the tutorial scene, as the notebook builds it."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                             "golden", "lsbg.npz"))
    images, filters = g["images"], [str(c) for c in g["channels"]]
    model_frame = scarlet.Frame(images.shape, psf=scarlet.GaussianPSF(sigma=0.8), channels=filters)
    observation = scarlet.Observation(images, psf=scarlet.ImagePSF(g["psfs"].copy()),
                                      channels=filters).match(model_frame)
    detect_image = np.sum(images, axis=0)
    coeffs = scarlet.wavelet.starlet_transform(detect_image, scales=3)
    support = scarlet.wavelet.get_multiresolution_support(detect_image, coeffs, 0.1, K=3,
                                                          epsilon=1e-1, max_iter=20)
    detect = support * coeffs
    detect[detect < 0] = 0
    footprints = get_footprints(detect[1], min_separation=0, min_area=10, thresh=0)
    centers = [(peak.y, peak.x) for fp in footprints for peak in fp.peaks]
    sources, skipped = scarlet.initialization.init_all_sources(
        model_frame, centers, observation, max_components=1, min_snr=50, thresh=1,
        fallback=True, silent=True, set_spectra=False)
    if with_starlet:
        np.random.seed(0)
        sources.append(scarlet.StarletSource(model_frame))
    return scarlet.Blend(sources, observation), observation


if __name__ == "__main__":
    n_iter = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    t0 = time.time()
    blend, observation = build()
    t1 = time.time()
    n, logL = blend.fit(n_iter, e_rel=1e-6)
    t2 = time.time()
    coeffs = blend.sources[-1].children[1].parameters[0]
    print("frame %s, %d sources, starlet coefficients %s"
          % (tuple(blend.frame.shape), len(blend.sources), coeffs.shape))
    print("detection and initialisation %.2f s" % (t1 - t0))
    print("fit: %d iterations in %.2f s (%.1f ms per iteration), logL %.1f -> %.1f"
          % (n, t2 - t1, 1e3 * (t2 - t1) / n, -blend.loss[0], logL))
    print("non-zero coefficients per plane:", [int((p != 0).sum()) for p in np.asarray(coeffs)])
    plain, _ = build(with_starlet=False)
    t3 = time.time()
    n0, logL0 = plain.fit(n_iter, e_rel=1e-6)
    t4 = time.time()
    print("without the starlet source: %d iterations in %.2f s (%.1f ms per iteration), logL %.1f"
          % (n0, t4 - t3, 1e3 * (t4 - t3) / n0, logL0))
