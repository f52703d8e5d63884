"""scarlet.lite's wavelet initialisation on the GPU detection chain against the reference's
run on hsc_cosmos_35 (tests/golden/detect.npz), and a fit started from it."""

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def _observation(hsc):
    import scarlet_amd as scarlet
    from scarlet_amd import lite

    images = hsc["images"].astype(np.float32)
    weights = hsc["weights"].astype(np.float32)
    variance = (1 / weights).astype(np.float32)
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * 5).get_model().astype(np.float32)
    return lite.LiteObservation(images, variance, weights, hsc["psfs"].astype(np.float32),
                                model_psf=model_psf[0][None])


def test_init_all_sources_wavelets_matches_the_reference_and_fits(hsc):
    from scarlet_amd import lite

    g = golden("detect")
    obs = _observation(hsc)
    centers = [tuple(int(v) for v in c) for c in g["init_centers"]]
    sources = lite.init_all_sources_wavelets(obs, centers, min_snr=50)
    assert [len(s.components) for s in sources] == list(g["init_n_comp_of"])
    for i, src in enumerate(sources):
        for j, c in enumerate(src.components):
            assert tuple(c.bbox.origin) + tuple(c.bbox.shape) == \
                tuple(g["init_box_%d_%d" % (i, j)]), (i, j)
            ref = g["init_morph_%d_%d" % (i, j)]
            assert c.morph.shape == ref.shape
            assert np.abs(c.morph - ref).max() < 1e-5, (i, j)
            ref = g["init_sed_%d_%d" % (i, j)]
            assert np.abs(c.sed - ref).max() <= 1e-5 * np.abs(ref).max(), (i, j)
    blend = lite.LiteBlend(lite.parameterize_sources(sources, obs, lite.init_adaprox_component),
                           obs)
    blend.fit(20, e_rel=1e-9)
    loss = np.array(blend.loss)
    assert len(loss) >= 2 and np.all(np.isfinite(loss))
    # the loss here is the log-likelihood: the fit improves it (the first adaprox steps
    # overshoot and oscillate, as in test_lite_init_all_sources_main_matches_the_reference)
    # and settles: the last steps move it by little against the improvement
    assert loss[-1] > loss[0]
    assert np.abs(np.diff(loss[-4:])).max() < 0.02 * (loss[-1] - loss[0])


def test_lite_tutorial_chain_gives_the_reference_centres(hsc):
    from scarlet_amd import detect

    g = golden("detect")
    obs = _observation(hsc)
    det = detect.get_detect_wavelets(obs.images, obs.variance, scales=3)
    _, middle_tree = detect.get_blend_structures(det)
    centers = [(peak.y, peak.x) for box in middle_tree.query(obs.bbox[1:])
               for peak in box.footprint.peaks]
    assert centers == [tuple(v) for v in g["lite_centers"].tolist()]
