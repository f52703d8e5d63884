"""Hand-built blends for scarlet.render_blends: the catalogue of tests/measure_sources_cases.py --
``zero weight`` is a device case here -- and five more:

    alone        one source on a 25 x 31 frame of 2 bands, 5 x 5 stamp: its flux is the image
                 wherever its rendering is positive
    apart        two 5 x 5 boxes in opposite corners of a 33 x 37 frame, 5 x 5 stamp: no component
                 reaches the middle of the frame (MIDDLE), where every image is exactly zero; the
                 second box has a column of zeros, so its region has pixels where the scene is zero
    clamped      25 x 31 frame, the 11 x 11 difference kernel with negative lobes of ``lobes``: a
                 faint wide source under the lobe of a bright compact one, so that the ratio rules
                 meet R_k < 0, R_tot <= 0 and R_k > R_tot > 0
    stock        a PointSource and a GaussianSource next to an image component
    subset null  a NullRenderer of bands 1 and 2 of three; a pixel without weight

``catalogue()`` builds fresh objects on every call; an entry is ``(name, blend, expect)`` as in
measure_sources_cases."""

import numpy as np

import measure_sources_cases as mc
from init_blends_cases import scene

# rows and columns of ``apart`` no component reaches: the boxes grown by 2 end at 6 and begin at 26
# (rows), end at 6 and begin at 30 (columns)
MIDDLE = (slice(7, 26), slice(7, 30))


def catalogue():
    import scarlet_amd as scarlet

    out = [(name, blend, "device" if name == "zero weight" else expect)
           for name, blend, expect in mc.catalogue()]
    rng = np.random.RandomState(17)

    def add(name, frame, obs, sources):
        mc._weights(obs, rng)
        out.append((name, scarlet.Blend(sources, [obs]), "device"))

    frame, obs = scene(31, (2, 25, 31), (5, 5), [(12, 15, 2.0, 2.0)])
    add("alone", frame, obs, [mc.component(frame, rng, (6, 8, 13, 15))])

    frame, obs = scene(32, (2, 33, 37), (5, 5), [(2, 2, 2.0, 1.5), (30, 34, 1.0, 1.5)])
    edge = rng.uniform(0.05, 1.0, (5, 5))
    edge[:, 0] = 0  # (the first column of its region gets exact zeros only)
    add("apart", frame, obs, [mc.component(frame, rng, (0, 0, 5, 5)),
                              mc.component(frame, rng, (28, 32, 5, 5), image=edge)])

    frame, obs = scene(5, (3, 25, 31), (11, 11), [(12, 15, 3.0, 1.0)])
    bright = mc.component(frame, rng, (11, 14, 3, 3), image=50 * rng.uniform(0.5, 1.0, (3, 3)))
    faint = mc.component(frame, rng, (4, 6, 17, 19), image=rng.uniform(1e-3, 3e-3, (17, 19)))
    add("clamped", frame, obs, [bright, faint])

    # (one model PSF for all bands: a PointSource's morphology is then one image, not one per band)
    _, seen = scene(33, (3, 25, 31), (5, 5), [(8, 9, 3.0, 0.9), (15, 20, 2.0, 2.0)])
    frame = scarlet.Frame((3, 25, 31), psf=scarlet.GaussianPSF(sigma=0.8), channels=seen.channels)
    obs = scarlet.Observation(seen.data, psf=seen.psf, weights=seen.weights,
                              channels=seen.channels).match(frame)
    add("stock", frame, obs,
        [scarlet.PointSource(frame, (8, 9), obs),
         scarlet.GaussianSource(frame, (15, 20), 1.8, np.zeros(2), obs),
         mc.component(frame, rng, (10, 4, 9, 11))])

    channels = ["c0", "c1", "c2"]
    frame = scarlet.Frame((3, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 3), channels=channels)
    data = rng.normal(0, 0.1, (2, 25, 31)).astype(np.float32)
    obs = scarlet.Observation(data, psf=frame.psf, weights=np.full(data.shape, 100, np.float32),
                              channels=channels[1:]).match(frame)
    add("subset null", frame, obs, [mc.component(frame, rng, (4, 6, 11, 9)),
                                    mc.component(frame, rng, (-2, 20, 9, 14))])
    obs.weights[0, 5, 7] = 0
    return out


def device_cases(cat):
    return [(name, blend) for name, blend, expect in cat if expect == "device"]
