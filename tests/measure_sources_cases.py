"""Hand-built blends for scarlet.measure_blends: the smallest shapes at which each step of
csrc/measure_sources.hip can still go wrong.  Nothing is initialised and no GPU is needed to
build them: every component is a FactorizedComponent of a TabulatedSpectrum (float32) and an
ImageMorphology with a positive random float64 image.

    tiny      9 x 11 frame of 3 bands, 5 x 5 stamp: smaller than a tile; boxes overhang the frame on
              all sides (negative origins); a 1 x 1 box; a NullSource
    tiles     25 x 31 frame of 1 band, rectangular 5 x 9 stamp: a 17 x 17 box (one pixel into a
              second tile both ways once grown and clipped), a 16 x 16 box, a 3 x 3 box whose grown
              box lies inside one tile
    null      33 x 37 frame, NullRenderer: the region is the box, so the 16 x 16 box at (0, 0) is
              exactly one tile and the 17 x 17 box has four; a tie for the brightest pixel across two
              bands and two pixels
    limit     33 x 37 frame, 63 x 63 stamp (a match_psf difference kernel with negative lobes): the
              window at its limit, the taps of every tile leave the frame
    lobes     25 x 31 frame, 11 x 11 difference kernel with negative lobes; a source of two
              components with different boxes; a nested CombinedComponent; a free psf_shift
    list map  an observation of bands 0 and 2 of a 3-band frame (list channel_map)
    slice map an observation of bands 1 and 2 (slice channel_map)
    six       a frame of 6 bands with two observations of 3 bands each

and one blend per reason the device path refuses.  ``catalogue()`` builds fresh objects on every
call; an entry is ``(name, blend, expect)`` with ``expect`` "device", "runtime" (the values send
it to the per-source functions) or the start of the reason ``plan_measure_blends`` gives."""

import numpy as np

from init_blends_cases import scene


def component(frame, rng, rect, sed=None, image=None):
    import scarlet_amd as scarlet

    y0, x0, h, w = rect
    C = frame.C
    box = scarlet.Box((C, h, w), origin=(0, y0, x0))
    sed = rng.uniform(0.5, 2.0, C).astype(np.float32) if sed is None else np.asarray(sed, np.float32)
    image = rng.uniform(0.05, 1.0, (h, w)) if image is None else np.asarray(image, np.float64)
    return scarlet.FactorizedComponent(
        frame, scarlet.TabulatedSpectrum(frame, sed, bbox=box[0]),
        scarlet.ImageMorphology(frame, image, bbox=box[1:]))


def _weights(obs, rng):
    """Positive weights that differ from pixel to pixel."""
    obs.weights = (obs.weights * rng.uniform(0.5, 1.5, obs.weights.shape)).astype(np.float32)
    return obs


def _blend(frame, observations, sources):
    import scarlet_amd as scarlet

    return scarlet.Blend(sources, observations)


def _subset(seed, shape, stamp, channels, frame):
    """An observation of the bands ``channels`` matched to ``frame``."""
    _, obs = scene(seed, (len(channels),) + tuple(shape[1:]), stamp, [])
    obs.channels = list(channels)
    return obs.match(frame)


def catalogue():
    import scarlet_amd as scarlet

    out = []
    rng = np.random.RandomState(11)

    def add(name, expect, frame, observations, sources):
        observations = observations if isinstance(observations, (list, tuple)) else [observations]
        for obs in observations:
            if type(obs.weights) is np.ndarray:
                _weights(obs, rng)
        out.append((name, _blend(frame, list(observations), sources), expect))

    frame, obs = scene(1, (3, 9, 11), (5, 5), [])
    add("tiny", "device", frame, obs,
        [component(frame, rng, (-2, -3, 13, 17)), component(frame, rng, (-1, 4, 5, 9)),
         scarlet.NullSource(frame), component(frame, rng, (4, 5, 1, 1)),
         component(frame, rng, (6, -2, 5, 6))])

    frame, obs = scene(2, (1, 25, 31), (5, 9), [])
    add("tiles", "device", frame, obs,
        [component(frame, rng, (3, 5, 17, 17)), component(frame, rng, (2, 4, 16, 16)),
         component(frame, rng, (12, 20, 3, 3)), component(frame, rng, (20, 25, 9, 9))])

    frame, obs = scene(3, (3, 33, 37), (11, 11), [], null=True)
    tie = rng.uniform(0.05, 0.9, (7, 9))
    tie[2, 3] = tie[5, 1] = 1.0
    add("null", "device", frame, obs,
        [component(frame, rng, (0, 0, 16, 16)), component(frame, rng, (8, 9, 17, 17)),
         component(frame, rng, (20, 25, 7, 9), sed=[1.0, 2.0, 2.0], image=tie)])

    frame, obs = scene(4, (2, 33, 37), (63, 63), [])
    add("limit", "device", frame, obs,
        [component(frame, rng, (9, 11, 15, 15)), component(frame, rng, (25, 30, 5, 5))])

    frame, obs = scene(5, (3, 25, 31), (11, 11), [])
    obs.match(frame, renderer=scarlet.ConvolutionRenderer(obs, frame, psf_shift=np.array([0.2, -0.3])))
    two = scarlet.CombinedComponent([component(frame, rng, (3, 4, 13, 15)),
                                     component(frame, rng, (5, 6, 7, 9))])
    nested = scarlet.CombinedComponent([
        scarlet.CombinedComponent([component(frame, rng, (10, 12, 9, 9)),
                                   component(frame, rng, (11, 13, 5, 6))]),
        component(frame, rng, (10, 14, 4, 7))])
    add("lobes", "device", frame, obs, [two, nested, component(frame, rng, (18, 22, 9, 11))])

    channels = ["c0", "c1", "c2"]
    frame = scarlet.Frame((3, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 3), channels=channels)
    add("list map", "device", frame, _subset(6, (3, 25, 31), (5, 5), ["c0", "c2"], frame),
        [component(frame, rng, (4, 6, 11, 9)), component(frame, rng, (15, 20, 7, 7))])
    frame = scarlet.Frame((3, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 3), channels=channels)
    add("slice map", "device", frame, _subset(7, (3, 25, 31), (5, 5), ["c1", "c2"], frame),
        [component(frame, rng, (4, 6, 11, 9))])

    channels = ["c%d" % c for c in range(6)]
    frame = scarlet.Frame((6, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 6), channels=channels)
    first = _subset(8, (3, 25, 31), (5, 5), channels[:3], frame)
    second = _subset(9, (3, 25, 31), (5, 5), channels[3:], frame)
    add("six", "device", frame, [first, second],
        [component(frame, rng, (4, 6, 11, 9)), component(frame, rng, (-3, 18, 12, 20))])

    # ---- one blend per reason the device path refuses
    def plain(seed, stamp=(5, 5)):
        frame, obs = scene(seed, (3, 25, 31), stamp, [])
        return frame, obs, [component(frame, rng, (4, 6, 11, 9)), component(frame, rng, (12, 14, 7, 7))]

    def wcs(scale, n):
        w = scarlet.LinearWCS(np.array([n / 2, n / 2]), np.zeros(2), np.eye(2) * scale, np.ones(2))
        w.array_shape = (n, n)
        return w

    frame = scarlet.Frame((2, 20, 20), psf=scarlet.GaussianPSF(sigma=(0.8,) * 2),
                          channels=["a", "b"], wcs=wcs(1e-4, 20))
    y, x = np.mgrid[:11, :11] - 5
    psf = np.repeat(np.exp(-(y * y + x * x) / (2 * 1.5 ** 2))[None], 2, axis=0).astype(np.float32)
    low = scarlet.Observation(rng.rand(2, 10, 10).astype(np.float32), psf=scarlet.ImagePSF(psf),
                              weights=np.full((2, 10, 10), 400, np.float32), channels=["a", "b"],
                              wcs=wcs(2e-4, 10)).match(frame)
    add("resolution", "renderer ResolutionRenderer", frame, low,
        [component(frame, rng, (4, 6, 9, 9))])

    class Doubling(scarlet.Renderer):
        """A user's renderer: twice the model."""

        def get_model(self, *parameters):
            return lambda model: 2 * self.map_channels(model)

    frame, obs, sources = plain(21)
    obs.match(frame, renderer=Doubling(obs, frame))
    add("user renderer", "renderer Doubling", frame, obs, sources)

    frame, obs, sources = plain(22)
    cube = scarlet.CubeComponent(frame, rng.uniform(0.1, 1, (3, 5, 5)),
                                 bbox=scarlet.Box((3, 5, 5), origin=(0, 8, 9)))
    add("cube", "CubeComponent", frame, obs, sources + [cube])

    frame, obs, sources = plain(23)
    add("multiply", "CombinedComponent('multiply')", frame, obs,
        [scarlet.CombinedComponent([sources[0], component(frame, rng, (6, 7, 5, 5))],
                                   operation="multiply")])

    frame, obs, sources = plain(24)
    add("zero weight", "a weight that is zero", frame, obs, sources)
    out[-1][1].observations[0].weights[1, 3, 4] = 0

    frame, obs, sources = plain(25, stamp=(6, 6))
    add("even stamp", "even difference-kernel stamp", frame, obs, sources)

    frame, obs, sources = plain(27)
    # (a Parameter refuses such a value when it is made: it turns up later, as in a fit gone wrong)
    bad = component(frame, rng, (2, 3, 7, 7))
    add("not finite", "runtime", frame, obs, sources + [bad])
    np.asarray(bad.children[1].parameters[0])[3, 3] = np.inf
    return out


def leaves_the_box():
    """A blend the plan refuses and no function can measure: ``CombinedComponent.get_model``
    cannot place a child that leaves the container's box (the first child's)."""
    import scarlet_amd as scarlet

    rng = np.random.RandomState(12)
    frame, obs = scene(26, (3, 25, 31), (5, 5), [])
    leaves = [component(frame, rng, (4, 6, 5, 5)), component(frame, rng, (3, 6, 5, 5))]
    return scarlet.Blend([scarlet.CombinedComponent(leaves)], [obs])


def device_cases(cat):
    return [(name, blend) for name, blend, expect in cat if expect == "device"]
