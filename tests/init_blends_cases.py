"""A ragged catalogue of small hand-made scenes for initialization.init_blends: the smallest
shapes at which each step of csrc/init_sources.hip can still go wrong.

    9 x 11    fewer pixels than a workgroup has threads; every box leaves the frame on all sides
    25 x 31   odd sides, a source on an edge, two sources within one box of each other
    32 x 32   even sides (the parity branch of the symmetry's centred range), a source on
              (h / 2, w / 2): the whole-array branch
    33 x 37   strided loops take a second, partial trip; NullRenderer
    64 x 48   more pixels than two trips of a workgroup; zero-weight pixels in a stamp and a source

``catalogue()`` builds fresh objects on every call (sources keep references to their frame and
observation).  Every entry is ``(name, frame, centers, observations, expect)`` with ``expect`` one
of "device", "refused" (the plan sends it to the loop) or "runtime" (its values do).  The option
sets the tests run the whole catalogue with are ``OPTIONS``."""

import numpy as np

OPTIONS = {
    # bright sources get two components, the faintest none (a compact source)
    "two": dict(thresh=0.5, max_components=2, min_components=0, min_snr=10),
    "box": dict(thresh=2, max_components=1, min_snr=50, boxsize=15),
    "plain": dict(),
}
SIGMA_NOISE = 0.05


def gaussian_stamps(C, ph, pw, s0=1.3):
    y, x = np.arange(ph) - ph // 2, np.arange(pw) - pw // 2
    return np.stack([np.exp(-(y[:, None] ** 2 + x[None, :] ** 2) / (2 * (s0 + 0.1 * c) ** 2))
                     for c in range(C)]).astype(np.float32)


def scene(seed, shape, stamp, sources, null=False, no_weight=(), faint=(), nan=()):
    """``(frame, observation)``: Gaussian blobs ``(y, x, flux, sigma)`` of a spectrum that rises
    with the band, noise of ``SIGMA_NOISE``, weights ``1 / SIGMA_NOISE**2`` except zero in the
    pixels ``no_weight``; the pixels ``faint`` hold a tenth of the noise in every band (a source
    there has nothing above the threshold), the pixels ``nan`` NaN."""
    import scarlet_amd as scarlet

    C, H, W = shape
    rng = np.random.RandomState(seed)
    channels = ["c%d" % c for c in range(C)]
    yy, xx = np.mgrid[:H, :W]
    data = rng.normal(0, SIGMA_NOISE, shape)
    for y, x, flux, sigma in sources:
        blob = np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * sigma ** 2))
        data += flux * (1 + 0.3 * np.arange(C))[:, None, None] * blob[None]
    for y, x in faint:
        data[:, y, x] = 0.1 * SIGMA_NOISE
    for y, x in nan:
        data[0, y, x] = np.nan
    data = data.astype(np.float32)
    weights = np.full(shape, 1 / SIGMA_NOISE ** 2, np.float32)
    for y, x in no_weight:
        weights[:, y, x] = 0
    if null:
        # one PSF object for both frames, a stamp per band: rendering is the identity
        psf = scarlet.GaussianPSF(sigma=tuple(0.8 + 0.1 * c for c in range(C)), boxsize=stamp[0])
        frame = scarlet.Frame(shape, psf=psf, channels=channels)
        obs = scarlet.Observation(data, psf=psf, weights=weights, channels=channels)
    else:
        frame = scarlet.Frame(shape, psf=scarlet.GaussianPSF(sigma=(0.8,) * C), channels=channels)
        obs = scarlet.Observation(data, psf=scarlet.ImagePSF(gaussian_stamps(C, *stamp)),
                                  weights=weights, channels=channels)
    return frame, obs.match(frame)


def catalogue():
    out = []

    def add(name, expect, centers, frame_obs, observations=None):
        frame, obs = frame_obs
        out.append((name, frame, [tuple(float(v) for v in c) for c in centers],
                    obs if observations is None else observations, expect))

    add("tiny", "device", [(0, 0), (4, 5)],
        scene(1, (3, 9, 11), (5, 5), [(0, 0, 3.0, 1.5), (4, 5, 1.2, 1.2)]))
    add("odd", "device", [(0, 15), (12, 14), (14, 17), (20, 5)],
        scene(2, (5, 25, 31), (11, 11), [(0, 15, 0.1, 1.5), (12, 14, 6.0, 2.0), (14, 17, 0.8, 1.2),
                                          (20, 5, 0.05, 1.0)]))
    add("even", "device", [(16, 16), (10, 20.4)],
        scene(3, (1, 32, 32), (11, 7), [(16, 16, 4.0, 2.5), (10, 20, 1.5, 1.5)]))
    add("null", "device", [(16, 18), (30, 3), (5, 30)],
        scene(4, (3, 33, 37), (11, 11), [(16, 18, 2.5, 2.0), (30, 3, 1.1, 1.4)], null=True,
              faint=[(5, 30)]))
    add("wide", "device", [(31, 24), (8, 40), (50, 10), (63, 47)],
        scene(5, (5, 64, 48), (11, 11), [(31, 24, 8.0, 3.0), (8, 40, 1.0, 1.5), (50, 10, 1.6, 2.0),
                                          (63, 47, 2.2, 1.5)],
              no_weight=[(31, 26), (32, 26), (9, 41), (0, 0)]))
    # two centres that round to one pixel: the identical-model screen of set_spectra_to_match
    add("twins", "device", [(12.2, 14.1), (11.9, 13.8), (5, 5)],
        scene(6, (3, 25, 31), (5, 5), [(12, 14, 2.0, 1.8), (5, 5, 1.3, 1.3)]))
    # two observations of three bands each on a frame of six
    import scarlet_amd as scarlet

    _, obs = scene(7, (3, 25, 31), (5, 5), [(12, 14, 2.0, 1.8)])
    _, other = scene(8, (3, 25, 31), (5, 5), [(12, 14, 2.0, 1.8)])
    other.channels = ["c3", "c4", "c5"]
    frame = scarlet.Frame((6, 25, 31), psf=scarlet.GaussianPSF(sigma=(0.8,) * 6),
                          channels=["c%d" % c for c in range(6)])
    add("two observations", "refused", [(12, 14)], (frame, obs.match(frame)),
        observations=(obs, other.match(frame)))
    add("even stamp", "refused", [(12, 14)], scene(9, (3, 25, 31), (6, 6), [(12, 14, 2.0, 1.8)]))
    add("off the frame", "refused", [(12, 14), (-3, 5)],
        scene(10, (3, 25, 31), (5, 5), [(12, 14, 2.0, 1.8)]))
    add("nan", "runtime", [(12, 14), (5, 5)],
        scene(11, (3, 25, 31), (5, 5), [(12, 14, 2.0, 1.8), (5, 5, 1.3, 1.3)], nan=[(13, 14)]))
    return out


def snr_ratio(frame, center, observations, min_snr):
    """``snr / min_snr`` of ``init_source`` at ``center``, in float64 on the host."""
    obs = observations[0] if isinstance(observations, tuple) else observations
    index = np.round(obs.get_pixel(center)).astype("int")
    psf = np.asarray(obs.psf.get_model(), np.float64)
    bbox = obs.psf.bbox + (0, *index)
    img = bbox.extract_from(obs.data).astype(np.float64)
    var = bbox.extract_from(np.where(obs.weights > 0, 1 / np.maximum(obs.weights, 1e-30), 0))
    ok = ~bbox.extract_from(obs.weights == 0)
    num = sum(float(img[c][ok[c]] @ psf[c][ok[c]]) for c in range(obs.C))
    den = sum(float((psf[c][ok[c]] * var[c][ok[c]].astype(np.float64)) @ psf[c][ok[c]])
              for c in range(obs.C))
    return num / np.sqrt(den) / min_snr


def same_sources(a, b, spectra="equal", bound=None):
    """Assert that two results ``(sources, skipped)`` of one blend are the same: classes,
    ``skipped``, boxes, centres, step rules, flags, constraint chains, morphologies bit for bit;
    the spectra bit for bit (``spectra="equal"``) or not compared (None)."""
    from numpy.testing import assert_array_equal

    import scarlet_amd as scarlet

    (sa, ka), (sb, kb) = a, b
    assert list(ka) == list(kb)
    assert [type(s) for s in sa] == [type(s) for s in sb]
    for s, t in zip(sa, sb):
        assert_array_equal(np.asarray(s.center), np.asarray(t.center))
        cs = s.children if isinstance(s, scarlet.CombinedComponent) else [s]
        ct = t.children if isinstance(t, scarlet.CombinedComponent) else [t]
        assert len(cs) == len(ct)
        for c, d in zip(cs, ct):
            (spec_c, morph_c), (spec_d, morph_d) = c.children, d.children
            assert morph_c.bbox == morph_d.bbox and spec_c.bbox == spec_d.bbox
            assert c.bbox == d.bbox
            assert (morph_c.shifting, morph_c.resizing) == (morph_d.shifting, morph_d.resizing)
            assert_array_equal(morph_c.pixel_center, morph_d.pixel_center)
            assert (morph_c.shift is None) == (morph_d.shift is None)
            pc, pd = morph_c.parameters[0], morph_d.parameters[0]
            assert pc.dtype == pd.dtype == np.float64
            assert_array_equal(np.asarray(pc), np.asarray(pd))
            assert pc.step == pd.step and pc.fixed == pd.fixed
            assert ([type(k) for k in pc.constraint.constraints]
                    == [type(k) for k in pd.constraint.constraints])
            qc, qd = spec_c.parameters[0], spec_d.parameters[0]
            assert qc.dtype == qd.dtype
            assert qc.step.func is qd.step.func and qc.step.keywords["factor"] == qd.step.keywords["factor"]
            assert_array_equal(qc.step.keywords["minimum"], qd.step.keywords["minimum"])
            assert type(qc.constraint) is type(qd.constraint)
            if spectra == "equal":
                assert_array_equal(np.asarray(qc), np.asarray(qd))


#: the blends whose spectra the loop has to make (``set_spectra=True`` only): the twins' models
#: are identical
SPECTRA_RUNTIME = ("twins",)


def hand_components(frame, centers, seed=0):
    """One FactorizedComponent per centre with a unit float32 spectrum and an elliptical
    Gaussian morphology in a 15 x 15 box on the rounded pixel (boxes leave small frames)."""
    import scarlet_amd as scarlet

    rng = np.random.RandomState(seed)
    C = frame.C
    comps = []
    y, x = np.mgrid[:15, :15] - 7
    for center in centers:
        py, px = np.round(frame.get_pixel(center)).astype(int)
        sy, sx = rng.uniform(1.0, 3.0, 2)
        morph = np.exp(-(y ** 2) / (2 * sy ** 2) - (x ** 2) / (2 * sx ** 2))
        box = scarlet.Box((C, 15, 15), origin=(0, int(py) - 7, int(px) - 7))
        comps.append(scarlet.FactorizedComponent(
            frame, scarlet.TabulatedSpectrum(frame, np.ones(C, dtype=np.float32), bbox=box[0]),
            scarlet.ImageMorphology(frame, morph.astype(np.float64), bbox=box[1:])))
    return comps


def spectra_of(components):
    return [np.array(c.children[0].parameters[0]) for c in components]


def normal_equations(sp, b, data, weights, dtype=np.float64):
    """NumPy restatement of the spectra launches for blend ``b`` of the tables of
    ``initialization.pack_spectra``: per band the columns -- the morphology, zero outside its box
    and outside the frame, convolved "same" with the band's stamp by direct taps -- and from them
    ``(bands, K K + 3 K)``: G = A^T W A, r = A^T W d, sum a w and sum a over the region."""
    bl = sp["blends"][b]
    H, W, C, kh, kw, K = (int(bl[f]) for f in ("h", "w", "bands", "kh", "kw", "n_comp"))
    morphs = np.concatenate([m.reshape(-1) for m in sp["morphs"]])
    stamps = np.concatenate([s.reshape(-1) for s in sp["stamps"]])
    stamps = stamps[bl["stamp_off"]:bl["stamp_off"] + C * kh * kw].reshape(C, kh, kw).astype(dtype)
    cols = np.zeros((K, C, H, W), dtype)
    for j in range(K):
        d = sp["components"][bl["comp0"] + j]
        y0, x0, h, w = (int(d[f]) for f in ("y0", "x0", "h", "w"))
        m = morphs[d["morph_off"]:d["morph_off"] + h * w].reshape(h, w)
        padded = np.zeros((H + kh - 1, W + kw - 1), dtype)
        ys, ye, xs, xe = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        padded[kh // 2 + ys:kh // 2 + ye, kw // 2 + xs:kw // 2 + xe] = m[ys - y0:ye - y0, xs - x0:xe - x0]
        for c in range(C):
            for ky in range(kh):
                for kx in range(kw):
                    cols[j, c] += stamps[c, ky, kx] * padded[kh - 1 - ky:kh - 1 - ky + H,
                                                             kw - 1 - kx:kw - 1 - kx + W]
    ry, rx = slice(bl["y0"], bl["y0"] + bl["fh"]), slice(bl["x0"], bl["x0"] + bl["fw"])
    outside = np.ones((H, W), bool)
    outside[ry, rx] = False
    assert not cols[:, :, outside].any()  # the region holds all the convolved models reach
    out = np.zeros((C, K * K + 3 * K), dtype)
    for c in range(C):
        a = cols[:, c, ry, rx].reshape(K, -1)
        w_ = weights[c][ry, rx].reshape(-1).astype(dtype)
        d_ = data[c][ry, rx].reshape(-1).astype(dtype)
        aw = a * w_
        out[c] = np.concatenate([(aw @ a.T).reshape(-1), aw @ d_, aw.sum(axis=1), a.sum(axis=1)])
    return out


def longdouble_spectra(sp, b, data, weights):
    """The normal-equation solution of blend ``b`` in ``np.longdouble`` with direct convolution:
    ``(K, bands)`` and the ``seen`` ratios ``(bands, K)``."""
    sums = normal_equations(sp, b, data, weights, np.longdouble)
    C, K = sums.shape[0], int(sp["blends"][b]["n_comp"])
    spectra, ratios = np.zeros((K, C), np.longdouble), np.zeros((C, K), np.longdouble)
    for c in range(C):
        G, rest = sums[c, :K * K].reshape(K, K), sums[c, K * K:].reshape(3, K)
        ratios[c] = rest[1] / rest[2] / np.mean(weights[c].astype(np.longdouble))
        seen = np.flatnonzero(ratios[c] > 0.1)
        A, rhs = G[np.ix_(seen, seen)].copy(), rest[0][seen].copy()
        n = len(seen)
        for i in range(n):  # Gaussian elimination with partial pivoting, in longdouble
            piv = i + int(np.argmax(np.abs(A[i:, i])))
            A[[i, piv]], rhs[[i, piv]] = A[[piv, i]], rhs[[piv, i]]
            for r in range(i + 1, n):
                f = A[r, i] / A[i, i]
                A[r, i:] -= f * A[i, i:]
                rhs[r] -= f * rhs[i]
        x = np.zeros(n, np.longdouble)
        for i in range(n - 1, -1, -1):
            x[i] = (rhs[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
        spectra[seen, c] = x
    return spectra, ratios


def constrained(components, values):
    """``values`` (K, bands) after each spectrum parameter's own constraint, as
    ``set_spectra_to_match`` ends."""
    out = np.array(values)
    for row, comp in zip(out, components):
        p = comp.children[0].parameters[0]
        if p.constraint is not None:
            row[:] = p.constraint(row.copy(), 0)
    return out


def spectra_distance(values, truth):
    """Largest distance of the ``(K, bands)`` ``values`` from ``truth``, relative to each
    component's largest band."""
    truth = np.asarray(truth, np.longdouble)
    scale = np.abs(truth).max(axis=1, keepdims=True)
    return float((np.abs(np.asarray(values, np.longdouble) - truth) / scale).max())
