"""Oracle of the starlet source model: ``oracle.pgm`` extended by subclassing.

TEST INFRASTRUCTURE ONLY.  ``StarletComponent`` is a ``pgm.Component`` whose ``morph`` holds the
``(planes, h, w)`` starlet coefficients (reference morphology.py:516-604): the model uses their
generation-2 reconstruction (wavelet.py:284-311), the proximal operator is positivity followed
by a hard threshold per plane, and the gradient of the coefficients is the closed-form cascade
of B-spline passes (the reconstruction is linear and every pass symmetric).  ``StarletScene``
adds that cascade to ``pgm.Scene.parameter_gradients`` and the shrink rule of
``StarletMorphology.update`` to the 10-iteration hook of ``fit``.  Everything is float64 NumPy.
"""

import numpy as np

from oracle import pgm

TAPS = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])


def bspline(image, j):
    """B_j: the separable 5-tap B-spline at spacing 2**j; taps that fall outside the image
    are dropped (wavelet.py:154-191)."""
    d = 2 ** j

    def along(x, axis):
        n = x.shape[axis]
        out = x * TAPS[2]
        for tap, shift in ((TAPS[0], -2 * d), (TAPS[1], -d), (TAPS[3], d), (TAPS[4], 2 * d)):
            if abs(shift) >= n:
                continue
            dst, src = [slice(None)] * 2, [slice(None)] * 2
            if shift < 0:
                dst[axis], src[axis] = slice(-shift, None), slice(None, n + shift)
            else:
                dst[axis], src[axis] = slice(None, n - shift), slice(shift, None)
            out[tuple(dst)] += x[tuple(src)] * tap
        return out

    return along(along(np.asarray(image, dtype=np.float64), 0), 1)


def reconstruct(coeffs):
    """c = coeffs[S]; c = B_j c + coeffs[j] for j = S-1 .. 0."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    c = coeffs[-1]
    for j in range(len(coeffs) - 2, -1, -1):
        c = bspline(c, j) + coeffs[j]
    return c


def cascade(g, scales):
    """Gradient w.r.t. the coefficients from the gradient ``g`` w.r.t. the image:
    a_0 = g, a_{j+1} = B_j a_j; plane j < S gets a_j, the last plane a_S."""
    a = np.asarray(g, dtype=np.float64)
    out = [a]
    for j in range(scales):
        a = bspline(a, j)
        out.append(a)
    return np.stack(out)


def transform(image, scales):
    """Generation-2 starlet transform (wavelet.py:220-266), float64."""
    c = np.asarray(image, dtype=np.float64)
    out = np.zeros((scales + 1,) + c.shape)
    for j in range(scales):
        smooth = bspline(c, j)
        out[j] = c - bspline(smooth, j)
        c = smooth
    out[-1] = c
    return out


def get_scales(shape):
    return int(np.log2(min(shape[-2:]))) - 1


def norm(shape):
    """``Starlet.norm``: per-plane 2-norm of the transform of a centred Dirac."""
    dirac = np.zeros(shape)
    dirac[shape[0] // 2, shape[1] // 2] = 1
    return np.sqrt(np.sum(transform(dirac, get_scales(shape)) ** 2, axis=(-2, -1)))


def thresholds(shape, threshold):
    t = threshold * norm(shape)
    t[-1] = 0
    return t


class StarletComponent(pgm.Component):
    """``morph`` = coefficients (planes, h, w); ``thresh`` = absolute threshold per plane."""

    def __init__(self, sed, coeffs, origin, thresh, floor=0.0, sed_rel_step=1e-2,
                 coeffs_step=1e-2, **kw):
        kw.setdefault("monotonic", None)
        super().__init__(sed, coeffs, origin, morph_step=coeffs_step, **kw)
        self.thresh = np.asarray(thresh, dtype=np.float64)
        assert self.thresh.shape == (coeffs.shape[0],)
        self.floor = floor
        self.sed_rel_step = sed_rel_step

    def model_morph(self):
        return reconstruct(self.morph)

    def sed_step(self, it=0):
        return np.maximum(self.sed_min_step, self.sed_rel_step * self.sed.mean())

    def morph_prox(self, x, step):
        # (what the last proximal evaluation was given: the tests' "pre-threshold value")
        self.last_pre = np.array(x, dtype=np.float64)
        x = np.maximum(x, self.floor)
        x[np.abs(x) < self.thresh[:, None, None].astype(x.dtype)] = 0
        return x


def shrink_component(c, thresh=1e-8):
    """``StarletMorphology.update`` (morphology.py:572-604) on a StarletComponent: shrink
    only, by ``shrink_box(get_model(), thresh)``; coefficients and moments are sliced, planes
    and step kept.  True if the box changed."""
    if c.fixed[1]:
        return False
    image = c.model_morph()
    size = max(image.shape)
    dist = 0
    while (dist < (min(image.shape) + 1) // 2
           and np.all(image[dist, :] <= thresh) and np.all(image[-dist - 1, :] <= thresh)
           and np.all(image[:, dist] <= thresh) and np.all(image[:, -dist - 1] <= thresh)):
        dist += 1
    newsize = pgm.get_minimal_boxsize(size - 2 * dist)
    if newsize >= size:
        return False
    d = (size - newsize) // 2
    sl = (slice(None), slice(d, d + newsize), slice(d, d + newsize))
    c.origin = (c.origin[0] + d, c.origin[1] + d)
    c.morph = c.morph[sl].copy()
    c.m_morph, c.v_morph, c.vhat_morph = c.m_morph[sl].copy(), c.v_morph[sl].copy(), c.vhat_morph[sl].copy()
    return True


class StarletScene(pgm.Scene):
    def parameter_gradients(self, G):
        out = super().parameter_gradients(G)
        for k, c in enumerate(self.components):
            if isinstance(c, StarletComponent):
                g_sed, g_image = out[k]
                out[k] = (g_sed, cascade(g_image, c.morph.shape[0] - 1))
        return out

    def fit(self, max_iter=200, e_rel=1e-3, min_iter=1, prox_max_iter=10, resizing=False,
            b1=0.9, b2=0.999, eps=1e-8):
        """``pgm.Scene.fit`` with the hook of a starlet component at the resize hook."""
        it = 0
        while it < max_iter:
            local = 0
            restart = False
            while it + local < max_iter:
                self.step(local, e_rel, prox_max_iter, b1, b2, eps)
                self.check_parameters()
                if resizing and local > 0 and local % 10 == 0:
                    for group in self._groups():
                        for c in group:
                            if isinstance(c, pgm.PointComponent) or not getattr(c, "resizing", True):
                                continue
                            hook = shrink_component if isinstance(c, StarletComponent) \
                                else pgm.resize_component
                            if hook(c):
                                restart = True
                                break
                    if restart:
                        break
                if local > min_iter and abs(self.loss[-1] - self.loss[-2]) < e_rel * abs(
                        self.loss[-1]):
                    return len(self.loss), -self.loss[-1]
                local += 1
            if not restart:
                break
            it = len(self.loss)
        return len(self.loss), -self.loss[-1]


def fixture_scene(g, hsc, dtype64=False, state_dtype=np.float64):
    """``StarletScene`` of ``tests/golden/starlet_source.npz`` (``g``) on the observation of
    the ``hsc_cosmos_35`` fixture (``hsc``): ``init_all_sources(max_components=1)``, sources 0
    and 2 as starlet sources, the full-frame random starlet source last."""
    def value(name, k):
        key = "%s64_%d" % (name, k)
        return g[key if dtype64 and key in g.files else "%s_%d" % (name, k)].copy()

    starlet = set(int(k) for k in g["starlet_of"])
    comps = []
    for k in range(int(g["n_sources"])):
        common = dict(sed_min_step=g["sed_step_minimum_%d" % k],
                      sed_zero=float(g["sed_zero_%d" % k]), state_dtype=state_dtype)
        if k in starlet:
            comps.append(StarletComponent(
                value("sed", k), value("coeffs", k), g["origin_%d" % k], g["thresh_%d" % k],
                sed_rel_step=float(g["sed_step_factor_%d" % k]), **common))
        else:
            comps.append(pgm.Component(value("sed", k), value("morph", k), g["origin_%d" % k],
                                       **common))
    dt = np.float64 if dtype64 else np.float32
    images = hsc["images"].astype(dt)
    weights, kernel = hsc["weights"].astype(dt), hsc["diff_kernel"].astype(dt)
    if dtype64:  # the float64 frame's own observation
        kernel = g["diff_kernel64"]
        weights = g["weights64"] if "weights64" in g.files else weights
    return StarletScene(images.shape, images, weights, kernel, comps, dtype=dt)
