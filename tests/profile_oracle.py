"""Oracle of the profile sources (GaussianSource, SpergelSource): ``oracle.pgm`` extended by
subclassing.

TEST INFRASTRUCTURE ONLY.  ``ProfileComponent`` is a ``pgm.Component`` whose morphology is the
closed-form profile of six float64 numbers ``params = (cy, cx, radius, e1, e2, nu)`` (reference
morphology.py:210-473) on a square box; ``ProfileScene`` adds the hand-written gradient of those
numbers to ``pgm.Scene.parameter_gradients``, their AMSGrad / proximal updates -- four
``Parameter``s: centre, radius, ellipticity, nu -- to ``step`` and the box rule of
``ProfileMorphology.update`` to the 10-iteration hook of ``fit``.  Everything is float64 NumPy
with scipy's ``kv``, ``gamma`` and ``digamma``.

The gradient w.r.t. ``nu`` follows the reference's fit, not calculus: autograd is told that
``kv`` has no derivative w.r.t. its order (morphology.py:380-381), so only the paths through
``(u/2)^nu``, ``Gamma(nu + 1)`` and ``c_nu`` remain.
"""

import numpy as np
from scipy.special import digamma, gamma, kv

from oracle import pgm

GAUSSIAN, SPERGEL = 0, 1
GROUPS = ("center", "radius", "ellipticity", "nu")
SLOTS = (slice(0, 2), slice(2, 3), slice(3, 5), slice(5, 6))
Z = np.array([-0.00788962, 0.0735303, -0.27770785, 0.99483285, 1.25227402])


def cnu(nu):
    return Z[0] * nu ** 4 + Z[1] * nu ** 3 + Z[2] * nu ** 2 + Z[3] * nu + Z[4]


def dcnu(nu):
    return 4 * Z[0] * nu ** 3 + 3 * Z[1] * nu ** 2 + 2 * Z[2] * nu + Z[3]


def radial(kind, R2, nu, partials=True):
    """``f(R2)``, ``df/dR2`` and ``df/dnu`` (the fit's rule) at fixed ``R2``."""
    if kind == GAUSSIAN:
        f = np.exp(-R2 / 2)
        return f, -0.5 * f, np.zeros_like(f)
    c = cnu(nu)
    rho = np.sqrt(R2 + 1e-4)
    u = rho * c
    pref = (u / 2) ** nu / gamma(nu + 1)
    f = pref * kv(nu, u)
    if not partials:
        return f, None, None
    df_du = nu / u * f - pref * (kv(nu - 1, u) + kv(nu + 1, u)) / 2
    df_dnu = f * (np.log(u / 2) - digamma(nu + 1)) + df_du * rho * dcnu(nu)
    return f, df_du * c / (2 * rho), df_dnu


def evaluate(kind, params, Y, X, partials=True):
    """The profile on the grid ``Y[:, None], X[None, :]`` (frame pixels) and its six partials
    ``(6, h, w)`` in the order of ``params``."""
    cy, cx, r, e1, e2, nu = (float(p) for p in params)
    y = (np.asarray(Y, dtype=np.float64) - cy)[:, None]
    x = (np.asarray(X, dtype=np.float64) - cx)[None, :]
    s = 1 / np.sqrt(1 - (e1 ** 2 + e2 ** 2))
    Xp = ((1 - e1) * x - e2 * y) * s
    Yp = (-e2 * x + (1 + e1) * y) * s
    R2 = (Yp ** 2 + Xp ** 2) / r ** 2
    f, fR, fnu = radial(kind, R2, nu, partials)
    if not partials:
        return f, None
    dR_dx = 2 * (Xp * s * (1 - e1) - Yp * s * e2) / r ** 2
    dR_dy = 2 * (-Xp * s * e2 + Yp * s * (1 + e1)) / r ** 2
    dXp1, dYp1 = e1 * s ** 2 * Xp - s * x, e1 * s ** 2 * Yp + s * y
    dXp2, dYp2 = e2 * s ** 2 * Xp - s * y, e2 * s ** 2 * Yp - s * x
    d = np.stack([
        -fR * dR_dy,
        -fR * dR_dx,
        fR * (-2 * R2 / r),
        fR * 2 * (Xp * dXp1 + Yp * dYp1) / r ** 2,
        fR * 2 * (Xp * dXp2 + Yp * dYp2) / r ** 2,
        fnu + np.zeros_like(f),
    ])
    return f, d


def prox(group, x):
    """The proximal operators of morphology.py:319-326, 472-473 (none on the centre)."""
    if group == 1:
        return np.maximum(x, 1e-2)
    if group == 2:
        norm2 = (x ** 2).sum()
        return x / (np.sqrt(norm2) * 1.1) if norm2 > 1 else x
    if group == 3:
        return np.maximum(np.minimum(4.0, x), -0.85)
    return x


def get_box(params):
    """``ProfileMorphology.get_box`` (morphology.py:302-317): (origin y, x, side)."""
    side = pgm.get_minimal_boxsize(10 * float(params[2]))
    return (int(round(float(params[0]))) - side // 2, int(round(float(params[1]))) - side // 2, side)


class ProfileComponent(pgm.Component):
    """``params`` the six doubles; ``size`` the side of the box, centred on ``round(centre)``
    unless ``origin`` is given; ``step`` / ``rel_step`` per group (``rel_step`` > 0:
    ``relative_step``, parameter.py:126-129); ``fixed_groups`` a bit mask."""

    def __init__(self, sed, kind, params, size, origin=None, step=(0.01, 0.0, 0.01, 0.01),
                 rel_step=(0.0, 0.1, 0.0, 0.0), fixed_groups=0, sed_rel_step=1e-2, **kw):
        self.kind = kind
        self.params = np.array(params, dtype=np.float64)
        self.size = int(size)
        if origin is None:
            origin = tuple(int(round(float(c))) - self.size // 2 for c in self.params[:2])
        self.steps, self.rel_steps = np.array(step, dtype=float), np.array(rel_step, dtype=float)
        self.fixed_groups = fixed_groups | (0 if kind == SPERGEL else 8)
        self.m_p, self.v_p, self.vhat_p = np.zeros(6), np.zeros(6), np.zeros(6)
        self.g_params = np.zeros(6)
        self.sed_rel_step = sed_rel_step
        self._cache = None
        kw.setdefault("monotonic", None)
        # (a unit step on a zero gradient: pgm.Scene.step leaves the derived image as it is)
        super().__init__(sed, np.zeros((self.size, self.size)), origin, morph_step=1.0, **kw)

    # the image is derived from the parameters; pgm.Component assigns it once (ignored)
    @property
    def morph(self):
        key = (self.params.tobytes(), self.origin, self.size)
        if self._cache is None or self._cache[0] != key:
            self._cache = (key,) + evaluate(self.kind, self.params, *self.grid())
        return self._cache[1]

    @morph.setter
    def morph(self, value):
        pass

    @property
    def partials(self):
        self.morph
        return self._cache[2]

    def grid(self):
        return (np.arange(self.size) + self.origin[0], np.arange(self.size) + self.origin[1])

    def model_morph(self):
        return self.morph

    def sed_step(self, it=0):
        return np.maximum(self.sed_min_step, self.sed_rel_step * self.sed.mean())

    def morph_prox(self, x, step):
        return x

    def group_step(self, g):
        if self.rel_steps[g]:
            return max(self.steps[g], self.rel_steps[g] * float(np.mean(self.params[SLOTS[g]])))
        return self.steps[g]

    def update_params(self, it, e_rel, prox_max_iter, b1, b2, eps):
        """Each group is a Parameter of its own (blend.py:120-145): steps on the pre-update
        values, a zero gradient for a fixed one (blend.py:107-115)."""
        alphas = [self.group_step(g) for g in range(4)]
        for g in range(4 if self.kind == SPERGEL else 3):
            sl = SLOTS[g]
            fixed = bool(self.fixed_groups >> g & 1)
            grad = np.zeros(sl.stop - sl.start) if fixed else self.g_params[sl]
            if fixed and alphas[g] == 0:
                # Parameter(fixed=True, step=None): no motion; the constraint still acts
                pgm.amsgrad_phi_psi(it, grad, self.m_p[sl], self.v_p[sl], self.vhat_p[sl], b1, b2, eps)
                self.params[sl] = prox(g, self.params[sl])
                continue
            pgm.adaprox_update(it, self.params[sl], grad, self.m_p[sl], self.v_p[sl],
                               self.vhat_p[sl], alphas[g], None if g == 0 else (
                                   lambda x, step, g=g: prox(g, x)),
                               e_rel, prox_max_iter, b1, b2, eps)

    def update_box(self):
        """``ProfileMorphology.update`` (morphology.py:288-300); True if the box changed."""
        oy, ox, side = get_box(self.params)
        if (oy, ox, side) == (self.origin[0], self.origin[1], self.size):
            return False
        self.origin, self.size = (oy, ox), side
        self.m_morph = self.v_morph = self.vhat_morph = np.zeros((side, side))
        return True


class ProfileScene(pgm.Scene):
    def parameter_gradients(self, G):
        out = super().parameter_gradients(G)
        for k, c in enumerate(self.components):
            if isinstance(c, ProfileComponent):
                g_sed, g_image = out[k]
                c.g_params = np.einsum("yx,pyx->p", g_image, c.partials)
                out[k] = (g_sed, np.zeros_like(g_image))
        return out

    def profile_gradients(self):
        """``(g_sed, g_params)`` of every profile component at the current parameters."""
        _, grads = self.loss_and_gradients()
        self.loss.pop()
        return {k: (grads[k][0], c.g_params.copy()) for k, c in enumerate(self.components)
                if isinstance(c, ProfileComponent)}

    def step(self, it, e_rel, prox_max_iter=10, b1=0.9, b2=0.999, eps=1e-8):
        # pgm.Scene.step moves the spectra (and, with a zero gradient and no constraint, leaves
        # the derived images alone); the profile parameters follow from the same evaluation
        super().step(it, e_rel, prox_max_iter, b1, b2, eps)
        for c in self.components:
            if isinstance(c, ProfileComponent):
                c.update_params(it, e_rel, prox_max_iter, b1, b2, eps)

    def check_parameters(self):
        super().check_parameters()
        for k, c in enumerate(self.components):
            if isinstance(c, ProfileComponent) and not np.isfinite(c.params).all():
                raise ArithmeticError("component {} is not finite".format(k))

    def boxes(self):
        return [tuple(c.origin) + tuple(c.morph.shape[-2:]) for c in self.components]

    def fit(self, max_iter=200, e_rel=1e-3, min_iter=1, prox_max_iter=10, resizing=False,
            b1=0.9, b2=0.999, eps=1e-8):
        """``pgm.Scene.fit`` with the hook of a profile component at the resize hook.
        ``self.box_history``: the boxes of all components at the start and after every restart."""
        self.box_history = [self.boxes()]
        it = 0
        while it < max_iter:
            local = 0
            restart = False
            while it + local < max_iter:
                self.step(local, e_rel, prox_max_iter, b1, b2, eps)
                self.check_parameters()
                if resizing and local > 0 and local % 10 == 0:
                    # every source is asked (blend.py:284-292 catches each UpdateException)
                    for c in self.components:
                        if isinstance(c, pgm.PointComponent) or not getattr(c, "resizing", True):
                            continue
                        changed = c.update_box() if isinstance(c, ProfileComponent) \
                            else pgm.resize_component(c)
                        restart = restart or changed
                    if restart:
                        self.box_history.append(self.boxes())
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
    """``ProfileScene`` of ``tests/golden/profile_source.npz`` (``g``) on the observation of the
    ``hsc_cosmos_35`` fixture (``hsc``)."""
    def value(name, k):
        key = "%s64_%d" % (name, k)
        return g[key if dtype64 and key in g.files else "%s_%d" % (name, k)].copy()

    comps = []
    for k in range(int(g["n_sources"])):
        common = dict(sed_min_step=g["sed_step_minimum_%d" % k],
                      sed_zero=float(g["sed_zero_%d" % k]), state_dtype=state_dtype)
        kind = str(g["kinds"][k])
        if kind == "extended":
            comps.append(pgm.Component(value("sed", k), value("morph", k), g["origin_%d" % k],
                                       **common))
            continue
        spergel = kind == "spergel"
        comps.append(ProfileComponent(
            value("sed", k), SPERGEL if spergel else GAUSSIAN, g["params_%d" % k],
            int(g["shape_%d" % k][0]), origin=tuple(int(o) for o in g["origin_%d" % k]),
            rel_step=(0.0, 0.01 if spergel else 0.1, 0.0, 0.0),
            sed_rel_step=float(g["sed_step_factor_%d" % k]), **common))
    dt = np.float64 if dtype64 else np.float32
    images = hsc["images"].astype(dt)
    weights, kernel = hsc["weights"].astype(dt), hsc["diff_kernel"].astype(dt)
    if dtype64:  # the float64 frame's own observation
        kernel = g["diff_kernel64"]
        weights = g["weights64"] if "weights64" in g.files else weights
    return ProfileScene(images.shape, images, weights, kernel, comps, dtype=dt)
