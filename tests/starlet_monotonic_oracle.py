"""Oracle of monotonic starlet sources: ``starlet_oracle`` extended by subclassing.

TEST INFRASTRUCTURE ONLY.  ``MonotonicStarletComponent`` is a ``StarletComponent`` whose proximal
operator is the ``MonotonicMaskConstraint`` of ``StarletMorphology(monotonic=True)`` (reference
constraint.py:237-259): ``oracle.proxops.prox_monotonic_mask`` about the middle of the box on
every plane of the stack, in the place of positivity and thresholds.  The middle follows the
box, so the shrink hook of ``starlet_oracle`` re-centres it as morphology.py:584-586 does.
"""

import numpy as np

from oracle import proxops

import starlet_oracle as so


def mask_planes(stack, center_radius=1, variance=0.0, max_iter=3):
    """``MonotonicMaskConstraint((h // 2, w // 2), ...)`` on a ``(planes, h, w)`` stack in the
    stack's own dtype (float32 or float64).  Returns the new stack and the number of pixels
    that were interpolated: valid ones that do not hold their input any more."""
    stack = np.ascontiguousarray(stack)
    assert stack.ndim == 3 and stack.dtype in (np.float32, np.float64)
    center = (stack.shape[1] // 2, stack.shape[2] // 2)
    out = np.empty_like(stack)
    interpolated = 0
    for p, plane in enumerate(stack):
        valid, out[p], _ = proxops.prox_monotonic_mask(
            plane.copy(), 0, center, center_radius=center_radius, variance=variance,
            max_iter=max_iter)
        interpolated += int(np.sum(valid & (out[p] != plane)))
    return out, interpolated


class MonotonicStarletComponent(so.StarletComponent):
    """``morph`` = coefficients (planes, h, w) kept monotonic plane by plane about
    ``center``.  ``cast32``: the operator sees its argument rounded to float32, as the device
    holds it (its result is exact in either format but for the interpolated values)."""

    def __init__(self, sed, coeffs, origin, center_radius=1, variance=0.0, max_iter=3,
                 cast32=False, **kw):
        super().__init__(sed, coeffs, origin, np.zeros(len(coeffs)), **kw)
        self.center_radius, self.variance, self.max_iter = center_radius, variance, max_iter
        self.cast32 = cast32
        self.interpolated = 0

    @property
    def center(self):
        return tuple(n // 2 for n in self.morph.shape[-2:])

    def morph_prox(self, x, step):
        self.last_pre = np.array(x, dtype=np.float64)
        arg = x.astype(np.float32) if self.cast32 else np.ascontiguousarray(x)
        out, n = mask_planes(arg, self.center_radius, self.variance, self.max_iter)
        self.interpolated += n
        return out.astype(x.dtype)


def shrink_component(c, thresh=1e-8):
    """``starlet_oracle.shrink_component`` (what ``StarletScene.fit`` calls for any
    ``StarletComponent``): ``c.center`` is the middle of whatever box the coefficients have,
    so the operator is re-centred on the new box at its next call."""
    return so.shrink_component(c, thresh)


def fixture_scene(g, gm, hsc, state_dtype=np.float64, cast32=False):
    """``StarletScene`` of the fixture scene with the sources of ``starlet_monotonic.npz``
    (``gm``) monotonic and the others those of ``starlet_source.npz`` (``g``)."""
    sc = so.fixture_scene(g, hsc, state_dtype=state_dtype)
    for k in (int(k) for k in gm["starlet_of"]):
        old = sc.components[k]
        sc.components[k] = MonotonicStarletComponent(
            gm["sed_%d" % k].copy(), gm["coeffs_%d" % k].copy(), gm["origin_%d" % k],
            center_radius=int(gm["center_radius_%d" % k]), variance=float(gm["variance_%d" % k]),
            max_iter=int(gm["max_iter_%d" % k]), cast32=cast32,
            coeffs_step=float(gm["step_%d" % k]), sed_rel_step=old.sed_rel_step,
            sed_min_step=old.sed_min_step, sed_zero=old.sed_zero, state_dtype=state_dtype)
    return sc
