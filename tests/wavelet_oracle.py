"""Float64 NumPy restatement of the starlet transform, its inverse, the band coadd and the
multiresolution support ("ground") of scarlet/wavelet.py and detect.py, written from their
behaviour.  tests/test_wavelet_host.py pins it to the arrays the reference produced
(tests/golden/detect.npz); the GPU tests then compare the kernels with it bit for bit at
shapes and options the goldens do not hold.

Every function works for any extent and any scale: a B-spline tap whose neighbour lies
outside the image is skipped, so a spacing of ``2**j >= extent`` leaves the centre tap only."""

import numpy as np

TAPS = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)


def bspline(image, j):
    """B_j in float64, the reference's order of additions"""
    d = 2 ** j
    taps = TAPS

    def one(x):  # along axis 0
        n = x.shape[0]
        out = x * taps[2]
        if 2 * d < n:
            out[2 * d:] += x[:n - 2 * d] * taps[0]
        if d < n:
            out[d:] += x[:n - d] * taps[1]
            out[:n - d] += x[d:] * taps[3]
        if 2 * d < n:
            out[:n - 2 * d] += x[2 * d:] * taps[4]
        return out

    return one(one(np.asarray(image, dtype=np.float64)).T).T


def transform(image, scales, generation=2):
    """``(scales+1, H, W)`` float64 coefficients; ``scales`` is used as given"""
    c = np.asarray(image, dtype=np.float64)
    out = np.zeros((scales + 1,) + c.shape)
    for j in range(scales):
        nxt = bspline(c, j)
        out[j] = c - (bspline(nxt, j) if generation == 2 else nxt)
        c = nxt
    out[-1] = c
    return out


def reconstruction(coeffs, generation=2):
    """image of ``(scales+1, H, W)`` coefficients: the planes added one after another
    (generation 1) or ``c <- B_j(c) + w_j`` from the last scale down (generation 2)"""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    if generation == 1:
        return plane_sum(coeffs)
    c = coeffs[-1]
    for j in range(len(coeffs) - 2, -1, -1):
        c = bspline(c, j) + coeffs[j]
    return c


def plane_sum(stack):
    """``((p0 + p1) + p2) ...`` in the stack's own type: what ``np.sum(stack, axis=0)`` does
    for planes of more than one pixel.  (For a 1 x 1 plane NumPy reduces a contiguous vector,
    pairwise from 8 entries on; the library adds one after another there as well, and so does
    this.)"""
    stack = np.asarray(stack)
    acc = stack[0].copy()
    for plane in stack[1:]:
        acc = acc + plane
    return acc


def coadd(images):
    """sum of the bands, band after band, in the images' own type"""
    return plane_sum(images)


def same_bits(a, b):
    """equal shapes, types and values, NaNs at the same places, zeros of the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def support(image_dtype, coeffs, sigma, K=3, epsilon=1e-1, max_iter=20, perturb=1.0):
    """Multiresolution support of ``(planes, H, W)`` coefficients for an image of dtype
    ``image_dtype`` and noise ``sigma``.  Plane by plane ``M = |w| > K sigma_j``; ``sigma_j``
    starts as ``sigma`` in the image's dtype and is then the standard deviation of the
    plane with its significant coefficients zeroed, until every non-zero ``sigma_j`` moved
    by less than ``epsilon`` (relative to the new one) or ``max_iter`` masks were made.
    Returns ``(M as int, iterations, thresholds_used)``: the mask of the last thresholds,
    the number of masks made, and the ``(iterations, planes)`` float64 thresholds.

    ``perturb`` scales every estimated ``sigma_j`` (not the first): the tests rerun with
    ``1 +- r`` to show that a case does not hinge on the rounding of the standard deviation."""
    coeffs = np.asarray(coeffs)
    sigma_j = np.ones((len(coeffs),), dtype=image_dtype) * sigma
    last = sigma_j
    used = []
    for it in range(max_iter):
        thr = K * sigma_j
        used.append(np.asarray(thr, dtype=np.float64))
        M = np.abs(coeffs) > thr[:, None, None]
        sigma_j = np.std(coeffs * (~M).astype(int), axis=(1, 2)) * perturb
        moved = sigma_j > 0
        if np.all(np.abs(sigma_j[moved] - last[moved]) / sigma_j[moved] < epsilon):
            break
        last = sigma_j
    return M.astype(int), it + 1, np.stack(used)


def rounding_margin_ok(image_dtype, coeffs, sigma, K, epsilon, max_iter):
    """The two conditions under which a support computed with standard deviations summed in
    another order must equal :func:`support` exactly.  ``r = npix * 2**-52`` bounds the
    relative error of a float64 sum of ``npix`` terms in any order.
    (a) rerunning with every ``sigma_j`` scaled by ``1 - r`` and ``1 + r`` gives the same
        number of iterations;
    (b) no coefficient has ``| |w| - thr | <= r * thr`` for a threshold the loop used.
    A threshold of exactly 0 is left out of (b): it comes from a ``sigma_j`` of exactly 0, a
    plane whose insignificant coefficients are all ``+-0``, which sums to 0 in every order.
    Returns ``(a, b)``."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    r = coeffs[0].size * 2.0 ** -52
    _, iters, used = support(image_dtype, coeffs, sigma, K, epsilon, max_iter)
    a = all(support(image_dtype, coeffs, sigma, K, epsilon, max_iter, perturb=f)[1] == iters
            for f in (1 - r, 1 + r))
    mag = np.abs(coeffs)
    b = True
    for thr in used:
        t = thr[:, None, None]
        with np.errstate(invalid="ignore"):
            close = (np.abs(mag - t) <= r * t) & (t != 0)
        b = b and not close.any()
    return a, b
