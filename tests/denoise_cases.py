"""The cases of the denoising tests: small deterministic images at the shapes where
csrc/denoise_batch.hip takes another path -- no scale at all (2 x 2), one scale, odd and oblong
extents, more than one block of pixels, the last size of the batch path (256 x 256 = 65536
pixels) and the first beyond it -- in float32 and float64, with every option both ways.

The oracle's results are computed once per case and shared (``oracle_result``); the tests that
compare bit for bit keep the cases for which ``wavelet_oracle.rounding_margin_ok`` holds
(``exact_cases``): the support's standard deviations are summed in another order on the device
than in NumPy, and a case whose support hinges on that rounding proves nothing either way."""

import collections
import itertools

import numpy as np

import denoise_oracle

Case = collections.namedtuple("Case", "name image sigma k positive max_iter")

SMALL_SHAPES = [(2, 2), (4, 4), (5, 7), (16, 16), (33, 17), (64, 48)]
LIMIT_SHAPE = (256, 256)   # 65536 pixels: the last one the batch path takes
BEYOND_SHAPE = (257, 256)  # goes one by one
NOISE = 0.5


def make_image(shape, dtype, seed):
    """a blob or two on a sloping background, with noise of standard deviation ``NOISE``"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[0], :shape[1]]
    image = rng.normal(0.0, NOISE, shape) + 0.01 * (x - y)
    for _ in range(2):
        cy, cx = rng.uniform(0, shape[0]), rng.uniform(0, shape[1])
        image += 8 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * (1 + shape[0] / 16) ** 2))
    return image.astype(dtype)


def _cases():
    out = []
    # every option both ways on a one-scale float32 image and a three-scale float64 one
    for shape, dtype in (((5, 7), np.float32), ((33, 17), np.float64)):
        image = make_image(shape, dtype, 11)
        for sigma, positive, max_iter, k in itertools.product((None, 0.8 * NOISE), (True, False),
                                                              (1, 2, 20), (1, 3)):
            name = "%dx%d_%s_s%s_p%d_i%d_k%d" % (shape + (np.dtype(dtype).name,
                                                          "N" if sigma is None else "G",
                                                          positive, max_iter, k))
            out.append(Case(name, image, sigma, k, positive, max_iter))
    # every shape in both dtypes with the defaults
    for n, shape in enumerate(SMALL_SHAPES):
        for dtype in (np.float32, np.float64):
            out.append(Case("%dx%d_%s" % (shape + (np.dtype(dtype).name,)),
                            make_image(shape, dtype, 20 + n), None, 3, True, 20))
    # the two sides of the batch path's limit (two loop iterations keep the oracle quick)
    out.append(Case("limit_float32", make_image(LIMIT_SHAPE, np.float32, 31), None, 3, True, 2))
    out.append(Case("beyond_float64", make_image(BEYOND_SHAPE, np.float64, 32), NOISE, 3, False, 2))
    # special images
    out.append(Case("zeros", np.zeros((16, 16), np.float32), None, 3, True, 20))
    nan = make_image((16, 16), np.float64, 33)
    nan[5, 9] = np.nan
    out.append(Case("nan", nan, None, 3, True, 2))
    out.append(Case("nan_sigma", nan, NOISE, 3, True, 2))
    return out


CASES = _cases()
_results, _margins = {}, {}


def oracle_result(case):
    """``denoise_oracle.denoise`` of the case, computed once; do not modify"""
    if case.name not in _results:
        with np.errstate(invalid="ignore"):
            x = denoise_oracle.denoise(case.image, case.sigma, case.k, 1e-1, case.max_iter,
                                       case.positive)
        x.setflags(write=False)
        _results[case.name] = x
    return _results[case.name]


def margin_ok(case):
    if case.name not in _margins:
        _margins[case.name] = denoise_oracle.margin_ok(case.image, case.sigma, case.k, 1e-1,
                                                       case.max_iter)
    return _margins[case.name]


def exact_cases():
    """the cases whose support does not hinge on the rounding of a standard deviation"""
    return [case for case in CASES if margin_ok(case)]


def ragged_list():
    """one image per shape, float32 and float64 alternating, the one beyond the limit in the
    middle: the list of the batch tests"""
    shapes = SMALL_SHAPES[:3] + [BEYOND_SHAPE] + SMALL_SHAPES[3:] + [LIMIT_SHAPE]
    return [make_image(shape, np.float32 if n % 2 else np.float64, 40 + n)
            for n, shape in enumerate(shapes)]
