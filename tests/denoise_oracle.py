"""Float64 NumPy restatement of ``apply_wavelet_denoising`` (scarlet/wavelet.py:424-465): the
loop of Starck et al. 2011, section 4.1, composed of ``wavelet_oracle``'s transform,
reconstruction and support.  tests/test_denoise_host.py pins it to the reference's own
denoisings (tests/golden/interpolate_observation.npz); the GPU tests then compare the kernels
with it bit for bit at shapes and options the goldens do not hold."""

import numpy as np

import wavelet_oracle as wo


def scales_of(shape):
    """all the scales of an image: ``int(log2(min(shape))) - 1``"""
    return int(np.log2(min(shape[-2:]))) - 1


def as_image(image):
    """float32 and float64 stay, everything else becomes float64"""
    image = np.asarray(image)
    return image if image.dtype in (np.float32, np.float64) else image.astype(np.float64)


def noise_level(image):
    """the ``sigma=None`` default: the median absolute deviation, in the image's dtype"""
    return np.median(np.absolute(image - np.median(image)))


def denoise(image, sigma=None, k=3, epsilon=1e-1, max_iter=20, positive=True):
    """``x = R(T(image))``, then ``max_iter`` times ``x = x + R(M * (T(image) - T(x)))`` and
    ``x[x < 0] = 0`` if ``positive``; ``M`` the "ground" support of ``T(image)``, itself with
    at most ``max_iter`` iterations"""
    image = as_image(image)
    scales = scales_of(image.shape)
    image_coeffs = wo.transform(image, scales)
    if sigma is None:
        sigma = noise_level(image)
    M, _, _ = wo.support(image.dtype, image_coeffs, sigma, k, epsilon, max_iter)
    x = wo.reconstruction(image_coeffs)
    for _ in range(max_iter):
        coeffs = wo.transform(x, scales)
        x = x + wo.reconstruction(M * (image_coeffs - coeffs))
        if positive:
            x[x < 0] = 0
    return x


def margin_ok(image, sigma=None, k=3, epsilon=1e-1, max_iter=20):
    """both conditions of ``wavelet_oracle.rounding_margin_ok`` for the support of this
    denoising: then a support whose standard deviations are summed in another order is the
    same, and with it every later number"""
    image = as_image(image)
    image_coeffs = wo.transform(image, scales_of(image.shape))
    if sigma is None:
        sigma = noise_level(image)
    with np.errstate(invalid="ignore"):
        a, b = wo.rounding_margin_ok(image.dtype, image_coeffs, sigma, k, epsilon, max_iter)
    return bool(a and b)
