// Starlet ("a trous" B-spline wavelet) transform, its inverse and the multiresolution
// support of the reference's scarlet/wavelet.py:154-408, for the detection step
// (scarlet/detect.py:362-399).
//
// B_j (bspline_convolve, wavelet.py:154-191) is the separable 5-tap B-spline
// (1/16, 1/4, 3/8, 1/4, 1/16) at spacing d = 2^j with zeros outside the image: first along
// axis 0, then along axis 1, each pixel summed in the reference's order (bspline_tap of
// starlet_device.h, which holds the arithmetic this file shares with detect_batch.hip).  The
// reference computes in float64 (a float32 image times an np.float64 tap is float64 under
// NumPy 2), and this file is compiled without FMA contraction, so the coefficients are the
// reference's bit for bit.
//
// One kernel does a 1-D pass along either axis.  Both read the five taps straight from
// global memory: along axis 0 a wavefront reads five rows y-2d .. y+2d at the same 64
// columns, along axis 1 five shifted copies of the same 64-column segment; every read is
// coalesced and the re-reads hit L1/L2 (a dilation of 1024 rows is 32 KB of a 4096-wide
// float64 row per tap, well inside the Infinity Cache).  Nothing is staged in LDS, so any
// dilation works.  Per generation-2 scale the transform makes four passes (B_j(c) = c_{j+1},
// then B_j(c_{j+1}) with w_j = c_j - ... fused into the last one): nine plane-sized
// float64 streams.
//
// The multiresolution support ("ground" branch, wavelet.py:381-407) runs its per-plane
// standard deviations on the device as deterministic two-pass float64 reductions; the
// convergence test on a handful of numbers per iteration stays on the host.
#include <vector>

#include "common.h"
#include "starlet_device.h"

namespace smi {
namespace {

constexpr int kT = kSupportT;
constexpr int kMaxGridY = 65535;

template <typename T>
__global__ __launch_bounds__(kT) void to_f64_kernel(const T *in, double *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// One 1-D B-spline pass at spacing d over `rows` = n*H image rows of width W.
// AXIS 0: neighbours are rows y +- d, y +- 2d of the same image; AXIS 1: columns x +- d, x +- 2d.
//   out  != null: out[p] = conv (+ addend[p] when addend != null)
//   diff != null: diff[p] = diff[p] - conv
// out / diff / addend may alias each other elementwise (same p), never `in`.
template <int AXIS>
__global__ __launch_bounds__(kT) void bspline_pass_kernel(const double *__restrict__ in, int rows,
                                                         int H, int W, int d, double *out,
                                                         const double *addend, double *diff) {
    // 64-bit throughout: the last block's x, row + gridDim.y, u + 2d and the offsets 2d * W
    // all pass INT32_MAX for sizes the entry points admit (rows and W up to INT32_MAX, d up
    // to max(H, W))
    const int64_t x = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (x >= W) return;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const int64_t p = row * W + x;
        const double acc = bspline_tap<AXIS, double, int64_t>(in + p, row % H, x, H, W, d);
        if (out) out[p] = addend ? acc + addend[p] : acc;
        if (diff) diff[p] = diff[p] - acc;
    }
}

// generation-1 reconstruction: np.sum(starlets, axis=0), planes added one after another
__global__ __launch_bounds__(kT) void plane_sum_kernel(const double *in, int planes,
                                                       int64_t plane, double *out) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= plane) return;
    out[i] = strided_sum(in + i, planes, plane);
}

// np.sum(images, axis=0) of the bands, in the images' own type
template <typename T>
__global__ __launch_bounds__(kT) void coadd_kernel(const T *in, int bands, int64_t plane,
                                                   T *out) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= plane) return;
    out[i] = strided_sum(in + i, bands, plane);
}

// Plane pl = b * planes + k (image b, scale k) of the coefficients: PASS 0 sums v = w * ~M,
// PASS 1 sums (v - mean)^2.  Block partials go to part[pl * gridDim.x + blockIdx.x].
template <int PASS>
__global__ __launch_bounds__(kT) void support_stat_kernel(const double *coeffs, int planes,
                                                          int64_t plane_stride,
                                                          int64_t image_stride, int64_t npix,
                                                          const double *thr, const double *mean,
                                                          double *part) {
    __shared__ double sh[kT / 64];
    const int pl = blockIdx.y, b = pl / planes, k = pl - b * planes;
    const double *w = coeffs + k * plane_stride + b * image_stride;
    const double acc = support_partial<int64_t>(w, (int64_t)blockIdx.x * kT + threadIdx.x,
                                                (int64_t)gridDim.x * kT, npix, thr[pl], PASS,
                                                PASS ? mean[pl] : 0.0);
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(int64_t)pl * gridDim.x + blockIdx.x] = s;
}

// one block per plane: total of its partials; PASS 0 -> mean = total / npix, PASS 1 -> total
template <int PASS>
__global__ __launch_bounds__(kT) void support_final_kernel(const double *part, int nb,
                                                           int64_t npix, double *res) {
    __shared__ double sh[kT / 64];
    const int pl = blockIdx.x;
    double acc = 0;
    for (int i = threadIdx.x; i < nb; i += kT) acc += part[(int64_t)pl * nb + i];
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) res[pl] = PASS ? s : s / (double)npix;
}

// M = |w| > thr as int, and M * w
__global__ __launch_bounds__(kT) void support_mask_kernel(const double *coeffs, int planes,
                                                          int64_t plane_stride,
                                                          int64_t image_stride, int64_t npix,
                                                          const double *thr, int32_t *M,
                                                          double *Mw) {
    const int pl = blockIdx.y, b = pl / planes, k = pl - b * planes;
    const int64_t off = k * plane_stride + b * image_stride;
    const double t = thr[pl];
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < npix; q += (int64_t)gridDim.x * kT) {
        const double x = coeffs[off + q];
        const int m = support_member(x, t);
        if (M) M[off + q] = m;
        if (Mw) Mw[off + q] = support_masked(m, x);
    }
}

template <int AXIS>
int bspline_pass(const double *in, int rows, int H, int W, int d, double *out,
                 const double *addend, double *diff, hipStream_t st) {
    const dim3 grid((unsigned)(((int64_t)W + kT - 1) / kT), rows < kMaxGridY ? rows : kMaxGridY);
    hipLaunchKernelGGL(bspline_pass_kernel<AXIS>, grid, dim3(kT), 0, st, in, rows, H, W, d, out,
                       addend, diff);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

// B_j(in) -> out (+ addend) and/or diff -= B_j(in); `tmp` holds the axis-0 pass
int bspline(const double *in, int rows, int H, int W, int j, double *tmp, double *out,
            const double *addend, double *diff, hipStream_t st) {
    const int d = bspline_spacing(j, H, W);  // the kernel forms 2 * d in 64 bits
    int rc = bspline_pass<0>(in, rows, H, W, d, tmp, nullptr, nullptr, st);
    if (rc) return rc;
    return bspline_pass<1>(tmp, rows, H, W, d, out, addend, diff, st);
}

int grid1(int64_t n) { return (int)((n + kT - 1) / kT); }

template <typename T>
int starlet_transform(const T *d_images, int32_t n, int32_t H, int32_t W, int32_t scales,
                      int32_t generation, double *d_coeffs, double *d_work, void *stream) {
    SMI_REQUIRE(n > 0 && H > 0 && W > 0 && scales >= 0, "bad sizes");
    SMI_REQUIRE(generation == 1 || generation == 2, "generation must be 1 or 2");
    SMI_REQUIRE(scales < 31, "too many scales");
    SMI_REQUIRE((int64_t)n * H <= INT32_MAX, "too many image rows");
    int rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_images && d_coeffs && (d_work || scales == 0), "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t plane = (int64_t)n * H * W;
    const int rows = n * H;
    // c_0 = the image in float64 in plane 0
    hipLaunchKernelGGL(to_f64_kernel<T>, dim3(grid1(plane)), dim3(kT), 0, st, d_images, d_coeffs,
                       plane);
    SMI_HIP(hipGetLastError());
    for (int j = 0; j < scales; ++j) {
        double *c = d_coeffs + j * plane, *next = c + plane;
        if (generation == 1) {
            // c_{j+1} = B_j(c_j), w_j = c_j - c_{j+1} (in place over c_j)
            rc = bspline(c, rows, H, W, j, d_work, next, nullptr, c, st);
        } else {
            // c_{j+1} = B_j(c_j), then w_j = c_j - B_j(c_{j+1})
            rc = bspline(c, rows, H, W, j, d_work, next, nullptr, nullptr, st);
            if (!rc) rc = bspline(next, rows, H, W, j, d_work, nullptr, nullptr, c, st);
        }
        if (rc) return rc;
    }
    return SMI_OK;
}

int starlet_reconstruction(const double *d_coeffs, int32_t n, int32_t H, int32_t W,
                           int32_t scales, int32_t generation, double *d_image, double *d_work,
                           void *stream) {
    SMI_REQUIRE(n > 0 && H > 0 && W > 0 && scales >= 0, "bad sizes");
    SMI_REQUIRE(generation == 1 || generation == 2, "generation must be 1 or 2");
    SMI_REQUIRE(scales < 31, "too many scales");
    SMI_REQUIRE((int64_t)n * H <= INT32_MAX, "too many image rows");
    int rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_coeffs && d_image && (d_work || generation == 1 || scales == 0),
                "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t plane = (int64_t)n * H * W;
    if (generation == 1) {
        hipLaunchKernelGGL(plane_sum_kernel, dim3(grid1(plane)), dim3(kT), 0, st, d_coeffs,
                           scales + 1, plane, d_image);
        SMI_HIP(hipGetLastError());
        return SMI_OK;
    }
    // c = c_scales; c <- B_j(c) + w_j for j = scales-1 .. 0
    SMI_HIP(hipMemcpyAsync(d_image, d_coeffs + scales * plane, plane * sizeof(double),
                           hipMemcpyDeviceToDevice, st));
    for (int j = scales - 1; j >= 0; --j) {
        rc = bspline(d_image, n * H, H, W, j, d_work, d_image, d_coeffs + j * plane, nullptr, st);
        if (rc) return rc;
    }
    return SMI_OK;
}

int multiresolution_support(const double *d_coeffs, int32_t n, int32_t planes, int32_t H,
                            int32_t W, int64_t plane_stride, int64_t image_stride,
                            const double *sigma0, const double *thresh0, double K,
                            double epsilon, int32_t max_iter, int32_t *d_support,
                            double *d_masked, int32_t *iterations, void *stream) {
    SMI_REQUIRE(n > 0 && planes > 0 && H > 0 && W > 0, "bad sizes");
    SMI_REQUIRE((int64_t)n * planes <= kMaxGridY, "too many planes");
    SMI_REQUIRE(max_iter > 0, "max_iter must be positive");
    int rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_coeffs && sigma0 && thresh0, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int np = n * planes;
    const int64_t npix = (int64_t)H * W;
    const int nb = (int)support_blocks<int64_t>(np, npix);

    DevBuf<double> d_thr, d_mean, d_ss, d_part;
    SMI_HIP(d_thr.alloc(np));
    SMI_HIP(d_mean.alloc(np));
    SMI_HIP(d_ss.alloc(np));
    SMI_HIP(d_part.alloc((size_t)np * nb));

    std::vector<double> thr(thresh0, thresh0 + np), last(sigma0, sigma0 + np), ss(np);
    std::vector<char> done(n, 0);
    std::vector<int32_t> iters(n, 0);
    const dim3 grid(nb, np);
    for (int it = 0; it < max_iter; ++it) {
        SMI_HIP(hipMemcpyAsync(d_thr.p, thr.data(), np * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(support_stat_kernel<0>, grid, dim3(kT), 0, st, d_coeffs, planes,
                           plane_stride, image_stride, npix, d_thr.p, nullptr, d_part.p);
        hipLaunchKernelGGL(support_final_kernel<0>, dim3(np), dim3(kT), 0, st, d_part.p, nb, npix,
                           d_mean.p);
        hipLaunchKernelGGL(support_stat_kernel<1>, grid, dim3(kT), 0, st, d_coeffs, planes,
                           plane_stride, image_stride, npix, d_thr.p, d_mean.p, d_part.p);
        hipLaunchKernelGGL(support_final_kernel<1>, dim3(np), dim3(kT), 0, st, d_part.p, nb, npix,
                           d_ss.p);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipMemcpyAsync(ss.data(), d_ss.p, np * sizeof(double), hipMemcpyDeviceToHost, st));
        SMI_HIP(hipStreamSynchronize(st));
        bool all_done = true;
        for (int b = 0; b < n; ++b) {
            if (done[b]) continue;
            iters[b] = it + 1;
            const int o = b * planes;
            // converged: its mask is the one of this iteration's thresholds
            done[b] = support_converged(&ss[o], planes, (double)npix, K, epsilon,
                                        it + 1 == max_iter, &last[o], &thr[o]);
            if (!done[b]) all_done = false;
        }
        if (all_done) break;
    }
    if (d_support || d_masked) {
        SMI_HIP(hipMemcpyAsync(d_thr.p, thr.data(), np * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(support_mask_kernel, grid, dim3(kT), 0, st, d_coeffs, planes,
                           plane_stride, image_stride, npix, d_thr.p, d_support, d_masked);
        SMI_HIP(hipGetLastError());
    }
    // the device buffers are freed on return: finish the work that reads them first
    SMI_HIP(hipStreamSynchronize(st));
    if (iterations)
        for (int b = 0; b < n; ++b) iterations[b] = iters[b];
    return SMI_OK;
}

template <typename T>
int coadd(const T *d_images, int32_t bands, int32_t H, int32_t W, T *d_out, void *stream) {
    SMI_REQUIRE(bands > 0 && H > 0 && W > 0, "bad sizes");
    int rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_images && d_out, "null argument");
    const int64_t plane = (int64_t)H * W;
    hipLaunchKernelGGL(coadd_kernel<T>, dim3(grid1(plane)), dim3(kT), 0, (hipStream_t)stream,
                       d_images, bands, plane, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_starlet_transform_f32(const float *d_images, int32_t n, int32_t H, int32_t W,
                              int32_t scales, int32_t generation, double *d_coeffs,
                              double *d_work, void *stream) {
    return smi::starlet_transform<float>(d_images, n, H, W, scales, generation, d_coeffs, d_work,
                                         stream);
}
int smi_starlet_transform_f64(const double *d_images, int32_t n, int32_t H, int32_t W,
                              int32_t scales, int32_t generation, double *d_coeffs,
                              double *d_work, void *stream) {
    return smi::starlet_transform<double>(d_images, n, H, W, scales, generation, d_coeffs,
                                          d_work, stream);
}
int smi_starlet_reconstruction_f64(const double *d_coeffs, int32_t n, int32_t H, int32_t W,
                                   int32_t scales, int32_t generation, double *d_image,
                                   double *d_work, void *stream) {
    return smi::starlet_reconstruction(d_coeffs, n, H, W, scales, generation, d_image, d_work,
                                       stream);
}
int smi_multiresolution_support_f64(const double *d_coeffs, int32_t n, int32_t planes,
                                    int32_t H, int32_t W, int64_t plane_stride,
                                    int64_t image_stride, const double *sigma0,
                                    const double *thresh0, double K, double epsilon,
                                    int32_t max_iter, int32_t *d_support, double *d_masked,
                                    int32_t *iterations, void *stream) {
    return smi::multiresolution_support(d_coeffs, n, planes, H, W, plane_stride, image_stride,
                                        sigma0, thresh0, K, epsilon, max_iter, d_support,
                                        d_masked, iterations, stream);
}
int smi_coadd_f32(const float *d_images, int32_t bands, int32_t H, int32_t W, float *d_out,
                  void *stream) {
    return smi::coadd<float>(d_images, bands, H, W, d_out, stream);
}
int smi_coadd_f64(const double *d_images, int32_t bands, int32_t H, int32_t W, double *d_out,
                  void *stream) {
    return smi::coadd<double>(d_images, bands, H, W, d_out, stream);
}

}  // extern "C"
