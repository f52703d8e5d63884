// apply_wavelet_denoising (reference scarlet/wavelet.py:424-465; Starck et al. 2011, section
// 4.1) for a ragged list of images, resident on the device:
//   set-up   image_coeffs = T(image), all scales, generation 2
//            M = the "ground" multiresolution support of image_coeffs
//            x = R(image_coeffs)
//   loop     max_iter times  x = x + R(M * (image_coeffs - T(x))),  x[x < 0] = 0 if positive
// Everything is float64 in the reference's operation order (this file is compiled without FMA
// contraction), and every number comes from the functions of starlet_device.h: an image's
// result is, bit for bit, the one of the chain smi_starlet_transform_* ->
// smi_multiresolution_support_f64 -> smi_starlet_reconstruction_f64 with the element-wise
// steps in NumPy between them, whatever else is in the list.
//
// The list is ragged -- extents and scale counts differ -- so, as in detect_batch.hip, every
// kernel takes a table of tasks (one per image, validated on the host before anything is
// launched) with grid.y = task, and a task with scales <= j leaves a pass of scale j at once.
// The element-wise stages ride on the passes next to them:
//   masked difference   d_j = M_j * (image_coeffs_j - w_j) where the last pass of scale j of
//                       the forward transform forms w_j = c_j - B_j(c_{j+1}); the same thread
//                       masks the last plane c_S when j + 1 is the task's last scale
//   add and clip        x = max(x + (B_0(c) + d_0), 0) in the last pass of the reconstruction
// The running reconstruction lives in the plane of the last scale, which it has consumed.  A
// task without a scale (an image 2 or 3 pixels high or wide) has T(x) = x and R(d) = d_0: its
// whole iteration is one element-wise step, done by the first launch of the iteration.
//
// Launches, S = the largest scale count of the table (smi_denoise_launches):
//   transform   1 + 4 S          widen to float64, four passes per scale
//   support     2                one workgroup per image runs all iterations; M from the
//                                thresholds it leaves in the scratch
//   iterate     2 S + max_iter * max(6 S, 1)
//                                R(image_coeffs), then 4 S forward and 2 S inverse passes
// whatever the number of images.  Nothing is allocated, copied to the host or waited for; no
// workgroup waits for another and nothing is accumulated in global memory.
//
// The limit of the support stage is detect_batch.hip's: 65536 pixels, one workgroup per image.
// A larger image takes the transform and iterate stages here and its support from
// smi_multiresolution_support_f64 between them.
#include <algorithm>

#include "common.h"
#include "starlet_device.h"

namespace smi {
namespace {

constexpr int kT = kSupportT;
constexpr int32_t kMaxScales = 30;
constexpr int64_t kMaxPassPixels = (int64_t)1 << 30;  // a pixel index is an int

// the buffers of a call; a task's coefficient-shaped slices (ic, M, cur) start at coeff_off,
// its plane-shaped ones (x, work) at plane_off
struct Planes {
    double *ic;        // image_coeffs
    int32_t *M;        // the support
    double *cur;       // T(x), then the masked difference, then the running reconstruction
    double *x, *work;
};
enum : int { kIc = 0, kCur = 1, kX = 2, kWork = 3 };
constexpr int kLast = -1;  // plane selector: the task's last plane
struct Sel {
    int buf, plane;
};

__device__ __forceinline__ double *plane_ptr(const Planes &b, const smi_denoise_task &t,
                                             int64_t npix, Sel s) {
    const int64_t k = s.plane == kLast ? t.scales : s.plane;
    switch (s.buf) {
    case kIc: return b.ic + t.coeff_off + k * npix;
    case kCur: return b.cur + t.coeff_off + k * npix;
    case kX: return b.x + t.plane_off;
    default: return b.work + t.plane_off;
    }
}

// M * (image_coeffs - w): the reference's int * float product
__device__ __forceinline__ double masked_difference(int m, double ic, double w) {
    return support_masked(m, ic - w);
}
// x + r, then x[x < 0] = 0: a NaN and -0.0 stay
__device__ __forceinline__ double denoise_update(double x, double r, int positive) {
    const double v = x + r;
    return positive && v < 0 ? 0.0 : v;
}

// B_j along AXIS at pixel p of plane `in` of the task
template <int AXIS>
__device__ __forceinline__ double tap_at(const smi_denoise_task &t, const double *in, int p,
                                         int j) {
    const int y = p / t.w, x = p - y * t.w;
    return bspline_tap<AXIS, double, int64_t>(in + p, y, x, t.h, t.w,
                                              bspline_spacing(j, t.h, t.w));
}

// ---------------------------------------------------------------------------- kernels
template <typename T>
__global__ __launch_bounds__(kT) void denoise_widen_kernel(const smi_denoise_task *tasks,
                                                           const T *images, double *ic) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p < npix) ic[t.coeff_off + p] = (double)images[t.image_off + p];
}

// One 1-D B-spline pass of scale j over every task with more than j scales: out[p] = conv.
// `in_top` is read in the place of `in` by a task whose last scale is j (the reconstruction
// starts from the last plane of another stack than it continues in).  `whole` != 0 (the first
// launch of an iteration, j = 0): a task without a scale does its iteration here, from
// image_coeffs (1: the first iteration, x = R(image_coeffs) = plane 0) or from x (2).
template <int AXIS>
__global__ __launch_bounds__(kT) void denoise_pass_kernel(const smi_denoise_task *tasks, int j,
                                                          Sel in, Sel in_top, Sel out, int whole,
                                                          int positive, Planes b) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= npix) return;
    if (t.scales <= j) {
        if (whole && t.scales == 0) {
            const double ic = b.ic[t.coeff_off + p];
            const double x = whole == 1 ? ic : b.x[t.plane_off + p];
            const double d = masked_difference(b.M[t.coeff_off + p], ic, x);
            b.x[t.plane_off + p] = denoise_update(x, d, positive);
        }
        return;
    }
    const double *src = plane_ptr(b, t, npix, j == t.scales - 1 ? in_top : in);
    plane_ptr(b, t, npix, out)[p] = tap_at<AXIS>(t, src, p, j);
}

// the last pass of scale j of T(image): w_j = c_j - B_j(c_{j+1}) in place over c_j
__global__ __launch_bounds__(kT) void denoise_diff_kernel(const smi_denoise_task *tasks, int j,
                                                          Planes b) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= npix || t.scales <= j) return;
    const double acc = tap_at<1>(t, b.work + t.plane_off, p, j);
    double *c = b.ic + t.coeff_off + (int64_t)j * npix + p;
    *c = *c - acc;
}

// the last pass of scale j of T(x), with the masked difference: c_0 = x itself
__global__ __launch_bounds__(kT) void denoise_masked_kernel(const smi_denoise_task *tasks, int j,
                                                            Planes b) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= npix || t.scales <= j) return;
    const double acc = tap_at<1>(t, b.work + t.plane_off, p, j);
    const int64_t e = t.coeff_off + (int64_t)j * npix + p;
    const double c = j == 0 ? b.x[t.plane_off + p] : b.cur[e];
    b.cur[e] = masked_difference(b.M[e], b.ic[e], c - acc);
    if (j + 1 == t.scales) {
        const int64_t l = e + npix;
        b.cur[l] = masked_difference(b.M[l], b.ic[l], b.cur[l]);
    }
}

// the last pass of scale j of a reconstruction: c <- B_j(c) + w_j with w = image_coeffs
// (setup) or the masked difference; at j = 0 the result is x (setup) or goes into it
__global__ __launch_bounds__(kT) void denoise_add_kernel(const smi_denoise_task *tasks, int j,
                                                         int setup, int positive, Planes b) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= npix || t.scales <= j) return;
    const double acc = tap_at<1>(t, b.work + t.plane_off, p, j);
    const int64_t e = t.coeff_off + (int64_t)j * npix + p;
    const double r = acc + (setup ? b.ic[e] : b.cur[e]);
    if (j > 0) {
        b.cur[t.coeff_off + (int64_t)t.scales * npix + p] = r;
    } else {
        double *x = b.x + t.plane_off + p;
        *x = setup ? r : denoise_update(*x, r, positive);
    }
}

__global__ __launch_bounds__(kT) void denoise_support_kernel(const smi_denoise_task *tasks,
                                                             const double *ic, double K,
                                                             double epsilon, int max_iter,
                                                             double *thr_out,
                                                             int32_t *iterations) {
    const smi_denoise_task t = tasks[blockIdx.x];
    support_workgroup(ic + t.coeff_off, t.scales + 1, t.h * t.w, t.sigma0, t.thresh0, K, epsilon,
                      max_iter, thr_out + (int64_t)blockIdx.x * kSupportSlots,
                      iterations ? iterations + blockIdx.x : nullptr);
}

__global__ __launch_bounds__(kT) void denoise_mask_kernel(const smi_denoise_task *tasks,
                                                          const double *ic, const double *thr,
                                                          int32_t *M) {
    const smi_denoise_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w, n = (t.scales + 1) * npix;
    const double *th = thr + (int64_t)blockIdx.y * kSupportSlots;
    for (int e = blockIdx.x * kT + threadIdx.x; e < n; e += gridDim.x * kT)
        M[t.coeff_off + e] = support_member(ic[t.coeff_off + e], th[e / npix]);
}

// ---------------------------------------------------------------------------- host
unsigned blocks_for(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

int launches(int32_t top, int32_t max_iter, int32_t stages) {
    int n = 0;
    if (stages & SMI_DENOISE_TRANSFORM) n += 1 + 4 * top;
    if (stages & SMI_DENOISE_SUPPORT) n += 2;
    if (stages & SMI_DENOISE_ITERATE) n += 2 * top + max_iter * std::max(6 * top, 1);
    return n;
}

template <typename T>
int denoise(int32_t n, const smi_denoise_task *tasks, const void *d_tasks, int32_t stages,
            double K, double epsilon, int32_t max_iter, int32_t positive, const T *d_images,
            int64_t n_images, double *d_coeffs, int32_t *d_support, double *d_current,
            int64_t n_coeffs, double *d_x, double *d_work, int64_t n_planes,
            int32_t *d_iterations, void *d_scratch, int64_t scratch_bytes, void *stream) {
    SMI_REQUIRE(n >= 0 && n <= 65535, "task count");
    SMI_REQUIRE((tasks && d_tasks) || n == 0, "null descriptor table");
    SMI_REQUIRE(stages > 0 && stages <= 7, "stages");
    SMI_REQUIRE(max_iter > 0, "max_iter must be positive");
    SMI_REQUIRE(n_images >= 0 && n_coeffs >= 0 && n_planes >= 0, "negative buffer size");
    const bool transform = stages & SMI_DENOISE_TRANSFORM, support = stages & SMI_DENOISE_SUPPORT,
               iterate = stages & SMI_DENOISE_ITERATE;
    SMI_REQUIRE((d_images || !n_images || !transform) && (d_coeffs || !n_coeffs) &&
                    (d_work || !n_planes),
                "null buffer");
    SMI_REQUIRE(!(support || iterate) || d_support || !n_coeffs, "null support");
    SMI_REQUIRE(!iterate || ((d_current || !n_coeffs) && (d_x || !n_planes)), "null buffer");
    SMI_REQUIRE(!support || (scratch_bytes >= (int64_t)n * kSupportSlots * (int64_t)sizeof(double) &&
                             (d_scratch || n == 0)),
                "scratch too small");
    // largest[j]: pixels of the largest image among the tasks with more than j scales
    int64_t largest[kMaxScales + 1] = {0}, all = 0, all_planes = 0;
    int32_t top = 0;
    int64_t coeff_end = 0, plane_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_denoise_task &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && (int64_t)t.h * t.w <= kMaxPassPixels, "image extent");
        SMI_REQUIRE(t.scales >= 0 && t.scales <= kMaxScales, "scales");
        const int64_t npix = (int64_t)t.h * t.w;
        SMI_REQUIRE(!support || npix <= kSupportMaxPixels,
                    "more pixels than the support stage takes");
        SMI_REQUIRE(!transform || in_buffer(t.image_off, npix, n_images),
                    "image outside its buffer");
        SMI_REQUIRE(t.coeff_off >= coeff_end &&
                        in_buffer(t.coeff_off, (t.scales + 1) * npix, n_coeffs),
                    "coefficients outside their buffer or shared with another task");
        coeff_end = t.coeff_off + (t.scales + 1) * npix;
        SMI_REQUIRE(t.plane_off >= plane_end && in_buffer(t.plane_off, npix, n_planes),
                    "plane outside its buffer or shared with another task");
        plane_end = t.plane_off + npix;
        for (int32_t j = 0; j < t.scales; ++j) largest[j] = std::max(largest[j], npix);
        top = std::max(top, t.scales);
        all = std::max(all, npix);
        all_planes = std::max(all_planes, (t.scales + 1) * npix);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const smi_denoise_task *dt = (const smi_denoise_task *)d_tasks;
    const Planes b{d_coeffs, d_support, d_current, d_x, d_work};
    const dim3 threads(kT);
    const Sel work{kWork, 0}, x{kX, 0}, last{kCur, kLast};
    if (transform) {
        hipLaunchKernelGGL((denoise_widen_kernel<T>), dim3(blocks_for(all), n), threads, 0, st, dt,
                           d_images, d_coeffs);
        for (int32_t j = 0; j < top; ++j) {
            // c_{j+1} = B_j(c_j), then w_j = c_j - B_j(c_{j+1})
            const dim3 grid(blocks_for(largest[j]), n);
            const Sel cj{kIc, j}, next{kIc, j + 1};
            hipLaunchKernelGGL(denoise_pass_kernel<0>, grid, threads, 0, st, dt, j, cj, cj, work, 0,
                               0, b);
            hipLaunchKernelGGL(denoise_pass_kernel<1>, grid, threads, 0, st, dt, j, work, work,
                               next, 0, 0, b);
            hipLaunchKernelGGL(denoise_pass_kernel<0>, grid, threads, 0, st, dt, j, next, next,
                               work, 0, 0, b);
            hipLaunchKernelGGL(denoise_diff_kernel, grid, threads, 0, st, dt, j, b);
        }
    }
    if (support) {
        double *d_thr = (double *)d_scratch;
        hipLaunchKernelGGL(denoise_support_kernel, dim3(n), threads, 0, st, dt, d_coeffs, K,
                           epsilon, max_iter, d_thr, d_iterations);
        hipLaunchKernelGGL(denoise_mask_kernel, dim3(std::min(blocks_for(all_planes), 1024u), n),
                           threads, 0, st, dt, d_coeffs, d_thr, d_support);
    }
    if (iterate) {
        // x = R(image_coeffs): c = c_S, c <- B_j(c) + w_j from the last scale down
        for (int32_t j = top - 1; j >= 0; --j) {
            const dim3 grid(blocks_for(largest[j]), n);
            hipLaunchKernelGGL(denoise_pass_kernel<0>, grid, threads, 0, st, dt, j, last,
                               Sel{kIc, kLast}, work, 0, 0, b);
            hipLaunchKernelGGL(denoise_add_kernel, grid, threads, 0, st, dt, j, 1, 0, b);
        }
        for (int32_t it = 0; it < max_iter; ++it) {
            const int whole = it == 0 ? 1 : 2;
            if (top == 0)
                hipLaunchKernelGGL(denoise_pass_kernel<0>, dim3(blocks_for(all), n), threads, 0, st,
                                   dt, 0, x, x, work, whole, positive, b);
            for (int32_t j = 0; j < top; ++j) {
                // the first launch covers every task: those without a scale finish there
                const dim3 grid(blocks_for(largest[j]), n), first(blocks_for(all), n);
                const Sel cj = j == 0 ? x : Sel{kCur, j}, next{kCur, j + 1};
                hipLaunchKernelGGL(denoise_pass_kernel<0>, j == 0 ? first : grid, threads, 0, st,
                                   dt, j, cj, cj, work, j == 0 ? whole : 0, positive, b);
                hipLaunchKernelGGL(denoise_pass_kernel<1>, grid, threads, 0, st, dt, j, work, work,
                                   next, 0, 0, b);
                hipLaunchKernelGGL(denoise_pass_kernel<0>, grid, threads, 0, st, dt, j, next, next,
                                   work, 0, 0, b);
                hipLaunchKernelGGL(denoise_masked_kernel, grid, threads, 0, st, dt, j, b);
            }
            for (int32_t j = top - 1; j >= 0; --j) {
                const dim3 grid(blocks_for(largest[j]), n);
                hipLaunchKernelGGL(denoise_pass_kernel<0>, grid, threads, 0, st, dt, j, last, last,
                                   work, 0, 0, b);
                hipLaunchKernelGGL(denoise_add_kernel, grid, threads, 0, st, dt, j, 0, positive, b);
            }
        }
    }
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_denoise_scratch_bytes(int32_t n, int64_t *bytes) {
    SMI_REQUIRE(n >= 0 && bytes, "task count or null result");
    *bytes = (int64_t)n * smi::kSupportSlots * (int64_t)sizeof(double);
    return SMI_OK;
}
int smi_denoise_launches(int32_t top_scales, int32_t max_iter, int32_t stages, int32_t *launches) {
    SMI_REQUIRE(top_scales >= 0 && top_scales <= smi::kMaxScales && max_iter > 0 && stages > 0 &&
                    stages <= 7 && launches,
                "scales, iterations, stages or null result");
    SMI_REQUIRE(!(stages & SMI_DENOISE_ITERATE) || (int64_t)max_iter * (6 * top_scales + 1) < INT32_MAX / 2,
                "max_iter");
    *launches = smi::launches(top_scales, max_iter, stages);
    return SMI_OK;
}
int smi_denoise_f32(int32_t n, const smi_denoise_task *tasks, const void *d_tasks, int32_t stages,
                    double K, double epsilon, int32_t max_iter, int32_t positive,
                    const float *d_images, int64_t n_images, double *d_coeffs, int32_t *d_support,
                    double *d_current, int64_t n_coeffs, double *d_x, double *d_work,
                    int64_t n_planes, int32_t *d_iterations, void *d_scratch,
                    int64_t scratch_bytes, void *stream) {
    return smi::denoise<float>(n, tasks, d_tasks, stages, K, epsilon, max_iter, positive, d_images,
                               n_images, d_coeffs, d_support, d_current, n_coeffs, d_x, d_work,
                               n_planes, d_iterations, d_scratch, scratch_bytes, stream);
}
int smi_denoise_f64(int32_t n, const smi_denoise_task *tasks, const void *d_tasks, int32_t stages,
                    double K, double epsilon, int32_t max_iter, int32_t positive,
                    const double *d_images, int64_t n_images, double *d_coeffs, int32_t *d_support,
                    double *d_current, int64_t n_coeffs, double *d_x, double *d_work,
                    int64_t n_planes, int32_t *d_iterations, void *d_scratch,
                    int64_t scratch_bytes, void *stream) {
    return smi::denoise<double>(n, tasks, d_tasks, stages, K, epsilon, max_iter, positive, d_images,
                                n_images, d_coeffs, d_support, d_current, n_coeffs, d_x, d_work,
                                n_planes, d_iterations, d_scratch, scratch_bytes, stream);
}

}  // extern "C"
