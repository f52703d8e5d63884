// get_detect_wavelets (reference scarlet/detect.py:362-399) for a catalogue of blends: the
// coadd of the bands, the starlet transform, the multiresolution support and M * w of every
// blend, in a number of launches that depends on the largest number of scales only.  The
// catalogue is ragged -- frames, band counts and scale counts differ -- so every kernel takes
// a table of tasks (one per blend, validated on the host before anything is launched) and
// grid.y = task; the row, the column and the extents a kernel needs come from the task, never
// from the position in the packed buffers.
//
// Every blend's numbers are those of the per-image chain of starlet.hip for that blend alone
// (smi_coadd_* -> smi_starlet_transform_* -> smi_multiresolution_support_f64 with n = 1), bit
// for bit: the arithmetic is shared with starlet.hip through starlet_device.h.
//   coadd     the sum of the bands in the images' type, then to float64 as plane 0
//   passes    a task with scales <= j leaves at once
//   support   one workgroup owns a blend and runs all of its iterations, convergence test
//             included.  The per-image call sums a plane in support_blocks() blocks and adds
//             the partials in a final block; the workgroup here walks those blocks one after
//             another, so sigma_j, the iteration count and every mask bit equal the per-image
//             call's whatever the data
//   mask      M and M * w from the thresholds the support kernel left in the scratch
//
// The limit: one workgroup reads planes * npix coefficients twice per iteration.  At 65536
// pixels that is 32 virtual blocks, 256 pixels per thread, pass and plane -- beyond it a single
// CU would do alone what the per-image call spreads over more than 32 blocks per plane, and the
// launches and copies batching saves no longer outweigh that.
//
// Nothing is allocated, copied to the host or waited for; no workgroup waits for another and
// nothing is accumulated in global memory.
#include <algorithm>

#include "common.h"
#include "starlet_device.h"

namespace smi {
namespace {

constexpr int kT = kSupportT;
constexpr int32_t kMaxScales = 30;
constexpr int kThrSlots = kSupportSlots;             // thresholds of a task in the scratch
constexpr int64_t kMaxPixels = kSupportMaxPixels;    // pixels of a frame
constexpr int kWork = -1, kNone = -2;                // plane selectors of the pass kernel

// ---------------------------------------------------------------------------- coadd
template <typename T>
__global__ __launch_bounds__(kT) void detect_coadd_kernel(const smi_detect_task *tasks,
                                                          const T *images, double *coeffs) {
    const smi_detect_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w;
    const T *in = images + t.image_off;
    double *out = coeffs + t.coeff_off;
    for (int p = blockIdx.x * kT + threadIdx.x; p < npix; p += gridDim.x * kT) {
        out[p] = (double)strided_sum(in + p, t.bands, npix);
    }
}

// ---------------------------------------------------------------------------- passes
// One 1-D B-spline pass of scale j over every task with more than j scales.  `in`, `out`,
// `diff` select a plane of the task's coefficients, its work plane (kWork) or nothing (kNone):
//   out  : out[p] = conv        diff : diff[p] = diff[p] - conv
// out / diff never select the plane `in` reads.
template <int AXIS>
__global__ __launch_bounds__(kT) void detect_pass_kernel(const smi_detect_task *tasks, int j,
                                                         int in_sel, int out_sel, int diff_sel,
                                                         double *coeffs, double *work) {
    const smi_detect_task t = tasks[blockIdx.y];
    if (t.scales <= j) return;
    const int npix = t.h * t.w;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= npix) return;
    const int y = p / t.w, x = p - y * t.w;
    double *base = coeffs + t.coeff_off, *wk = work + t.work_off;
    const double *c = (in_sel == kWork ? wk : base + (int64_t)in_sel * npix) + p;
    const double acc =
        bspline_tap<AXIS, double, int64_t>(c, y, x, t.h, t.w, bspline_spacing(j, t.h, t.w));
    if (out_sel != kNone) (out_sel == kWork ? wk : base + (int64_t)out_sel * npix)[p] = acc;
    if (diff_sel != kNone) {
        double *d = base + (int64_t)diff_sel * npix + p;
        *d = *d - acc;
    }
}

// ---------------------------------------------------------------------------- support
// The multiresolution support of the blend of this workgroup (support_workgroup of
// starlet_device.h, which denoise_batch.hip runs as well).
__global__ __launch_bounds__(kT) void detect_support_kernel(const smi_detect_task *tasks,
                                                            const double *coeffs, double K,
                                                            double epsilon, int max_iter,
                                                            double *thr_out,
                                                            int32_t *iterations) {
    const smi_detect_task t = tasks[blockIdx.x];
    support_workgroup(coeffs + t.coeff_off, t.scales + 1, t.h * t.w, t.sigma0, t.thresh0, K,
                      epsilon, max_iter, thr_out + (int64_t)blockIdx.x * kThrSlots,
                      iterations + blockIdx.x);
}

// M = |w| > thr as int, and M * w
__global__ __launch_bounds__(kT) void detect_mask_kernel(const smi_detect_task *tasks,
                                                         const double *coeffs, const double *thr,
                                                         int32_t *M, double *Mw) {
    const smi_detect_task t = tasks[blockIdx.y];
    const int npix = t.h * t.w, n = (t.scales + 1) * npix;
    const double *th = thr + (int64_t)blockIdx.y * kThrSlots;
    for (int e = blockIdx.x * kT + threadIdx.x; e < n; e += gridDim.x * kT) {
        const double x = coeffs[t.coeff_off + e];
        const int m = support_member(x, th[e / npix]);
        if (M) M[t.coeff_off + e] = m;
        Mw[t.coeff_off + e] = support_masked(m, x);
    }
}

// ---------------------------------------------------------------------------- host
unsigned blocks_for(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

template <typename T>
int detect_wavelets(int32_t n, const smi_detect_task *tasks, const void *d_tasks, double K,
                    double epsilon, int32_t max_iter, int32_t generation, const T *d_images,
                    int64_t n_images, double *d_coeffs, int64_t n_coeffs, double *d_work,
                    int64_t n_work, double *d_masked, int32_t *d_support, int32_t *d_iterations,
                    void *d_scratch, int64_t scratch_bytes, void *stream) {
    SMI_REQUIRE(n >= 0 && n <= 65535, "task count");
    SMI_REQUIRE((tasks && d_tasks) || n == 0, "null descriptor table");
    SMI_REQUIRE(max_iter > 0, "max_iter must be positive");
    SMI_REQUIRE(generation == 1 || generation == 2, "generation must be 1 or 2");
    SMI_REQUIRE(n_images >= 0 && n_coeffs >= 0 && n_work >= 0, "negative buffer size");
    SMI_REQUIRE((d_images || !n_images) && ((d_coeffs && d_masked) || !n_coeffs) &&
                    (d_work || !n_work), "null buffer");
    SMI_REQUIRE(d_iterations || n == 0, "null iteration counts");
    SMI_REQUIRE(scratch_bytes >= (int64_t)n * kThrSlots * (int64_t)sizeof(double) &&
                    (d_scratch || n == 0), "scratch too small");
    // largest[j]: pixels of the largest frame among the tasks with more than j scales
    // (largest[0] covers every task with a scale; every task is in `all`)
    int64_t largest[kMaxScales + 1] = {0}, all = 0, all_planes = 0;
    int32_t top = 0;
    int64_t coeff_end = 0, work_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_detect_task &t = tasks[i];
        SMI_REQUIRE(t.bands > 0 && t.h > 0 && t.w > 0 && (int64_t)t.h * t.w <= kMaxPixels,
                    "bands or frame extent");
        SMI_REQUIRE(t.scales >= 0 && t.scales <= kMaxScales, "scales");
        const int64_t npix = (int64_t)t.h * t.w;
        SMI_REQUIRE(in_buffer(t.image_off, t.bands * npix, n_images),
                    "images outside their buffer");
        SMI_REQUIRE(t.coeff_off >= coeff_end &&
                        in_buffer(t.coeff_off, (t.scales + 1) * npix, n_coeffs),
                    "coefficients outside their buffer or shared with another task");
        coeff_end = t.coeff_off + (t.scales + 1) * npix;
        SMI_REQUIRE(t.work_off >= work_end && in_buffer(t.work_off, npix, n_work),
                    "work plane outside its buffer or shared with another task");
        work_end = t.work_off + npix;
        for (int32_t j = 0; j < t.scales; ++j) largest[j] = std::max(largest[j], npix);
        top = std::max(top, t.scales);
        all = std::max(all, npix);
        all_planes = std::max(all_planes, (t.scales + 1) * npix);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const smi_detect_task *dt = (const smi_detect_task *)d_tasks;
    double *d_thr = (double *)d_scratch;
    hipLaunchKernelGGL((detect_coadd_kernel<T>), dim3(blocks_for(all), n), dim3(kT), 0, st, dt,
                       d_images, d_coeffs);
    for (int32_t j = 0; j < top; ++j) {
        const dim3 grid(blocks_for(largest[j]), n);
        // c_{j+1} = B_j(c_j); generation 1: w_j = c_j - c_{j+1} in place over c_j,
        // generation 2: w_j = c_j - B_j(c_{j+1})
        hipLaunchKernelGGL(detect_pass_kernel<0>, grid, dim3(kT), 0, st, dt, j, j, kWork, kNone,
                           d_coeffs, d_work);
        hipLaunchKernelGGL(detect_pass_kernel<1>, grid, dim3(kT), 0, st, dt, j, kWork, j + 1,
                           generation == 1 ? j : kNone, d_coeffs, d_work);
        if (generation == 2) {
            hipLaunchKernelGGL(detect_pass_kernel<0>, grid, dim3(kT), 0, st, dt, j, j + 1, kWork,
                               kNone, d_coeffs, d_work);
            hipLaunchKernelGGL(detect_pass_kernel<1>, grid, dim3(kT), 0, st, dt, j, kWork, kNone,
                               j, d_coeffs, d_work);
        }
    }
    hipLaunchKernelGGL(detect_support_kernel, dim3(n), dim3(kT), 0, st, dt, d_coeffs, K, epsilon,
                       max_iter, d_thr, d_iterations);
    hipLaunchKernelGGL(detect_mask_kernel, dim3(std::min(blocks_for(all_planes), 1024u), n),
                       dim3(kT), 0, st, dt, d_coeffs, d_thr, d_support, d_masked);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_detect_wavelets_scratch_bytes(int32_t n, int64_t *bytes) {
    SMI_REQUIRE(n >= 0 && bytes, "task count or null result");
    *bytes = (int64_t)n * smi::kThrSlots * (int64_t)sizeof(double);
    return SMI_OK;
}
int smi_detect_wavelets_f32(int32_t n, const smi_detect_task *tasks, const void *d_tasks, double K,
                            double epsilon, int32_t max_iter, int32_t generation,
                            const float *d_images, int64_t n_images, double *d_coeffs,
                            int64_t n_coeffs, double *d_work, int64_t n_work, double *d_masked,
                            int32_t *d_support, int32_t *d_iterations, void *d_scratch,
                            int64_t scratch_bytes, void *stream) {
    return smi::detect_wavelets<float>(n, tasks, d_tasks, K, epsilon, max_iter, generation,
                                       d_images, n_images, d_coeffs, n_coeffs, d_work, n_work,
                                       d_masked, d_support, d_iterations, d_scratch,
                                       scratch_bytes, stream);
}
int smi_detect_wavelets_f64(int32_t n, const smi_detect_task *tasks, const void *d_tasks, double K,
                            double epsilon, int32_t max_iter, int32_t generation,
                            const double *d_images, int64_t n_images, double *d_coeffs,
                            int64_t n_coeffs, double *d_work, int64_t n_work, double *d_masked,
                            int32_t *d_support, int32_t *d_iterations, void *d_scratch,
                            int64_t scratch_bytes, void *stream) {
    return smi::detect_wavelets<double>(n, tasks, d_tasks, K, epsilon, max_iter, generation,
                                        d_images, n_images, d_coeffs, n_coeffs, d_work, n_work,
                                        d_masked, d_support, d_iterations, d_scratch,
                                        scratch_bytes, stream);
}

}  // extern "C"
