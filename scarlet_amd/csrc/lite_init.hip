// lite.init_blends: the wavelet initialisation of scarlet.lite (reference
// scarlet/lite/initialization.py:422-605) for a catalogue of blends, a fixed number of launches
// per chunk.  Every entry takes host descriptor tables (validated here, before anything is
// launched), the same tables on the device, and packed device buffers the caller owns (torch
// tensors in lite/initialization.py); nothing is allocated, copied or synchronised here.
//
//   coadd   detectlets / bulgelets / disklets of a blend: its wavelet planes clipped at 0 and
//           added plane after plane, the way np.sum(axis=0) adds them
//   snr     calculate_snr per source: the PSF stamp on the centre, zero outside the frame,
//           accumulated in float64 by one wavefront
//   taps    the centre pixel of apply_filter (operators_pybind11.cc:39-56) per task and band:
//           accumulator from 0, taps in row-major order, one rounded multiply and one rounded
//           add per tap, taps that leave the plane skipped.  The chain of a band is serial:
//           one lane per band
//   masks   prox_monotonic_mask(X, 0, center, max_iter=0) per (source, plane) task by one
//           workgroup: the refitted seed, flood_fill of mask_device.h with variance 0 and
//           threshold 0, then the valid map, the bounds and the value at the seed
//   crop    where(valid, plane, 0) cut to the projected box, zero outside the frame, divided
//           by its maximum (IEEE division)
//   fit     per two-component source and band the five float64 sums of the normal equations
//           of multifit_seds over the union box: both morphologies convolved with the band's
//           stamp (zero outside the box), and the image (zero outside the frame)
//
// No workgroup waits for another, nothing is accumulated in global memory, and every loop
// bound is a descriptor field validated on the host.
#include <type_traits>

#include "common.h"
#include "rounded_math.h"
#include "mask_device.h"

namespace smi {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int32_t kMaxExtent = 1 << 14;    // frame and box sides
constexpr int64_t kMaxPixels = 1 << 22;    // pixels of a frame the one-workgroup fill takes
constexpr int32_t kMaxStamp = 255;         // stamp sides
constexpr int32_t kMaxPlanes = 64;

// ---------------------------------------------------------------------------- coadd
template <typename T>
__global__ __launch_bounds__(kThreads) void coadd_kernel(const smi_lite_init_coadd *tasks,
                                                         const T *wavelets, T *coadds) {
    const smi_lite_init_coadd t = tasks[blockIdx.y];
    const T *src = wavelets + t.wavelet_off;
    T *dst = coadds + t.coadd_off;
    const int64_t N = t.n_pix;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < N;
         p += (int64_t)gridDim.x * kThreads) {
        for (int k = 0; k < 3; ++k) {
            // wavelets[wavelets < 0] = 0; np.sum(planes, axis=0): the first plane, then one
            // rounded add per further plane (an empty selection sums to 0)
            T acc = 0;
            for (int s = 0; s < t.count[k]; ++s) {
                T v = src[(int64_t)(t.first[k] + s * t.step[k]) * N + p];
                if (v < 0) v = 0;
                acc = s == 0 ? v : add_rn(acc, v);
            }
            dst[(int64_t)k * N + p] = acc;
        }
    }
}

// ---------------------------------------------------------------------------- snr
__device__ __forceinline__ double wave_sum(double v) {
    // fixed order: lane i adds lane i + 32, then + 16, ...; lane 0 holds the sum
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kWave) void snr_kernel(const smi_lite_init_snr *tasks, int C,
                                                    const T *images, const T *variance,
                                                    const T *psfs, double *out) {
    const smi_lite_init_snr t = tasks[blockIdx.x];
    const int stamp = t.ph * t.pw, n = C * stamp;
    const int fy0 = t.cy - t.ph / 2, fx0 = t.cx - t.pw / 2;
    double num = 0, den = 0;
    for (int e = threadIdx.x; e < n; e += kWave) {
        const int c = e / stamp, r = e - c * stamp;
        const int i = r / t.pw, j = r - i * t.pw;
        const int y = fy0 + i, x = fx0 + j;
        if (y < 0 || y >= t.h || x < 0 || x >= t.w) continue;  // extract_from fills with 0
        const int64_t at = t.image_off + ((int64_t)c * t.h + y) * t.w + x;
        const double p = (double)psfs[t.psf_off + e];
        num += (double)images[at] * p;
        den += p * (double)variance[at] * p;
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (threadIdx.x == 0) {
        out[2 * (int64_t)blockIdx.x] = num;
        out[2 * (int64_t)blockIdx.x + 1] = den;
    }
}

// ---------------------------------------------------------------------------- taps
template <typename T>
__global__ __launch_bounds__(kWave) void taps_kernel(const smi_lite_init_taps *tasks, int C,
                                                     const T *planes, const T *stamps, T *out) {
    const smi_lite_init_taps t = tasks[blockIdx.x];
    const T *plane = planes + t.plane_off;
    for (int band = threadIdx.x; band < C; band += kWave) {
        const T *k = stamps + t.stamp_off + (int64_t)band * t.kh * t.kw;
        T acc = 0;
        for (int ky = 0; ky < t.kh; ++ky) {
            const int y = t.cy - (ky - t.kh / 2);
            if (y < 0 || y >= t.h) continue;
            for (int kx = 0; kx < t.kw; ++kx) {
                const int x = t.cx - (kx - t.kw / 2);
                if (x < 0 || x >= t.w) continue;
                acc = add_rn(acc, mul_rn(k[ky * t.kw + kx], plane[(int64_t)y * t.w + x]));
            }
        }
        out[t.out_off + band] = acc;
    }
    if (threadIdx.x == 0) out[t.out_off + C] = plane[(int64_t)t.cy * t.w + t.cx];
}

// ---------------------------------------------------------------------------- masks
template <typename T>
struct MaskTaskShared {
    FillShared fill;
    int32_t bounds[4];
    int start;
};

template <typename T>
__global__ __launch_bounds__(kMaskT) void mask_kernel(const smi_lite_init_mask *tasks,
                                                      const T *planes, int32_t *visited,
                                                      uint8_t *unchecked_all, uint8_t *orphans_all,
                                                      uint8_t *valid_all, int32_t *bounds_out,
                                                      T *seed_out) {
    __shared__ MaskTaskShared<T> sh;
    const smi_lite_init_mask t = tasks[blockIdx.x];
    const T *plane = planes + t.plane_off;
    const int rows = t.h, cols = t.w, N = rows * cols, tid = threadIdx.x;
    int32_t *vis = visited + t.pix_off;
    uint8_t *unchecked = unchecked_all + t.pix_off, *orphans = orphans_all + t.pix_off;
    uint8_t *valid = valid_all + t.valid_off;
    // get_center (operator.py:99-129), radius 1: the first maximum, in row-major order, of
    // the window clipped to the plane
    if (tid == 0) {
        const int y0 = max(t.cy - 1, 0), x0 = max(t.cx - 1, 0);
        const int y1 = min(t.cy + 1, rows - 1), x1 = min(t.cx + 1, cols - 1);
        int bi = y0, bj = x0;
        T best = plane[y0 * cols + x0];
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const T val = plane[y * cols + x];
                if (val > best) best = val, bi = y, bj = x;
            }
        sh.start = bi * cols + bj;
        sh.bounds[0] = sh.bounds[1] = bi;
        sh.bounds[2] = sh.bounds[3] = bj;
    }
    __syncthreads();
    const int start = sh.start;
    for (int p = tid; p < N; p += kMaskT) {
        vis[p] = 0;
        unchecked[p] = p != start;
        orphans[p] = 0;
    }
    __syncthreads();
    flood_fill<T>(start, plane, rows, cols, unchecked, orphans, vis, 1, 0.0, 0.0, sh.bounds,
                  &sh.fill);
    // valid = ~(unchecked | orphans)
    for (int p = tid; p < N; p += kMaskT) valid[p] = !(unchecked[p] | orphans[p]);
    if (tid == 0) {
        for (int k = 0; k < 4; ++k) bounds_out[4 * (int64_t)blockIdx.x + k] = sh.bounds[k];
        seed_out[blockIdx.x] = plane[start];
    }
}

// ---------------------------------------------------------------------------- crop
template <typename T>
__global__ __launch_bounds__(kThreads) void crop_kernel(const smi_lite_init_crop *tasks,
                                                        const T *planes, const uint8_t *valid_all,
                                                        T *out_all) {
    __shared__ T best_of[kThreads / kWave];
    __shared__ T peak;
    const smi_lite_init_crop t = tasks[blockIdx.x];
    const T *plane = planes + t.plane_off;
    const uint8_t *valid = valid_all + t.valid_off;
    T *out = out_all + t.out_off;
    const int n = t.bh * t.bw, tid = threadIdx.x;
    T best = -INFINITY;  // np.max of the box (which is never empty)
    for (int e = tid; e < n; e += kThreads) {
        const int i = e / t.bw, j = e - i * t.bw;
        const int y = t.y0 + i, x = t.x0 + j;
        T v = 0;
        if (y >= 0 && y < t.h && x >= 0 && x < t.w) {
            const int64_t p = (int64_t)y * t.w + x;
            if (valid[p]) v = plane[p];
        }
        out[e] = v;
        if (v > best) best = v;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const T other = __shfl_down(best, off, kWave);
        if (other > best) best = other;
    }
    if ((tid & (kWave - 1)) == 0) best_of[tid / kWave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kThreads / kWave; ++i)
            if (best_of[i] > best) best = best_of[i];
        peak = best;
    }
    __syncthreads();
    const T m = peak;
    for (int e = tid; e < n; e += kThreads) out[e] = div_rn(out[e], m);  // own elements only
}

// ---------------------------------------------------------------------------- fit
// sum over the taps of K[ky][kx] * M[i - (ky - kh / 2)][j - (kx - kw / 2)], M the morphology
// on its box at (my, mx) of the union box and 0 elsewhere
template <typename T>
__device__ __forceinline__ double convolved_at(const double *k, int kh, int kw, const T *m,
                                               int my, int mx, int mh, int mw, int i, int j) {
    const int ky_hi = min(kh - 1, i + kh / 2 - my), ky_lo = max(0, i + kh / 2 - my - mh + 1);
    const int kx_hi = min(kw - 1, j + kw / 2 - mx), kx_lo = max(0, j + kw / 2 - mx - mw + 1);
    double acc = 0;
    for (int ky = ky_lo; ky <= ky_hi; ++ky) {
        const T *row = m + (int64_t)(i + kh / 2 - ky - my) * mw;
        for (int kx = kx_lo; kx <= kx_hi; ++kx)
            acc += k[ky * kw + kx] * (double)row[j + kw / 2 - kx - mx];
    }
    return acc;
}

template <typename T, typename I>
__global__ __launch_bounds__(kThreads) void fit_kernel(const smi_lite_init_fit *tasks,
                                                       const T *morphs, const I *images,
                                                       const double *stamps, double *out) {
    __shared__ double part[5][kThreads];
    const smi_lite_init_fit t = tasks[blockIdx.x];
    const int band = blockIdx.y, C = gridDim.y, tid = threadIdx.x;
    const double *k = stamps + t.stamp_off + (int64_t)band * t.kh * t.kw;
    const T *a = morphs + t.a_off, *b = morphs + t.b_off;
    const I *img = images + t.image_off + (int64_t)band * t.h * t.w;
    double s[5] = {0, 0, 0, 0, 0};
    const int n = t.fh * t.fw;
    for (int e = tid; e < n; e += kThreads) {
        const int i = e / t.fw, j = e - i * t.fw;
        const double va = convolved_at<T>(k, t.kh, t.kw, a, t.a_y0 - t.y0, t.a_x0 - t.x0, t.a_h,
                                          t.a_w, i, j);
        const double vb = convolved_at<T>(k, t.kh, t.kw, b, t.b_y0 - t.y0, t.b_x0 - t.x0, t.b_h,
                                          t.b_w, i, j);
        const int y = t.y0 + i, x = t.x0 + j;
        const double d = (y >= 0 && y < t.h && x >= 0 && x < t.w)
                             ? (double)img[(int64_t)y * t.w + x] : 0.0;
        s[0] += va * va, s[1] += va * vb, s[2] += vb * vb, s[3] += va * d, s[4] += vb * d;
    }
    for (int q = 0; q < 5; ++q) part[q][tid] = s[q];
    __syncthreads();
    // fixed tree: the same bits on every run
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (tid < half)
            for (int q = 0; q < 5; ++q) part[q][tid] += part[q][tid + half];
        __syncthreads();
    }
    if (tid < 5) out[((int64_t)blockIdx.x * C + band) * 5 + tid] = part[tid][0];
}

// ---------------------------------------------------------------------------- host checks
#define SMI_TABLES(n, host, dev)                                                   \
    SMI_REQUIRE((n) >= 0, "negative count");                                       \
    SMI_REQUIRE(((host) && (dev)) || (n) == 0, "null descriptor table")

template <typename T>
int init_coadd(int32_t n, const smi_lite_init_coadd *tasks, const void *d_tasks,
               const T *d_wavelets, int64_t n_wavelets, T *d_coadds, int64_t n_coadds,
               void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n <= 65535, "too many blends for one launch");
    SMI_REQUIRE(n_wavelets >= 0 && n_coadds >= 0, "negative buffer size");
    SMI_REQUIRE((d_wavelets || !n_wavelets) && (d_coadds || !n_coadds), "null buffer");
    int64_t largest = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_coadd &t = tasks[i];
        SMI_REQUIRE(t.n_pix > 0 && t.n_pix <= kMaxPixels, "frame extent");
        SMI_REQUIRE(t.n_planes > 0 && t.n_planes <= kMaxPlanes, "wavelet planes");
        SMI_REQUIRE(in_buffer(t.wavelet_off, t.n_planes * t.n_pix, n_wavelets),
                    "wavelets outside their buffer");
        SMI_REQUIRE(in_buffer(t.coadd_off, 3 * t.n_pix, n_coadds), "coadds outside their buffer");
        for (int k = 0; k < 3; ++k) {
            SMI_REQUIRE(t.count[k] >= 0 && t.count[k] <= t.n_planes, "plane count");
            if (t.count[k] == 0) continue;
            const int64_t last = t.first[k] + (int64_t)(t.count[k] - 1) * t.step[k];
            SMI_REQUIRE(t.first[k] >= 0 && t.first[k] < t.n_planes && last >= 0 &&
                            last < t.n_planes && t.step[k] >= -kMaxPlanes && t.step[k] <= kMaxPlanes,
                        "plane selection outside the tensor");
        }
        largest = std::max(largest, t.n_pix);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    const unsigned bx = (unsigned)std::min<int64_t>((largest + kThreads - 1) / kThreads, 1024);
    hipLaunchKernelGGL((coadd_kernel<T>), dim3(bx, n), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_lite_init_coadd *)d_tasks, d_wavelets, d_coadds);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int init_snr(int32_t C, int32_t n, const smi_lite_init_snr *tasks, const void *d_tasks,
             const T *d_images, const T *d_variance, int64_t n_image, const T *d_psfs,
             int64_t n_psf, double *d_out, int64_t n_out, void *stream) {
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_image >= 0 && n_psf >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE(((d_images && d_variance) || !n_image) && (d_psfs || !n_psf) && (d_out || !n_out),
                "null buffer");
    SMI_REQUIRE(2 * (int64_t)n <= n_out, "results outside the output buffer");
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_snr &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "frame extent");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w,
                    "centre outside its frame");
        SMI_REQUIRE(t.ph > 0 && t.pw > 0 && t.ph <= kMaxStamp && t.pw <= kMaxStamp &&
                        (int64_t)C * t.ph * t.pw <= INT32_MAX, "PSF stamp extent");
        SMI_REQUIRE(in_buffer(t.image_off, (int64_t)C * t.h * t.w, n_image),
                    "frame outside the image buffer");
        SMI_REQUIRE(in_buffer(t.psf_off, (int64_t)C * t.ph * t.pw, n_psf),
                    "PSF outside its buffer");
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((snr_kernel<T>), dim3(n), dim3(kWave), 0, (hipStream_t)stream,
                       (const smi_lite_init_snr *)d_tasks, C, d_images, d_variance, d_psfs, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int init_taps(int32_t C, int32_t n, const smi_lite_init_taps *tasks, const void *d_tasks,
              const T *d_planes, int64_t n_plane, const T *d_stamps, int64_t n_stamp, T *d_out,
              int64_t n_out, void *stream) {
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_plane >= 0 && n_stamp >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE((d_planes || !n_plane) && (d_stamps || !n_stamp) && (d_out || !n_out),
                "null buffer");
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_taps &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "plane extent");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w,
                    "centre outside its frame");
        SMI_REQUIRE(t.kh > 0 && t.kw > 0 && t.kh % 2 == 1 && t.kw % 2 == 1 && t.kh <= kMaxStamp &&
                        t.kw <= kMaxStamp, "the stamp must have odd height and width");
        SMI_REQUIRE(in_buffer(t.plane_off, (int64_t)t.h * t.w, n_plane),
                    "plane outside its buffer");
        SMI_REQUIRE(in_buffer(t.stamp_off, (int64_t)C * t.kh * t.kw, n_stamp),
                    "stamp outside its buffer");
        SMI_REQUIRE(in_buffer(t.out_off, (int64_t)C + 1, n_out),
                    "results outside the output buffer");
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((taps_kernel<T>), dim3(n), dim3(kWave), 0, (hipStream_t)stream,
                       (const smi_lite_init_taps *)d_tasks, C, d_planes, d_stamps, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int init_masks(int32_t n, const smi_lite_init_mask *tasks, const void *d_tasks, const T *d_planes,
               int64_t n_plane, int32_t *d_visited, uint8_t *d_unchecked, uint8_t *d_orphans,
               int64_t n_scratch, uint8_t *d_valid, int64_t n_valid, int32_t *d_bounds,
               T *d_values, int64_t n_results, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_plane >= 0 && n_scratch >= 0 && n_valid >= 0 && n_results >= 0,
                "negative buffer size");
    SMI_REQUIRE((d_planes || !n_plane) && ((d_visited && d_unchecked && d_orphans) || !n_scratch) &&
                    (d_valid || !n_valid) && ((d_bounds && d_values) || !n_results),
                "null buffer");
    SMI_REQUIRE(n <= n_results, "results outside the output buffers");
    // the state of a task is its own: scratch ranges in table order must not overlap, nor
    // may two tasks write one valid map
    int64_t scratch_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_mask &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent &&
                        (int64_t)t.h * t.w <= kMaxPixels, "plane extent");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w,
                    "centre outside its frame");
        const int64_t N = (int64_t)t.h * t.w;
        SMI_REQUIRE(in_buffer(t.plane_off, N, n_plane), "plane outside its buffer");
        SMI_REQUIRE(t.pix_off >= scratch_end && in_buffer(t.pix_off, N, n_scratch),
                    "task state outside the scratch buffer or shared with another task");
        scratch_end = t.pix_off + N;
        SMI_REQUIRE(in_buffer(t.valid_off, N, n_valid), "valid map outside its buffer");
        SMI_REQUIRE(i == 0 || t.valid_off >= tasks[i - 1].valid_off +
                                                 (int64_t)tasks[i - 1].h * tasks[i - 1].w,
                    "valid maps must follow each other");
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((mask_kernel<T>), dim3(n), dim3(kMaskT), 0, (hipStream_t)stream,
                       (const smi_lite_init_mask *)d_tasks, d_planes, d_visited, d_unchecked,
                       d_orphans, d_valid, d_bounds, d_values);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int init_crop(int32_t n, const smi_lite_init_crop *tasks, const void *d_tasks, const T *d_planes,
              int64_t n_plane, const uint8_t *d_valid, int64_t n_valid, T *d_out, int64_t n_out,
              void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_plane >= 0 && n_valid >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE((d_planes || !n_plane) && (d_valid || !n_valid) && (d_out || !n_out),
                "null buffer");
    int64_t out_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_crop &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "plane extent");
        SMI_REQUIRE(t.bh > 0 && t.bw > 0 && t.bh <= kMaxExtent && t.bw <= kMaxExtent,
                    "box extent");
        SMI_REQUIRE(t.y0 >= -kMaxExtent && t.y0 <= kMaxExtent && t.x0 >= -kMaxExtent &&
                        t.x0 <= kMaxExtent, "box origin");
        const int64_t N = (int64_t)t.h * t.w;
        SMI_REQUIRE(in_buffer(t.plane_off, N, n_plane), "plane outside its buffer");
        SMI_REQUIRE(in_buffer(t.valid_off, N, n_valid), "valid map outside its buffer");
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, (int64_t)t.bh * t.bw, n_out),
                    "morphology outside the output buffer or shared with another");
        out_end = t.out_off + (int64_t)t.bh * t.bw;
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((crop_kernel<T>), dim3(n), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_lite_init_crop *)d_tasks, d_planes, d_valid, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

// a morphology's box: not empty, inside the union box, its pixels inside the buffer
int check_fit_box(const smi_lite_init_fit &t, int32_t y0, int32_t x0, int32_t h, int32_t w,
                  int64_t off, int64_t n_morph) {
    SMI_REQUIRE(h > 0 && w > 0 && y0 >= t.y0 && x0 >= t.x0 && h <= t.fh - (y0 - t.y0) &&
                    w <= t.fw - (x0 - t.x0), "a morphology's box leaves the union box");
    SMI_REQUIRE(in_buffer(off, (int64_t)h * w, n_morph), "morphology outside its buffer");
    return SMI_OK;
}

template <typename T, typename I>
int init_fit(int32_t C, int32_t n, const smi_lite_init_fit *tasks, const void *d_tasks,
             const T *d_morphs, int64_t n_morph, const I *d_images, int64_t n_image,
             const double *d_stamps, int64_t n_stamp, double *d_out, int64_t n_out,
             void *stream) {
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_morph >= 0 && n_image >= 0 && n_stamp >= 0 && n_out >= 0,
                "negative buffer size");
    SMI_REQUIRE((d_morphs || !n_morph) && (d_images || !n_image) && (d_stamps || !n_stamp) &&
                    (d_out || !n_out), "null buffer");
    SMI_REQUIRE((int64_t)n * C * 5 <= n_out, "sums outside the output buffer");
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_fit &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "frame extent");
        SMI_REQUIRE(t.fh > 0 && t.fw > 0 && t.fh <= kMaxExtent && t.fw <= kMaxExtent &&
                        t.y0 >= -kMaxExtent && t.y0 <= kMaxExtent && t.x0 >= -kMaxExtent &&
                        t.x0 <= kMaxExtent, "union box");
        SMI_REQUIRE(t.kh > 0 && t.kw > 0 && t.kh % 2 == 1 && t.kw % 2 == 1 && t.kh <= kMaxStamp &&
                        t.kw <= kMaxStamp, "the stamp must have odd height and width");
        int rc = check_fit_box(t, t.a_y0, t.a_x0, t.a_h, t.a_w, t.a_off, n_morph);
        if (rc) return rc;
        rc = check_fit_box(t, t.b_y0, t.b_x0, t.b_h, t.b_w, t.b_off, n_morph);
        if (rc) return rc;
        SMI_REQUIRE(in_buffer(t.image_off, (int64_t)C * t.h * t.w, n_image),
                    "frame outside the image buffer");
        SMI_REQUIRE(in_buffer(t.stamp_off, (int64_t)C * t.kh * t.kw, n_stamp),
                    "stamp outside its buffer");
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((fit_kernel<T, I>), dim3(n, C), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_lite_init_fit *)d_tasks, d_morphs, d_images, d_stamps, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

#define SMI_LITE_INIT_ENTRIES(SUFFIX, T)                                                          \
    int smi_lite_init_coadd_##SUFFIX(int32_t n, const smi_lite_init_coadd *tasks,                 \
                                     const void *d_tasks, const T *d_wavelets,                    \
                                     int64_t n_wavelets, T *d_coadds, int64_t n_coadds,           \
                                     void *stream) {                                              \
        return smi::init_coadd<T>(n, tasks, d_tasks, d_wavelets, n_wavelets, d_coadds, n_coadds,  \
                                  stream);                                                        \
    }                                                                                             \
    int smi_lite_init_snr_##SUFFIX(int32_t C, int32_t n, const smi_lite_init_snr *tasks,          \
                                   const void *d_tasks, const T *d_images, const T *d_variance,   \
                                   int64_t n_image, const T *d_psfs, int64_t n_psf,               \
                                   double *d_out, int64_t n_out, void *stream) {                  \
        return smi::init_snr<T>(C, n, tasks, d_tasks, d_images, d_variance, n_image, d_psfs,      \
                                n_psf, d_out, n_out, stream);                                     \
    }                                                                                             \
    int smi_lite_init_taps_##SUFFIX(int32_t C, int32_t n, const smi_lite_init_taps *tasks,        \
                                    const void *d_tasks, const T *d_planes, int64_t n_plane,      \
                                    const T *d_stamps, int64_t n_stamp, T *d_out, int64_t n_out,  \
                                    void *stream) {                                               \
        return smi::init_taps<T>(C, n, tasks, d_tasks, d_planes, n_plane, d_stamps, n_stamp,      \
                                 d_out, n_out, stream);                                           \
    }                                                                                             \
    int smi_lite_init_masks_##SUFFIX(int32_t n, const smi_lite_init_mask *tasks,                  \
                                     const void *d_tasks, const T *d_planes, int64_t n_plane,     \
                                     int32_t *d_visited, uint8_t *d_unchecked,                    \
                                     uint8_t *d_orphans, int64_t n_scratch, uint8_t *d_valid,     \
                                     int64_t n_valid, int32_t *d_bounds, T *d_values,             \
                                     int64_t n_results, void *stream) {                           \
        return smi::init_masks<T>(n, tasks, d_tasks, d_planes, n_plane, d_visited, d_unchecked,   \
                                  d_orphans, n_scratch, d_valid, n_valid, d_bounds, d_values,     \
                                  n_results, stream);                                             \
    }                                                                                             \
    int smi_lite_init_crop_##SUFFIX(int32_t n, const smi_lite_init_crop *tasks,                   \
                                    const void *d_tasks, const T *d_planes, int64_t n_plane,      \
                                    const uint8_t *d_valid, int64_t n_valid, T *d_out,            \
                                    int64_t n_out, void *stream) {                                \
        return smi::init_crop<T>(n, tasks, d_tasks, d_planes, n_plane, d_valid, n_valid, d_out,   \
                                 n_out, stream);                                                  \
    }                                                                                             \
    int smi_lite_init_fit_##SUFFIX(int32_t C, int32_t n, const smi_lite_init_fit *tasks,          \
                                   const void *d_tasks, const T *d_morphs, int64_t n_morph,       \
                                   const void *d_images, int32_t images_f64, int64_t n_image,     \
                                   const double *d_stamps, int64_t n_stamp, double *d_out,        \
                                   int64_t n_out, void *stream) {                                 \
        if (images_f64)                                                                           \
            return smi::init_fit<T, double>(C, n, tasks, d_tasks, d_morphs, n_morph,              \
                                            (const double *)d_images, n_image, d_stamps, n_stamp, \
                                            d_out, n_out, stream);                                \
        return smi::init_fit<T, float>(C, n, tasks, d_tasks, d_morphs, n_morph,                   \
                                       (const float *)d_images, n_image, d_stamps, n_stamp,       \
                                       d_out, n_out, stream);                                     \
    }

SMI_LITE_INIT_ENTRIES(f32, float)
SMI_LITE_INIT_ENTRIES(f64, double)

}  // extern "C"
