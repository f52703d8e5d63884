// lite.init_blends_main: the scarlet-main initialisation of scarlet.lite (reference
// scarlet/lite/initialization.py:188-247, 321-419, use_mask=False) for a catalogue of blends.
// The conventions are those of lite_init.hip: every entry takes a host descriptor table
// (validated here, before anything is launched), the same table on the device, and packed device
// buffers the caller owns; nothing is allocated, copied or synchronised here.  Together with the
// entries of lite_init.hip it reuses, a chunk takes at most EIGHT launches, whatever its blends
// and sources: main_coadd, snr, taps (detection images), taps (model PSFs), main_sweep, crop,
// main_split, fit.
//
//   main_coadd  detect = sum(images / noise_rms**2, axis=0) of a blend: true division, the bands
//               added in order, all in the data type
//   main_sweep  per source, by one workgroup with the source's image in LDS:
//               prox_uncentered_symmetry(detect.copy(), 0, centre, "sdss") while loading, then
//               prox_weighted_monotonic(shape, "angle", min_gradient=0, centre) level by level,
//               then morph[~(morph > thresh)] = 0; writes the plane, the bounds of its pixels > 0
//               and its maximum
//   main_split  bulge = max(morph - level, 0) and disk = min(morph, level) of a normalised
//               cut-out, each divided by its own maximum
//
// The sweep needs neither the (8, H W) weight table nor the radial sort of the reference.  With
// (Y, X) the offset of a pixel from the centre, the cosine of direction i is
// cos(arctan2(-Y, -X) - arctan2(dy_i, dx_i)): one table over relative offsets, made by the host
// with NumPy (so its bits are NumPy's), serves every centre of every frame.  A direction counts
// when its neighbour lies in the frame and strictly nearer the centre; the eight cosines (zeros
// where it does not count) are added in direction order and divided in float64, then cast to the
// data type, as getRadialMonotonicWeights and the native sweep do.  With M = max(|Y|, |X|) and
// m = min(|Y|, |X|) the level 2 M + m - 1 of a strictly nearer 8-neighbour is strictly smaller
// (same M: m drops by one; M - 1: m grows by at most one; M + 1 is never nearer), so the pixels of
// one level never read each other and level after level gives the sequential result.
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "rounded_math.h"

namespace smi {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kMaxSweepThreads = 256;
constexpr int32_t kMaxExtent = 1 << 14;
constexpr int64_t kMaxPixels = 1 << 22;
// LDS of a CU, all of which one workgroup may take, less the reduction scratch of the kernel
constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
template <typename T>
constexpr int64_t max_sweep_pixels() { return (kLdsBytes - kLdsReserve) / sizeof(T); }

// order of the neighbours in every table of the reference (operator.py:84): the 3 x 3 window
// in row-major order without its middle
__host__ __device__ constexpr int dir_dy(int i) { return (i < 4 ? i : i + 1) / 3 - 1; }
__host__ __device__ constexpr int dir_dx(int i) { return (i < 4 ? i : i + 1) % 3 - 1; }

// ---------------------------------------------------------------------------- coadd
template <typename T>
__global__ __launch_bounds__(kThreads) void main_coadd_kernel(
    const smi_lite_init_main_coadd *tasks, const T *images, const T *nr2_all, T *detect) {
    const smi_lite_init_main_coadd t = tasks[blockIdx.y];
    const T *src = images + t.image_off;
    const T *nr2 = nr2_all + t.nr2_off;
    T *dst = detect + t.detect_off;
    const int64_t N = t.n_pix;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < N;
         p += (int64_t)gridDim.x * kThreads) {
        // np.sum(axis=0): the first band, then one rounded add per further band
        T acc = div_rn(src[p], nr2[0]);
        for (int c = 1; c < t.bands; ++c) acc = add_rn(acc, div_rn(src[(int64_t)c * N + p], nr2[c]));
        dst[p] = acc;
    }
}

// ---------------------------------------------------------------------------- sweep
// the rows (or columns) [lo, hi) of the largest sub-array centred on `c` the way
// uncentered_operator cuts it (operator.py:207-260): the shift of the centre from n / 2, doubled,
// one more for an even extent
__device__ __forceinline__ void centred_range(int n, int c, int *lo, int *hi) {
    int d = 2 * (c - n / 2);
    if (n % 2 == 0) d += 1;
    *lo = d > 0 ? d : 0;
    *hi = d < 0 ? n + d : n;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off, kWave);
        if (o > v) v = o;
    }
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, kWave));
    return v;
}

template <typename T>
__global__ __launch_bounds__(kMaxSweepThreads) void main_sweep_kernel(
    const smi_lite_init_main_sweep *tasks, const T *planes, const double *cosines, int ry, int rx,
    T *out_all, int32_t *bounds_out, T *peak_out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int red_i[4][kMaxSweepThreads / kWave];
    __shared__ T red_v[kMaxSweepThreads / kWave];
    T *img = reinterpret_cast<T *>(lds_raw);
    const smi_lite_init_main_sweep t = tasks[blockIdx.x];
    const T *plane = planes + t.plane_off;
    T *out = out_all + t.out_off;
    const int h = t.h, w = t.w, cy = t.cy, cx = t.cx, N = h * w;
    const int tid = threadIdx.x, nt = blockDim.x;

    // ---- load: X[ys, xs] = minimum(X[ys, xs], X[ys, xs][::-1, ::-1]); the rest as it is.  A
    // centre on (h / 2, w / 2) takes the whole array (also for even extents)
    int y_lo = 0, y_hi = h, x_lo = 0, x_hi = w;
    if (!(cy == h / 2 && cx == w / 2)) {
        centred_range(h, cy, &y_lo, &y_hi);
        centred_range(w, cx, &x_lo, &x_hi);
    }
    for (int p = tid; p < N; p += nt) {
        const int y = p / w, x = p - y * w;
        T v = plane[p];
        if (y >= y_lo && y < y_hi && x >= x_lo && x < x_hi) {
            const T o = plane[(y_lo + y_hi - 1 - y) * w + (x_lo + x_hi - 1 - x)];
            v = v < o ? v : o;
        }
        img[p] = v;
    }
    __syncthreads();

    // ---- sweep: level L holds the pixels with 2 M + m - 1 == L, eight per (M, m) -- the signs
    // of Y and X and which of them is the major one -- less the duplicates on axes and diagonals
    const int my = max(cy, h - 1 - cy), mx = max(cx, w - 1 - cx);
    const int m_max = max(my, mx);
    const int last = 2 * m_max + min(my, mx) - 1;  // the farthest corner has the highest level
    const int pitch = 2 * rx + 1;
    for (int L = 0; L <= last; ++L) {
        const int M_lo = (L + 3) / 3;                  // m = L + 1 - 2 M <= M
        const int M_hi = min((L + 1) / 2, m_max);      // m >= 0
        const int n_entries = 8 * (M_hi - M_lo + 1);
        for (int e = tid; e < n_entries; e += nt) {
            const int M = M_lo + (e >> 3), oct = e & 7;
            const int m = L + 1 - 2 * M;
            const bool swap = oct & 4, neg_major = oct & 1, neg_minor = oct & 2;
            if ((m == 0 && neg_minor) || (m == M && swap)) continue;  // the same pixel twice
            const int a = neg_major ? -M : M, b = neg_minor ? -m : m;
            const int Y = swap ? b : a, X = swap ? a : b;
            const int y = cy + Y, x = cx + X;
            if (y < 0 || y >= h || x < 0 || x >= w) continue;
            const double *cs = cosines + ((int64_t)(Y + ry) * pitch + (X + rx)) * 8;
            const int r2 = Y * Y + X * X;
            double c[8], total = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ny = Y + dir_dy(i), nx = X + dir_dx(i);
                const bool counts = cy + ny >= 0 && cy + ny < h && cx + nx >= 0 && cx + nx < w &&
                                    ny * ny + nx * nx < r2;
                c[i] = counts ? cs[i] : 0.0;
                total = __dadd_rn(total, c[i]);
            }
            if (total == 0) total = 1;
            T ref = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (c[i] > 0) {
                    const T wt = (T)__ddiv_rn(c[i], total);
                    if (wt > 0)
                        ref = add_rn(ref, mul_rn(img[(y + dir_dy(i)) * w + (x + dir_dx(i))], wt));
                }
            }
            const T lim = mul_rn(ref, (T)1);  // ref * (1 - min_gradient)
            const int p = y * w + x;
            if (lim < img[p]) img[p] = lim;
        }
        __syncthreads();
    }

    // ---- trim, the bounds of what is left, its maximum
    const double thresh = t.thresh;
    int b0 = INT_MAX, b1 = INT_MAX, b2 = INT_MAX, b3 = INT_MAX;  // min row, -max row, min col, -max col
    T best = -INFINITY;  // np.max of the plane; a thread without a pixel adds nothing to it
    for (int p = tid; p < N; p += nt) {
        T v = img[p];
        if (!((double)v > thresh)) v = 0;
        out[p] = v;
        if (v > best) best = v;
        if (v > 0) {
            const int y = p / w, x = p - y * w;
            b0 = min(b0, y), b1 = min(b1, -y), b2 = min(b2, x), b3 = min(b3, -x);
        }
    }
    best = wave_max(best);
    b0 = wave_min(b0), b1 = wave_min(b1), b2 = wave_min(b2), b3 = wave_min(b3);
    if ((tid & (kWave - 1)) == 0) {
        const int wv = tid / kWave;
        red_v[wv] = best;
        red_i[0][wv] = b0, red_i[1][wv] = b1, red_i[2][wv] = b2, red_i[3][wv] = b3;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < nt / kWave; ++k) {
            if (red_v[k] > best) best = red_v[k];
            b0 = min(b0, red_i[0][k]), b1 = min(b1, red_i[1][k]);
            b2 = min(b2, red_i[2][k]), b3 = min(b3, red_i[3][k]);
        }
        int32_t *bo = bounds_out + 4 * (int64_t)blockIdx.x;
        const bool none = b0 == INT_MAX;  // no pixel > 0: (0, -1, 0, -1)
        bo[0] = none ? 0 : b0, bo[1] = none ? -1 : -b1, bo[2] = none ? 0 : b2, bo[3] = none ? -1 : -b3;
        peak_out[blockIdx.x] = best;
    }
}

// ---------------------------------------------------------------------------- split
template <typename T>
__device__ __forceinline__ T block_max(T best, T *scratch, T *result) {
    best = wave_max(best);
    const int tid = threadIdx.x;
    __syncthreads();  // (scratch may still be read from a previous call)
    if ((tid & (kWave - 1)) == 0) scratch[tid / kWave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kThreads / kWave; ++i)
            if (scratch[i] > best) best = scratch[i];
        *result = best;
    }
    __syncthreads();
    return *result;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void main_split_kernel(const smi_lite_init_main_split *tasks,
                                                              T *morphs, T level) {
    __shared__ T scratch[kThreads / kWave];
    __shared__ T result;
    const smi_lite_init_main_split t = tasks[blockIdx.x];
    const T *morph = morphs + t.morph_off;
    T *bulge = morphs + t.bulge_off, *disk = morphs + t.disk_off;
    const int n = t.bh * t.bw, tid = threadIdx.x;
    T best_b = -INFINITY, best_d = -INFINITY;
    for (int e = tid; e < n; e += kThreads) {
        const T v = morph[e];
        // np.maximum(morph - level, 0), np.minimum(morph, level)
        const T d = add_rn(v, -level);
        const T b = d > 0 ? d : (T)0;
        const T k = v < level ? v : level;
        bulge[e] = b, disk[e] = k;
        if (b > best_b) best_b = b;
        if (k > best_d) best_d = k;
    }
    const T mb = block_max(best_b, scratch, &result);
    const T md = block_max(best_d, scratch, &result);
    for (int e = tid; e < n; e += kThreads) {  // own elements only
        bulge[e] = div_rn(bulge[e], mb);
        disk[e] = div_rn(disk[e], md);
    }
}

// ---------------------------------------------------------------------------- host checks
#define SMI_TABLES(n, host, dev)                                                   \
    SMI_REQUIRE((n) >= 0, "negative count");                                       \
    SMI_REQUIRE(((host) && (dev)) || (n) == 0, "null descriptor table")

template <typename T>
int main_coadd(int32_t n, const smi_lite_init_main_coadd *tasks, const void *d_tasks,
               const T *d_images, int64_t n_image, const T *d_nr2, int64_t n_nr2, T *d_detect,
               int64_t n_detect, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n <= 65535, "too many blends for one launch");
    SMI_REQUIRE(n_image >= 0 && n_nr2 >= 0 && n_detect >= 0, "negative buffer size");
    SMI_REQUIRE((d_images || !n_image) && (d_nr2 || !n_nr2) && (d_detect || !n_detect),
                "null buffer");
    int64_t largest = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_main_coadd &t = tasks[i];
        SMI_REQUIRE(t.n_pix > 0 && t.n_pix <= kMaxPixels, "frame extent");
        SMI_REQUIRE(t.bands > 0 && t.bands <= 65535, "bands");
        SMI_REQUIRE(in_buffer(t.image_off, (int64_t)t.bands * t.n_pix, n_image),
                    "frame outside the image buffer");
        SMI_REQUIRE(in_buffer(t.nr2_off, t.bands, n_nr2), "noise levels outside their buffer");
        SMI_REQUIRE(in_buffer(t.detect_off, t.n_pix, n_detect),
                    "detection image outside its buffer");
        largest = std::max(largest, t.n_pix);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    const unsigned bx = (unsigned)std::min<int64_t>((largest + kThreads - 1) / kThreads, 1024);
    hipLaunchKernelGGL((main_coadd_kernel<T>), dim3(bx, n), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_lite_init_main_coadd *)d_tasks, d_images, d_nr2, d_detect);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int main_sweep(int32_t n, const smi_lite_init_main_sweep *tasks, const void *d_tasks,
               const T *d_planes, int64_t n_plane, const double *d_cos, int64_t n_cos, int32_t ry,
               int32_t rx, T *d_out, int64_t n_out, int32_t *d_bounds, T *d_peaks,
               int64_t n_results, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_plane >= 0 && n_out >= 0 && n_results >= 0 && n_cos >= 0,
                "negative buffer size");
    SMI_REQUIRE((d_planes || !n_plane) && (d_out || !n_out) && (d_cos || !n_cos) &&
                    ((d_bounds && d_peaks) || !n_results), "null buffer");
    SMI_REQUIRE(n <= n_results, "results outside the output buffers");
    SMI_REQUIRE(ry >= 0 && rx >= 0 && ry < kMaxExtent && rx < kMaxExtent &&
                    n_cos == (int64_t)(2 * ry + 1) * (2 * rx + 1) * 8,
                "the cosine table does not have (2 ry + 1) (2 rx + 1) 8 entries");
    int64_t out_end = 0, largest = 0;
    int widest = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_main_sweep &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "plane extent");
        const int64_t N = (int64_t)t.h * t.w;
        SMI_REQUIRE(N <= max_sweep_pixels<T>(), "frame beyond the LDS image of the sweep");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w,
                    "centre outside its frame");
        SMI_REQUIRE(t.h - 1 <= ry && t.w - 1 <= rx, "frame beyond the cosine table");
        SMI_REQUIRE(in_buffer(t.plane_off, N, n_plane), "plane outside its buffer");
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, N, n_out),
                    "swept plane outside the output buffer or shared with another");
        out_end = t.out_off + N;
        largest = std::max(largest, N);
        // a level holds at most eight pixels for each of its M / 3 + 1 values of M
        const int m_max = std::max(std::max(t.cy, t.h - 1 - t.cy), std::max(t.cx, t.w - 1 - t.cx));
        widest = std::max(widest, 8 * (m_max / 3 + 1));
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    const size_t lds = (size_t)largest * sizeof(T);
    static size_t cfg[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(main_sweep_kernel<T>), lds, cfg)))
        return rc;
    // the workgroup is as wide as the widest level, not as the frame
    const int threads = std::min(kMaxSweepThreads, (widest + kWave - 1) / kWave * kWave);
    hipLaunchKernelGGL((main_sweep_kernel<T>), dim3(n), dim3(threads), lds, (hipStream_t)stream,
                       (const smi_lite_init_main_sweep *)d_tasks, d_planes, d_cos, ry, rx, d_out,
                       d_bounds, d_peaks);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

template <typename T>
int main_split(int32_t n, const smi_lite_init_main_split *tasks, const void *d_tasks, T *d_morphs,
               int64_t n_morph, double level, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_morph >= 0, "negative buffer size");
    SMI_REQUIRE(d_morphs || !n_morph, "null buffer");
    int64_t end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_lite_init_main_split &t = tasks[i];
        SMI_REQUIRE(t.bh > 0 && t.bw > 0 && t.bh <= kMaxExtent && t.bw <= kMaxExtent,
                    "box extent");
        const int64_t N = (int64_t)t.bh * t.bw;
        SMI_REQUIRE(in_buffer(t.morph_off, N, n_morph), "morphology outside its buffer");
        // bulge and disk are written: after everything an earlier task touches, and apart
        SMI_REQUIRE(t.morph_off >= end && t.bulge_off >= t.morph_off + N &&
                        t.disk_off >= t.bulge_off + N && in_buffer(t.disk_off, N, n_morph),
                    "bulge or disk outside the buffer or shared with another morphology");
        end = t.disk_off + N;
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL((main_split_kernel<T>), dim3(n), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_lite_init_main_split *)d_tasks, d_morphs, (T)level);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

#define SMI_LITE_INIT_MAIN_ENTRIES(SUFFIX, T)                                                     \
    int smi_lite_init_main_coadd_##SUFFIX(int32_t n, const smi_lite_init_main_coadd *tasks,       \
                                          const void *d_tasks, const T *d_images,                 \
                                          int64_t n_image, const T *d_nr2, int64_t n_nr2,         \
                                          T *d_detect, int64_t n_detect, void *stream) {          \
        return smi::main_coadd<T>(n, tasks, d_tasks, d_images, n_image, d_nr2, n_nr2, d_detect,   \
                                  n_detect, stream);                                              \
    }                                                                                             \
    int smi_lite_init_main_sweep_##SUFFIX(int32_t n, const smi_lite_init_main_sweep *tasks,       \
                                          const void *d_tasks, const T *d_planes,                 \
                                          int64_t n_plane, const double *d_cos, int64_t n_cos,    \
                                          int32_t ry, int32_t rx, T *d_out, int64_t n_out,        \
                                          int32_t *d_bounds, T *d_peaks, int64_t n_results,       \
                                          void *stream) {                                         \
        return smi::main_sweep<T>(n, tasks, d_tasks, d_planes, n_plane, d_cos, n_cos, ry, rx,     \
                                  d_out, n_out, d_bounds, d_peaks, n_results, stream);            \
    }                                                                                             \
    int smi_lite_init_main_split_##SUFFIX(int32_t n, const smi_lite_init_main_split *tasks,       \
                                          const void *d_tasks, T *d_morphs, int64_t n_morph,      \
                                          double level, void *stream) {                           \
        return smi::main_split<T>(n, tasks, d_tasks, d_morphs, n_morph, level, stream);           \
    }

SMI_LITE_INIT_MAIN_ENTRIES(f32, float)
SMI_LITE_INIT_MAIN_ENTRIES(f64, double)

}  // extern "C"
