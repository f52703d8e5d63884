// The starlet arithmetic (reference scarlet/wavelet.py:154-408) shared by the kernels of
// starlet.hip -- (n, H, W) stacks of one call, float64 -- of detect_batch.hip -- a ragged table
// of blends, float64 --, of denoise_batch.hip -- the denoising loop of a ragged list of images,
// float64 -- and of starlet_source.hip -- the float32 passes inside the fit loop.
// detect_batch.hip promises every blend the bits of its own starlet.hip chain, and
// lite.init_blends mixes the two paths by frame size: the promise holds because both files
// compute with the functions below, not with copies of them.  A kernel of any of the files
// finds its pixel, plane and thresholds its own way -- grids, loops, barriers and the LDS
// layout stay with the kernel -- and calls these for the numbers.
#pragma once
#include <cmath>

#include "common.h"

namespace smi {
namespace {

// threads of a workgroup that calls block_sum or support_partial
constexpr int kSupportT = 256;

// ---------------------------------------------------------------------------- B-spline
constexpr double kTapOuter = 1.0 / 16, kTapInner = 1.0 / 4, kTapCentre = 3.0 / 8;

// B_j at pixel (y, x) of an (h, w) image along AXIS (0: rows y +- d, y +- 2d; 1: columns),
// c = the pixel itself.  The reference's order,
//   ((((c*h2 + c[-2d]*h0) + c[-d]*h1) + c[+d]*h3) + c[+2d]*h4),
// a term whose neighbour lies outside the image skipped.  I = the index type: 2 * d and the
// offset 2 * d * w are formed in it.
template <int AXIS, typename T, typename I>
__device__ __forceinline__ T bspline_tap(const T *c, I y, I x, I h, I w, I d) {
    const I u = AXIS == 0 ? y : x, L = AXIS == 0 ? h : w, s = AXIS == 0 ? w : (I)1;
    const I d1 = d, d2 = 2 * d1;
    T acc = c[0] * (T)kTapCentre;
    if (u >= d2) acc = acc + *(c - d2 * s) * (T)kTapOuter;
    if (u >= d1) acc = acc + *(c - d1 * s) * (T)kTapInner;
    if (u + d1 < L) acc = acc + *(c + d1 * s) * (T)kTapInner;
    if (u + d2 < L) acc = acc + *(c + d2 * s) * (T)kTapOuter;
    return acc;
}

// The spacing of scale j: a spacing of max(h, w) or more reaches no neighbour along either
// axis, the same result as 2^j.  Every caller admits j <= 30 (starlet.hip: scales < 31,
// detect_batch.hip: scales <= 30, starlet_source.hip: planes <= 31, so j <= 29), where 1 << j
// is an int.
__host__ __device__ inline int bspline_spacing(int j, int h, int w) {
    const int d = 1 << j, m = h > w ? h : w;
    return d < m ? d : m;
}

// ((b0 + b1) + b2) ... of the n values in[0], in[stride], ... in their own type: np.sum over
// the bands of an image, or over the planes of a generation-1 transform
template <typename T>
__device__ __forceinline__ T strided_sum(const T *in, int n, int64_t stride) {
    T acc = in[0];
    for (int k = 1; k < n; ++k) acc = acc + in[(int64_t)k * stride];
    return acc;
}

// ---------------------------------------------------------------------------- support
// sum over a workgroup of kSupportT threads in a fixed order (the same bits on every run);
// thread 0 holds it.  sh: kSupportT / 64 doubles of LDS
__device__ inline double block_sum(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kSupportT / 64; ++w) t += sh[w];
    __syncthreads();
    return t;
}

// Blocks of kSupportT threads that sum one plane of npix pixels, planes_total planes at a
// time: enough to fill the chip, at least ~8 pixels per thread.  The partials of a plane are
// added block by block, so the number is part of the result's bits.
template <typename I>
__host__ __device__ inline I support_blocks(I planes_total, I npix) {
    const I want = (2048 + planes_total - 1) / planes_total;
    const I cap = (npix + 8 * kSupportT - 1) / (8 * kSupportT);
    const I nb = want < cap ? want : cap;
    return nb > 1 ? nb : 1;
}

// M = |w| > thr, and M * w in float64: -0.0 for a negative w outside the support, as the
// reference's int * float product
__device__ __forceinline__ int support_member(double x, double thr) { return fabs(x) > thr ? 1 : 0; }
__device__ __forceinline__ double support_masked(int m, double x) { return (double)m * x; }

// One thread's share of a plane's statistics over v = w * (|w| <= thr), starlets *
// (~M).astype(int) of the reference, at the pixels first, first + stride, ...: pass 0 sums v,
// pass 1 sums (v - mean)^2
template <typename I>
__device__ __forceinline__ double support_partial(const double *w, I first, I stride, I npix,
                                                  double thr, int pass, double mean) {
    double acc = 0;
    for (I q = first; q < npix; q += stride) {
        const double x = w[q];
        const double v = x * (support_member(x, thr) ? 0.0 : 1.0);
        if (pass) {
            const double e = v - mean;
            acc += e * e;
        } else {
            acc += v;
        }
    }
    return acc;
}

// The end of an iteration for one image.  ss[k] = sum of (v - mean)^2 of plane k on entry,
// sigma_k = std(w * ~M) on return.  Converged (returns true) when every sigma > 0 moved by
// less than epsilon of itself; a NaN sigma fails `> 0` and leaves the test.  Otherwise,
// unless this was the last iteration, last = sigma and thr = K * sigma: at max_iter the
// thresholds of the last iteration stay.
__host__ __device__ inline bool support_converged(double *ss, int planes, double npix, double K,
                                                  double epsilon, bool last_iter, double *last,
                                                  double *thr) {
    bool conv = true;
    for (int k = 0; k < planes; ++k) {
        const double sig = sqrt(ss[k] / npix);
        ss[k] = sig;
        if (sig > 0 && !(fabs(sig - last[k]) / sig < epsilon)) conv = false;
    }
    if (!conv && !last_iter)
        for (int k = 0; k < planes; ++k) {
            last[k] = ss[k];
            thr[k] = K * ss[k];
        }
    return conv;
}

// ---------------------------------------------------------------------------- one workgroup
// The whole multiresolution support of one image -- `planes` planes of npix pixels at w0 -- by
// the workgroup of kSupportT threads that calls this, every thread of it: all iterations,
// convergence test included (detect_batch.hip, denoise_batch.hip).  starlet.hip's per-image
// call sums a plane in support_blocks() blocks and adds the partials in a final block; the
// workgroup walks those blocks one after another, so sigma_j, the iteration count and every
// mask bit equal that call's whatever the data.  npix <= kSupportMaxPixels (the partials of a
// plane fit `part`), planes <= kSupportSlots.  Pass 0 of a plane: mean of v = w * ~M; pass 1:
// sum of (v - mean)^2.  thr_out[planes] receives the final thresholds, *iterations the count.
constexpr int kSupportSlots = 32;
constexpr int64_t kSupportMaxPixels = 1 << 16;
constexpr int kSupportMaxVirtual = kSupportMaxPixels / (8 * kSupportT);

__device__ inline void support_workgroup(const double *w0, int planes, int npix, double sigma0,
                                         double thresh0, double K, double epsilon, int max_iter,
                                         double *thr_out, int32_t *iterations) {
    __shared__ double sh[kSupportT / 64];
    __shared__ double part[kSupportMaxVirtual];
    __shared__ double s_thr[kSupportSlots], s_last[kSupportSlots], s_mean[kSupportSlots],
        s_ss[kSupportSlots];
    __shared__ int s_done;
    const int tid = threadIdx.x;
    const int nb = support_blocks<int>(planes, npix);  // <= kSupportMaxVirtual
    if (tid < planes) {
        s_thr[tid] = thresh0;
        s_last[tid] = sigma0;
    }
    __syncthreads();
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
        for (int pass = 0; pass < 2; ++pass) {
            for (int k = 0; k < planes; ++k) {
                const double *w = w0 + (int64_t)k * npix;
                const double thr = s_thr[k];
                const double m = pass ? s_mean[k] : 0.0;
                for (int vb = 0; vb < nb; ++vb) {  // block vb of the per-image call's grid
                    const double acc = support_partial<int>(w, vb * kSupportT + tid,
                                                            nb * kSupportT, npix, thr, pass, m);
                    const double s = block_sum(acc, sh);
                    if (tid == 0) part[vb] = s;
                }
                __syncthreads();
                double acc = 0;  // the final block: partials i, i + 256, ...
                for (int i = tid; i < nb; i += kSupportT) acc += part[i];
                const double s = block_sum(acc, sh);
                if (tid == 0) {
                    if (pass)
                        s_ss[k] = s;
                    else
                        s_mean[k] = s / (double)npix;
                }
            }
            __syncthreads();
        }
        iters = it + 1;
        if (tid == 0)
            s_done = support_converged(s_ss, planes, (double)npix, K, epsilon, it + 1 == max_iter,
                                       s_last, s_thr);
        __syncthreads();
        if (s_done) break;
    }
    if (tid < planes) thr_out[tid] = s_thr[tid];
    if (tid == 0 && iterations) *iterations = iters;
}

}  // namespace
}  // namespace smi
