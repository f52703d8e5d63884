// The 16 x 16 tile whose pixels are sums over the taps of a stamp: what lite_spectra.hip and
// measure_sources.hip share.  An image is staged in LDS as float64 on the window the tile's taps
// reach, (16 + kh - 1) x (16 + kw - 1) with zeros where the image has no pixel, and every thread
// of the tile runs the tap loop over it.
#pragma once

#include "common.h"

namespace smi {
namespace window {

constexpr int kTile = 16;

// Row pitch in doubles of the window: 16 (mod 32), so that the two rows of 16 pixels a
// half-wavefront reads (ds_read_b64: 32 bank pairs per half) fall on different banks.
__host__ __device__ inline int window_pitch(int kw) { return (kw - 1 + 31) / 32 * 32 + kTile; }

// a value every lane of the wavefront holds, as one the compiler keeps in a scalar register
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The taps ky (rows; likewise columns) under which some pixel of the tile meets the image's rows
// [r0, r0 + h) of the window: all others add exact zeros (finite stamps) and are skipped.
__device__ __forceinline__ void tap_range(int k, int r0, int h, int *lo, int *hi) {
    *lo = uniform(max(0, k - (r0 + h)));
    *hi = uniform(min(k - 1, k - 1 - r0 + kTile - 1));
}

// Pixel (i, j) of the tile = sum over the taps, rows then columns ascending, of K[ky][kx] *
// window[i + kh - 1 - ky][j + kw - 1 - kx], in float64; the taps are read at wave-uniform
// addresses.
template <typename K>
__device__ __forceinline__ double tap_sum(const double *win, int wp, int i, int j, int kh, int kw,
                                          const K *kern, int ky_lo, int ky_hi, int kx_lo,
                                          int kx_hi) {
    double acc = 0;
    for (int ky = ky_lo; ky <= ky_hi; ++ky) {
        const double *row = win + (i + kh - 1 - ky) * wp + j + kw - 1;
        const K *k = kern + ky * kw;
#pragma unroll 4
        for (int kx = kx_lo; kx <= kx_hi; ++kx) acc += (double)k[kx] * row[-kx];
    }
    return acc;
}

}  // namespace window
}  // namespace smi
