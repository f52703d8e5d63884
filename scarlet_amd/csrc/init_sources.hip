// initialization.init_blends: the morphology part of initialization.init_all_sources
// (reference scarlet/initialization.py:30-170, 287-363; source.py:249-522) for a catalogue of
// blends.  The conventions are those of lite_init_main.hip: every entry takes a host descriptor
// table (validated here, before anything is launched), the same table on the device, and packed
// device buffers the caller owns; nothing is allocated, copied or synchronised here; every loop
// bound is a descriptor field.  A chunk takes FIVE launches, whatever its blends and sources:
//
//   psf_snr  per (source, band), over the box of the observation's PSF stamp on the source's
//            pixel: sum d p, sum p p and sum p var p in float64.  Pixels beyond the frame hold
//            zero data and zero noise and pixels without weight are left out, as
//            get_psf_spectrum does; the caller marks them with a negated variance (the coadd
//            of the loop reads the variance cube as it is, also there: sweep takes its
//            magnitude).  The stamps are float64.  Lane l of the one wavefront adds
//            the stamp entries l, l + 64, ... in that order and one lane adds the 64 partial
//            sums in lane order: an order the stamp alone fixes.
//   sweep    per source, by one workgroup with the source's plane in LDS as float64: the coadd
//            of build_initialization_image with the source's pixel spectrum (w = 1 / var in the
//            data type where var > 0, else 0; w *= s_c; the bands of w d added in order from
//            zero), prox_uncentered_symmetry(.., "sdss") about the pixel, the 'flat' monotonic
//            sweep without minimal gradient level by level, then
//            morph[~(morph > thresh * sqrt(sum_c s_c w_c))] = 0 with the noise level formed again
//            at that point; writes the plane, the bounds of its pixels > 0 and its maximum
//   crop     per source: the cut-out of a square box (zeros beyond the frame) divided by its
//            maximum -- one lit pixel in the middle where nothing is left --, np.maximum with the
//            floor the host made for the box side (the peak-normalised model PSF), for two
//            components the split of MultiExtendedSource.init_morphs at a percentage of the
//            peak, each layer divided by its own maximum; and whether anything written is not
//            finite, or the cut-out was empty
//   spectra_tiles, spectra_reduce  the float64 weighted normal equations of
//            set_spectra_to_match, tile by tile (below)
//
// The level argument in the header of lite_init_main.hip covers the 'flat' weights unchanged:
// the neighbours that count are the same (inside the frame and strictly nearer the centre), each
// with weight 1 / their number, and the reference adds the products in direction order.
// No atomics, no workgroup waits for another: a source's bits depend on its own task alone.
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "rounded_math.h"

namespace smi {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int32_t kMaxExtent = 1 << 14;
constexpr int32_t kMaxStamp = 63;
constexpr int32_t kMaxBands = 65535;
constexpr int32_t kMaxSide = 1 << 12;
// LDS of a CU, all of which one workgroup may take, less the reduction scratch of the kernel
constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
constexpr int64_t kMaxSweepPixels = (kLdsBytes - kLdsReserve) / sizeof(double);

// order of the neighbours in every table of the reference (operator.py:84): the 3 x 3 window
// in row-major order without its middle
__host__ __device__ constexpr int dir_dy(int i) { return (i < 4 ? i : i + 1) / 3 - 1; }
__host__ __device__ constexpr int dir_dx(int i) { return (i < 4 ? i : i + 1) % 3 - 1; }

__device__ __forceinline__ double wave_max(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, kWave);
        if (o > v) v = o;
    }
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, kWave));
    return v;
}

// ---------------------------------------------------------------------------- psf_snr
__global__ __launch_bounds__(kWave) void psf_snr_kernel(const smi_init_sources_psf_snr *tasks,
                                                        const float *data, const float *var,
                                                        const double *psfs, double *out) {
    __shared__ double part[3][kWave];
    const smi_init_sources_psf_snr t = tasks[blockIdx.x];
    const int c = blockIdx.y;
    if (c >= t.bands) return;
    const int64_t N = (int64_t)t.h * t.w;
    const float *d = data + t.cube_off + c * N, *v = var + t.cube_off + c * N;
    const double *p = psfs + t.psf_off + (int64_t)c * t.ph * t.pw;
    const int y0 = t.cy - t.ph / 2, x0 = t.cx - t.pw / 2, n = t.ph * t.pw;
    const int lane = threadIdx.x;
    double dp = 0, pp = 0, pvp = 0;
    for (int e = lane; e < n; e += kWave) {
        const int sy = e / t.pw, sx = e - sy * t.pw;
        const int y = y0 + sy, x = x0 + sx;
        const double pe = p[e];
        if (y < 0 || y >= t.h || x < 0 || x >= t.w) {  // zero data, zero noise, not masked
            pp = __dadd_rn(pp, __dmul_rn(pe, pe));
            continue;
        }
        const int64_t q = (int64_t)y * t.w + x;
        const double s2 = (double)v[q];
        if (!(s2 > 0)) continue;  // no weight: masked
        dp = __dadd_rn(dp, __dmul_rn((double)d[q], pe));
        pp = __dadd_rn(pp, __dmul_rn(pe, pe));
        pvp = __dadd_rn(pvp, __dmul_rn(__dmul_rn(pe, s2), pe));
    }
    part[0][lane] = dp, part[1][lane] = pp, part[2][lane] = pvp;
    __syncthreads();
    if (lane < 3) {
        double total = 0;
        for (int l = 0; l < kWave; ++l) total = __dadd_rn(total, part[lane][l]);
        out[t.out_off + 3 * (int64_t)c + lane] = total;
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

__global__ __launch_bounds__(kThreads) void sweep_kernel(const smi_init_sources_sweep *tasks,
                                                         const float *data, const float *var,
                                                         const double *spectra, double *out_all,
                                                         int32_t *bounds_out, double *peak_out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int red_i[4][kThreads / kWave];
    __shared__ double red_v[kThreads / kWave];
    double *img = reinterpret_cast<double *>(lds_raw);
    const smi_init_sources_sweep t = tasks[blockIdx.x];
    const float *d = data + t.cube_off, *v = var + t.cube_off;
    const double *spec = spectra + t.spec_off;
    double *out = out_all + t.out_off;
    const int h = t.h, w = t.w, cy = t.cy, cx = t.cx, N = h * w, C = t.bands;
    const int tid = threadIdx.x, nt = blockDim.x;

    // ---- coadd: weight = where(var > 0, 1 / var, 0) (the quotient in the data type);
    // weight *= s_c; (weight * d).sum(axis=(0, 1)) from zero, band after band
    for (int p = tid; p < N; p += nt) {
        double acc = 0;
        for (int c = 0; c < C; ++c) {
            const float vc = fabsf(v[(int64_t)c * N + p]);  // (negated: no weight)
            double wt = vc > 0.f ? (double)div_rn(1.f, vc) : 0.0;
            wt = mul_rn(wt, spec[c]);
            acc = add_rn(acc, mul_rn(wt, (double)d[(int64_t)c * N + p]));
        }
        img[p] = acc;
    }
    __syncthreads();

    // ---- symmetry: X[ys, xs] = minimum(X[ys, xs], X[ys, xs][::-1, ::-1]); the rest as it is.
    // A centre on (h / 2, w / 2) takes the whole array (also for even extents).  The thread of
    // the first pixel of a pair writes both.
    int y_lo = 0, y_hi = h, x_lo = 0, x_hi = w;
    if (!(cy == h / 2 && cx == w / 2)) {
        centred_range(h, cy, &y_lo, &y_hi);
        centred_range(w, cx, &x_lo, &x_hi);
    }
    for (int p = tid; p < N; p += nt) {
        const int y = p / w, x = p - y * w;
        if (y >= y_lo && y < y_hi && x >= x_lo && x < x_hi) {
            const int q = (y_lo + y_hi - 1 - y) * w + (x_lo + x_hi - 1 - x);
            if (p < q) {
                const double a = img[p], b = img[q];
                const double m = a < b ? a : b;
                img[p] = m, img[q] = m;
            }
        }
    }
    __syncthreads();

    // ---- sweep: level L holds the pixels with 2 M + m - 1 == L, eight per (M, m) -- the signs
    // of Y and X and which of them is the major one -- less the duplicates on axes and diagonals
    const int my = max(cy, h - 1 - cy), mx = max(cx, w - 1 - cx);
    const int m_max = max(my, mx);
    const int last = 2 * m_max + min(my, mx) - 1;  // the farthest corner has the highest level
    for (int L = 0; L <= last; ++L) {
        const int M_lo = (L + 3) / 3;              // m = L + 1 - 2 M <= M
        const int M_hi = min((L + 1) / 2, m_max);  // m >= 0
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
            const int r2 = Y * Y + X * X;
            bool counts[8];
            int n_counts = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ny = Y + dir_dy(i), nx = X + dir_dx(i);
                counts[i] = cy + ny >= 0 && cy + ny < h && cx + nx >= 0 && cx + nx < w &&
                            ny * ny + nx * nx < r2;
                n_counts += counts[i];
            }
            // cosw / total of getRadialMonotonicWeights: 1.0 / count
            const double wt = div_rn(1.0, (double)(n_counts ? n_counts : 1));
            double ref = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (counts[i])
                    ref = add_rn(ref, mul_rn(img[(y + dir_dy(i)) * w + (x + dir_dx(i))], wt));
            const double lim = mul_rn(ref, 1.0);  // ref * (1 - min_gradient)
            const int p = y * w + x;
            if (lim < img[p]) img[p] = lim;
        }
        __syncthreads();
    }

    // ---- trim at thresh * std, std = sqrt((spectrum * weight).sum(axis=(0, 1))) formed again;
    // the bounds of what is left, its maximum
    const double thresh = t.thresh;
    int b0 = INT_MAX, b1 = INT_MAX, b2 = INT_MAX, b3 = INT_MAX;  // min row, -max row, min col, -max col
    double best = -INFINITY;
    for (int p = tid; p < N; p += nt) {
        double acc = 0;
        for (int c = 0; c < C; ++c) {
            const float vc = fabsf(v[(int64_t)c * N + p]);  // (negated: no weight)
            double wt = vc > 0.f ? (double)div_rn(1.f, vc) : 0.0;
            wt = mul_rn(wt, spec[c]);
            acc = add_rn(acc, mul_rn(spec[c], wt));
        }
        const double bg = mul_rn(__dsqrt_rn(acc), thresh);
        double val = img[p];
        if (!(val > bg)) val = 0;
        out[p] = val;
        if (val > best) best = val;
        if (val > 0) {
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

// ---------------------------------------------------------------------------- crop
__device__ __forceinline__ double block_max(double best, double *scratch, double *result) {
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

__global__ __launch_bounds__(kThreads) void crop_kernel(const smi_init_sources_crop *tasks,
                                                        const double *planes, const double *floors,
                                                        double *out_all, int32_t *flags) {
    __shared__ double scratch[kThreads / kWave];
    __shared__ double result;
    __shared__ int bad_any;
    const smi_init_sources_crop t = tasks[blockIdx.x];
    const double *plane = planes + t.plane_off, *floor_img = floors + t.floor_off;
    const int side = t.side, n = side * side, tid = threadIdx.x;
    double *first = out_all + t.out_off, *second = first + n;
    if (tid == 0) bad_any = 0;
    // ---- bbox.extract_from(morph): zeros beyond the frame
    double best = -INFINITY;
    for (int e = tid; e < n; e += kThreads) {
        const int by = e / side, bx = e - by * side;
        const int y = t.y0 + by, x = t.x0 + bx;
        const double val = (y >= 0 && y < t.h && x >= 0 && x < t.w) ? plane[(int64_t)y * t.w + x] : 0.0;
        first[e] = val;  // (own elements only, here and below)
        if (val > best) best = val;
    }
    const double peak = block_max(best, scratch, &result);
    // ---- image /= image.max(), or CenterOnConstraint(tiny=1) of an empty image; then the floor
    const int middle = (side / 2) * side + side / 2;
    best = -INFINITY;
    for (int e = tid; e < n; e += kThreads) {
        double val = first[e];
        if (peak > 0)
            val = div_rn(val, peak);
        else if (e == middle)
            val = val > 1.0 ? val : 1.0;
        const double fl = floor_img[e];
        val = val >= fl ? val : fl;  // np.maximum of finite values
        first[e] = val;
        if (val > best) best = val;
    }
    bool bad = false;
    if (t.layers == 2) {
        // ---- MultiExtendedSource.init_morphs with one percentile: cut = perc * peak / 100
        const double top = block_max(best, scratch, &result);
        const double cut = div_rn(mul_rn(t.percentile, top), 100.0);
        double best0 = -INFINITY, best1 = -INFINITY;
        for (int e = tid; e < n; e += kThreads) {
            const double val = first[e];
            const bool inside = val > cut;
            const double lo = inside ? cut : val;
            const double hi = inside ? add_rn(val, -cut) : 0.0;
            first[e] = lo, second[e] = hi;
            if (lo > best0) best0 = lo;
            if (hi > best1) best1 = hi;
        }
        const double m0 = block_max(best0, scratch, &result);
        const double m1 = block_max(best1, scratch, &result);
        for (int e = tid; e < n; e += kThreads) {
            const double lo = div_rn(first[e], m0), hi = div_rn(second[e], m1);
            first[e] = lo, second[e] = hi;
            bad = bad || !isfinite(lo) || !isfinite(hi);
        }
    } else {
        for (int e = tid; e < n; e += kThreads) bad = bad || !isfinite(first[e]);
    }
    __syncthreads();
    if (bad) bad_any = 1;  // (every writer stores the same value)
    __syncthreads();
    if (tid == 0) flags[blockIdx.x] = bad_any | (peak > 0 ? 0 : 2);
}

// ---------------------------------------------------------------------------- spectra
// The weighted counterpart of lite_spectra.hip (a second copy of its tile scheme: the columns
// here are clipped to the frame, carry weights, and two more sums per component are formed).
// A blend's REGION is the part of its frame the convolved models can reach; it is cut into
// 16 x 16 tiles.  Per (tile, band) one workgroup keeps in LDS the columns of the components
// present there -- the morphology, zero outside its box and outside the frame, convolved "same"
// with the band's stamp, thread = pixel, taps in row-major order -- and the data and weight
// columns.  Then per pair of columns 8 consecutive lanes add the 8 segments of 32 pixels, each
// in pixel order, and a fixed butterfly adds the 8: G = sum (a_p w) a_q, r = sum (a_p w) d,
// sum a_p w and sum a_p.  A tile writes its full table, exact zeros for what is not present.
constexpr int kTile = 16;
constexpr int kSegs = 8, kSegLen = kThreads / kSegs;  // 8 x 32 pixels
constexpr int kPitch = kThreads + kSegs;              // doubles of a column: one pad per segment
constexpr int kMaxComponents = 64;                    // of a blend: one wavefront finds the present
constexpr int kMaxPresent = 32;                       // on one tile: 34 columns, 70 KiB
constexpr int32_t kMaxCoord = 1 << 24;
static_assert(kThreads == kTile * kTile, "one thread per pixel of a tile");

struct Tile {
    int y0, x0, h, w;  // in region coordinates
};

__host__ __device__ inline Tile tile_of(const smi_init_sources_spectra_blend &bl, int tile) {
    const int tiles_x = (bl.fw + kTile - 1) / kTile;
    Tile t;
    t.y0 = (tile / tiles_x) * kTile, t.x0 = (tile % tiles_x) * kTile;
    t.h = bl.fh - t.y0 < kTile ? bl.fh - t.y0 : kTile;
    t.w = bl.fw - t.x0 < kTile ? bl.fw - t.x0 : kTile;
    return t;
}
__host__ __device__ inline int tiles_of(const smi_init_sources_spectra_blend &bl) {
    return ((bl.fh + kTile - 1) / kTile) * ((bl.fw + kTile - 1) / kTile);
}
// entries of a blend's table per band: G (K x K), r, sum m w, sum m
__host__ __device__ inline int entries_of(int K) { return K * K + 3 * K; }
// row pitch in doubles of the window a morphology is staged in: 16 (mod 32)
__host__ __device__ inline int window_pitch(int kw) { return (kw - 1 + 31) / 32 * 32 + kTile; }

// does the component's box, grown by the stamp's half, meet the tile?
__host__ __device__ inline bool present_on(const smi_init_sources_spectra_blend &bl,
                                           const smi_init_sources_spectra_component &d,
                                           const Tile &t) {
    const int cy = d.y0 - bl.y0, cx = d.x0 - bl.x0, kh = bl.kh, kw = bl.kw;
    return cy - kh / 2 < t.y0 + t.h && cy + d.h + kh / 2 > t.y0 && cx - kw / 2 < t.x0 + t.w &&
           cx + d.w + kw / 2 > t.x0;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(kThreads) void spectra_tiles_kernel(
    const smi_init_sources_spectra_blend *blends, const smi_init_sources_spectra_component *comps,
    const int32_t *work, const float *data, const float *weights, const double *stamps,
    const double *morphs, double *part) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int slot_of[kMaxComponents];  // component -> its column, -1: not present
    __shared__ int comp_of[kMaxComponents];  // column -> component
    __shared__ int n_present;
    const int tid = threadIdx.x, band = blockIdx.y;
    const int b = work[2 * blockIdx.x], tile = work[2 * blockIdx.x + 1];
    const smi_init_sources_spectra_blend bl = blends[b];
    if (band >= bl.bands) return;  // (the whole workgroup)
    const int kh = bl.kh, kw = bl.kw, K = bl.n_comp;
    const int wh = kTile + kh - 1, ww = kTile + kw - 1, wp = window_pitch(kw);
    double *win = reinterpret_cast<double *>(lds_raw);  // a morphology under the tile's taps
    double *col = win + wh * wp;
    const Tile t = tile_of(bl, tile);
    const double *kern = stamps + bl.stamp_off + (int64_t)band * kh * kw;

    if (tid < kWave) {  // the first wavefront: present components keep their order
        bool hit = false;
        if (tid < K) hit = present_on(bl, comps[bl.comp0 + tid], t);
        const unsigned long long mask = __ballot(hit);
        const int slot = __popcll(mask & ((1ull << tid) - 1ull));
        if (tid < K) slot_of[tid] = hit ? slot : -1;
        if (hit) comp_of[slot] = tid;
        if (tid == 0) n_present = __popcll(mask);
    }
    __syncthreads();
    const int P = uniform(n_present);  // <= kMaxPresent: the host walked the same tiles

    // ---- the columns: thread = pixel
    {
        const int i = tid / kTile, j = tid % kTile;
        const bool inside = i < t.h && j < t.w;
        const int at = tid + tid / kSegLen;
        for (int s = 0; s < P; ++s) {
            const smi_init_sources_spectra_component d = comps[bl.comp0 + uniform(comp_of[s])];
            // window (r, c) is region pixel (t.y0 - kh / 2 + r, t.x0 - kw / 2 + c), i.e. frame
            // pixel (fy0 + r, fx0 + c); 0 outside the morphology's box and outside the frame
            const int fy0 = bl.y0 + t.y0 - kh / 2, fx0 = bl.x0 + t.x0 - kw / 2;
            const int r0 = d.y0 - fy0, c0 = d.x0 - fx0;
            const double *m = morphs + d.morph_off;
            for (int e = tid; e < wh * ww; e += kThreads) {
                const int r = e / ww, c = e - r * ww;
                const int yy = r - r0, xx = c - c0, fy = fy0 + r, fx = fx0 + c;
                win[r * wp + c] = (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w && fy >= 0 &&
                                   fy < bl.h && fx >= 0 && fx < bl.w)
                                      ? m[(int64_t)yy * d.w + xx] : 0.0;
            }
            __syncthreads();
            // pixel (i, j) = sum over the taps, rows then columns ascending, of K[ky][kx] *
            // window[i + kh - 1 - ky][j + kw - 1 - kx]; taps under which no pixel of the tile
            // meets the morphology's rows and columns add exact zeros (finite stamps): skipped
            const int ky_lo = uniform(max(0, kh - (r0 + d.h)));
            const int ky_hi = uniform(min(kh - 1, kh - 1 - r0 + kTile - 1));
            const int kx_lo = uniform(max(0, kw - (c0 + d.w)));
            const int kx_hi = uniform(min(kw - 1, kw - 1 - c0 + kTile - 1));
            double acc = 0;
            for (int ky = ky_lo; ky <= ky_hi; ++ky) {
                const double *row = win + (i + kh - 1 - ky) * wp + j + kw - 1;
                const double *k = kern + ky * kw;
                for (int kx = kx_lo; kx <= kx_hi; ++kx) acc += k[kx] * row[-kx];
            }
            col[s * kPitch + at] = inside ? acc : 0.0;
            __syncthreads();  // (the window is staged again)
        }
        double dv = 0, wv = 0;
        if (inside) {  // (the region lies inside the frame)
            const int64_t q = bl.cube_off + ((int64_t)band * bl.h + bl.y0 + t.y0 + i) * bl.w +
                              bl.x0 + t.x0 + j;
            dv = (double)data[q], wv = (double)weights[q];
        }
        col[P * kPitch + at] = dv;
        col[(P + 1) * kPitch + at] = wv;
    }
    __syncthreads();

    const int E = entries_of(K);
    double *dst = part + bl.part_off + ((int64_t)tile * bl.bands + band) * E;
    // ---- exact zeros for what is not present on this tile
    for (int e = tid; e < E; e += kThreads) {
        const bool absent = e < K * K ? (slot_of[e / K] < 0 || slot_of[e % K] < 0)
                                      : slot_of[(e - K * K) % K] < 0;
        if (absent) dst[e] = 0.0;
    }
    // ---- the sums: item = (column sp; column sq >= sp, the data, ones or unweighted ones;
    // segment)
    const double *wcol = col + (P + 1) * kPitch;
    const int n_items = P * (P + 3) * kSegs;
    for (int base = 0; base < n_items; base += kThreads) {  // (uniform: every lane shuffles)
        const int item = base + tid;
        const int seg = item % kSegs, pair = item / kSegs;
        const int sp = pair / (P + 3), sq = pair % (P + 3);
        const bool active = item < n_items && sq >= sp;
        double acc = 0;
        if (active) {
            const double *u = col + sp * kPitch + seg * (kSegLen + 1);
            const double *wt = wcol + seg * (kSegLen + 1);
            if (sq <= P) {
                const double *v = col + sq * kPitch + seg * (kSegLen + 1);
                for (int i = 0; i < kSegLen; ++i) acc += (u[i] * wt[i]) * v[i];
            } else if (sq == P + 1) {
                for (int i = 0; i < kSegLen; ++i) acc += u[i] * wt[i];
            } else {
                for (int i = 0; i < kSegLen; ++i) acc += u[i];
            }
        }
        acc += __shfl_xor(acc, 1, kWave);
        acc += __shfl_xor(acc, 2, kWave);
        acc += __shfl_xor(acc, 4, kWave);
        if (active && seg == 0) {
            const int gp = comp_of[sp];
            if (sq >= P) {
                dst[K * K + (sq - P) * K + gp] = acc;
            } else {
                const int gq = comp_of[sq];
                dst[gp * K + gq] = acc;
                dst[gq * K + gp] = acc;
            }
        }
    }
}

// one thread per entry adds the tiles of its blend and band in tile order
__global__ __launch_bounds__(kThreads) void spectra_reduce_kernel(
    const smi_init_sources_spectra_blend *blends, const double *part, double *out) {
    const smi_init_sources_spectra_blend bl = blends[blockIdx.x];
    const int band = blockIdx.y;
    if (band >= bl.bands) return;
    const int E = entries_of(bl.n_comp), n_tiles = tiles_of(bl);
    const double *src = part + bl.part_off + (int64_t)band * E;
    for (int e = threadIdx.x; e < E; e += kThreads) {
        double s = 0;
        for (int t = 0; t < n_tiles; ++t) s += src[(int64_t)t * bl.bands * E + e];
        out[bl.out_off + (int64_t)band * E + e] = s;
    }
}

// ---------------------------------------------------------------------------- host checks
#define SMI_TABLES(n, host, dev)                                                  \
    SMI_REQUIRE((n) >= 0, "negative count");                                       \
    SMI_REQUIRE(((host) && (dev)) || (n) == 0, "null descriptor table")

int psf_snr(int32_t n, const smi_init_sources_psf_snr *tasks, const void *d_tasks,
            const float *d_data, const float *d_var, int64_t n_cube, const double *d_psfs,
            int64_t n_psf, double *d_out, int64_t n_out, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_cube >= 0 && n_psf >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE(((d_data && d_var) || !n_cube) && (d_psfs || !n_psf) && (d_out || !n_out),
                "null buffer");
    int32_t most = 0;
    int64_t out_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_init_sources_psf_snr &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "frame extent");
        SMI_REQUIRE(t.bands > 0 && t.bands <= kMaxBands, "bands");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w, "centre outside its frame");
        SMI_REQUIRE(t.ph > 0 && t.pw > 0 && t.ph <= kMaxStamp && t.pw <= kMaxStamp, "stamp extent");
        SMI_REQUIRE(in_buffer(t.cube_off, (int64_t)t.bands * t.h * t.w, n_cube),
                    "cube outside the data buffers");
        SMI_REQUIRE(in_buffer(t.psf_off, (int64_t)t.bands * t.ph * t.pw, n_psf),
                    "stamps outside their buffer");
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, 3 * (int64_t)t.bands, n_out),
                    "sums outside the output buffer or shared with another source");
        out_end = t.out_off + 3 * (int64_t)t.bands;
        most = std::max(most, t.bands);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL(psf_snr_kernel, dim3(n, most), dim3(kWave), 0, (hipStream_t)stream,
                       (const smi_init_sources_psf_snr *)d_tasks, d_data, d_var, d_psfs, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

int sweep(int32_t n, const smi_init_sources_sweep *tasks, const void *d_tasks, const float *d_data,
          const float *d_var, int64_t n_cube, const double *d_spectra, int64_t n_spectra,
          double *d_out, int64_t n_out, int32_t *d_bounds, double *d_peaks, int64_t n_results,
          void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_cube >= 0 && n_spectra >= 0 && n_out >= 0 && n_results >= 0,
                "negative buffer size");
    SMI_REQUIRE(((d_data && d_var) || !n_cube) && (d_spectra || !n_spectra) && (d_out || !n_out) &&
                    ((d_bounds && d_peaks) || !n_results), "null buffer");
    SMI_REQUIRE(n <= n_results, "results outside the output buffers");
    int64_t out_end = 0, largest = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_init_sources_sweep &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "plane extent");
        const int64_t N = (int64_t)t.h * t.w;
        SMI_REQUIRE(N <= kMaxSweepPixels, "frame beyond the LDS image of the sweep");
        SMI_REQUIRE(t.bands > 0 && t.bands <= kMaxBands, "bands");
        SMI_REQUIRE(t.cy >= 0 && t.cy < t.h && t.cx >= 0 && t.cx < t.w, "centre outside its frame");
        SMI_REQUIRE(in_buffer(t.cube_off, t.bands * N, n_cube), "cube outside the data buffers");
        SMI_REQUIRE(in_buffer(t.spec_off, t.bands, n_spectra), "spectrum outside its buffer");
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, N, n_out),
                    "swept plane outside the output buffer or shared with another");
        out_end = t.out_off + N;
        largest = std::max(largest, N);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    const size_t lds = (size_t)largest * sizeof(double);
    static size_t cfg[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(sweep_kernel), lds, cfg))) return rc;
    hipLaunchKernelGGL(sweep_kernel, dim3(n), dim3(kThreads), lds, (hipStream_t)stream,
                       (const smi_init_sources_sweep *)d_tasks, d_data, d_var, d_spectra, d_out,
                       d_bounds, d_peaks);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

int crop(int32_t n, const smi_init_sources_crop *tasks, const void *d_tasks, const double *d_planes,
         int64_t n_plane, const double *d_floors, int64_t n_floor, double *d_out, int64_t n_out,
         int32_t *d_flags, int64_t n_flags, void *stream) {
    SMI_TABLES(n, tasks, d_tasks);
    SMI_REQUIRE(n_plane >= 0 && n_floor >= 0 && n_out >= 0 && n_flags >= 0, "negative buffer size");
    SMI_REQUIRE((d_planes || !n_plane) && (d_floors || !n_floor) && (d_out || !n_out) &&
                    (d_flags || !n_flags), "null buffer");
    SMI_REQUIRE(n <= n_flags, "flags outside their buffer");
    int64_t out_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_init_sources_crop &t = tasks[i];
        SMI_REQUIRE(t.h > 0 && t.w > 0 && t.h <= kMaxExtent && t.w <= kMaxExtent, "plane extent");
        SMI_REQUIRE(t.side > 0 && t.side <= kMaxSide && t.side % 2 == 1, "box side");
        SMI_REQUIRE(t.y0 > -kMaxSide - kMaxExtent && t.y0 < kMaxExtent + kMaxSide &&
                        t.x0 > -kMaxSide - kMaxExtent && t.x0 < kMaxExtent + kMaxSide, "box origin");
        SMI_REQUIRE(t.layers == 1 || t.layers == 2, "one or two layers");
        SMI_REQUIRE(t.percentile > 0 && t.percentile < 100, "percentile outside (0, 100)");
        const int64_t N = (int64_t)t.side * t.side;
        SMI_REQUIRE(in_buffer(t.plane_off, (int64_t)t.h * t.w, n_plane), "plane outside its buffer");
        SMI_REQUIRE(in_buffer(t.floor_off, N, n_floor), "floor outside its buffer");
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, t.layers * N, n_out),
                    "cut-out outside the output buffer or shared with another");
        out_end = t.out_off + t.layers * N;
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL(crop_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_init_sources_crop *)d_tasks, d_planes, d_floors, d_out, d_flags);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

// the fields of a blend both spectra launches walk: counts, region and where its sums go
int check_spectra_blend(const smi_init_sources_spectra_blend &bl, int64_t n_part, int64_t n_out,
                        int64_t *part_end, int64_t *out_end) {
    SMI_REQUIRE(bl.h > 0 && bl.w > 0 && bl.h <= kMaxExtent && bl.w <= kMaxExtent, "frame extent");
    SMI_REQUIRE(bl.bands > 0 && bl.bands <= kMaxBands, "bands");
    SMI_REQUIRE(bl.n_comp >= 1 && bl.n_comp <= kMaxComponents, "components of a blend");
    SMI_REQUIRE(bl.y0 >= 0 && bl.x0 >= 0 && bl.fh > 0 && bl.fw > 0 && bl.fh <= bl.h - bl.y0 &&
                    bl.fw <= bl.w - bl.x0, "region outside its frame");
    const int64_t E = entries_of(bl.n_comp);
    const int64_t need = (int64_t)tiles_of(bl) * bl.bands * E;
    SMI_REQUIRE(bl.part_off >= *part_end && in_buffer(bl.part_off, need, n_part),
                "tile sums outside their buffer or shared with another blend");
    SMI_REQUIRE(bl.out_off >= *out_end && in_buffer(bl.out_off, bl.bands * E, n_out),
                "a blend's sums outside the output buffer or shared with another");
    *part_end = bl.part_off + need, *out_end = bl.out_off + bl.bands * E;
    return SMI_OK;
}

int spectra_tiles(int32_t n, const smi_init_sources_spectra_blend *blends, const void *d_blends,
                  int32_t n_comps, const smi_init_sources_spectra_component *comps,
                  const void *d_comps, int32_t n_work, const int32_t *work, const void *d_work,
                  const float *d_data, const float *d_weights, int64_t n_cube,
                  const double *d_stamps, int64_t n_stamp, const double *d_morphs, int64_t n_morph,
                  double *d_part, int64_t n_part, int64_t n_out, void *stream) {
    SMI_TABLES(n, blends, d_blends);
    SMI_TABLES(n_comps, comps, d_comps);
    SMI_TABLES(n_work, work, d_work);
    SMI_REQUIRE(n_cube >= 0 && n_stamp >= 0 && n_morph >= 0 && n_part >= 0 && n_out >= 0,
                "negative buffer size");
    SMI_REQUIRE(((d_data && d_weights) || !n_cube) && (d_stamps || !n_stamp) &&
                    (d_morphs || !n_morph) && (d_part || !n_part), "null buffer");
    int64_t part_end = 0, out_end = 0, at = 0;
    int32_t most = 0;
    size_t lds = 0;
    for (int32_t b = 0; b < n; ++b) {
        const smi_init_sources_spectra_blend &bl = blends[b];
        int rc = check_spectra_blend(bl, n_part, n_out, &part_end, &out_end);
        if (rc) return rc;
        SMI_REQUIRE(bl.kh > 0 && bl.kw > 0 && bl.kh % 2 == 1 && bl.kw % 2 == 1,
                    "the stamp must have odd height and width");
        SMI_REQUIRE(bl.kh <= kMaxStamp && bl.kw <= kMaxStamp, "stamp beyond the kernel's limit");
        SMI_REQUIRE(in_buffer(bl.cube_off, (int64_t)bl.bands * bl.h * bl.w, n_cube),
                    "cube outside the data buffers");
        SMI_REQUIRE(in_buffer(bl.stamp_off, (int64_t)bl.bands * bl.kh * bl.kw, n_stamp),
                    "stamps outside their buffer");
        SMI_REQUIRE(bl.comp0 >= 0 && bl.n_comp <= n_comps - bl.comp0, "component range");
        for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c) {
            const smi_init_sources_spectra_component &d = comps[c];
            SMI_REQUIRE(d.h > 0 && d.w > 0 && d.h <= kMaxSide && d.w <= kMaxSide,
                        "component extent");
            SMI_REQUIRE(d.y0 >= -kMaxCoord && d.y0 <= kMaxCoord && d.x0 >= -kMaxCoord &&
                            d.x0 <= kMaxCoord, "component origin");
            SMI_REQUIRE(in_buffer(d.morph_off, (int64_t)d.h * d.w, n_morph),
                        "morphology outside its buffer");
        }
        const int32_t tiles = tiles_of(bl);
        int max_present = 0;
        for (int32_t t = 0; t < tiles; ++t, ++at) {
            SMI_REQUIRE(at < n_work && work[2 * at] == b && work[2 * at + 1] == t,
                        "the work list is not every tile of every blend in order");
            const Tile tl = tile_of(bl, t);
            int present = 0;
            for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c)
                present += present_on(bl, comps[c], tl);
            SMI_REQUIRE(present <= kMaxPresent, "components present on one tile");
            max_present = std::max(max_present, present);
        }
        lds = std::max(lds, ((size_t)(max_present + 2) * kPitch +
                             (size_t)(kTile + bl.kh - 1) * window_pitch(bl.kw)) * sizeof(double));
        most = std::max(most, bl.bands);
    }
    SMI_REQUIRE(at == n_work, "the work list is not every tile of every blend in order");
    SMI_REQUIRE(lds <= kLdsBytes - kLdsReserve, "columns and window beyond the LDS of a CU");
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    static size_t cfg[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(spectra_tiles_kernel), lds, cfg)))
        return rc;
    hipLaunchKernelGGL(spectra_tiles_kernel, dim3(n_work, most), dim3(kThreads), lds,
                       (hipStream_t)stream, (const smi_init_sources_spectra_blend *)d_blends,
                       (const smi_init_sources_spectra_component *)d_comps,
                       (const int32_t *)d_work, d_data, d_weights, d_stamps, d_morphs, d_part);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

int spectra_reduce(int32_t n, const smi_init_sources_spectra_blend *blends, const void *d_blends,
                   const double *d_part, int64_t n_part, double *d_out, int64_t n_out,
                   void *stream) {
    SMI_TABLES(n, blends, d_blends);
    SMI_REQUIRE(n_part >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE((d_part || !n_part) && (d_out || !n_out), "null buffer");
    int64_t part_end = 0, out_end = 0;
    int32_t most = 0;
    for (int32_t b = 0; b < n; ++b) {
        int rc = check_spectra_blend(blends[b], n_part, n_out, &part_end, &out_end);
        if (rc) return rc;
        most = std::max(most, blends[b].bands);
    }
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipLaunchKernelGGL(spectra_reduce_kernel, dim3(n, most), dim3(kThreads), 0, (hipStream_t)stream,
                       (const smi_init_sources_spectra_blend *)d_blends, d_part, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_init_sources_spectra_tiles_f32(
    int32_t n, const smi_init_sources_spectra_blend *blends, const void *d_blends, int32_t n_comps,
    const smi_init_sources_spectra_component *comps, const void *d_comps, int32_t n_work,
    const int32_t *work, const void *d_work, const float *d_data, const float *d_weights,
    int64_t n_cube, const double *d_stamps, int64_t n_stamp, const double *d_morphs,
    int64_t n_morph, double *d_part, int64_t n_part, int64_t n_out, void *stream) {
    return smi::spectra_tiles(n, blends, d_blends, n_comps, comps, d_comps, n_work, work, d_work,
                              d_data, d_weights, n_cube, d_stamps, n_stamp, d_morphs, n_morph,
                              d_part, n_part, n_out, stream);
}

int smi_init_sources_spectra_reduce_f32(int32_t n, const smi_init_sources_spectra_blend *blends,
                                        const void *d_blends, const double *d_part, int64_t n_part,
                                        double *d_out, int64_t n_out, void *stream) {
    return smi::spectra_reduce(n, blends, d_blends, d_part, n_part, d_out, n_out, stream);
}

int smi_init_sources_psf_snr_f32(int32_t n, const smi_init_sources_psf_snr *tasks, const void *d_tasks,
                             const float *d_data, const float *d_var, int64_t n_cube,
                             const double *d_psfs, int64_t n_psf, double *d_out, int64_t n_out,
                             void *stream) {
    return smi::psf_snr(n, tasks, d_tasks, d_data, d_var, n_cube, d_psfs, n_psf, d_out, n_out,
                        stream);
}

int smi_init_sources_sweep_f32(int32_t n, const smi_init_sources_sweep *tasks, const void *d_tasks,
                           const float *d_data, const float *d_var, int64_t n_cube,
                           const double *d_spectra, int64_t n_spectra, double *d_out,
                           int64_t n_out, int32_t *d_bounds, double *d_peaks, int64_t n_results,
                           void *stream) {
    return smi::sweep(n, tasks, d_tasks, d_data, d_var, n_cube, d_spectra, n_spectra, d_out, n_out,
                      d_bounds, d_peaks, n_results, stream);
}

int smi_init_sources_crop_f32(int32_t n, const smi_init_sources_crop *tasks, const void *d_tasks,
                          const double *d_planes, int64_t n_plane, const double *d_floors,
                          int64_t n_floor, double *d_out, int64_t n_out, int32_t *d_flags,
                          int64_t n_flags, void *stream) {
    return smi::crop(n, tasks, d_tasks, d_planes, n_plane, d_floors, n_floor, d_out, n_out,
                     d_flags, n_flags, stream);
}

}  // extern "C"
