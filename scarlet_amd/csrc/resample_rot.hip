// Multi-resolution rendering between ROTATED pixel grids (reference scarlet/renderer.py:319-363,
// 498-524, ResolutionRenderer with isrot): path 2 of a Resampler (resample.hip).
//
// The reference Fourier-shifts the padded difference kernel D in 2-D to shifts[:, a] for every
// low-resolution row a (the operator, op[a] = h^2 shift(D, s_a)), per call the padded model m by
// -other_shifts[:, b] for every column b, and contracts out[a, b] = sum_yx op[a] shifted[b] per
// band.  A 2-D shift is rfftn, times exp(-2 pi i (f_y s_y + f_x s_x)) with f_y = fftfreq(Fy),
// f_x = rfftfreq(Fx), irfftn (the ifftshift / fftshift around it are common to both images and
// drop out of the inner product).  With Parseval's identity for real images the map reads
//
//   out[c, a, b] = sum_{ky, kx} Re( E[c, a, ky, kx] conj( Mh[c, ky, kx] beta[b, ky, kx] ) )
//
//   E[c, a]  = h^2 rfftn(D[c]) alpha'[a]        made once, float64 -> float32 complex
//   beta[b]  = w_kx / (Fy Fx) beta'[b]          w = 1 for kx = 0 and the x-Nyquist term, else 2
//   Mh[c]    = rfftn(m[c])                      per rendering
//
// alpha'[a], beta'[b]: the phase tables of s_a and of -o_b.  The edge-column rule: irfftn returns
// a real image, so on the two self-conjugate columns (kx = 0; kx = Fx / 2 for even Fx) it keeps
// the Hermitian part along y of a shifted spectrum only.  The transforms of D and m are
// Hermitian there themselves, so the projection falls on the tables: t'[ky] = (t[ky] +
// conj(t[-ky mod Fy])) / 2 on those columns, t' = t elsewhere.  Pure phases everywhere are a
// different map (6e-6 .. 4.9e-5 of the peak on the white-noise models of the tests).
//
// Per rendering: the transform of the model rows along x, then along y (float64 sums, Mh
// stored as float32 complex), and the contraction -- per band a complex product with M = n_a,
// N = n_b, K = Fy Kx: block tiles of up to 64 x 64 outputs, K cut into slices (rot_slice_terms)
// that are one workgroup each; conj(Mh beta) is formed while a tile is staged into LDS, never in
// memory.  E is read once per 64 columns b, i.e. once for observations of up to 64 x 64
// pixels.  The sum order: inside a slice k ascending in one float64 fma chain per output (terms
// e.x s.x, -e.y s.y, with s = conj(Mh beta) formed in float64 from the float32 operands and
// kept in LDS as float32 complex), across slices z ascending.  It depends on the shapes alone.
//
// The transpose runs the transposed chain: Mbar[c, k] = sum_a E[c, a, k] (sum_b r[c, a, b]
// conj(beta[b, k])) (b ascending; a = w (mod 4) per wavefront, combined (0 + 1) + (2 + 3)), the
// inverse transform along y, then along x taking the real part.  No n_b shifted models and no
// n_a x n_b x K array ever exist.
//
// LDS: up to 33 KB for the contraction's two tiles, 36 KB for the transpose (32 KB beta tile +
// 4 KB for the four partial sums), whatever the sizes; the row transforms keep a row and its
// twiddles in dynamic LDS -- 24 bytes per pixel forward (48 KB at Fx = 2048), 16 (Kx + Fx) bytes
// back (49 168 bytes at Fx = 2048) -- which is what limits Fx to 2048, under the 64 KB a kernel
// gets without asking for more.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

namespace smi {
namespace {

constexpr size_t kRotGuard = 256;  // guard elements behind every work array
constexpr int kTile = 64;          // columns b per LDS chunk of the transpose
constexpr int kStage = 32;         // k per LDS stage

// fftfreq(Fy)[ky] s_y + rfftfreq(Fx)[kx] s_x -> exp(-2 pi i .)
__device__ inline double2 rot_phase(int ky, int kx, int Fy, int Fx, double sy, double sx) {
    const int qy = 2 * ky < Fy ? ky : ky - Fy;
    const double t = (double)qy / (double)Fy * sy + (double)kx / (double)Fx * sx;
    double s, c;
    sincospi(-2.0 * t, &s, &c);
    return make_double2(c, s);
}

// the phase table with the edge-column rule
__device__ inline double2 rot_table(int ky, int kx, int Fy, int Fx, double sy, double sx) {
    double2 p = rot_phase(ky, kx, Fy, Fx, sy, sx);
    if (kx == 0 || 2 * kx == Fx) {
        const double2 q = rot_phase((Fy - ky) % Fy, kx, Fy, Fx, sy, sx);
        p.x = 0.5 * (p.x + q.x);
        p.y = 0.5 * (p.y - q.y);
    }
    return p;
}

// T[row][kx] = sum_x in[row][x] tw[(kx x) mod Fx], kx < Kx; tw[j] = exp(-2 pi i j / Fx).  One
// workgroup per row.
__global__ __launch_bounds__(256) void rot_rows_forward_kernel(const float *in, const double2 *tw,
                                                               double2 *T, int Fx, int Kx) {
    extern __shared__ double rot_sm[];
    double *row = rot_sm;
    double2 *t = reinterpret_cast<double2 *>(rot_sm + ((Fx + 1) & ~1));
    const int64_t r = blockIdx.x;
    for (int x = threadIdx.x; x < Fx; x += 256) {
        row[x] = (double)in[r * Fx + x];
        t[x] = tw[x];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < Kx; k += 256) {
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int x = 0; x < Fx; ++x) {
            const double a = row[x];
            const double2 w = t[j];
            re = fma(a, w.x, re);
            im = fma(a, w.y, im);
            j += k;
            if (j >= Fx) j -= Fx;
        }
        T[r * Kx + k] = make_double2(re, im);
    }
}

// g[row][x] = sum_kx Re(T[row][kx] conj(tw[(kx x) mod Fx])), x < Fx.  One workgroup per row.
__global__ __launch_bounds__(256) void rot_rows_inverse_kernel(const double2 *T, const double2 *tw,
                                                               float *g, int Fx, int Kx) {
    extern __shared__ double rot_sm[];
    double2 *row = reinterpret_cast<double2 *>(rot_sm);
    double2 *t = row + Kx;
    const int64_t r = blockIdx.x;
    for (int k = threadIdx.x; k < Kx; k += 256) row[k] = T[r * Kx + k];
    for (int x = threadIdx.x; x < Fx; x += 256) t[x] = tw[x];
    __syncthreads();
    for (int x = threadIdx.x; x < Fx; x += 256) {
        double v = 0.0;
        int j = 0;
        for (int k = 0; k < Kx; ++k) {
            const double2 a = row[k], w = t[j];
            v = fma(a.x, w.x, v);
            v = fma(a.y, w.y, v);
            j += x;
            if (j >= Fx) j -= Fx;
        }
        g[r * Fx + x] = (float)v;
    }
}

__device__ inline void rot_store(double2 *p, double re, double im) { *p = make_double2(re, im); }
__device__ inline void rot_store(float2 *p, double re, double im) {
    *p = make_float2((float)re, (float)im);
}

// out[c][q][kx] = sum_y T[c][y][kx] tw[(q y) mod Fy] (inverse: conj(tw)), q < Fy; tw[j] =
// exp(-2 pi i j / Fy).  Grid (ceil(Kx / 64), Fy, C); wavefront w takes y = w (mod 4) in
// ascending order, the four sums are combined (0 + 1) + (2 + 3).
template <typename Out>
__global__ __launch_bounds__(256) void rot_cols_kernel(const double2 *T, const double2 *tw,
                                                       Out *out, int Fy, int Kx, int inverse) {
    __shared__ double2 red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane, q = blockIdx.y;
    const int64_t plane = (int64_t)blockIdx.z * Fy * Kx;
    double re = 0.0, im = 0.0;
    if (k < Kx) {
        const int step = (int)(((int64_t)4 * q) % Fy);
        int j = (int)(((int64_t)w * q) % Fy);
        for (int y = w; y < Fy; y += 4) {
            const double2 a = T[plane + (int64_t)y * Kx + k];
            double2 t = tw[j];
            if (inverse) t.y = -t.y;
            re = fma(a.x, t.x, re);
            re = fma(-a.y, t.y, re);
            im = fma(a.x, t.y, im);
            im = fma(a.y, t.x, im);
            j += step;
            if (j >= Fy) j -= Fy;
        }
    }
    red[w][lane] = make_double2(re, im);
    __syncthreads();
    if (w == 0 && k < Kx) {
        const double sr = (red[0][lane].x + red[1][lane].x) + (red[2][lane].x + red[3][lane].x);
        const double si = (red[0][lane].y + red[1][lane].y) + (red[2][lane].y + red[3][lane].y);
        rot_store(out + plane + (int64_t)q * Kx + k, sr, si);
    }
}

// E[c][a][k] = scale Dhat[c][k] alpha'[a][k]; grid (ceil(Fy Kx / 256), n_a, C)
__global__ __launch_bounds__(256) void rot_build_E_kernel(const double2 *Dhat, const double *shifts,
                                                          double scale, float2 *E, int n_a, int Fy,
                                                          int Fx, int Kx) {
    const int64_t K = (int64_t)Fy * Kx;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int a = blockIdx.y, c = blockIdx.z;
    const int ky = (int)(k / Kx), kx = (int)(k - (int64_t)ky * Kx);
    const double2 p = rot_table(ky, kx, Fy, Fx, shifts[a], shifts[n_a + a]);
    const double2 d = Dhat[(int64_t)c * K + k];
    E[((int64_t)c * n_a + a) * K + k] = make_float2((float)(scale * (d.x * p.x - d.y * p.y)),
                                                    (float)(scale * (d.x * p.y + d.y * p.x)));
}

// beta[b][k] = w_kx / (Fy Fx) beta'[b][k], the table of -other_shifts[:, b]; grid
// (ceil(Fy Kx / 256), n_b)
__global__ __launch_bounds__(256) void rot_build_beta_kernel(const double *other, float2 *beta,
                                                             int n_b, int Fy, int Fx, int Kx) {
    const int64_t K = (int64_t)Fy * Kx;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int b = blockIdx.y;
    const int ky = (int)(k / Kx), kx = (int)(k - (int64_t)ky * Kx);
    const double2 p = rot_table(ky, kx, Fy, Fx, -other[b], -other[n_b + b]);
    const double sc = ((kx == 0 || 2 * kx == Fx) ? 1.0 : 2.0) / ((double)Fy * (double)Fx);
    beta[(int64_t)b * K + k] = make_float2((float)(sc * p.x), (float)(sc * p.y));
}

// The contraction.  Block tile of 16 TI x 16 TJ outputs, grid (ceil(n_b / (16 TJ)), ceil(n_a /
// (16 TI)), C n_slices), 256 threads as 16 x 16: thread (ta, tb) owns the outputs a = a0 + ta +
// 16 i, b = b0 + tb + 16 j, i < TI, j < TJ (TI, TJ <= 4 follow n_a, n_b: a 36 x 36 observation
// takes 48 x 48 tiles, nine sums per thread instead of sixteen).  Slice z covers k in
// [z kslice, ...); a stage of 32 k is brought into LDS as Es[k][a] = E[c][a][k] and Ss[k][b] =
// conj(Mh[c][k] beta[b][k]) (zeros outside the matrix), and every output adds Re(e s) =
// e.x s.x - e.y s.y for k ascending in float64: the tile shape does not change the order of
// an output's terms.  n_slices == 1: the tile goes to out (float), else to part[c][z][a][b]
// (double) for rot_reduce_kernel.
template <int TI, int TJ>
__global__ __launch_bounds__(256) void rot_contract_kernel(const float2 *E, const float2 *Mh,
                                                           const float2 *beta, float *out,
                                                           double *part, int n_a, int n_b,
                                                           int64_t K, int kslice, int n_slices) {
    __shared__ float2 Es[kStage][16 * TI + 1], Ss[kStage][16 * TJ + 1];
    const int c = blockIdx.z / n_slices, z = blockIdx.z - c * n_slices;
    const int a0 = blockIdx.y * 16 * TI, b0 = blockIdx.x * 16 * TJ;
    const int tid = threadIdx.x, ta = tid >> 4, tb = tid & 15;
    const int64_t k_lo = (int64_t)z * kslice, k_hi = k_lo + kslice < K ? k_lo + kslice : K;
    const float2 *Ec = E + (int64_t)c * n_a * K;
    const float2 *Mc = Mh + (int64_t)c * K;
    double acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = 0.0;
    // staging: thread t takes k = t % 32 of the rows t / 32 + 8 q (32 consecutive k: 256 bytes)
    const int sk = tid & (kStage - 1), sr = tid / kStage;
    for (int64_t k0 = k_lo; k0 < k_hi; k0 += kStage) {
        const int64_t k = k0 + sk;
        const bool k_in = k < k_hi;
        const float2 m = k_in ? Mc[k] : make_float2(0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 2 * TI; ++q) {
            const int row = sr + 8 * q, a = a0 + row;
            Es[sk][row] = (k_in && a < n_a) ? Ec[(int64_t)a * K + k] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < 2 * TJ; ++q) {
            const int row = sr + 8 * q, b = b0 + row;
            float2 s = make_float2(0.f, 0.f);
            if (k_in && b < n_b) {
                const float2 bt = beta[(int64_t)b * K + k];
                // (the product in float64 from the float32 operands, rounded to float32 once)
                s.x = (float)((double)m.x * bt.x - (double)m.y * bt.y);
                s.y = (float)-((double)m.x * bt.y + (double)m.y * bt.x);
            }
            Ss[sk][row] = s;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kStage; ++kk) {
            double ex[TI], ey[TI], sx[TJ], sy[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const float2 e = Es[kk][ta + 16 * i];
                ex[i] = (double)e.x;
                ey[i] = -(double)e.y;
            }
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const float2 s = Ss[kk][tb + 16 * j];
                sx[j] = (double)s.x;
                sy[j] = (double)s.y;
            }
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) {
                    acc[i][j] = fma(ex[i], sx[j], acc[i][j]);
                    acc[i][j] = fma(ey[i], sy[j], acc[i][j]);
                }
        }
        __syncthreads();
    }
    const int64_t MN = (int64_t)n_a * n_b;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int a = a0 + ta + 16 * i, b = b0 + tb + 16 * j;
            if (a < n_a && b < n_b) {
                if (n_slices == 1)
                    out[(int64_t)c * MN + (int64_t)a * n_b + b] = (float)acc[i][j];
                else
                    part[((int64_t)c * n_slices + z) * MN + (int64_t)a * n_b + b] = acc[i][j];
            }
        }
}

// out[c][i] = sum_z part[c][z][i], z ascending; grid (ceil(MN / 256), C)
__global__ __launch_bounds__(256) void rot_reduce_kernel(const double *part, float *out, int64_t MN,
                                                         int n_slices) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    const double *p = part + (int64_t)blockIdx.y * n_slices * MN + i;
    double t = 0.0;
    for (int z = 0; z < n_slices; ++z) t += p[(int64_t)z * MN];
    out[(int64_t)blockIdx.y * MN + i] = (float)t;
}

// Mbar[c][k] = sum_a E[c][a][k] G[a], G[a] = sum_b resid[c][a][b] conj(beta[b][k]).  Grid
// (ceil(K / 64), C), four wavefronts with the lanes along k.  The columns b come in chunks of 64
// whose beta tile lies in LDS; wavefront w takes the rows a = w (mod 4), b ascending inside a
// chunk, and adds E G of every (a, chunk) to its sum as it goes (chunks ascending, then a
// ascending inside); the four sums are combined (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void rot_mbar_kernel(const float2 *E, const float2 *beta,
                                                       const float *resid, double2 *Mbar, int n_a,
                                                       int n_b, int64_t K) {
    __shared__ float2 Bs[kTile][64];
    __shared__ double2 red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    const bool k_in = k < K;
    const float2 *Ec = E + (int64_t)c * n_a * K;
    const float *rc = resid + (int64_t)c * n_a * n_b;
    double re = 0.0, im = 0.0;
    for (int b0 = 0; b0 < n_b; b0 += kTile) {
        const int nb = min(kTile, n_b - b0);
        for (int bb = w; bb < nb; bb += 4)
            Bs[bb][lane] = k_in ? beta[(int64_t)(b0 + bb) * K + k] : make_float2(0.f, 0.f);
        __syncthreads();
        if (k_in)
            for (int a = w; a < n_a; a += 4) {
                const float *ra = rc + (int64_t)a * n_b + b0;
                double gx = 0.0, gy = 0.0;
                for (int bb = 0; bb < nb; ++bb) {
                    const double r = (double)ra[bb];
                    const float2 bt = Bs[bb][lane];
                    gx = fma(r, (double)bt.x, gx);
                    gy = fma(-r, (double)bt.y, gy);
                }
                const float2 e = Ec[(int64_t)a * K + k];
                re = fma((double)e.x, gx, re);
                re = fma(-(double)e.y, gy, re);
                im = fma((double)e.x, gy, im);
                im = fma((double)e.y, gx, im);
            }
        __syncthreads();
    }
    red[w][lane] = make_double2(re, im);
    __syncthreads();
    if (w == 0 && k_in) {
        const double sr = (red[0][lane].x + red[1][lane].x) + (red[2][lane].x + red[3][lane].x);
        const double si = (red[0][lane].y + red[1][lane].y) + (red[2][lane].y + red[3][lane].y);
        Mbar[(int64_t)c * K + k] = make_double2(sr, si);
    }
}

}  // namespace

struct RotResampler {
    int C = 0, n_a = 0, n_b = 0, Fy = 0, Fx = 0, Kx = 0;
    int kslice = 0, n_slices = 0;
    float2 *E = nullptr;     // [C][n_a][Fy][Kx]
    float2 *beta = nullptr;  // [n_b][Fy][Kx]
    double2 *twx = nullptr, *twy = nullptr;  // exp(-2 pi i j / F)
    // work arrays, each followed by kRotGuard guard elements
    double2 *T = nullptr;    // [C][Fy][Kx]: rows transformed along x / columns transformed back
    float2 *Mh = nullptr;    // [C][Fy][Kx]
    double2 *Mbar = nullptr; // [C][Fy][Kx]
    double *part = nullptr;  // [C][n_slices][n_a][n_b] (n_slices > 1)
};

// terms per slice of the contraction and their number: 64 terms, longer where that would
// give more than 256 slices; a multiple of the stage.  (A slice is a workgroup: the 7 320 terms
// of the tutorial's size are 115 slices per band, two workgroups per compute unit for five
// bands; with slices of 256 terms the 145 workgroups left 111 units idle.)
static void rot_slice_terms(int64_t K, int *kslice, int *n_slices) {
    int64_t ks = (K + 255) / 256;
    ks = (ks + kStage - 1) / kStage * kStage;
    if (ks < 64) ks = 64;
    *kslice = (int)ks;
    *n_slices = (int)((K + ks - 1) / ks);
}

// What a rotated resampler launches, from the shapes alone (host only; rot_forward and
// rot_create follow it to the letter): 16 x 16 threads with TI x TJ outputs each -- the smallest
// tile that holds the observation, 64 x 64 beyond that --, the tiles along a and b, the terms
// per slice and the slices of K = Fy Kx, and the chunks of 64 columns b of the transpose.
RotPlan rot_plan(int n_a, int n_b, int Fy, int Fx) {
    RotPlan p;
    p.ti = std::min(4, (n_a + 15) / 16);
    p.tj = std::min(4, (n_b + 15) / 16);
    p.tiles_a = (n_a + 16 * p.ti - 1) / (16 * p.ti);
    p.tiles_b = (n_b + 16 * p.tj - 1) / (16 * p.tj);
    rot_slice_terms((int64_t)Fy * (Fx / 2 + 1), &p.kslice, &p.n_slices);
    p.b_chunks = (n_b + kTile - 1) / kTile;
    return p;
}

static size_t rot_plane(const RotResampler *r) { return (size_t)r->C * r->Fy * r->Kx; }

// NaN bytes in the work arrays, the guard pattern behind them
int rot_fill_work(RotResampler *r) {
    const size_t n = rot_plane(r);
    SMI_HIP(hipMemset(r->T, 0xff, n * sizeof(double2)));
    SMI_HIP(hipMemset(r->T + n, 0xa5, kRotGuard * sizeof(double2)));
    SMI_HIP(hipMemset(r->Mh, 0xff, n * sizeof(float2)));
    SMI_HIP(hipMemset(r->Mh + n, 0xa5, kRotGuard * sizeof(float2)));
    SMI_HIP(hipMemset(r->Mbar, 0xff, n * sizeof(double2)));
    SMI_HIP(hipMemset(r->Mbar + n, 0xa5, kRotGuard * sizeof(double2)));
    if (r->part) {
        const size_t np = (size_t)r->C * r->n_slices * r->n_a * r->n_b;
        SMI_HIP(hipMemset(r->part, 0xff, np * sizeof(double)));
        SMI_HIP(hipMemset(r->part + np, 0xa5, kRotGuard * sizeof(double)));
    }
    return SMI_OK;
}

namespace {

size_t rot_row_lds(int Fx) {
    return (size_t)((Fx + 1) & ~1) * sizeof(double) + (size_t)Fx * sizeof(double2);
}

void rot_twiddles(int F, std::vector<double2> *tw) {
    const double step = 2.0 * 3.14159265358979323846 / (double)F;
    tw->resize(F);
    for (int j = 0; j < F; ++j) (*tw)[j] = make_double2(std::cos(step * j), -std::sin(step * j));
}

}  // namespace

void rot_destroy(RotResampler *r) {
    if (!r) return;
    for (void *p : {(void *)r->E, (void *)r->beta, (void *)r->twx, (void *)r->twy, (void *)r->T,
                    (void *)r->Mh, (void *)r->Mbar, (void *)r->part})
        if (p) (void)hipFree(p);
    delete r;
}

int rot_create(const float *kernel, double scale, const double *shifts, const double *other_shifts,
               int C, int n_a, int n_b, int Fy, int Fx, RotResampler **out) {
    SMI_REQUIRE(Fx <= 2048, "a rotated resampler keeps a row and its twiddles in LDS: rows of at "
                            "most 2048 pixels");
    SMI_REQUIRE(Fy <= 65535 && n_a <= 65535 && n_b <= 65535, "a rotated resampler: grid limit");
    auto *r = new RotResampler;
    *out = r;
    r->C = C; r->n_a = n_a; r->n_b = n_b; r->Fy = Fy; r->Fx = Fx; r->Kx = Fx / 2 + 1;
    const int Kx = r->Kx;
    const int64_t K = (int64_t)Fy * Kx;
    const RotPlan plan = rot_plan(n_a, n_b, Fy, Fx);
    r->kslice = plan.kslice;
    r->n_slices = plan.n_slices;
    SMI_REQUIRE((int64_t)C * r->n_slices <= 65535, "a rotated resampler: bands x slices exceed "
                                                   "the grid's z limit");
    const size_t n = rot_plane(r);
    std::vector<double2> twx, twy;
    rot_twiddles(Fx, &twx);
    rot_twiddles(Fy, &twy);
    float *d_kernel = nullptr;
    double *d_shifts = nullptr, *d_other = nullptr;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&r->E, (size_t)C * n_a * K * sizeof(float2)));
        SMI_HIP(hipMalloc((void **)&r->beta, (size_t)n_b * K * sizeof(float2)));
        SMI_HIP(hipMalloc((void **)&r->twx, Fx * sizeof(double2)));
        SMI_HIP(hipMalloc((void **)&r->twy, Fy * sizeof(double2)));
        SMI_HIP(hipMalloc((void **)&r->T, (n + kRotGuard) * sizeof(double2)));
        SMI_HIP(hipMalloc((void **)&r->Mh, (n + kRotGuard) * sizeof(float2)));
        SMI_HIP(hipMalloc((void **)&r->Mbar, (n + kRotGuard) * sizeof(double2)));
        if (r->n_slices > 1)
            SMI_HIP(hipMalloc((void **)&r->part,
                              ((size_t)C * r->n_slices * n_a * n_b + kRotGuard) * sizeof(double)));
        SMI_HIP(hipMalloc((void **)&d_kernel, (size_t)C * Fy * Fx * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&d_shifts, 2 * n_a * sizeof(double)));
        SMI_HIP(hipMalloc((void **)&d_other, 2 * n_b * sizeof(double)));
        SMI_HIP(hipMemcpy(r->twx, twx.data(), Fx * sizeof(double2), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(r->twy, twy.data(), Fy * sizeof(double2), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_kernel, kernel, (size_t)C * Fy * Fx * sizeof(float),
                          hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_shifts, shifts, 2 * n_a * sizeof(double), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_other, other_shifts, 2 * n_b * sizeof(double), hipMemcpyHostToDevice));
        // Dhat = rfftn(kernel) in float64 (in Mbar), then the two tables
        hipLaunchKernelGGL(rot_rows_forward_kernel, dim3((unsigned)(C * Fy)), dim3(256),
                           rot_row_lds(Fx), nullptr, d_kernel, r->twx, r->T, Fx, Kx);
        hipLaunchKernelGGL(rot_cols_kernel<double2>, dim3((Kx + 63) / 64, Fy, C), dim3(256), 0,
                           nullptr, r->T, r->twy, r->Mbar, Fy, Kx, 0);
        const unsigned kb = (unsigned)((K + 255) / 256);
        hipLaunchKernelGGL(rot_build_E_kernel, dim3(kb, n_a, C), dim3(256), 0, nullptr, r->Mbar,
                           d_shifts, scale, r->E, n_a, Fy, Fx, Kx);
        hipLaunchKernelGGL(rot_build_beta_kernel, dim3(kb, n_b), dim3(256), 0, nullptr, d_other,
                           r->beta, n_b, Fy, Fx, Kx);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipDeviceSynchronize());
        return rot_fill_work(r);
    };
    const int rc = run();
    for (void *p : {(void *)d_kernel, (void *)d_shifts, (void *)d_other})
        if (p) (void)hipFree(p);
    return rc;
}

// model [C][Fy][Fx] -> out [C][n_a][n_b] (device pointers)
int rot_forward(RotResampler *r, const float *model, float *out, hipStream_t s) {
    const int Kx = r->Kx;
    const int64_t K = (int64_t)r->Fy * Kx, MN = (int64_t)r->n_a * r->n_b;
    hipLaunchKernelGGL(rot_rows_forward_kernel, dim3((unsigned)(r->C * r->Fy)), dim3(256),
                       rot_row_lds(r->Fx), s, model, r->twx, r->T, r->Fx, Kx);
    hipLaunchKernelGGL(rot_cols_kernel<float2>, dim3((Kx + 63) / 64, r->Fy, r->C), dim3(256), 0, s,
                       r->T, r->twy, r->Mh, r->Fy, Kx, 0);
    const RotPlan plan = rot_plan(r->n_a, r->n_b, r->Fy, r->Fx);
    const int ti = plan.ti, tj = plan.tj;
    const dim3 grid(plan.tiles_b, plan.tiles_a, r->C * r->n_slices);
#define SMI_ROT_CONTRACT(TI, TJ)                                                               \
    hipLaunchKernelGGL((rot_contract_kernel<TI, TJ>), grid, dim3(256), 0, s, r->E, r->Mh,       \
                       r->beta, out, r->part, r->n_a, r->n_b, K, r->kslice, r->n_slices)
#define SMI_ROT_CONTRACT_ROW(TI)                                                               \
    switch (tj) {                                                                              \
    case 1: SMI_ROT_CONTRACT(TI, 1); break;                                                    \
    case 2: SMI_ROT_CONTRACT(TI, 2); break;                                                    \
    case 3: SMI_ROT_CONTRACT(TI, 3); break;                                                    \
    default: SMI_ROT_CONTRACT(TI, 4); break;                                                   \
    }
    switch (ti) {
    case 1: SMI_ROT_CONTRACT_ROW(1); break;
    case 2: SMI_ROT_CONTRACT_ROW(2); break;
    case 3: SMI_ROT_CONTRACT_ROW(3); break;
    default: SMI_ROT_CONTRACT_ROW(4); break;
    }
#undef SMI_ROT_CONTRACT_ROW
#undef SMI_ROT_CONTRACT
    if (r->n_slices > 1)
        hipLaunchKernelGGL(rot_reduce_kernel, dim3((unsigned)((MN + 255) / 256), r->C), dim3(256),
                           0, s, r->part, out, MN, r->n_slices);
    return SMI_OK;
}

// resid [C][n_a][n_b] -> gpad [C][Fy][Fx] (device pointers): the transpose of rot_forward
int rot_adjoint(RotResampler *r, const float *resid, float *gpad, hipStream_t s) {
    const int Kx = r->Kx;
    const int64_t K = (int64_t)r->Fy * Kx;
    hipLaunchKernelGGL(rot_mbar_kernel, dim3((unsigned)((K + 63) / 64), r->C), dim3(256), 0, s,
                       r->E, r->beta, resid, r->Mbar, r->n_a, r->n_b, K);
    hipLaunchKernelGGL(rot_cols_kernel<double2>, dim3((Kx + 63) / 64, r->Fy, r->C), dim3(256), 0,
                       s, r->Mbar, r->twy, r->T, r->Fy, Kx, 1);
    hipLaunchKernelGGL(rot_rows_inverse_kernel, dim3((unsigned)(r->C * r->Fy)), dim3(256),
                       (size_t)(Kx + r->Fx) * sizeof(double2), s, r->T, r->twx, gpad, r->Fx, Kx);
    return SMI_OK;
}

// did the guard bands behind the work arrays come back untouched?  (synchronises)
int rot_guards_ok(RotResampler *r, bool *ok) {
    const size_t n = rot_plane(r);
    std::vector<unsigned char> h(kRotGuard * sizeof(double2));
    *ok = true;
    auto check = [&](const void *p, size_t bytes) -> int {
        SMI_HIP(hipMemcpy(h.data(), p, bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < bytes; ++i) *ok = *ok && h[i] == 0xa5;
        return SMI_OK;
    };
    int rc = check(r->T + n, kRotGuard * sizeof(double2));
    if (!rc) rc = check(r->Mh + n, kRotGuard * sizeof(float2));
    if (!rc) rc = check(r->Mbar + n, kRotGuard * sizeof(double2));
    if (!rc && r->part)
        rc = check(r->part + (size_t)r->C * r->n_slices * r->n_a * r->n_b,
                   kRotGuard * sizeof(double));
    return rc;
}

}  // namespace smi
