// Multi-resolution rendering (reference scarlet/renderer.py:262-547, ResolutionRenderer):
// a high-resolution model is convolved with the difference kernel and resampled onto a
// low-resolution pixel grid.  For unrotated grids the reference does this per band as
//
//   model_conv[y, x, b] = (model shifted along x by the sub-pixel position of LR column b)
//   out[a, b]           = sum_{y, x} op[a, y, x] * model_conv[y, x, b]
//
// with op[a] = difference kernel shifted along y to LR row a (renderer.py:478-545).  Both
// steps are linear in the model, so the host precomputes the two operators once
// (scarlet_amd/renderer.py) and a rendering is two matrix products per band:
//
//   B[(y, x), b] = sum_x' model[y, x'] * P[(x, b), x']      (F_y x F_x) . (F_x x F_x n_b)
//   out[a, b]    = sum_{(y, x)} A[a, (y, x)] * B[(y, x), b]  (n_a x F_y F_x) . (F_y F_x x n_b)
//
// The products run on the matrix cores: v_mfma_f32_32x32x2_f32 tiles (f32 inputs, f32
// accumulation = an fmaf chain in k order), staged through LDS.  The reductions are long
// (the second product sums F_y F_x ~ 4e4..2e5 terms), so K is cut into slices of a few
// hundred terms: inside a slice the accumulation is float32, across slices the partial
// tiles are summed in double by a second kernel -- that keeps the renderings within
// ~1e-7 of the reference's float64 evaluation and gives a small output enough workgroups
// to fill the chip.  The bands of an observation are one batched launch.
//
// Between rotated grids the reference shifts kernel and model in 2-D instead; a resampler made
// by resampler_create_rotated evaluates that map in Fourier space (path 2, resample_rot.hip:
// the map, its sum order and the edge-column rule are described there and above
// smi_resampler_create in include/scarlet_amd.h) and holds neither A nor Pt.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"

namespace smi {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBK = 16;          // k depth of a block tile
constexpr int kPad = 4;          // LDS row padding (floats)
constexpr int kSliceTerms = 320; // float32 accumulation length inside a slice

// C_b[M x N] = A_b[M x K] . B_b[K x N] for b < n_batch (row major; the batch strides may
// be 0).  blockIdx.z = batch * n_slices + slice; slice z covers K in [z kslice, ...).
// n_slices == 1: the tile goes straight to C (float); otherwise to Cpart[b][z][M][N]
// (double) for reduce_slices_kernel.
//
// Block tile 64 TM x 64 TN, four wavefronts as 2 x 2, each with TM x TN tiles of
// v_mfma_f32_32x32x2_f32.  The operators of a rendering come in very different shapes --
// 300 x 15 000 outputs over 300 terms, 50 x 50 outputs over 90 000 terms, 90 000 x 50 over
// 50 -- so a dimension of up to 96 takes one MFMA tile per wavefront (round 2's single
// 128 x 128 tile spent 85 % of the matrix-core time of a 50 x 50 product on padding), and a
// wavefront skips the MFMA tiles that lie outside the matrix altogether (300 rows = 2.5 x 128:
// the last 64 rows of the third tile row are not computed).  The LDS tiles are double
// buffered: global loads of tile k + 1 are in flight during the products of tile k, their
// LDS stores go to the other buffer, one barrier per tile.
template <int TM, int TN, int BK = kBK>
__global__ __launch_bounds__(256) void gemm_mfma_kernel(const float *A, int64_t strideA,
                                                        const float *B, int64_t strideB,
                                                        float *C, int64_t strideC, double *Cpart,
                                                        int M, int N, int K, int kslice,
                                                        int n_slices) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    __shared__ float As[2][BK][BM + kPad], Bs[2][BK][BN + kPad];
    const int batch = blockIdx.z / n_slices, z = blockIdx.z - batch * n_slices;
    A += batch * strideA;
    B += batch * strideB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
    const int k_lo = z * kslice, k_hi = min(K, k_lo + kslice);

    // global -> registers -> LDS.  A tile: BM rows x BK k, thread t takes k = t % BK of
    // the rows t / BK + (256 / BK) q (a row's BK floats are one 64- or 128-byte segment); B
    // tile: BK k x BN columns, thread t takes column t % BN of the rows t / BN + (256 / BN) q.
    constexpr int RA = 256 / BK, QA = BM / RA, RB = 256 / BN, QB = BK / RB;
    const int a_k = tid % BK, a_r = tid / BK, b_n = tid % BN, b_k = tid / BN;
    float ra[QA], rb[QB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
            const int m = m0 + a_r + RA * q, k = k0 + a_k;
            ra[q] = (m < M && k < k_hi) ? A[(int64_t)m * K + k] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int kb = k0 + b_k + RB * q, n = n0 + b_n;
            rb[q] = (kb < k_hi && n < N) ? B[(int64_t)kb * N + n] : 0.f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < QA; ++q) As[buf][a_k][a_r + RA * q] = ra[q];
#pragma unroll
        for (int q = 0; q < QB; ++q) Bs[buf][b_k + RB * q][b_n] = rb[q];
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    // MFMA tiles of this wavefront that hold anything (wave-uniform)
    bool on[TM][TN];
    bool any = false, full = true;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            on[i][j] = m0 + wm + 32 * i < M && n0 + wn + 32 * j < N;
            any |= on[i][j];
            full &= on[i][j];
        }

    fetch(k_lo);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
        const bool more = k0 + BK < k_hi;
        if (more) fetch(k0 + BK);  // in flight during the products
        // operand layout of v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5]
        // and B[k = l >> 5][j = l & 31]
        if (any) {
            const int kk = lane >> 5, ij = lane & 31;
            auto products = [&](auto all_on) {
#pragma unroll
                for (int ks = 0; ks < BK; ks += 2) {
                    float a[TM], b[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[i] = As[buf][ks + kk][wm + 32 * i + ij];
#pragma unroll
                    for (int j = 0; j < TN; ++j) b[j] = Bs[buf][ks + kk][wn + 32 * j + ij];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            if (decltype(all_on)::value || on[i][j])
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
            };
            // (straight-line code for a wavefront whose tiles are all inside: a branch per
            // MFMA keeps the scheduler from moving the LDS reads ahead of the products)
            if (full) products(std::true_type{});
            else products(std::false_type{});
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // accumulator layout of the 32 x 32 tile: lane l, register e -> row 8 (e / 4) +
    // 4 (l >> 5) + e % 4, column l & 31
    double *Cz = Cpart ? Cpart + ((int64_t)batch * n_slices + z) * M * N : nullptr;
    float *Cb = C + batch * strideC;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + 32 * i + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
                const int n = n0 + wn + 32 * j + (lane & 31);
                if (m < M && n < N) {
                    if (Cz)
                        Cz[(int64_t)m * N + n] = (double)acc[i][j][e];
                    else
                        Cb[(int64_t)m * N + n] = acc[i][j][e];
                }
            }
}

// C_b = sum over the slices of Cpart[b][z] (double), b < n_batch.  A workgroup of sixteen
// wavefronts per 64 outputs: wavefront w sums the slices w, w + 16, ... four at a time (the
// loads of a group are independent: a wavefront that adds one slice after the other waits for
// every load in turn, which is what this kernel used to spend its 20 us on), the sixteen sums
// are combined in a fixed order.
__global__ __launch_bounds__(1024) void reduce_slices_kernel(const double *Cpart, float *C,
                                                            int64_t strideC, int64_t MN,
                                                            int n_slices) {
    __shared__ double part[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    double t = 0.0;
    if (i < MN) {
        const double *p = Cpart + (int64_t)b * n_slices * MN + i;
        int z = w;
        for (; z + 48 < n_slices; z += 64) {
            const double v0 = p[(int64_t)z * MN], v1 = p[(int64_t)(z + 16) * MN];
            const double v2 = p[(int64_t)(z + 32) * MN], v3 = p[(int64_t)(z + 48) * MN];
            t += (v0 + v1) + (v2 + v3);
        }
        for (; z < n_slices; z += 16) t += p[(int64_t)z * MN];
    }
    part[w][lane] = t;
    __syncthreads();
    if (w == 0 && i < MN) {
        double total = 0.0;
#pragma unroll
        for (int q = 0; q < 16; q += 4)
            total += (part[q][lane] + part[q + 1][lane]) + (part[q + 2][lane] + part[q + 3][lane]);
        C[b * strideC + i] = (float)total;
    }
}

}  // namespace

// What gemm() launches for an M x N x K product of n_batch matrices with `scratch_elems`
// doubles for the slice partials (host only): the variant gemm_mfma_kernel<tm, tn, bk>, the
// terms per slice (a multiple of kBK) and the number of slices.  Refuses a grid the device
// cannot launch.
int gemm_plan(int M, int N, int K, int n_batch, size_t scratch_elems, GemmPlan *p) {
    SMI_REQUIRE(M > 0 && N > 0 && K > 0 && n_batch > 0 && p, "gemm: bad sizes");
    // one MFMA tile per wavefront along a dimension of up to 96 (see the kernel)
    int tm = M <= 96 ? 1 : 2, tn = N <= 96 ? 1 : 2;
    auto n_tiles = [&](int a, int b) {
        return (int64_t)((M + 64 * a - 1) / (64 * a)) * ((N + 64 * b - 1) / (64 * b)) * n_batch;
    };
    // (a product of a few hundred rows and columns -- the transforms of the spectral path --
    // is 45 workgroups in 128 x 128 tiles and 125 in 64 x 64 tiles)
    const bool few = n_tiles(tm, tn) * std::max(1, (K + kSliceTerms - 1) / kSliceTerms) < 200;
    if (few) tm = tn = 1;
    const int64_t tiles = n_tiles(tm, tn);
    // slices of ~kSliceTerms terms (float32 accumulation length); fewer when the tiles
    // alone fill the chip several times over and the partials would not fit the scratch.
    // (Round 4: fewer, longer slices -- 18 instead of 47 for the 300 x 300 x 15 000 product, 61
    // instead of 169 MB of partials -- were measured and are slower, 260 against 230 us: the
    // 2 115 workgroups of the fine slicing hide each other's load latency, 810 do not.)
    int n_slices = std::max(1, (K + kSliceTerms - 1) / kSliceTerms);
    const size_t MN = (size_t)M * N;
    while (n_slices > 1 && ((size_t)n_slices * n_batch * MN > scratch_elems ||
                            (tiles >= 2048 && K <= 4 * kSliceTerms)))
        --n_slices;
    int kslice = (K + n_slices - 1) / n_slices;
    kslice = (kslice + kBK - 1) / kBK * kBK;
    n_slices = (K + kslice - 1) / kslice;
    // (a workgroup alone on its CU waits for every k-tile's loads: twice the depth per tile
    // where the grid does not fill the chip)
    p->tm = tm;
    p->tn = tn;
    p->bk = few ? 2 * kBK : kBK;
    p->kslice = kslice;
    p->n_slices = n_slices;
    SMI_REQUIRE((int64_t)n_slices * n_batch <= 65535,
                "gemm: slices x batch exceed the grid's z limit");
    return SMI_OK;
}

// gemm_plan with the slicing given: the tile variant and the k depth follow the number of
// products in the launch -- neither changes the order in which the terms of an output are
// added -- while the slices, which do (float32 inside, double across), are the caller's: those
// gemm_plan gives ONE member of the launch by itself.
int gemm_plan_sliced(int M, int N, int K, int n_batch, int kslice, int n_slices, GemmPlan *p) {
    SMI_REQUIRE(M > 0 && N > 0 && K > 0 && n_batch > 0 && p, "gemm: bad sizes");
    SMI_REQUIRE(kslice > 0 && kslice % kBK == 0 && n_slices == (K + kslice - 1) / kslice,
                "gemm: the slices do not cover K");
    int tm = M <= 96 ? 1 : 2, tn = N <= 96 ? 1 : 2;
    auto n_tiles = [&](int a, int b) {
        return (int64_t)((M + 64 * a - 1) / (64 * a)) * ((N + 64 * b - 1) / (64 * b)) * n_batch;
    };
    const bool few = n_tiles(tm, tn) * n_slices < 200;
    if (few) tm = tn = 1;
    p->tm = tm;
    p->tn = tn;
    p->bk = few ? 2 * kBK : kBK;
    p->kslice = kslice;
    p->n_slices = n_slices;
    SMI_REQUIRE((int64_t)n_slices * n_batch <= 65535,
                "gemm: slices x batch exceed the grid's z limit");
    return SMI_OK;
}

namespace {

// the launch of a plan: n_batch products, partials of the slices in `scratch` (n_slices x
// n_batch x M x N doubles when n_slices > 1)
int gemm_launch(const GemmPlan &p, const float *A, int64_t strideA, const float *B,
                int64_t strideB, float *C, int64_t strideC, int n_batch, double *scratch, int M,
                int N, int K, hipStream_t s) {
    const int bm = 64 * p.tm, bn = 64 * p.tn, kslice = p.kslice, n_slices = p.n_slices;
    const size_t MN = (size_t)M * N;
    const dim3 grid((N + bn - 1) / bn, (M + bm - 1) / bm, n_slices * n_batch);
    double *part = n_slices > 1 ? scratch : nullptr;
#define SMI_GEMM(TM, TN, BK)                                                                   \
    hipLaunchKernelGGL((gemm_mfma_kernel<TM, TN, BK>), grid, dim3(256), 0, s, A, strideA, B,   \
                       strideB, C, strideC, part, M, N, K, kslice, n_slices)
    if (p.bk == 2 * kBK) SMI_GEMM(1, 1, 2 * kBK);
    else if (p.tm == 1 && p.tn == 1) SMI_GEMM(1, 1, kBK);
    else if (p.tm == 1) SMI_GEMM(1, 2, kBK);
    else if (p.tn == 1) SMI_GEMM(2, 1, kBK);
    else SMI_GEMM(2, 2, kBK);
#undef SMI_GEMM
    if (n_slices > 1)
        hipLaunchKernelGGL(reduce_slices_kernel, dim3((unsigned)((MN + 63) / 64), n_batch),
                           dim3(1024), 0, s, scratch, C, strideC, (int64_t)MN, n_slices);
    return SMI_OK;
}

int gemm(const float *A, int64_t strideA, const float *B, int64_t strideB, float *C,
         int64_t strideC, int n_batch, double *scratch, size_t scratch_elems, int M, int N, int K,
         hipStream_t s) {
    GemmPlan p;
    const int rc = gemm_plan(M, N, K, n_batch, scratch_elems, &p);
    if (rc) return rc;
    return gemm_launch(p, A, strideA, B, strideB, C, strideC, n_batch, scratch, M, N, K, s);
}

// products of one launch of gemm_pooled: slices x products within the grid's z limit (and the
// reduction's y limit)
int gemm_pooled_chunk(int n_slices) { return std::max(1, 65535 / n_slices); }

// n_batch products whose slicing is given (gemm_plan_sliced): cut into launches of at most
// gemm_pooled_chunk products, which share `scratch` (n_slices x chunk x M x N doubles) one
// after the other on the stream.  Needs strideB == 0 or whole products per batch entry.
int gemm_pooled(int kslice, int n_slices, const float *A, int64_t strideA, const float *B,
                float *C, int64_t strideC, int n_batch, double *scratch, int M, int N, int K,
                hipStream_t s) {
    const int chunk = gemm_pooled_chunk(n_slices);
    for (int b0 = 0; b0 < n_batch; b0 += chunk) {
        const int nb = std::min(chunk, n_batch - b0);
        GemmPlan p;
        int rc = gemm_plan_sliced(M, N, K, nb, kslice, n_slices, &p);
        if (rc) return rc;
        rc = gemm_launch(p, A + b0 * strideA, strideA, B, 0, C + b0 * strideC, strideC, nb,
                         scratch, M, N, K, s);
        if (rc) return rc;
    }
    return SMI_OK;
}

__global__ void transpose_kernel(const float *in, float *out, int rows, int cols) {
    __shared__ float tile[32][33];
    const int c = blockIdx.x * 32 + threadIdx.x, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8)
        if (r0 + j < rows && c < cols) tile[j][threadIdx.x] = in[(int64_t)(r0 + j) * cols + c];
    __syncthreads();
    const int r = r0 + threadIdx.x, c0 = blockIdx.x * 32;
    for (int j = threadIdx.y; j < 32; j += 8)
        if (c0 + j < cols && r < rows) out[(int64_t)(c0 + j) * rows + r] = tile[threadIdx.x][j];
}

void launch_transpose(const float *in, float *out, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0,
                       s, in, out, rows, cols);
}


// ---------------------------------------------------------------------------------------
// The spectral path.  The reference shifts the padded model along x by a phase ramp between
// a real transform and its inverse on the padded grid (renderer.py:414-476), so the shift
// operator of a low-resolution column b is a circulant matrix: P[x', x, b] = s_b[(x - x') mod
// F_x].  With the transforms along x of the model rows, of the operator rows and of s_b
// (hat = sum_x . exp(-2 pi i k x / F_x), k <= F_x / 2, w_k = 1 for k = 0 and the Nyquist
// term, else 2), Parseval's identity turns the two dense products into
//
//   Mh[y, k]   = hat(model[y, :])[k]                           F_y x F_x x (F_x + 2)
//   G[a, k]    = sum_y conj(E[a, y, k]) Mh[y, k]               E = hat(A[a, y, :]), read once
//   out[a, b]  = Re sum_k beta[b, k] G[a, k]                   beta = w_k hat(s_b)[k] / F_x
//
// -- the same linear map (exact in exact arithmetic; checked against the dense products on
// every fixture pair), 3.2 GFLOP -> 0.13 GFLOP per 300 x 300 band and 90 MB of E through HBM
// instead of 450 MB of shifted models.  The adjoint runs the transposed chain:
//
//   Gbar[a, k] = sum_b resid[a, b] conj(beta[b, k])
//   Mbar[y, k] = sum_a Gbar[a, k] E[a, y, k]
//   g[y, x]    = sum_k Re(Mbar[y, k]) cos(2 pi k x / F_x) - Im(Mbar[y, k]) sin(2 pi k x / F_x)
//
// E is made on the device at set-up from the float32 operator the caller hands over, in
// float64 (row_dft_kernel); the sums over y, a, b and k run in float64 as well, the two
// transforms along x on the matrix cores (gemm above, K = F_x or F_x + 2 terms in float32).
// An operator Pt that is not circulant keeps the dense products.
// ---------------------------------------------------------------------------------------

// out[row][k] = scale_k sum_x in[row][x] tw[(k x) mod Fx], k < Kx; tw[j] = exp(-2 pi i j / Fx)
// in float64.  hermitian != 0: scale_k = w_k / Fx (the beta table), else 1.
__global__ __launch_bounds__(256) void row_dft_kernel(const float *in, const double2 *tw,
                                                      float2 *out, int Fx, int Kx, int hermitian) {
    extern __shared__ double dft_sm[];
    double *row = dft_sm;
    double2 *t = reinterpret_cast<double2 *>(dft_sm + ((Fx + 1) & ~1));
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
        if (hermitian) {
            const double sc = ((k == 0 || 2 * k == Fx) ? 1.0 : 2.0) / (double)Fx;
            re *= sc;
            im *= sc;
        }
        out[r * Kx + k] = make_float2((float)re, (float)im);
    }
}

// The kernels of the spectral path and of the low-resolution term take a blend dimension: with
// a member table `tab` (LowResMember, common.h) blockIdx.z -- blockIdx.x / y where noted -- is
// the member m of a pool of observations of one shape class; its operators E and beta come
// from the table, its work arrays are slice m of the pooled ones, and a member whose blend has
// stopped (state >= 2) is skipped: nothing of it is written again.  Without a table the
// kernels serve one resampler as before.  The order in which every sum is formed is the same
// in both uses, so a member gets the bits of its own resampler.

// One workgroup per (low-resolution row a, band c): G[k] = sum_y conj(E[c][a][y][k]) Mh[c][y][k]
// (wavefront w takes the rows y = w, w + 16, ..., four loads of E in flight per lane; lanes
// along k, so a wavefront reads 512 contiguous bytes of E per row), the sixteen partial sums
// combined in a fixed order, then out[c][a][b] = Re sum_k beta[b][k] G[k] by sixteen lanes
// per column b.  E is read exactly once per rendering.
__global__ __launch_bounds__(1024) void spectral_forward_kernel(const float2 *E, const float2 *Mh,
                                                                const float2 *beta, float *out,
                                                                int n_a, int n_b, int Fy, int Kx,
                                                                const LowResMember *tab,
                                                                const int32_t *state) {
    extern __shared__ double2 fwd_sm[];
    if (tab) {
        const LowResMember mb = tab[blockIdx.z];
        if (state[mb.blend] >= 2) return;
        E = mb.E;
        beta = mb.beta;
        Mh += (int64_t)blockIdx.z * gridDim.y * Fy * Kx;
        out += (int64_t)blockIdx.z * gridDim.y * n_a * n_b;
    }
    double2 *red = fwd_sm;         // [16][64]
    double2 *G = fwd_sm + 16 * 64;  // [Kx]
    const int a = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float2 *Ea = E + ((int64_t)c * n_a + a) * Fy * Kx;
    const float2 *Mc = Mh + (int64_t)c * Fy * Kx;
    for (int k0 = 0; k0 < Kx; k0 += 64) {
        const int k = k0 + lane;
        double re = 0.0, im = 0.0;
        if (k < Kx) {
            auto term = [&](float2 e, float2 m) {
                re = fma((double)e.x, (double)m.x, re);
                re = fma((double)e.y, (double)m.y, re);
                im = fma((double)e.x, (double)m.y, im);
                im = fma(-(double)e.y, (double)m.x, im);
            };
            int y = w;
            for (; y + 48 < Fy; y += 64) {
                const float2 e0 = Ea[(int64_t)y * Kx + k], e1 = Ea[(int64_t)(y + 16) * Kx + k];
                const float2 e2 = Ea[(int64_t)(y + 32) * Kx + k], e3 = Ea[(int64_t)(y + 48) * Kx + k];
                const float2 m0 = Mc[(int64_t)y * Kx + k], m1 = Mc[(int64_t)(y + 16) * Kx + k];
                const float2 m2 = Mc[(int64_t)(y + 32) * Kx + k], m3 = Mc[(int64_t)(y + 48) * Kx + k];
                term(e0, m0);
                term(e1, m1);
                term(e2, m2);
                term(e3, m3);
            }
            for (; y < Fy; y += 16) term(Ea[(int64_t)y * Kx + k], Mc[(int64_t)y * Kx + k]);
        }
        red[w * 64 + lane] = make_double2(re, im);
        __syncthreads();
        if (w == 0 && k < Kx) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                sr += red[q * 64 + lane].x;
                si += red[q * 64 + lane].y;
            }
            G[k] = make_double2(sr, si);
        }
        __syncthreads();
    }
    const int part = tid & 15;
    for (int b0 = 0; b0 < n_b; b0 += 64) {
        const int b = b0 + (tid >> 4);
        double t = 0.0;
        if (b < n_b)
            for (int k = part; k < Kx; k += 16) {
                const float2 bt = beta[(int64_t)b * Kx + k];
                const double2 g = G[k];
                t = fma((double)bt.x, g.x, t);
                t = fma(-(double)bt.y, g.y, t);
            }
        for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if (b < n_b && part == 0) out[((int64_t)c * n_a + a) * n_b + b] = (float)t;
    }
}

// Gbar[ca][k] = sum_b resid[ca][b] conj(beta[b][k]); one workgroup per (band, row a) and
// member (blockIdx.y)
__global__ __launch_bounds__(256) void spectral_gbar_kernel(const float *resid, const float2 *beta,
                                                            float2 *Gbar, int n_b, int Kx,
                                                            const LowResMember *tab,
                                                            const int32_t *state) {
    extern __shared__ float gbar_sm[];
    if (tab) {
        const LowResMember mb = tab[blockIdx.y];
        if (state[mb.blend] >= 2) return;
        beta = mb.beta;
        resid += (int64_t)blockIdx.y * gridDim.x * n_b;
        Gbar += (int64_t)blockIdx.y * gridDim.x * Kx;
    }
    const int64_t ca = blockIdx.x;
    for (int b = threadIdx.x; b < n_b; b += 256) gbar_sm[b] = resid[ca * n_b + b];
    __syncthreads();
    for (int k = threadIdx.x; k < Kx; k += 256) {
        double re = 0.0, im = 0.0;
        for (int b = 0; b < n_b; ++b) {
            const float2 bt = beta[(int64_t)b * Kx + k];
            const double r = (double)gbar_sm[b];
            re = fma(r, (double)bt.x, re);
            im = fma(-r, (double)bt.y, im);
        }
        Gbar[ca * Kx + k] = make_float2((float)re, (float)im);
    }
}

// Mbar[c][y][k] = sum_a Gbar[c][a][k] E[c][a][y][k]; one workgroup of four wavefronts per
// (model row y, band c), wavefront w takes a = w, w + 4, ...
__global__ __launch_bounds__(256) void spectral_adjoint_kernel(const float2 *E, const float2 *Gbar,
                                                               float2 *Mbar, int n_a, int Fy,
                                                               int Kx, const LowResMember *tab,
                                                               const int32_t *state) {
    __shared__ double2 red[4][64];
    if (tab) {
        const LowResMember mb = tab[blockIdx.z];
        if (state[mb.blend] >= 2) return;
        E = mb.E;
        Gbar += (int64_t)blockIdx.z * gridDim.y * n_a * Kx;
        Mbar += (int64_t)blockIdx.z * gridDim.y * Fy * Kx;
    }
    const int y = blockIdx.x, c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float2 *Ec = E + ((int64_t)c * n_a * Fy + y) * Kx;
    const float2 *Gc = Gbar + (int64_t)c * n_a * Kx;
    const int64_t sa = (int64_t)Fy * Kx;
    for (int k0 = 0; k0 < Kx; k0 += 64) {
        const int k = k0 + lane;
        double re = 0.0, im = 0.0;
        if (k < Kx) {
            auto term = [&](float2 g, float2 e) {
                re = fma((double)g.x, (double)e.x, re);
                re = fma(-(double)g.y, (double)e.y, re);
                im = fma((double)g.x, (double)e.y, im);
                im = fma((double)g.y, (double)e.x, im);
            };
            int a = w;
            for (; a + 12 < n_a; a += 16) {
                const float2 e0 = Ec[a * sa + k], e1 = Ec[(a + 4) * sa + k];
                const float2 e2 = Ec[(a + 8) * sa + k], e3 = Ec[(a + 12) * sa + k];
                const float2 g0 = Gc[(int64_t)a * Kx + k], g1 = Gc[(int64_t)(a + 4) * Kx + k];
                const float2 g2 = Gc[(int64_t)(a + 8) * Kx + k], g3 = Gc[(int64_t)(a + 12) * Kx + k];
                term(g0, e0);
                term(g1, e1);
                term(g2, e2);
                term(g3, e3);
            }
            for (; a < n_a; a += 4) term(Gc[(int64_t)a * Kx + k], Ec[a * sa + k]);
        }
        red[w][lane] = make_double2(re, im);
        __syncthreads();
        if (w == 0 && k < Kx) {
            const double sr = (red[0][lane].x + red[1][lane].x) + (red[2][lane].x + red[3][lane].x);
            const double si = (red[0][lane].y + red[1][lane].y) + (red[2][lane].y + red[3][lane].y);
            Mbar[((int64_t)c * Fy + y) * Kx + k] = make_float2((float)sr, (float)si);
        }
        __syncthreads();
    }
}

}  // namespace

struct Resampler {
    int C = 0, n_a = 0, n_b = 0, Fy = 0, Fx = 0;
    float *A = nullptr;    // [C][n_a][Fy * Fx]
    float *Pt = nullptr;   // [Fx][Fx * n_b]  (transposed shift operator, shared by the bands)
    float *model = nullptr, *out = nullptr;
    // dense products (made on first use: an operator Pt that is not circulant, or asked for)
    float *B = nullptr;    // [C][Fy * Fx * n_b]
    double *scratch = nullptr;
    size_t scratch_elems = 0;
    float *At = nullptr;   // [C][Fy * Fx][n_a]: A transposed (left operand of the adjoint)
    float *P = nullptr;    // [Fx * n_b][Fx]
    // spectral path
    int path = 0;          // 0: dense products, 1: spectral, 2: rotated grids
    RotResampler *rot = nullptr;  // path 2 (resample_rot.hip): neither A nor Pt exist
    bool spectral = false; // Pt is circulant and the tables below exist
    int Kx = 0;            // Fx / 2 + 1
    float2 *E = nullptr;    // [C][n_a][Fy][Kx]: transforms along x of the operator rows
    float2 *beta = nullptr; // [n_b][Kx]
    float *Wx = nullptr;    // [Fx][2 Kx]: cos, -sin interleaved (forward transform as a product)
    float *WxT = nullptr;   // [2 Kx][Fx]
    float2 *Mh = nullptr;   // [C][Fy][Kx]: transforms of the model rows / Mbar of the adjoint
    float2 *Gbar = nullptr; // [C][n_a][Kx]
    double *sscratch = nullptr;  // slice partials of the two transforms when Fx > kSliceTerms
    size_t sscratch_elems = 0;
};

namespace {

// P[x', x, b] == P[0, (x - x') mod Fx, b] for all entries (to float32 rounding of the largest)?
bool circulant_along_x(const float *Pt, int Fx, int n_b) {
    float top = 0.f;
    for (size_t i = 0; i < (size_t)Fx * n_b; ++i) top = std::max(top, std::fabs(Pt[i]));
    const float tol = 4e-7f * top;
    for (int xp = 1; xp < Fx; ++xp) {
        const float *row = Pt + (size_t)xp * Fx * n_b;
        for (int x = 0; x < Fx; ++x) {
            int d = x - xp;
            if (d < 0) d += Fx;
            const float *a = row + (size_t)x * n_b, *b = Pt + (size_t)d * n_b;
            for (int q = 0; q < n_b; ++q)
                if (!(std::fabs(a[q] - b[q]) <= tol)) return false;
        }
    }
    return true;
}

int build_dense(Resampler *r) {
    if (r->B) return SMI_OK;
    const size_t plane = (size_t)r->Fy * r->Fx;
    const size_t nA = (size_t)r->C * r->n_a * plane, nB = (size_t)r->C * plane * r->n_b;
    // double partials of the sliced products: out (n_a x n_b, thousands of slices) and
    // the model-sized results of the adjoint (F_y x F_x, ~100 slices), all bands at once
    const size_t slices_out = (plane + kSliceTerms - 1) / kSliceTerms + 1;
    const size_t slices_g = ((size_t)r->Fx * r->n_b + kSliceTerms - 1) / kSliceTerms + 1;
    r->scratch_elems = (size_t)r->C * std::max((size_t)r->n_a * r->n_b * slices_out,
                                               plane * slices_g);
    SMI_HIP(hipMalloc((void **)&r->B, nB * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->scratch, r->scratch_elems * sizeof(double)));
    // At[C][Fy Fx][n_a]: the left operand of the adjoint's first product; P: its second
    SMI_HIP(hipMalloc((void **)&r->At, nA * sizeof(float)));
    for (int c = 0; c < r->C; ++c)
        launch_transpose(r->A + (size_t)c * r->n_a * plane, r->At + (size_t)c * r->n_a * plane,
                         r->n_a, (int)plane, nullptr);
    SMI_HIP(hipMalloc((void **)&r->P, (size_t)r->Fx * r->Fx * r->n_b * sizeof(float)));
    launch_transpose(r->Pt, r->P, r->Fx, r->Fx * r->n_b, nullptr);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipDeviceSynchronize());
    return SMI_OK;
}

// doubles for the slice partials of the two transforms of a resampler with C bands
size_t spectral_scratch_elems(int C, int Fy, int Fx) {
    const int Kx = Fx / 2 + 1;
    const size_t slices = (size_t)(std::max(Fx, 2 * Kx) + kSliceTerms - 1) / kSliceTerms + 1;
    return (size_t)C * Fy * std::max(Fx, 2 * Kx) * slices;
}

// the transform tables of a row of Fx pixels: twiddles (float64) and the two transforms along
// x as matrices, Wx [Fx][2 Kx] (cos, -sin interleaved) and its transpose
void transform_tables(int Fx, std::vector<double2> *tw, std::vector<float> *Wx,
                      std::vector<float> *WxT) {
    const int Kx = Fx / 2 + 1;
    const double step = 2.0 * 3.14159265358979323846 / (double)Fx;
    tw->resize(Fx);
    for (int j = 0; j < Fx; ++j) (*tw)[j] = make_double2(std::cos(step * j), -std::sin(step * j));
    Wx->resize((size_t)Fx * 2 * Kx);
    WxT->resize((size_t)2 * Kx * Fx);
    for (int x = 0; x < Fx; ++x)
        for (int k = 0; k < Kx; ++k) {
            const double2 w = (*tw)[(int)(((int64_t)k * x) % Fx)];
            (*Wx)[(size_t)x * 2 * Kx + 2 * k] = (*WxT)[(size_t)(2 * k) * Fx + x] = (float)w.x;
            (*Wx)[(size_t)x * 2 * Kx + 2 * k + 1] = (*WxT)[(size_t)(2 * k + 1) * Fx + x] = (float)w.y;
        }
}

int build_spectral(Resampler *r, const float *Pt_host) {
    const int Fx = r->Fx, Fy = r->Fy, Kx = Fx / 2 + 1, n_a = r->n_a, n_b = r->n_b, C = r->C;
    r->Kx = Kx;
    std::vector<double2> tw;
    std::vector<float> Wx, WxT, S((size_t)n_b * Fx);
    transform_tables(Fx, &tw, &Wx, &WxT);
    for (int b = 0; b < n_b; ++b)  // s_b[x] = P[x' = 0][x][b]
        for (int x = 0; x < Fx; ++x) S[(size_t)b * Fx + x] = Pt_host[(size_t)x * n_b + b];
    double2 *d_tw = nullptr;
    float *d_S = nullptr;
    SMI_HIP(hipMalloc((void **)&d_tw, Fx * sizeof(double2)));
    SMI_HIP(hipMalloc((void **)&d_S, S.size() * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->E, (size_t)C * n_a * Fy * Kx * sizeof(float2)));
    SMI_HIP(hipMalloc((void **)&r->beta, (size_t)n_b * Kx * sizeof(float2)));
    SMI_HIP(hipMalloc((void **)&r->Wx, Wx.size() * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->WxT, WxT.size() * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->Mh, (size_t)C * Fy * Kx * sizeof(float2)));
    SMI_HIP(hipMalloc((void **)&r->Gbar, (size_t)C * n_a * Kx * sizeof(float2)));
    r->sscratch_elems = spectral_scratch_elems(C, Fy, Fx);
    SMI_HIP(hipMalloc((void **)&r->sscratch, r->sscratch_elems * sizeof(double)));
    SMI_HIP(hipMemcpy(d_tw, tw.data(), Fx * sizeof(double2), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(d_S, S.data(), S.size() * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(r->Wx, Wx.data(), Wx.size() * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(r->WxT, WxT.data(), WxT.size() * sizeof(float), hipMemcpyHostToDevice));
    const size_t lds = (size_t)((Fx + 1) & ~1) * sizeof(double) + (size_t)Fx * sizeof(double2);
    hipLaunchKernelGGL(row_dft_kernel, dim3((unsigned)((size_t)C * n_a * Fy)), dim3(256), lds,
                       nullptr, r->A, d_tw, r->E, Fx, Kx, 0);
    hipLaunchKernelGGL(row_dft_kernel, dim3(n_b), dim3(256), lds, nullptr, d_S, d_tw, r->beta, Fx,
                       Kx, 1);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipDeviceSynchronize());
    (void)hipFree(d_tw);
    (void)hipFree(d_S);
    r->spectral = true;
    return SMI_OK;
}

}  // namespace

int resampler_create(const float *A, const float *Pt, int C, int n_a, int n_b, int Fy, int Fx,
                     Resampler **out) {
    auto *r = new Resampler;
    r->C = C; r->n_a = n_a; r->n_b = n_b; r->Fy = Fy; r->Fx = Fx;
    const size_t nA = (size_t)C * n_a * Fy * Fx, nP = (size_t)Fx * Fx * n_b;
    *out = r;
    SMI_HIP(hipMalloc((void **)&r->A, nA * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->Pt, nP * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->model, (size_t)C * Fy * Fx * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->out, (size_t)C * n_a * n_b * sizeof(float)));
    SMI_HIP(hipMemcpy(r->A, A, nA * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(r->Pt, Pt, nP * sizeof(float), hipMemcpyHostToDevice));
    // (the transform tables of a row live in LDS: 24 bytes per column)
    if (Fx <= 2048 && circulant_along_x(Pt, Fx, n_b)) {
        const int rc = build_spectral(r, Pt);
        if (rc) return rc;
        r->path = 1;
        return SMI_OK;
    }
    return build_dense(r);
}

int resampler_create_rotated(const float *kernel, double scale, const double *shifts,
                             const double *other_shifts, int C, int n_a, int n_b, int Fy, int Fx,
                             Resampler **out) {
    auto *r = new Resampler;
    r->C = C; r->n_a = n_a; r->n_b = n_b; r->Fy = Fy; r->Fx = Fx;
    r->path = 2;
    *out = r;
    SMI_HIP(hipMalloc((void **)&r->model, (size_t)C * Fy * Fx * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&r->out, (size_t)C * n_a * n_b * sizeof(float)));
    return rot_create(kernel, scale, shifts, other_shifts, C, n_a, n_b, Fy, Fx, &r->rot);
}

int resampler_get_path(const Resampler *r) { return r->path; }

int resampler_set_path(Resampler *r, int path) {
    if (r->path == 2) {
        SMI_REQUIRE(path == 2, "a resampler between rotated grids has no other path");
        return SMI_OK;
    }
    SMI_REQUIRE(path != 2, "path 2 is that of a resampler made by smi_resampler_create_rotated");
    SMI_REQUIRE(path == 0 || path == 1, "path is 0 (dense products) or 1 (spectral)");
    SMI_REQUIRE(path == 0 || r->spectral,
                "the shift operator of this resampler is not circulant: dense products only");
    if (path == 0) {
        const int rc = build_dense(r);
        if (rc) return rc;
    }
    r->path = path;
    return SMI_OK;
}

void resampler_destroy(Resampler *r) {
    if (!r) return;
    for (void *p : {(void *)r->A, (void *)r->Pt, (void *)r->model, (void *)r->B, (void *)r->out,
                    (void *)r->scratch, (void *)r->At, (void *)r->P, (void *)r->E,
                    (void *)r->beta, (void *)r->Wx, (void *)r->WxT, (void *)r->Mh,
                    (void *)r->Gbar, (void *)r->sscratch})
        if (p) (void)hipFree(p);
    rot_destroy(r->rot);
    delete r;
}

// r->model (device, padded) -> r->out, on stream s; all bands in one launch per product
static int resampler_forward(Resampler *r, hipStream_t s) {
    const int64_t plane = (int64_t)r->Fy * r->Fx;
    if (r->path == 2) return rot_forward(r->rot, r->model, r->out, s);
    if (r->path == 1) {
        const int Kx = r->Kx;
        int rc = gemm(r->model, plane, r->Wx, 0, reinterpret_cast<float *>(r->Mh),
                      (int64_t)r->Fy * 2 * Kx, r->C, r->sscratch, r->sscratch_elems, r->Fy, 2 * Kx,
                      r->Fx, s);
        if (rc) return rc;
        const size_t lds = (size_t)(16 * 64 + Kx) * sizeof(double2);
        hipLaunchKernelGGL(spectral_forward_kernel, dim3(r->n_a, r->C), dim3(1024), lds, s, r->E,
                           r->Mh, r->beta, r->out, r->n_a, r->n_b, r->Fy, Kx, nullptr, nullptr);
        return SMI_OK;
    }
    int rc = gemm(r->model, plane, r->Pt, 0, r->B, plane * r->n_b, r->C, r->scratch,
                  r->scratch_elems, r->Fy, r->Fx * r->n_b, r->Fx, s);
    if (rc) return rc;
    return gemm(r->A, (int64_t)r->n_a * plane, r->B, plane * r->n_b, r->out,
                (int64_t)r->n_a * r->n_b, r->C, r->scratch, r->scratch_elems, r->n_a, r->n_b,
                (int)plane, s);
}

// gradient of the padded bands from the weighted residual [C][n_a][n_b] (the transposed chain)
static int resampler_adjoint(Resampler *r, const float *resid, float *gpad, hipStream_t s) {
    const int64_t plane = (int64_t)r->Fy * r->Fx;
    if (r->path == 2) return rot_adjoint(r->rot, resid, gpad, s);
    if (r->path == 1) {
        const int Kx = r->Kx;
        hipLaunchKernelGGL(spectral_gbar_kernel, dim3(r->C * r->n_a), dim3(256),
                           r->n_b * sizeof(float), s, resid, r->beta, r->Gbar, r->n_b, Kx, nullptr,
                           nullptr);
        hipLaunchKernelGGL(spectral_adjoint_kernel, dim3(r->Fy, r->C), dim3(256), 0, s, r->E,
                           r->Gbar, r->Mh, r->n_a, r->Fy, Kx, nullptr, nullptr);
        return gemm(reinterpret_cast<float *>(r->Mh), (int64_t)r->Fy * 2 * Kx, r->WxT, 0, gpad,
                    plane, r->C, r->sscratch, r->sscratch_elems, r->Fy, r->Fx, 2 * Kx, s);
    }
    int rc = gemm(r->At, (int64_t)r->n_a * plane, resid, (int64_t)r->n_a * r->n_b, r->B,
                  plane * r->n_b, r->C, r->scratch, r->scratch_elems, (int)plane, r->n_b, r->n_a,
                  s);
    if (rc) return rc;
    return gemm(r->B, plane * r->n_b, r->P, 0, gpad, plane, r->C, r->scratch, r->scratch_elems,
                r->Fy, r->Fx, r->Fx * r->n_b, s);
}

int resampler_render(Resampler *r, const float *model, float *out) {
    const size_t plane = (size_t)r->Fy * r->Fx;
    SMI_HIP(hipMemcpy(r->model, model, r->C * plane * sizeof(float), hipMemcpyHostToDevice));
    int rc = resampler_forward(r, nullptr);
    if (rc) return rc;
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipDeviceSynchronize());
    SMI_HIP(hipMemcpy(out, r->out, (size_t)r->C * r->n_a * r->n_b * sizeof(float),
                      hipMemcpyDeviceToHost));
    return SMI_OK;
}

// the transposed chain on host buffers: resid [C][n_a][n_b] -> gpad [C][Fy][Fx], on the
// resampler's current path (the counterpart of resampler_render; test entry point)
int resampler_adjoint_host(Resampler *r, const float *resid, float *gpad) {
    const size_t n = (size_t)r->C * r->n_a * r->n_b, plane = (size_t)r->Fy * r->Fx;
    float *d_resid = nullptr, *d_gpad = nullptr;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&d_resid, n * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&d_gpad, r->C * plane * sizeof(float)));
        SMI_HIP(hipMemcpy(d_resid, resid, n * sizeof(float), hipMemcpyHostToDevice));
        const int rc = resampler_adjoint(r, d_resid, d_gpad, nullptr);
        if (rc) return rc;
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipDeviceSynchronize());
        SMI_HIP(hipMemcpy(gpad, d_gpad, r->C * plane * sizeof(float), hipMemcpyDeviceToHost));
        return SMI_OK;
    };
    const int rc = run();
    if (d_resid) (void)hipFree(d_resid);
    if (d_gpad) (void)hipFree(d_gpad);
    return rc;
}

// Rendering and transpose of a rotated resampler on host buffers, for the tests: out and gpad
// hold NaNs before the launches, a guard band of kGuard floats lies before and after each, and
// the work arrays of the rotated map carry guards of their own (rot_guards_ok).
int resampler_rotated_test(Resampler *r, const float *model, const float *resid, float *out,
                           float *gpad, int32_t *guard_ok) {
    SMI_REQUIRE(r->path == 2 && r->rot, "not a resampler between rotated grids");
    constexpr size_t kGuard = 256;
    const size_t plane = (size_t)r->C * r->Fy * r->Fx, n = (size_t)r->C * r->n_a * r->n_b;
    const uint32_t fbits = 0x7fc00000u, gbits = 0xa5a5a5a5u;
    float fnan, fguard;
    memcpy(&fnan, &fbits, 4);
    memcpy(&fguard, &gbits, 4);
    std::vector<float> h_out(n + 2 * kGuard, fnan), h_g(plane + 2 * kGuard, fnan);
    for (size_t i = 0; i < kGuard; ++i) {
        h_out[i] = h_out[kGuard + n + i] = fguard;
        h_g[i] = h_g[kGuard + plane + i] = fguard;
    }
    float *d_out = nullptr, *d_g = nullptr, *d_resid = nullptr;
    bool work_ok = false;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&d_out, h_out.size() * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&d_g, h_g.size() * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&d_resid, n * sizeof(float)));
        SMI_HIP(hipMemcpy(d_out, h_out.data(), h_out.size() * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_g, h_g.data(), h_g.size() * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_resid, resid, n * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(r->model, model, plane * sizeof(float), hipMemcpyHostToDevice));
        int rc = rot_fill_work(r->rot);  // whatever ran before: unwritten work elements are NaNs
        if (rc) return rc;
        if ((rc = rot_forward(r->rot, r->model, d_out + kGuard, nullptr))) return rc;
        if ((rc = rot_adjoint(r->rot, d_resid, d_g + kGuard, nullptr))) return rc;
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipDeviceSynchronize());
        SMI_HIP(hipMemcpy(h_out.data(), d_out, h_out.size() * sizeof(float), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(h_g.data(), d_g, h_g.size() * sizeof(float), hipMemcpyDeviceToHost));
        return rot_guards_ok(r->rot, &work_ok);
    };
    const int rc = run();
    for (void *p : {(void *)d_out, (void *)d_g, (void *)d_resid})
        if (p) (void)hipFree(p);
    if (rc) return rc;
    bool ok = work_ok;
    for (size_t i = 0; i < kGuard; ++i) {
        ok = ok && memcmp(&h_out[i], &fguard, 4) == 0 &&
             memcmp(&h_out[kGuard + n + i], &fguard, 4) == 0;
        ok = ok && memcmp(&h_g[i], &fguard, 4) == 0 &&
             memcmp(&h_g[kGuard + plane + i], &fguard, 4) == 0;
    }
    *guard_ok = ok ? 1 : 0;
    memcpy(out, h_out.data() + kGuard, n * sizeof(float));
    memcpy(gpad, h_g.data() + kGuard, plane * sizeof(float));
    return SMI_OK;
}

// gemm() on host operands, for the tests: C and the scratch hold NaNs before the launch, a
// guard band of kGuard floats lies before and after C and one of kGuard doubles after the
// scratch; *guard_ok tells whether all three came back untouched.
int gemm_test(const float *A, int64_t strideA, const float *B, int64_t strideB, float *C,
              int64_t strideC, int n_batch, int M, int N, int K, size_t scratch_elems,
              GemmPlan *plan, int32_t *guard_ok) {
    constexpr size_t kGuard = 256;
    const int rc0 = gemm_plan(M, N, K, n_batch, scratch_elems, plan);
    if (rc0) return rc0;
    SMI_REQUIRE(strideA >= 0 && strideB >= 0 && (n_batch == 1 || strideC >= (int64_t)M * N),
                "gemm_test: bad strides");
    const size_t nA = (size_t)(n_batch - 1) * strideA + (size_t)M * K;
    const size_t nB = (size_t)(n_batch - 1) * strideB + (size_t)K * N;
    const size_t nC = (size_t)(n_batch - 1) * strideC + (size_t)M * N;
    uint32_t fbits = 0x7fc00000u, gbits = 0xa5a5a5a5u;
    uint64_t dbits = 0x7ff8000000000000ull, gdbits = 0xa5a5a5a5a5a5a5a5ull;
    float fnan, fguard;
    double dnan, dguard;
    memcpy(&fnan, &fbits, 4);
    memcpy(&fguard, &gbits, 4);
    memcpy(&dnan, &dbits, 8);
    memcpy(&dguard, &gdbits, 8);
    std::vector<float> hC(nC + 2 * kGuard, fnan);
    std::vector<double> hS(scratch_elems + kGuard, dnan);
    for (size_t i = 0; i < kGuard; ++i) {
        hC[i] = hC[kGuard + nC + i] = fguard;
        hS[scratch_elems + i] = dguard;
    }
    float *dA = nullptr, *dB = nullptr, *dC = nullptr;
    double *dS = nullptr;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&dA, nA * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&dB, nB * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&dC, hC.size() * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&dS, hS.size() * sizeof(double)));
        SMI_HIP(hipMemcpy(dA, A, nA * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(dB, B, nB * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(dC, hC.data(), hC.size() * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(dS, hS.data(), hS.size() * sizeof(double), hipMemcpyHostToDevice));
        const int rc = gemm(dA, strideA, dB, strideB, dC + kGuard, strideC, n_batch, dS,
                            scratch_elems, M, N, K, nullptr);
        if (rc) return rc;
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipDeviceSynchronize());
        SMI_HIP(hipMemcpy(hC.data(), dC, hC.size() * sizeof(float), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(hS.data() + scratch_elems, dS + scratch_elems, kGuard * sizeof(double),
                          hipMemcpyDeviceToHost));
        return SMI_OK;
    };
    const int rc = run();
    for (void *p : {(void *)dA, (void *)dB, (void *)dC, (void *)dS})
        if (p) (void)hipFree(p);
    if (rc) return rc;
    bool ok = true;
    for (size_t i = 0; i < kGuard; ++i) {
        ok = ok && memcmp(&hC[i], &fguard, 4) == 0 && memcmp(&hC[kGuard + nC + i], &fguard, 4) == 0;
        ok = ok && memcmp(&hS[scratch_elems + i], &dguard, 8) == 0;
    }
    *guard_ok = ok ? 1 : 0;
    memcpy(C, hC.data() + kGuard, nC * sizeof(float));
    return SMI_OK;
}

// device time of `n_rep` renderings of the resident model (no host transfers): the
// figure the flops roofline of BASELINE config 5 is measured on
int resampler_time(Resampler *r, int n_rep, double *ms_per_render) {
    hipEvent_t e0, e1;
    SMI_HIP(hipEventCreate(&e0));
    SMI_HIP(hipEventCreate(&e1));
    int rc = resampler_forward(r, nullptr);  // warm-up
    if (rc) return rc;
    SMI_HIP(hipEventRecord(e0, nullptr));
    for (int i = 0; i < n_rep; ++i)
        if ((rc = resampler_forward(r, nullptr))) return rc;
    SMI_HIP(hipEventRecord(e1, nullptr));
    SMI_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SMI_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_render = (double)ms / n_rep;
    return SMI_OK;
}

// device time of `n_rep` transposes of a zero residual (no host transfers), on the resampler's
// current path
int resampler_time_adjoint(Resampler *r, int n_rep, double *ms_per_call) {
    const size_t n = (size_t)r->C * r->n_a * r->n_b, plane = (size_t)r->C * r->Fy * r->Fx;
    float *d_resid = nullptr, *d_gpad = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&d_resid, n * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&d_gpad, plane * sizeof(float)));
        SMI_HIP(hipMemset(d_resid, 0, n * sizeof(float)));
        SMI_HIP(hipEventCreate(&e0));
        SMI_HIP(hipEventCreate(&e1));
        int rc = resampler_adjoint(r, d_resid, d_gpad, nullptr);  // warm-up
        if (rc) return rc;
        SMI_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < n_rep; ++i)
            if ((rc = resampler_adjoint(r, d_resid, d_gpad, nullptr))) return rc;
        SMI_HIP(hipEventRecord(e1, nullptr));
        SMI_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        SMI_HIP(hipEventElapsedTime(&ms, e0, e1));
        *ms_per_call = (double)ms / n_rep;
        return SMI_OK;
    };
    const int rc = run();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_resid) (void)hipFree(d_resid);
    if (d_gpad) (void)hipFree(d_gpad);
    return rc;
}

// ---------------------------------------------------------------------------------------
// The low-resolution observation as a term of the fit (Blend._loss_func sums the
// observations' log-likelihoods, blend.py:265-271): rendering as above, residual
// w (m - d) and chi^2, and the transpose of the two products back to the model frame,
//
//   T[(y, x), b] = sum_a A[a, (y, x)] r[a, b]           (F_y F_x x n_a) . (n_a x n_b)
//   g[y, x']     = sum_{(x, b)} T[y, (x, b)] P[(x, b), x']   (F_y x F_x n_b) . (F_x n_b x F_x)
//
// LowRes is the term of a batch of one blend on either path of its resampler; LowResPool
// (below) holds the observations of one shape class of a batch of any size, each with its own
// operators, on the spectral path.
// ---------------------------------------------------------------------------------------
namespace {

// centred zero padding of the observed bands of the model cube (fft._pad, fft.py:82-113)
__global__ void lowres_pad_kernel(const float *P, int Py, int Px, const int32_t *channels, int H,
                                  int W, int y0, int x0, float *padded, int Fy, int Fx,
                                  const LowResMember *tab, const int32_t *state, int Cm) {
    if (tab) {  // member blockIdx.z: the cube of its blend, slice m of the padded pool
        const LowResMember mb = tab[blockIdx.z];
        if (state[mb.blend] >= 2) return;
        P += (int64_t)mb.blend * Cm * Py * Px;
        channels = mb.channels;
        padded += (int64_t)blockIdx.z * gridDim.y * Fy * Fx;
    }
    const int c = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Fy * Fx) return;
    const int y = i / Fx - y0, x = i % Fx - x0;
    const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    padded[(int64_t)c * Fy * Fx + i] = in ? P[((int64_t)channels[c] * Py + y) * Px + x] : 0.f;
}

// resid = w (m - d); term = log_norm + chi^2 / 2 (observation.py:147-186)
__global__ __launch_bounds__(1024) void lowres_residual_kernel(const float *rendered,
                                                               const float *data,
                                                               const float *weights, float *resid,
                                                               int n, double log_norm,
                                                               double *term,
                                                               const LowResMember *tab,
                                                               const int32_t *state) {
    __shared__ double part[16];
    if (tab) {  // one workgroup per member: the slot of its blend's term
        const LowResMember mb = tab[blockIdx.x];
        if (state[mb.blend] >= 2) return;
        rendered += (int64_t)blockIdx.x * n;
        resid += (int64_t)blockIdx.x * n;
        data = mb.data;
        weights = mb.weights;
        log_norm = mb.log_norm;
        term = mb.term;
    }
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float d = rendered[i] - data[i], w = weights[i];
        resid[i] = w * d;
        t += (double)w * d * d;
    }
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < 16; ++i) total += part[i];
        term[0] = log_norm + 0.5 * total;
    }
}

__global__ void lowres_add_kernel(const float *gpad, int Fy, int Fx, int y0, int x0,
                                  const int32_t *channels, int H, int W, float *Q, int Py,
                                  int Px, const LowResMember *tab, const int32_t *state,
                                  int Cm) {
    if (tab) {
        const LowResMember mb = tab[blockIdx.z];
        if (state[mb.blend] >= 2) return;
        Q += (int64_t)mb.blend * Cm * Py * Px;
        channels = mb.channels;
        gpad += (int64_t)blockIdx.z * gridDim.y * Fy * Fx;
    }
    const int c = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    Q[((int64_t)channels[c] * Py + y) * Px + x] +=
        gpad[((int64_t)c * Fy + y + y0) * Fx + x + x0];
}

}  // namespace

struct LowRes {
    Resampler *r = nullptr;  // not owned
    int H = 0, W = 0, y0 = 0, x0 = 0;
    int32_t *channels = nullptr;
    float *data = nullptr, *weights = nullptr, *resid = nullptr, *gpad = nullptr;
    double *term = nullptr;  // slot of the batch's array of extra loss terms (not owned)
    double log_norm = 0.0;
};

void lowres_destroy(LowRes *l) {
    if (!l) return;
    for (void *p : {(void *)l->channels, (void *)l->data, (void *)l->weights, (void *)l->resid,
                    (void *)l->gpad})
        if (p) (void)hipFree(p);
    delete l;
}

int lowres_create(Resampler *r, const int32_t *channels, const float *data, const float *weights,
                  double log_norm, int H, int W, double *term_slot, LowRes **out) {
    SMI_REQUIRE(r->Fy >= H && r->Fx >= W, "resampler FFT shape smaller than the model frame");
    auto *l = new LowRes;
    *out = l;
    l->r = r; l->H = H; l->W = W; l->log_norm = log_norm;
    l->y0 = (r->Fy - H + 1) / 2;
    l->x0 = (r->Fx - W + 1) / 2;
    const size_t plane = (size_t)r->Fy * r->Fx, n = (size_t)r->C * r->n_a * r->n_b;
    SMI_HIP(hipMalloc((void **)&l->channels, r->C * sizeof(int32_t)));
    SMI_HIP(hipMalloc((void **)&l->data, n * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&l->weights, n * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&l->resid, n * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&l->gpad, r->C * plane * sizeof(float)));
    l->term = term_slot;
    SMI_HIP(hipMemcpy(l->channels, channels, r->C * sizeof(int32_t), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(l->data, data, n * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(l->weights, weights, n * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemset(l->term, 0, sizeof(double)));
    return SMI_OK;
}

// model cube P [C_model][Py][Px] -> rendering (r->out), term, and with `backward` the
// gradient of chi^2 / 2 with respect to the padded observed bands (l->gpad)
int lowres_evaluate(LowRes *l, const float *P, int Py, int Px, int backward, hipStream_t s) {
    Resampler *r = l->r;
    const int plane = r->Fy * r->Fx, n = r->C * r->n_a * r->n_b;
    hipLaunchKernelGGL(lowres_pad_kernel, dim3((plane + 255) / 256, r->C), dim3(256), 0, s, P, Py,
                       Px, l->channels, l->H, l->W, l->y0, l->x0, r->model, r->Fy, r->Fx, nullptr,
                       nullptr, 0);
    int rc = resampler_forward(r, s);
    if (rc) return rc;
    hipLaunchKernelGGL(lowres_residual_kernel, dim3(1), dim3(1024), 0, s, r->out, l->data,
                       l->weights, l->resid, n, l->log_norm, l->term, nullptr, nullptr);
    if (!backward) return SMI_OK;
    return resampler_adjoint(r, l->resid, l->gpad, s);
}

void lowres_add_gradient(LowRes *l, float *Q, int Py, int Px, hipStream_t s) {
    Resampler *r = l->r;
    hipLaunchKernelGGL(lowres_add_kernel, dim3((l->H * l->W + 255) / 256, r->C), dim3(256), 0, s,
                       l->gpad, r->Fy, r->Fx, l->y0, l->x0, l->channels, l->H, l->W, Q, Py, Px,
                       nullptr, nullptr, 0);
}

int lowres_get_rendered(LowRes *l, float *out, hipStream_t s) {
    Resampler *r = l->r;
    SMI_HIP(hipMemcpyAsync(out, r->out, (size_t)r->C * r->n_a * r->n_b * sizeof(float),
                           hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    return SMI_OK;
}

bool resampler_shape(const Resampler *r, int *C, int *n_a, int *n_b, int *Fy, int *Fx) {
    *C = r->C; *n_a = r->n_a; *n_b = r->n_b; *Fy = r->Fy; *Fx = r->Fx;
    return r->path == 1;
}

// ---------------------------------------------------------------------------------------
// The low-resolution terms of a batch of blends.  Observations of one shape class (C, n_a,
// n_b, Fy, Fx) form a pool: every member owns its operators E and beta (a device table of
// pointers, LowResMember) and slice m of the pooled work arrays, and the chain above runs
// once for all of them -- pad, transform (one batched product over members x bands),
// spectral_forward over (a, band, member), one residual workgroup per member, gbar, adjoint,
// the transform back and the add into the member's blend of Q: nine launches per iteration
// whatever the number of blends.  The two batched products take the slices the member's own
// resampler gets (gemm_plan for its C bands and its own scratch), so every sum is formed in
// the order of the single fit.  A member holds neither A nor Pt on the device: E and beta are
// made from the host operators when it is added.
// ---------------------------------------------------------------------------------------
constexpr size_t kPoolGuard = 256;  // guard floats around the pooled outputs (lowres_pool_test)

struct LowResPool {
    int C = 0, n_a = 0, n_b = 0, Fy = 0, Fx = 0, Kx = 0;
    int H = 0, W = 0, y0 = 0, x0 = 0;
    int kslice_f = 0, nsl_f = 0, kslice_b = 0, nsl_b = 0;  // the member's own slicing
    struct Owned {
        float2 *E = nullptr, *beta = nullptr;
        float *data = nullptr, *weights = nullptr;
        int32_t *channels = nullptr;
    };
    std::vector<Owned> owned;
    std::vector<LowResMember> members;  // host copy of the table
    double2 *tw = nullptr;
    float *Wx = nullptr, *WxT = nullptr;
    // pooled work arrays of `cap` members (made by lowres_pool_ready)
    int cap = 0;
    bool dirty = true;
    LowResMember *table = nullptr;
    float *model = nullptr;   // [n][C][Fy][Fx]
    float *out = nullptr;     // kPoolGuard + [n][C][n_a][n_b] + kPoolGuard
    float *resid = nullptr;   // [n][C][n_a][n_b]
    float *gpad = nullptr;    // kPoolGuard + [n][C][Fy][Fx] + kPoolGuard
    float2 *Mh = nullptr;     // [n][C][Fy][Kx]
    float2 *Gbar = nullptr;   // [n][C][n_a][Kx]
    double *scratch = nullptr;
};

int lowres_gemm_plans(int C, int Fy, int Fx, int n_members, int adjoint, GemmPlan *own,
                      GemmPlan *pooled) {
    SMI_REQUIRE(C > 0 && Fy > 0 && Fx > 0 && n_members > 0 && own && pooled, "bad argument");
    const int Kx = Fx / 2 + 1;
    const int N = adjoint ? Fx : 2 * Kx, K = adjoint ? 2 * Kx : Fx;
    int rc = gemm_plan(Fy, N, K, C, spectral_scratch_elems(C, Fy, Fx), own);
    if (rc) return rc;
    const int64_t chunk = gemm_pooled_chunk(own->n_slices);
    return gemm_plan_sliced(Fy, N, K, (int)std::min<int64_t>(chunk, (int64_t)n_members * C),
                            own->kslice, own->n_slices, pooled);
}

int lowres_pool_create(int C, int n_a, int n_b, int Fy, int Fx, int H, int W, LowResPool **out) {
    SMI_REQUIRE(C > 0 && n_a > 0 && n_b > 0 && Fy > 0 && Fx > 0, "bad sizes");
    SMI_REQUIRE(Fy >= H && Fx >= W, "resampler FFT shape smaller than the model frame");
    SMI_REQUIRE(Fx <= 2048, "rows too long for the transform tables");
    auto *p = new LowResPool;
    *out = p;
    p->C = C; p->n_a = n_a; p->n_b = n_b; p->Fy = Fy; p->Fx = Fx; p->Kx = Fx / 2 + 1;
    p->H = H; p->W = W;
    p->y0 = (Fy - H + 1) / 2;
    p->x0 = (Fx - W + 1) / 2;
    GemmPlan own, pooled;
    int rc = lowres_gemm_plans(C, Fy, Fx, 1, 0, &own, &pooled);
    if (rc) return rc;
    p->kslice_f = own.kslice; p->nsl_f = own.n_slices;
    if ((rc = lowres_gemm_plans(C, Fy, Fx, 1, 1, &own, &pooled))) return rc;
    p->kslice_b = own.kslice; p->nsl_b = own.n_slices;
    std::vector<double2> tw;
    std::vector<float> Wx, WxT;
    transform_tables(Fx, &tw, &Wx, &WxT);
    SMI_HIP(hipMalloc((void **)&p->tw, Fx * sizeof(double2)));
    SMI_HIP(hipMalloc((void **)&p->Wx, Wx.size() * sizeof(float)));
    SMI_HIP(hipMalloc((void **)&p->WxT, WxT.size() * sizeof(float)));
    SMI_HIP(hipMemcpy(p->tw, tw.data(), Fx * sizeof(double2), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(p->Wx, Wx.data(), Wx.size() * sizeof(float), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(p->WxT, WxT.data(), WxT.size() * sizeof(float), hipMemcpyHostToDevice));
    return SMI_OK;
}

static void pool_free_work(LowResPool *p) {
    for (void *q : {(void *)p->table, (void *)p->model, (void *)p->out, (void *)p->resid,
                    (void *)p->gpad, (void *)p->Mh, (void *)p->Gbar, (void *)p->scratch})
        if (q) (void)hipFree(q);
    p->table = nullptr; p->model = p->out = p->resid = p->gpad = nullptr;
    p->Mh = p->Gbar = nullptr; p->scratch = nullptr;
    p->cap = 0;
}

void lowres_pool_destroy(LowResPool *p) {
    if (!p) return;
    pool_free_work(p);
    for (auto &o : p->owned)
        for (void *q : {(void *)o.E, (void *)o.beta, (void *)o.data, (void *)o.weights,
                        (void *)o.channels})
            if (q) (void)hipFree(q);
    for (void *q : {(void *)p->tw, (void *)p->Wx, (void *)p->WxT})
        if (q) (void)hipFree(q);
    delete p;
}

bool lowres_pool_matches(const LowResPool *p, int C, int n_a, int n_b, int Fy, int Fx) {
    return p->C == C && p->n_a == n_a && p->n_b == n_b && p->Fy == Fy && p->Fx == Fx;
}

int lowres_pool_size(const LowResPool *p) { return (int)p->members.size(); }

int lowres_pool_add(LowResPool *p, const float *A, const float *Pt, const Resampler *from,
                    const int32_t *channels, const float *data, const float *weights,
                    double log_norm, int blend, double *term_slot) {
    const int C = p->C, n_a = p->n_a, n_b = p->n_b, Fy = p->Fy, Fx = p->Fx, Kx = p->Kx;
    SMI_REQUIRE((A && Pt) || from, "no operators");
    SMI_REQUIRE(p->members.size() < 65535, "too many observations of one class");
    const size_t nE = (size_t)C * n_a * Fy * Kx, nB = (size_t)n_b * Kx;
    const size_t n = (size_t)C * n_a * n_b;
    p->owned.emplace_back();
    LowResPool::Owned &o = p->owned.back();
    float *d_A = nullptr, *d_S = nullptr;
    auto run = [&]() -> int {
        SMI_HIP(hipMalloc((void **)&o.E, nE * sizeof(float2)));
        SMI_HIP(hipMalloc((void **)&o.beta, nB * sizeof(float2)));
        if (A) {
            SMI_REQUIRE(circulant_along_x(Pt, Fx, n_b),
                        "the shift operator is not circulant: a low-resolution observation on "
                        "the dense path is fitted in a batch of its own");
            std::vector<float> S((size_t)n_b * Fx);
            for (int b = 0; b < n_b; ++b)  // s_b[x] = P[x' = 0][x][b]
                for (int x = 0; x < Fx; ++x) S[(size_t)b * Fx + x] = Pt[(size_t)x * n_b + b];
            const size_t nA = (size_t)C * n_a * Fy * Fx;
            SMI_HIP(hipMalloc((void **)&d_A, nA * sizeof(float)));
            SMI_HIP(hipMalloc((void **)&d_S, S.size() * sizeof(float)));
            SMI_HIP(hipMemcpy(d_A, A, nA * sizeof(float), hipMemcpyHostToDevice));
            SMI_HIP(hipMemcpy(d_S, S.data(), S.size() * sizeof(float), hipMemcpyHostToDevice));
            const size_t lds = (size_t)((Fx + 1) & ~1) * sizeof(double) + (size_t)Fx * sizeof(double2);
            hipLaunchKernelGGL(row_dft_kernel, dim3((unsigned)((size_t)C * n_a * Fy)), dim3(256),
                               lds, nullptr, d_A, p->tw, o.E, Fx, Kx, 0);
            hipLaunchKernelGGL(row_dft_kernel, dim3(n_b), dim3(256), lds, nullptr, d_S, p->tw,
                               o.beta, Fx, Kx, 1);
            SMI_HIP(hipGetLastError());
            SMI_HIP(hipDeviceSynchronize());
        } else {
            SMI_REQUIRE(from->spectral && lowres_pool_matches(p, from->C, from->n_a, from->n_b,
                                                              from->Fy, from->Fx),
                        "the resampler has no spectral tables of this class");
            SMI_HIP(hipMemcpy(o.E, from->E, nE * sizeof(float2), hipMemcpyDefault));
            SMI_HIP(hipMemcpy(o.beta, from->beta, nB * sizeof(float2), hipMemcpyDefault));
        }
        if (data) {
            SMI_HIP(hipMalloc((void **)&o.channels, C * sizeof(int32_t)));
            SMI_HIP(hipMalloc((void **)&o.data, n * sizeof(float)));
            SMI_HIP(hipMalloc((void **)&o.weights, n * sizeof(float)));
            SMI_HIP(hipMemcpy(o.channels, channels, C * sizeof(int32_t), hipMemcpyHostToDevice));
            SMI_HIP(hipMemcpy(o.data, data, n * sizeof(float), hipMemcpyHostToDevice));
            SMI_HIP(hipMemcpy(o.weights, weights, n * sizeof(float), hipMemcpyHostToDevice));
        }
        if (term_slot) SMI_HIP(hipMemset(term_slot, 0, sizeof(double)));
        return SMI_OK;
    };
    const int rc = run();
    if (d_A) (void)hipFree(d_A);
    if (d_S) (void)hipFree(d_S);
    if (rc) {
        for (void *q : {(void *)o.E, (void *)o.beta, (void *)o.data, (void *)o.weights,
                        (void *)o.channels})
            if (q) (void)hipFree(q);
        p->owned.pop_back();
        return rc;
    }
    LowResMember m;
    m.E = o.E; m.beta = o.beta; m.data = o.data; m.weights = o.weights; m.channels = o.channels;
    m.term = term_slot; m.log_norm = log_norm; m.blend = blend; m.unused = 0;
    p->members.push_back(m);
    p->dirty = true;
    return SMI_OK;
}

// the table and the pooled work arrays for the members there are now
static int lowres_pool_ready(LowResPool *p) {
    if (!p->dirty) return SMI_OK;
    const int n = (int)p->members.size();
    SMI_REQUIRE(n > 0, "an empty pool of low-resolution observations");
    if (n > p->cap) {
        pool_free_work(p);
        const size_t plane = (size_t)p->Fy * p->Fx, nc = (size_t)n * p->C;
        const size_t n_out = nc * p->n_a * p->n_b, n_pad = nc * plane;
        SMI_HIP(hipMalloc((void **)&p->table, n * sizeof(LowResMember)));
        SMI_HIP(hipMalloc((void **)&p->model, n_pad * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&p->out, (n_out + 2 * kPoolGuard) * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&p->resid, n_out * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&p->gpad, (n_pad + 2 * kPoolGuard) * sizeof(float)));
        SMI_HIP(hipMalloc((void **)&p->Mh, nc * p->Fy * p->Kx * sizeof(float2)));
        SMI_HIP(hipMalloc((void **)&p->Gbar, nc * p->n_a * p->Kx * sizeof(float2)));
        // (0xa5 bytes: the guard pattern; the work arrays themselves are written before read)
        SMI_HIP(hipMemset(p->out, 0xa5, (n_out + 2 * kPoolGuard) * sizeof(float)));
        SMI_HIP(hipMemset(p->gpad, 0xa5, (n_pad + 2 * kPoolGuard) * sizeof(float)));
        SMI_HIP(hipMemset(p->model, 0, n_pad * sizeof(float)));
        SMI_HIP(hipMemset(p->resid, 0, n_out * sizeof(float)));
        const int nsl = std::max(p->nsl_f, p->nsl_b);
        if (nsl > 1) {
            const size_t in_launch = std::min<size_t>(nc, (size_t)gemm_pooled_chunk(nsl));
            const size_t MN = (size_t)p->Fy * std::max(p->Fx, 2 * p->Kx);
            SMI_HIP(hipMalloc((void **)&p->scratch, (size_t)nsl * in_launch * MN * sizeof(double)));
        }
        p->cap = n;
    }
    SMI_HIP(hipMemcpy(p->table, p->members.data(), n * sizeof(LowResMember),
                      hipMemcpyHostToDevice));
    p->dirty = false;
    return SMI_OK;
}

// p->model (padded, all members) -> p->out + kPoolGuard
static int lowres_pool_forward(LowResPool *p, const int32_t *state, hipStream_t s) {
    const int n = (int)p->members.size(), Kx = p->Kx;
    const int64_t plane = (int64_t)p->Fy * p->Fx;
    int rc = gemm_pooled(p->kslice_f, p->nsl_f, p->model, plane, p->Wx,
                         reinterpret_cast<float *>(p->Mh), (int64_t)p->Fy * 2 * Kx, n * p->C,
                         p->scratch, p->Fy, 2 * Kx, p->Fx, s);
    if (rc) return rc;
    const size_t lds = (size_t)(16 * 64 + Kx) * sizeof(double2);
    hipLaunchKernelGGL(spectral_forward_kernel, dim3(p->n_a, p->C, n), dim3(1024), lds, s, nullptr,
                       p->Mh, nullptr, p->out + kPoolGuard, p->n_a, p->n_b, p->Fy, Kx, p->table,
                       state);
    return SMI_OK;
}

// p->resid -> p->gpad + kPoolGuard
static int lowres_pool_adjoint(LowResPool *p, const int32_t *state, hipStream_t s) {
    const int n = (int)p->members.size(), Kx = p->Kx;
    hipLaunchKernelGGL(spectral_gbar_kernel, dim3(p->C * p->n_a, n), dim3(256),
                       p->n_b * sizeof(float), s, p->resid, nullptr, p->Gbar, p->n_b, Kx, p->table,
                       state);
    hipLaunchKernelGGL(spectral_adjoint_kernel, dim3(p->Fy, p->C, n), dim3(256), 0, s, nullptr,
                       p->Gbar, p->Mh, p->n_a, p->Fy, Kx, p->table, state);
    return gemm_pooled(p->kslice_b, p->nsl_b, reinterpret_cast<float *>(p->Mh),
                       (int64_t)p->Fy * 2 * Kx, p->WxT, p->gpad + kPoolGuard,
                       (int64_t)p->Fy * p->Fx, n * p->C, p->scratch, p->Fy, p->Fx, 2 * Kx, s);
}

int lowres_pool_evaluate(LowResPool *p, const float *P, int Py, int Px, int Cm,
                         const int32_t *state, int backward, hipStream_t s) {
    int rc = lowres_pool_ready(p);
    if (rc) return rc;
    const int n = (int)p->members.size(), plane = p->Fy * p->Fx;
    hipLaunchKernelGGL(lowres_pad_kernel, dim3((plane + 255) / 256, p->C, n), dim3(256), 0, s, P,
                       Py, Px, nullptr, p->H, p->W, p->y0, p->x0, p->model, p->Fy, p->Fx, p->table,
                       state, Cm);
    if ((rc = lowres_pool_forward(p, state, s))) return rc;
    hipLaunchKernelGGL(lowres_residual_kernel, dim3(n), dim3(1024), 0, s, p->out + kPoolGuard,
                       nullptr, nullptr, p->resid, p->C * p->n_a * p->n_b, 0.0, nullptr, p->table,
                       state);
    if (!backward) return SMI_OK;
    return lowres_pool_adjoint(p, state, s);
}

int lowres_pool_add_gradient(LowResPool *p, float *Q, int Py, int Px, int Cm,
                             const int32_t *state, hipStream_t s) {
    const int rc = lowres_pool_ready(p);
    if (rc) return rc;
    const int n = (int)p->members.size();
    hipLaunchKernelGGL(lowres_add_kernel, dim3((p->H * p->W + 255) / 256, p->C, n), dim3(256), 0,
                       s, p->gpad + kPoolGuard, p->Fy, p->Fx, p->y0, p->x0, nullptr, p->H, p->W, Q,
                       Py, Px, p->table, state, Cm);
    return SMI_OK;
}

int lowres_pool_get_rendered(LowResPool *p, int member, float *out, hipStream_t s) {
    SMI_REQUIRE(member >= 0 && member < (int)p->members.size() && !p->dirty && p->out,
                "no rendering of this observation yet");
    const size_t n = (size_t)p->C * p->n_a * p->n_b;
    SMI_HIP(hipMemcpyAsync(out, p->out + kPoolGuard + member * n, n * sizeof(float),
                           hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    return SMI_OK;
}

int lowres_pool_test(int n, const float *A, const float *Pt, int C, int n_a, int n_b, int Fy,
                     int Fx, const float *models, const float *resid, float *out, float *gpad,
                     int32_t *guard_ok) {
    LowResPool *p = nullptr;
    int32_t *state = nullptr;
    auto run = [&]() -> int {
        int rc = lowres_pool_create(C, n_a, n_b, Fy, Fx, Fy, Fx, &p);
        if (rc) return rc;
        const size_t nA = (size_t)C * n_a * Fy * Fx, nP = (size_t)Fx * Fx * n_b;
        for (int m = 0; m < n; ++m)
            if ((rc = lowres_pool_add(p, A + m * nA, Pt + m * nP, nullptr, nullptr, nullptr,
                                      nullptr, 0.0, m, nullptr)))
                return rc;
        if ((rc = lowres_pool_ready(p))) return rc;
        const size_t n_pad = (size_t)n * C * Fy * Fx, n_out = (size_t)n * C * n_a * n_b;
        SMI_HIP(hipMalloc((void **)&state, n * sizeof(int32_t)));
        SMI_HIP(hipMemset(state, 0, n * sizeof(int32_t)));
        SMI_HIP(hipMemcpy(p->model, models, n_pad * sizeof(float), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(p->resid, resid, n_out * sizeof(float), hipMemcpyHostToDevice));
        if ((rc = lowres_pool_forward(p, state, nullptr))) return rc;
        if ((rc = lowres_pool_adjoint(p, state, nullptr))) return rc;
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipDeviceSynchronize());
        std::vector<float> h_out(n_out + 2 * kPoolGuard), h_g(n_pad + 2 * kPoolGuard);
        SMI_HIP(hipMemcpy(h_out.data(), p->out, h_out.size() * sizeof(float), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(h_g.data(), p->gpad, h_g.size() * sizeof(float), hipMemcpyDeviceToHost));
        const uint32_t gbits = 0xa5a5a5a5u;
        bool ok = true;
        for (size_t i = 0; i < kPoolGuard; ++i) {
            ok = ok && memcmp(&h_out[i], &gbits, 4) == 0 &&
                 memcmp(&h_out[kPoolGuard + n_out + i], &gbits, 4) == 0;
            ok = ok && memcmp(&h_g[i], &gbits, 4) == 0 &&
                 memcmp(&h_g[kPoolGuard + n_pad + i], &gbits, 4) == 0;
        }
        *guard_ok = ok ? 1 : 0;
        memcpy(out, h_out.data() + kPoolGuard, n_out * sizeof(float));
        memcpy(gpad, h_g.data() + kPoolGuard, n_pad * sizeof(float));
        return SMI_OK;
    };
    const int rc = run();
    if (state) (void)hipFree(state);
    lowres_pool_destroy(p);
    return rc;
}

}  // namespace smi
