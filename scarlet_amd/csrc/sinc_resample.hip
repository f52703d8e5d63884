// The two products of interpolation.interpolate_observation (reference
// scarlet/interpolation.py:427-463, 563-599) for a ragged catalogue: for every band X (Ho, Wo)
//   out = Sy . X . Sx^T      Sy (Hf, Ho), Sx (Wf, Wo) float64, out (Hf, Wf) float64
// in two stages, tmp = Sy . X and out = tmp . Sx^T, one launch each whatever the number of
// bands and blends.  The sinc matrices come from the host (NumPy's sinc, so that they are the
// reference's to the last digit); X is float32 or float64 and widened to float64 when it is
// read, as np.dot does.
//
// One task per band and blend (validated on the host before anything is launched), grid.y =
// task, grid.x = the kTile x kTile output tiles of the largest task; a workgroup beyond its
// task's tiles leaves at once.  A workgroup walks the inner dimension in steps of kTile: the
// tiles of the two factors go into LDS, zeros beyond the edges, and every thread owns one
// output element.
//
// The summation order is fixed: one accumulator per output element, starting from +0, the
// terms in ascending inner index, each step ONE fused multiply-add, acc = fma(a, b, acc) --
// written out as fma(), so the contraction setting of the build does not matter.  An output's
// bits therefore depend on its row of the left factor and its column of the right one alone:
// not on the list, the chunk, the grid or the tile it falls into.
//
// Nothing is allocated, copied to the host or waited for.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace smi {
namespace {

constexpr int kTile = SMI_SINC_TILE;
constexpr int kT = kTile * kTile;

// C (M, N) = A (M, K) . B with B (K, N) row-major, or, TRANS, B^T of the row-major (N, K)
template <typename TB, bool TRANS>
__device__ __forceinline__ void tile_product(const double *A, const TB *B, double *C, int M, int N,
                                             int K) {
    __shared__ double sa[kTile][kTile + 1], sb[kTile][kTile + 1];
    const int tiles_n = (N + kTile - 1) / kTile, tiles_m = (M + kTile - 1) / kTile;
    if ((int)blockIdx.x >= tiles_m * tiles_n) return;
    const int m0 = ((int)blockIdx.x / tiles_n) * kTile, n0 = ((int)blockIdx.x % tiles_n) * kTile;
    const int ty = threadIdx.x / kTile, tx = threadIdx.x % kTile;
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += kTile) {
        const int steps = K - k0 < kTile ? K - k0 : kTile;
        sa[ty][tx] = (m0 + ty < M && tx < steps) ? A[(int64_t)(m0 + ty) * K + k0 + tx] : 0.0;
        if (TRANS)  // rows of B are columns of the product: read along k, store transposed
            sb[tx][ty] = (n0 + ty < N && tx < steps) ? (double)B[(int64_t)(n0 + ty) * K + k0 + tx]
                                                     : 0.0;
        else
            sb[ty][tx] = (ty < steps && n0 + tx < N) ? (double)B[(int64_t)(k0 + ty) * N + n0 + tx]
                                                     : 0.0;
        __syncthreads();
        for (int k = 0; k < steps; ++k) acc = fma(sa[ty][k], sb[k][tx], acc);
        __syncthreads();
    }
    if (m0 + ty < M && n0 + tx < N) C[(int64_t)(m0 + ty) * N + n0 + tx] = acc;
}

// tmp = Sy . X
template <typename T>
__global__ __launch_bounds__(kT) void sinc_rows_kernel(const smi_sinc_task *tasks, const T *x,
                                                       const double *mats, double *tmp) {
    const smi_sinc_task t = tasks[blockIdx.y];
    tile_product<T, false>(mats + t.sy_off, x + t.x_off, tmp + t.tmp_off, t.hf, t.wo, t.ho);
}

// out = tmp . Sx^T
__global__ __launch_bounds__(kT) void sinc_cols_kernel(const smi_sinc_task *tasks,
                                                       const double *mats, const double *tmp,
                                                       double *out) {
    const smi_sinc_task t = tasks[blockIdx.y];
    tile_product<double, true>(tmp + t.tmp_off, mats + t.sx_off, out + t.out_off, t.hf, t.wf,
                               t.wo);
}

int64_t tiles(int64_t m, int64_t n) {
    return ((m + kTile - 1) / kTile) * ((n + kTile - 1) / kTile);
}

template <typename T>
int sinc_resample(int32_t n, const smi_sinc_task *tasks, const void *d_tasks, const T *d_x,
                  int64_t n_x, const double *d_mats, int64_t n_mats, double *d_tmp, int64_t n_tmp,
                  double *d_out, int64_t n_out, void *stream) {
    SMI_REQUIRE(n >= 0 && n <= 65535, "task count");
    SMI_REQUIRE((tasks && d_tasks) || n == 0, "null descriptor table");
    SMI_REQUIRE(n_x >= 0 && n_mats >= 0 && n_tmp >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE((d_x || !n_x) && (d_mats || !n_mats) && (d_tmp || !n_tmp) && (d_out || !n_out),
                "null buffer");
    int64_t rows_tiles = 0, cols_tiles = 0, tmp_end = 0, out_end = 0;
    for (int32_t i = 0; i < n; ++i) {
        const smi_sinc_task &t = tasks[i];
        SMI_REQUIRE(t.ho > 0 && t.wo > 0 && t.hf > 0 && t.wf > 0, "extent");
        SMI_REQUIRE(in_buffer(t.x_off, (int64_t)t.ho * t.wo, n_x), "band outside its buffer");
        SMI_REQUIRE(in_buffer(t.sy_off, (int64_t)t.hf * t.ho, n_mats) &&
                        in_buffer(t.sx_off, (int64_t)t.wf * t.wo, n_mats),
                    "matrix outside its buffer");
        SMI_REQUIRE(t.tmp_off >= tmp_end && in_buffer(t.tmp_off, (int64_t)t.hf * t.wo, n_tmp),
                    "intermediate outside its buffer or shared with another task");
        tmp_end = t.tmp_off + (int64_t)t.hf * t.wo;
        SMI_REQUIRE(t.out_off >= out_end && in_buffer(t.out_off, (int64_t)t.hf * t.wf, n_out),
                    "result outside its buffer or shared with another task");
        out_end = t.out_off + (int64_t)t.hf * t.wf;
        rows_tiles = std::max(rows_tiles, tiles(t.hf, t.wo));
        cols_tiles = std::max(cols_tiles, tiles(t.hf, t.wf));
    }
    SMI_REQUIRE(rows_tiles <= INT32_MAX && cols_tiles <= INT32_MAX, "too many tiles");
    if (n == 0) return SMI_OK;
    int rc = have_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const smi_sinc_task *dt = (const smi_sinc_task *)d_tasks;
    hipLaunchKernelGGL((sinc_rows_kernel<T>), dim3((unsigned)rows_tiles, n), dim3(kT), 0, st, dt,
                       d_x, d_mats, d_tmp);
    hipLaunchKernelGGL(sinc_cols_kernel, dim3((unsigned)cols_tiles, n), dim3(kT), 0, st, dt, d_mats,
                       d_tmp, d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_sinc_resample_f32(int32_t n, const smi_sinc_task *tasks, const void *d_tasks,
                          const float *d_x, int64_t n_x, const double *d_mats, int64_t n_mats,
                          double *d_tmp, int64_t n_tmp, double *d_out, int64_t n_out,
                          void *stream) {
    return smi::sinc_resample<float>(n, tasks, d_tasks, d_x, n_x, d_mats, n_mats, d_tmp, n_tmp,
                                     d_out, n_out, stream);
}
int smi_sinc_resample_f64(int32_t n, const smi_sinc_task *tasks, const void *d_tasks,
                          const double *d_x, int64_t n_x, const double *d_mats, int64_t n_mats,
                          double *d_tmp, int64_t n_tmp, double *d_out, int64_t n_out,
                          void *stream) {
    return smi::sinc_resample<double>(n, tasks, d_tasks, d_x, n_x, d_mats, n_mats, d_tmp, n_tmp,
                                      d_out, n_out, stream);
}

}  // extern "C"
