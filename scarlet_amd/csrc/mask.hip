// Seam 1, monotonic mask operators of the reference's native extension
// (scarlet/operators_pybind11.cc:58-232), used by operator.prox_monotonic_mask
// (operator.py:131-176), MonotonicityConstraint(use_mask=True) and the lite
// initialisation with use_mask=True.
//
// get_valid_monotonic_pixels is a recursive 4-neighbour flood fill: a pixel is accepted
// from an accepted neighbour c if image(p) < image(c) + variance and image(p) > thresh
// (thresh only for the neighbours of the start pixel; the recursion drops it to 0).
// A failed test leaves the pixel unchecked, so it can still be accepted from another
// side: the accepted set is the set reachable from the start along such steps and does
// not depend on the visiting order.  Likewise the final `orphans` (unaccepted pixels next
// to an accepted one) and `bounds` (bounding box of the accepted pixels).  The kernel
// therefore relaxes the whole image in parallel until nothing changes -- bit-identical
// maps to the depth-first recursion.
//
// linear_interpolate_invalid_pixels walks its pixel list in order and every step sees
// the model / maps left by the previous ones (and starts a flood fill when it fills a
// pixel), so the list is processed sequentially by one lane while the workgroup joins
// in for the fills.  All of the reference's quirks are kept: the comma-operator
// conditions of the column branches, `i > 2` / `i < rows - 2`, the `else if` bound
// updates; the unguarded i+-1 / j+-1 accesses of the non-recursive branch are guarded.
#include "common.h"
#include "mask_device.h"

namespace smi {
namespace {

constexpr int kT = kMaskT;

template <typename T>
__global__ __launch_bounds__(kT) void valid_pixels_kernel(int i, int j, const T *image, int rows,
                                                          int cols, uint8_t *unchecked,
                                                          uint8_t *orphans, int32_t *visited,
                                                          double variance, int32_t *bounds,
                                                          double thresh) {
    __shared__ FillShared sh;
    flood_fill<T>(i * cols + j, image, rows, cols, unchecked, orphans, visited, 1, variance, thresh,
                  bounds, &sh);
}

template <typename T>
__global__ __launch_bounds__(kT) void interpolate_kernel(const int32_t *row_idx,
                                                         const int32_t *col_idx, int n_idx,
                                                         uint8_t *unchecked, T *model, int rows,
                                                         int cols, uint8_t *orphans,
                                                         int32_t *visited, double variance,
                                                         int recursive, int32_t *bounds) {
    __shared__ FillShared sh;
    __shared__ int fill;
    int gen = 0;
    for (int n = 0; n < n_idx; ++n) {
        const int i = row_idx[n], j = col_idx[n];
        if (threadIdx.x == 0) {
            fill = interpolate_pixel<T>(i, j, unchecked, model, rows, cols, orphans, recursive,
                                        bounds);
            __threadfence_block();
        }
        __syncthreads();
        const int do_fill = fill;
        __syncthreads();
        if (do_fill)
            flood_fill<T>(i * cols + j, model, rows, cols, unchecked, orphans, visited, ++gen,
                          variance, 0.0, bounds, &sh);
    }
}

}  // namespace

template <typename T>
int mask_valid_host_buffers(int32_t i, int32_t j, const T *image, int32_t rows, int32_t cols,
                            uint8_t *unchecked, uint8_t *orphans, double variance,
                            int32_t *bounds, double thresh) {
    const size_t N = (size_t)rows * cols;
    DevBuf<T> d_img;
    DevBuf<uint8_t> d_un, d_or;
    DevBuf<int32_t> d_vis, d_b;
    SMI_HIP(d_img.alloc(N));
    SMI_HIP(d_un.alloc(N));
    SMI_HIP(d_or.alloc(N));
    SMI_HIP(d_vis.alloc(N));
    SMI_HIP(d_b.alloc(4));
    SMI_HIP(hipMemcpy(d_img.p, image, N * sizeof(T), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(d_un.p, unchecked, N, hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(d_or.p, orphans, N, hipMemcpyHostToDevice));
    SMI_HIP(hipMemset(d_vis.p, 0, N * sizeof(int32_t)));
    SMI_HIP(hipMemcpy(d_b.p, bounds, 4 * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(valid_pixels_kernel<T>, dim3(1), dim3(kT), 0, 0, i, j, d_img.p, rows, cols,
                       d_un.p, d_or.p, d_vis.p, variance, d_b.p, thresh);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipDeviceSynchronize());
    SMI_HIP(hipMemcpy(unchecked, d_un.p, N, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(orphans, d_or.p, N, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(bounds, d_b.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SMI_OK;
}

template <typename T>
int mask_interpolate_host_buffers(const int32_t *row_idx, const int32_t *col_idx, int32_t n_idx,
                                  uint8_t *unchecked, T *model, int32_t rows, int32_t cols,
                                  uint8_t *orphans, double variance, int32_t recursive,
                                  int32_t *bounds) {
    const size_t N = (size_t)rows * cols;
    DevBuf<T> d_model;
    DevBuf<uint8_t> d_un, d_or;
    DevBuf<int32_t> d_vis, d_b, d_r, d_c;
    SMI_HIP(d_model.alloc(N));
    SMI_HIP(d_un.alloc(N));
    SMI_HIP(d_or.alloc(N));
    SMI_HIP(d_vis.alloc(N));
    SMI_HIP(d_b.alloc(4));
    SMI_HIP(d_r.alloc(n_idx));
    SMI_HIP(d_c.alloc(n_idx));
    SMI_HIP(hipMemcpy(d_model.p, model, N * sizeof(T), hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(d_un.p, unchecked, N, hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(d_or.p, orphans, N, hipMemcpyHostToDevice));
    SMI_HIP(hipMemset(d_vis.p, 0, N * sizeof(int32_t)));
    SMI_HIP(hipMemcpy(d_b.p, bounds, 4 * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_idx) {
        SMI_HIP(hipMemcpy(d_r.p, row_idx, n_idx * sizeof(int32_t), hipMemcpyHostToDevice));
        SMI_HIP(hipMemcpy(d_c.p, col_idx, n_idx * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(interpolate_kernel<T>, dim3(1), dim3(kT), 0, 0, d_r.p, d_c.p, n_idx, d_un.p,
                       d_model.p, rows, cols, d_or.p, d_vis.p, variance, recursive, d_b.p);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipDeviceSynchronize());
    SMI_HIP(hipMemcpy(model, d_model.p, N * sizeof(T), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(unchecked, d_un.p, N, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(orphans, d_or.p, N, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(bounds, d_b.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SMI_OK;
}

template int mask_valid_host_buffers<float>(int32_t, int32_t, const float *, int32_t, int32_t,
                                            uint8_t *, uint8_t *, double, int32_t *, double);
template int mask_valid_host_buffers<double>(int32_t, int32_t, const double *, int32_t, int32_t,
                                             uint8_t *, uint8_t *, double, int32_t *, double);
template int mask_interpolate_host_buffers<float>(const int32_t *, const int32_t *, int32_t,
                                                  uint8_t *, float *, int32_t, int32_t, uint8_t *,
                                                  double, int32_t, int32_t *);
template int mask_interpolate_host_buffers<double>(const int32_t *, const int32_t *, int32_t,
                                                   uint8_t *, double *, int32_t, int32_t,
                                                   uint8_t *, double, int32_t, int32_t *);

}  // namespace smi
