// Device code of the monotonic mask operators (operators_pybind11.cc:58-232, operator.py:131-176)
// shared by the seam-1 kernels of mask.hip and by the starlet step kernel of starlet_source.hip,
// which runs prox_monotonic_mask on the coefficient planes of StarletMorphology(monotonic=True)
// inside its proximal sub-iterations.  Everything here is called by a whole workgroup of kMaskT
// threads; see mask.hip for why the parallel flood fill gives the maps of the depth-first recursion.
#pragma once
#include "common.h"

namespace smi {
namespace {

constexpr int kMaskT = 1024;

struct FillShared {
    int changed;
    int rmin, rmax, cmin, cmax;
};

template <typename T>
__device__ void flood_fill(int start, const T *image, int rows, int cols, uint8_t *unchecked,
                           uint8_t *orphans, int32_t *visited, int gen, double variance,
                           double thresh, int32_t *bounds, FillShared *sh) {
    const int tid = threadIdx.x, N = rows * cols;
    if (tid == 0) {
        visited[start] = gen;
        sh->rmin = bounds[0];
        sh->rmax = bounds[1];
        sh->cmin = bounds[2];
        sh->cmax = bounds[3];
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) sh->changed = 0;
        __syncthreads();
        for (int p = tid; p < N; p += kMaskT) {
            if (!unchecked[p] || visited[p] == gen) continue;
            const int r = p / cols, c = p - r * cols;
            const double val = (double)image[p];
            bool accept = false;
            const int nb[4] = {r > 0 ? p - cols : -1, r < rows - 1 ? p + cols : -1,
                               c > 0 ? p - 1 : -1, c < cols - 1 ? p + 1 : -1};
            for (int k = 0; k < 4; ++k) {
                const int q = nb[k];
                if (q < 0 || visited[q] != gen) continue;
                const double th = q == start ? thresh : 0.0;
                if (val < (double)image[q] + variance && val > th) accept = true;
            }
            if (accept) {
                visited[p] = gen;
                unchecked[p] = 0;
                sh->changed = 1;
            }
        }
        __syncthreads();
        const int again = sh->changed;
        __syncthreads();
        if (!again) break;
    }
    for (int p = tid; p < N; p += kMaskT) {
        const int r = p / cols, c = p - r * cols;
        if (visited[p] == gen) {
            if (p != start) {
                orphans[p] = 0;
                atomicMin(&sh->rmin, r);
                atomicMax(&sh->rmax, r);
                atomicMin(&sh->cmin, c);
                atomicMax(&sh->cmax, c);
            }
        } else if (unchecked[p]) {
            const bool touched = (r > 0 && visited[p - cols] == gen) ||
                                 (r < rows - 1 && visited[p + cols] == gen) ||
                                 (c > 0 && visited[p - 1] == gen) ||
                                 (c < cols - 1 && visited[p + 1] == gen);
            if (touched) orphans[p] = 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bounds[0] = sh->rmin;
        bounds[1] = sh->rmax;
        bounds[2] = sh->cmin;
        bounds[3] = sh->cmax;
    }
    __syncthreads();
}

// One entry (i, j) of linear_interpolate_invalid_pixels' list, by ONE lane.  True if the pixel
// was filled in the recursive mode: the workgroup then owes a flood_fill from it with thresh 0.
template <typename T>
__device__ bool interpolate_pixel(int i, int j, uint8_t *unchecked, T *model, int rows, int cols,
                                  uint8_t *orphans, int recursive, int32_t *bounds) {
#define AT(a, b) ((a) * cols + (b))
    if (!unchecked[AT(i, j)]) return false;
    bool fill = false;
    T total = 0;
    int valid = 0, pending = 0;
    unchecked[AT(i, j)] = 0;
    if (i < rows - 2 && model[AT(i + 2, j)] > model[AT(i + 1, j)]) {
        if (unchecked[AT(i + 2, j)] || unchecked[AT(i + 1, j)]) {
            pending = 1;
        } else {
            const T grad = model[AT(i + 2, j)] - model[AT(i + 1, j)];
            total += model[AT(i + 1, j)] - grad;
            valid += 1;
        }
    }
    if (i > 2 && model[AT(i - 2, j)] > model[AT(i - 1, j)]) {
        if (unchecked[AT(i - 2, j)] || unchecked[AT(i - 1, j)]) {
            pending = 1;
        } else {
            const T grad = model[AT(i - 2, j)] - model[AT(i - 1, j)];
            total += model[AT(i - 1, j)] - grad;
            valid += 1;
        }
    }
    if (j < cols - 2 && model[AT(i, j + 2)] > model[AT(i, j + 1)]) {
        if (unchecked[AT(i, j + 1)]) {  // `unchecked(i,j+2), unchecked(i,j+1)`
            pending = 1;
        } else {
            const T grad = model[AT(i, j + 2)] - model[AT(i, j + 1)];
            total += model[AT(i, j + 1)] - grad;
            valid += 1;
        }
    }
    if (j > 2 && model[AT(i, j - 2)] > model[AT(i, j - 1)]) {
        if (unchecked[AT(i, j - 1)]) {
            pending = 1;
        } else {
            const T grad = model[AT(i, j - 2)] - model[AT(i, j - 1)];
            total += model[AT(i, j - 1)] - grad;
            valid += 1;
        }
    }
    if (total > 0) {
        model[AT(i, j)] = total / valid;
        orphans[AT(i, j)] = 0;
        if (i < bounds[0]) bounds[0] = i;
        else if (i > bounds[1]) bounds[1] = i;
        if (j < bounds[2]) bounds[2] = j;
        else if (j > bounds[3]) bounds[3] = j;
        if (recursive) {
            fill = true;
        } else {
            if (i > 0 && unchecked[AT(i - 1, j)]) orphans[AT(i - 1, j)] = 1;
            if (i < rows - 1 && unchecked[AT(i + 1, j)]) orphans[AT(i + 1, j)] = 1;
            if (j > 0 && unchecked[AT(i, j - 1)]) orphans[AT(i, j - 1)] = 1;
            if (j < cols - 1 && unchecked[AT(i, j + 1)]) orphans[AT(i, j + 1)] = 1;
        }
    } else if (!pending) {
        orphans[AT(i, j)] = 1;
        model[AT(i, j)] = 0;
    }
#undef AT
    return fill;
}

// prox_monotonic_mask (operator.py:131-176) on one plane, in place, by the whole workgroup.
//
// State: `visited` (N int32) and `flags` (3 N bytes: the snapshot of the orphans that is the
// list of a pass, `unchecked`, `orphans`); `sh` holds the fill's shared words, the bounds and
// the hand-over between the lane that walks the list and the workgroup that fills.  Nothing
// has to be initialised by the caller, who must have made `plane` visible (a barrier) before
// the call; the function ends with a barrier.
struct MaskShared {
    FillShared fill;
    int32_t bounds[4];
    int start;    // centre pixel
    int next;     // where the list walk goes on
    int fill_at;  // pixel the workgroup fills from, -1: the pass is over
};

__device__ void monotonic_mask_plane(float *plane, int rows, int cols, int cy, int cx, int radius,
                                     double variance, int max_iter, int32_t *visited,
                                     uint8_t *flags, MaskShared *sh) {
    const int tid = threadIdx.x, N = rows * cols;
    uint8_t *snapshot = flags, *unchecked = flags + N, *orphans = flags + 2 * (size_t)N;
    // get_center (operator.py:132-147): the first maximum, in row-major order, of the window
    // clipped to the plane; radius 0 takes the centre as it is
    if (tid == 0) {
        int bi = cy, bj = cx;
        if (radius > 0) {
            const int y0 = max(cy - radius, 0), x0 = max(cx - radius, 0);
            const int y1 = min(cy + radius, rows - 1), x1 = min(cx + radius, cols - 1);
            bi = y0;
            bj = x0;
            float best = plane[y0 * cols + x0];
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) {
                    const float val = plane[y * cols + x];
                    if (val > best) {
                        best = val;
                        bi = y;
                        bj = x;
                    }
                }
        }
        sh->start = bi * cols + bj;
        sh->bounds[0] = sh->bounds[1] = bi;
        sh->bounds[2] = sh->bounds[3] = bj;
    }
    __syncthreads();
    const int start = sh->start;
    for (int p = tid; p < N; p += kMaskT) {
        visited[p] = 0;
        unchecked[p] = p != start;
        orphans[p] = 0;
    }
    __syncthreads();
    int gen = 1;
    flood_fill<float>(start, plane, rows, cols, unchecked, orphans, visited, gen, variance, 0.0,
                      sh->bounds, &sh->fill);
    for (int pass = 0; pass < max_iter; ++pass) {
        int waiting = 0;
        for (int p = tid; p < N; p += kMaskT) {
            const uint8_t o = orphans[p];
            snapshot[p] = o;
            waiting |= o & unchecked[p];
        }
        if (tid == 0) sh->next = 0;
        if (!__syncthreads_or(waiting)) break;
        // the list of this pass is the snapshot in row-major order (np.where(orphans)); one
        // lane walks it up to the next pixel it fills, the workgroup floods from there
        for (;;) {
            if (tid == 0) {
                int p = sh->next, at = -1;
                for (; p < N; ++p) {
                    if (!snapshot[p]) continue;
                    const int i = p / cols;
                    if (interpolate_pixel<float>(i, p - i * cols, unchecked, plane, rows, cols,
                                                 orphans, 1, sh->bounds)) {
                        at = p++;
                        break;
                    }
                }
                sh->next = p;
                sh->fill_at = at;
                __threadfence_block();
            }
            __syncthreads();
            const int at = sh->fill_at;
            __syncthreads();
            if (at < 0) break;
            flood_fill<float>(at, plane, rows, cols, unchecked, orphans, visited, ++gen, variance,
                              0.0, sh->bounds, &sh->fill);
        }
    }
    // model * (~unchecked & ~orphans)
    for (int p = tid; p < N; p += kMaskT)
        if (unchecked[p] | orphans[p]) plane[p] = 0.f;
    __syncthreads();
}

}  // namespace
}  // namespace smi
