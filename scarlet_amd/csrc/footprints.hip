// Footprints and peaks of device-resident detection planes: what csrc/detect.cpp computes on the
// host, for a batch of P planes [P][H][W] (float32 or float64) that never leave the device.
// Everything is integer-exact, so the results equal the host code's bit for bit.  The device
// code of the rules is footprints_device.h; footprints_batch.hip runs it for planes of
// different frames.
//
// The rules, per pixel (no patch of a footprint is ever formed):
//   label    a footprint's label is the smallest linear index y*W + x among its pixels
//            (4-connected pixels with (double)v > (double)thresh; a NaN is never in one).
//            Ascending label = the host's seed order.
//   record   inclusive bounds and area per label, by integer atomic min / max / add.
//   keep     (y1-y0+1)*(x1-x0+1) > min_area (64-bit) and area >= min_area; the rank of a kept
//            footprint is its position among the kept labels in ascending order.
//   peak     pixel p of kept footprint L is a peak iff v(p) > n(q) for each of its 8 neighbours
//            q inside L's box, n(q) = v(q) if label(q) == L, else 0 of the image's type.
//   masks    one byte per box pixel, the boxes one after another in rank order.
//
// Labelling is union-find with the root = the smallest index of the set:
//   1 tile_label     a 64 x 64 tile per workgroup in LDS (16 KiB of int32 labels: up to ten
//                    workgroups fit the 160 KiB of a CU).  A wavefront holds one tile row, so
//                    the horizontal runs come from one ballot; only vertical contacts are
//                    united, by atomicMin in LDS.  Every pixel then points at its tile's root.
//   2 merge_borders  one thread per pixel of a tile border row / column; the first pixel of
//                    every contact segment unites the two sides on the global parent array
//                    with a returning agent-scope atomic min.
//   3 flatten        label[p] = root of p; roots get their empty records.
// Each pass is one launch whatever the image holds.  No workgroup waits for another: a find
// walks towards strictly smaller indices until it meets a root, and a union retries only when
// its atomic min met a value smaller than the root it held, so max(a, b) falls at every retry.
// Parent words are read and written with agent-scope atomics in passes 2 and 3 (another XCD's
// update is not in this CU's L1); everything else is ordered by the kernel boundaries.
//   4 records        bounds and area.  A wavefront covers 64 pixels of one row, so the lanes
//                    that share a label are a bit mask: one lane per distinct label sends
//                    (y, ctz, 63 - clz, popcount) -- five atomics per label and wavefront
//                    instead of per pixel.
//   5-7 rank         keep flags, then an exclusive scan over the roots in index order of
//                    (kept, box area): per-chunk sums, one workgroup per plane over the chunk
//                    sums, per-chunk scan.  rank and mask offset land in the root's record.
//   8 count_peaks    peaks per plane (one add per wavefront).
// The fetch of a plane runs three more launches: the kept records in rank order, the mask
// bytes (one thread per byte, a binary search of the box offsets), the peak records in
// arrival order; the host then sorts the peaks by (rank, flux descending, index ascending)
// and applies the sequential min_separation filter of detect.cpp per footprint, so nothing
// depends on the arrival order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "footprints_device.h"  // the rules themselves, shared with footprints_batch.hip

namespace smi {
namespace {

struct PeakDev {
    int32_t rank, lin;
    double flux;
};

// what the fetch kernels read of the work buffer of plane `pl`
struct Work {
    int32_t *label;   // [P][N]
    int32_t *rec;     // [P][kRec][N], used at root indices
    long long *part;  // [P][nchunk][2]: kept roots, box pixels of a chunk (then their prefixes)
    long long *tot;   // [P][4]: kept, mask bytes, peaks
};

int64_t work_bytes(int64_t P, int64_t N) {
    return align16(P * N * 4) + align16(P * kRec * N * 4) + align16(P * nchunks(N) * 16) + P * 32;
}

Work carve(void *d_work, int64_t P, int64_t N) {
    char *p = (char *)d_work;
    Work w;
    w.label = (int32_t *)p;
    p += align16(P * N * 4);
    w.rec = (int32_t *)p;
    p += align16(P * kRec * N * 4);
    w.part = (long long *)p;
    p += align16(P * nchunks(N) * 16);
    w.tot = (long long *)p;
    return w;
}

// pass 1.  grid (tiles_x, min(tiles_y, kMaxGrid), P), block (64, kRows)
template <typename T>
__global__ __launch_bounds__(kT) void tile_label_kernel(const T *images, int H, int W, double th,
                                                        int32_t *parent, int tiles_y) {
    __shared__ int lab[kTile * kTile];
    const int64_t N = (int64_t)H * W;
    const T *im = images + (int64_t)blockIdx.z * N;
    int32_t *par = parent + (int64_t)blockIdx.z * N;
    for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y)
        label_tile<T>(im, par, H, W, th, blockIdx.x, ty, lab);
}

// pass 2.  grid (blocks, P)
__global__ __launch_bounds__(kT) void merge_borders_kernel(int32_t *parent, int H, int W,
                                                           int tiles_x, int tiles_y) {
    const int64_t N = (int64_t)H * W;
    int32_t *par = parent + (int64_t)blockIdx.y * N;
    const int64_t nv = (int64_t)(tiles_x - 1) * H, nh = (int64_t)(tiles_y - 1) * W;
    for (int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x; k < nv + nh;
         k += (int64_t)gridDim.x * kT)
        merge_border_pixel(par, H, W, nv, k);
}

// pass 3.  2-D mapping of passes 3, 4, 8 and the peak kernels: grid (ceil(W / 64),
// min(ceil(H / kRows), kMaxGrid), P), block (64, kRows); a wavefront = 64 pixels of one row
__global__ __launch_bounds__(kT) void flatten_kernel(int32_t *label, int32_t *rec, int H, int W) {
    const int64_t N = (int64_t)H * W;
    int32_t *lab = label + (int64_t)blockIdx.z * N;
    int32_t *rc = rec + (int64_t)blockIdx.z * kRec * N;
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y * kRows + threadIdx.y; y < H; y += gridDim.y * kRows)
        flatten_pixel(lab, rc, N, H, W, y * W + x);
}

// pass 4
__global__ __launch_bounds__(kT) void records_kernel(const int32_t *label, int32_t *rec, int H,
                                                     int W) {
    const int64_t N = (int64_t)H * W;
    const int32_t *lab = label + (int64_t)blockIdx.z * N;
    int32_t *rc = rec + (int64_t)blockIdx.z * kRec * N;
    // no lane leaves early: the ballots of record_row need the whole wavefront
    for (int y = blockIdx.y * kRows + threadIdx.y; y < H; y += gridDim.y * kRows)
        record_row(lab, rc, N, W, y, blockIdx.x * 64);
}

// passes 5 and 7.  grid (nchunk, P), block kT (1-D)
template <int FINAL>
__global__ __launch_bounds__(kT) void rank_kernel(const int32_t *label, int32_t *rec, int64_t N,
                                                  int min_area, long long *part) {
    __shared__ long long sh[kT / 64];
    rank_chunk<FINAL>(label + (int64_t)blockIdx.y * N, rec + (int64_t)blockIdx.y * kRec * N, N,
                      min_area, part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2,
                      blockIdx.x, sh);
}

// pass 6.  One workgroup per plane
__global__ __launch_bounds__(kT) void chunk_scan_kernel(long long *part, int64_t nchunk,
                                                        long long *tot) {
    __shared__ long long sh[kT / 64];
    scan_chunk_sums(part + (int64_t)blockIdx.x * nchunk * 2, nchunk, tot + 4 * blockIdx.x, sh);
}

// pass 8 (EMIT 0): tot[plane][2] += peaks, one add per wavefront.  Fetch (EMIT 1), one plane:
// the peaks go to out[] in arrival order, slots from *counter; a slot beyond `cap` (the count
// of pass 8) is not written
template <typename T, int EMIT>
__global__ __launch_bounds__(kT) void peaks_kernel(const T *images, const int32_t *label,
                                                   const int32_t *rec, int H, int W,
                                                   long long *tot, PeakDev *out,
                                                   unsigned int *counter, unsigned int cap) {
    const int64_t N = (int64_t)H * W;
    const T *im = images + (int64_t)blockIdx.z * N;
    const int32_t *lab = label + (int64_t)blockIdx.z * N;
    const int32_t *rc = rec + (int64_t)blockIdx.z * kRec * N;
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane;
    for (int y = blockIdx.y * kRows + threadIdx.y; y < H; y += gridDim.y * kRows) {
        int rank = -1;
        T v = T(0);
        const bool peak = x < W && peak_at<T>(im, lab, rc, N, W, y, x, &rank, &v);
        const unsigned long long m = __ballot(peak);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        if (!EMIT) {
            if (lane == leader)
                atomicAdd((unsigned long long *)(tot + 4 * blockIdx.z + 2),
                          (unsigned long long)__popcll(m));
        } else {
            unsigned int base = 0;
            if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(m));
            base = __shfl(base, leader, 64);
            const unsigned int slot = base + __popcll(m & ((1ull << lane) - 1ull));
            if (peak && slot < cap) {
                out[slot].rank = rank;
                out[slot].lin = y * W + x;
                out[slot].flux = (double)v;
            }
        }
    }
}

// fetch: bounds[rank][4], mask offset and root of the kept footprints of one plane
__global__ __launch_bounds__(kT) void compact_kernel(const int32_t *lab, const int32_t *rc,
                                                     int64_t N, int32_t *bounds, int32_t *moff,
                                                     int32_t *roots) {
    for (int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x; p < N; p += (int64_t)gridDim.x * kT) {
        if (lab[p] != (int)p) continue;
        const int r = rc[R_RANK * N + p];
        if (r < 0) continue;
        bounds[4 * r] = rc[R_Y0 * N + p];
        bounds[4 * r + 1] = rc[R_Y1 * N + p];
        bounds[4 * r + 2] = rc[R_X0 * N + p];
        bounds[4 * r + 3] = rc[R_X1 * N + p];
        moff[r] = rc[R_MOFF * N + p];
        roots[r] = (int)p;
    }
}

// fetch: one thread per mask byte; its footprint is the last rank with moff[rank] <= byte
__global__ __launch_bounds__(kT) void masks_kernel(const int32_t *lab, int W, const int32_t *bounds,
                                                   const int32_t *moff, const int32_t *roots,
                                                   int n, int64_t n_bytes, uint8_t *masks) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= n_bytes) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)moff[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    masks[k] = mask_byte(lab, W, bounds + 4 * lo, roots[lo], k - moff[lo]);
}

dim3 grid2d(int P, int H, int W) {
    const int64_t gy = ((int64_t)H + kRows - 1) / kRows;
    return dim3((unsigned)(((int64_t)W + 63) / 64), (unsigned)std::min<int64_t>(gy, kMaxGrid),
                (unsigned)P);
}

int check_sizes(int32_t P, int32_t H, int32_t W) {
    SMI_REQUIRE(P > 0 && H > 0 && W > 0, "bad sizes");
    SMI_REQUIRE(P <= kMaxGrid, "too many planes");
    SMI_REQUIRE((int64_t)H * W <= INT32_MAX, "footprints: more than 2^31 pixels in a plane");
    return SMI_OK;
}

template <typename T>
int label_planes(const T *d_images, int32_t P, int32_t H, int32_t W, int32_t min_area,
                 int32_t thresh, void *d_work, int64_t work_size, int32_t *counts, void *stream) {
    int rc = check_sizes(P, H, W);
    if (rc) return rc;
    rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_images && d_work && counts, "null argument");
    const int64_t N = (int64_t)H * W;
    SMI_REQUIRE(work_size >= work_bytes(P, N), "work buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const Work w = carve(d_work, P, N);
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const dim3 block2(64, kRows), g2 = grid2d(P, H, W);

    hipLaunchKernelGGL(tile_label_kernel<T>, dim3(tiles_x, std::min(tiles_y, kMaxGrid), P), block2,
                       0, st, d_images, H, W, (double)thresh, w.label, tiles_y);
    const int64_t n_border = (int64_t)(tiles_x - 1) * H + (int64_t)(tiles_y - 1) * W;
    if (n_border > 0) {
        const int64_t gb = std::min<int64_t>((n_border + kT - 1) / kT, 1 << 20);
        hipLaunchKernelGGL(merge_borders_kernel, dim3((unsigned)gb, P), dim3(kT), 0, st, w.label,
                           H, W, tiles_x, tiles_y);
    }
    hipLaunchKernelGGL(flatten_kernel, g2, block2, 0, st, w.label, w.rec, H, W);
    hipLaunchKernelGGL(records_kernel, g2, block2, 0, st, w.label, w.rec, H, W);
    const int64_t nch = nchunks(N);
    hipLaunchKernelGGL(rank_kernel<0>, dim3((unsigned)nch, P), dim3(kT), 0, st, w.label, w.rec, N,
                       min_area, w.part);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(P), dim3(kT), 0, st, w.part, nch, w.tot);
    hipLaunchKernelGGL(rank_kernel<1>, dim3((unsigned)nch, P), dim3(kT), 0, st, w.label, w.rec, N,
                       min_area, w.part);
    hipLaunchKernelGGL((peaks_kernel<T, 0>), g2, block2, 0, st, d_images, w.label, w.rec, H, W,
                       w.tot, (PeakDev *)nullptr, (unsigned int *)nullptr, 0u);
    SMI_HIP(hipGetLastError());
    std::vector<long long> tot((size_t)P * 4);
    SMI_HIP(hipMemcpyAsync(tot.data(), w.tot, tot.size() * sizeof(long long),
                           hipMemcpyDeviceToHost, st));
    SMI_HIP(hipStreamSynchronize(st));
    for (int pl = 0; pl < P; ++pl)
        if (tot[4 * pl + 1] > INT32_MAX || tot[4 * pl + 2] > INT32_MAX) {
            set_error("footprints: more than 2^31 mask pixels or peaks");
            return SMI_ERR_INVALID;
        }
    for (int pl = 0; pl < P; ++pl)
        for (int k = 0; k < 3; ++k) counts[3 * pl + k] = (int32_t)tot[4 * pl + k];
    return SMI_OK;
}

// layout of the fetch scratch for counts = (n, mask bytes, peaks)
struct Scratch {
    int64_t bounds, moff, roots, counter, peaks, masks, total;
};
Scratch scratch_layout(const int32_t *counts) {
    const int64_t n = counts[0], nm = counts[1], np = counts[2];
    Scratch s;
    s.bounds = 0;
    s.moff = s.bounds + align16(16 * n);
    s.roots = s.moff + align16(4 * n);
    s.counter = s.roots + align16(4 * n);
    s.peaks = s.counter + 16;
    s.masks = s.peaks + 16 * np;
    s.total = s.masks + align16(nm);
    return s;
}

template <typename T>
int fetch_plane(const T *d_images, int32_t P, int32_t H, int32_t W, int32_t plane,
                double min_separation, const int32_t *counts, const void *d_work,
                void *d_scratch, int64_t scratch_size, int32_t *bounds, uint8_t *masks,
                int32_t *peak_start, int32_t *peak_yx, double *peak_flux, void *stream) {
    int rc = check_sizes(P, H, W);
    if (rc) return rc;
    SMI_REQUIRE(plane >= 0 && plane < P, "no such plane");
    rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_images && d_work && counts, "null argument");
    const int32_t n = counts[0], nm = counts[1], np = counts[2];
    SMI_REQUIRE(n >= 0 && nm >= 0 && np >= 0, "bad counts");
    if (n == 0) {
        if (peak_start) peak_start[0] = 0;
        return SMI_OK;
    }
    SMI_REQUIRE(bounds && masks && peak_start, "null argument");
    SMI_REQUIRE((peak_yx && peak_flux) || np == 0, "null peak arrays");
    const Scratch sl = scratch_layout(counts);
    SMI_REQUIRE(d_scratch && scratch_size >= sl.total, "scratch buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const Work w = carve(const_cast<void *>(d_work), P, N);
    const int32_t *lab = w.label + (int64_t)plane * N;
    const int32_t *rec = w.rec + (int64_t)plane * kRec * N;
    char *sc = (char *)d_scratch;
    int32_t *d_bounds = (int32_t *)(sc + sl.bounds), *d_moff = (int32_t *)(sc + sl.moff);
    int32_t *d_roots = (int32_t *)(sc + sl.roots);
    unsigned int *d_counter = (unsigned int *)(sc + sl.counter);
    PeakDev *d_peaks = (PeakDev *)(sc + sl.peaks);
    uint8_t *d_masks = (uint8_t *)(sc + sl.masks);

    SMI_HIP(hipMemsetAsync(d_counter, 0, 16, st));
    const int64_t gc = std::min<int64_t>((N + kT - 1) / kT, 1 << 16);
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)gc), dim3(kT), 0, st, lab, rec, N, d_bounds,
                       d_moff, d_roots);
    hipLaunchKernelGGL(masks_kernel, dim3((unsigned)(((int64_t)nm + kT - 1) / kT)), dim3(kT), 0, st,
                       lab, W, d_bounds, d_moff, d_roots, n, (int64_t)nm, d_masks);
    if (np > 0)
        hipLaunchKernelGGL((peaks_kernel<T, 1>), grid2d(1, H, W), dim3(64, kRows), 0, st,
                           d_images + (int64_t)plane * N, lab, rec, H, W, (long long *)nullptr,
                           d_peaks, d_counter, (unsigned int)np);
    SMI_HIP(hipGetLastError());
    std::vector<PeakDev> pk((size_t)np);
    unsigned int emitted = 0;
    SMI_HIP(hipMemcpyAsync(bounds, d_bounds, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
    SMI_HIP(hipMemcpyAsync(masks, d_masks, (size_t)nm, hipMemcpyDeviceToHost, st));
    if (np > 0)
        SMI_HIP(hipMemcpyAsync(pk.data(), d_peaks, 16 * (size_t)np, hipMemcpyDeviceToHost, st));
    SMI_HIP(hipMemcpyAsync(&emitted, d_counter, sizeof(emitted), hipMemcpyDeviceToHost, st));
    SMI_HIP(hipStreamSynchronize(st));
    SMI_REQUIRE(emitted == (unsigned int)np, "footprints: the images changed since they were labelled");

    // the order of detect.cpp, then its min_separation filter (footprints_device.h)
    std::sort(pk.begin(), pk.end(), [](const PeakDev &a, const PeakDev &b) {
        if (a.rank != b.rank) return a.rank < b.rank;
        return peak_before(a, b);
    });
    select_peaks(
        pk, n, [](const PeakDev &p) { return p.rank; }, [W](const PeakDev &) { return W; },
        min_separation, peak_start, peak_yx, peak_flux);
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_footprints_device_work_bytes(int32_t P, int32_t H, int32_t W, int64_t *bytes) {
    SMI_REQUIRE(bytes, "null argument");
    int rc = smi::check_sizes(P, H, W);
    if (rc) return rc;
    *bytes = smi::work_bytes(P, (int64_t)H * W);
    return SMI_OK;
}
int smi_footprints_device_fetch_bytes(const int32_t *counts, int64_t *bytes) {
    SMI_REQUIRE(counts && bytes, "null argument");
    SMI_REQUIRE(counts[0] >= 0 && counts[1] >= 0 && counts[2] >= 0, "bad counts");
    *bytes = smi::scratch_layout(counts).total;
    return SMI_OK;
}
int smi_footprints_device_label_f32(const float *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t min_area, int32_t thresh, void *d_work,
                                    int64_t work_bytes, int32_t *counts, void *stream) {
    return smi::label_planes<float>(d_images, P, H, W, min_area, thresh, d_work, work_bytes,
                                    counts, stream);
}
int smi_footprints_device_label_f64(const double *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t min_area, int32_t thresh, void *d_work,
                                    int64_t work_bytes, int32_t *counts, void *stream) {
    return smi::label_planes<double>(d_images, P, H, W, min_area, thresh, d_work, work_bytes,
                                     counts, stream);
}
int smi_footprints_device_fetch_f32(const float *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t plane, double min_separation, const int32_t *counts,
                                    const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                    int32_t *bounds, uint8_t *masks, int32_t *peak_start,
                                    int32_t *peak_yx, double *peak_flux, void *stream) {
    return smi::fetch_plane<float>(d_images, P, H, W, plane, min_separation, counts, d_work,
                                   d_scratch, scratch_bytes, bounds, masks, peak_start, peak_yx,
                                   peak_flux, stream);
}
int smi_footprints_device_fetch_f64(const double *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t plane, double min_separation, const int32_t *counts,
                                    const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                    int32_t *bounds, uint8_t *masks, int32_t *peak_start,
                                    int32_t *peak_yx, double *peak_flux, void *stream) {
    return smi::fetch_plane<double>(d_images, P, H, W, plane, min_separation, counts, d_work,
                                    d_scratch, scratch_bytes, bounds, masks, peak_start, peak_yx,
                                    peak_flux, stream);
}

}  // extern "C"
