// lite.measure_blends: the sums a catalogue row is made of -- fluxes, first and second moments,
// the model's sum and sum of squares, the brightest pixel -- of the reweighted flux cubes of
// lite.weight_blends, for a catalogue of blends, three launches per chunk.  The cubes themselves
// are an optional output.
//
//   totals    the totals pass of reweight.hip (the tile of reweight_device.h) -> `total`
//   sources   per 32 x 32 tile of a source's rectangle and band: M = max(model, 0) and
//             f = min(M / total, 1) (0 where total == 0) * image per pixel, exactly as reweight.hip
//             forms them; f is stored when a cube buffer was given; the workgroup reduces
//                 sum M, sum M^2, sum f, sum y f, sum x f, sum y^2 f, sum y x f, sum x^2 f
//             in float64 (y, x: integers counted from the rectangle's corner) and the largest f
//             with the first row-major position that holds it, and writes one partial record
//   combine   one thread per (source, band) adds the partial records of the source's tiles
//
// Order of the sums.  Every term is formed in float64 from the pixel's M or f converted to
// double: the coordinate products y y, y x, x x are exact integers and multiply f in one
// rounded multiplication -- exact for float32 data while the weight stays below 2^29, i.e. for
// rectangles up to 23170 pixels a side -- and M^2 is exact for float32 data.  A term is added
//   1. in the thread: thread (row r = tid / 8, group g = tid % 8) of the tile owns the pixels
//      (r, 4 g + j), j = 0 .. 3, and adds the terms of those inside the rectangle to +0 in
//      order of j;
//   2. in the wavefront (eight rows of the tile): lane l adds the sum of lane l + 32, then of
//      l + 16, 8, 4, 2, 1 (lanes without a pixel hold +0);
//   3. in the workgroup: wavefront 0 + wavefront 1, + wavefront 2, + wavefront 3;
//   4. in the combine pass: +0, + tile 0, + tile 1, ... in row-major order of the tiles.
// The order is a function of the rectangle's (h, w) alone: not of the grid, of the chunk, of the
// other sources in the tables or of the device.  The peak compares (value, position) pairs --
// larger value, or equal value and smaller row-major position in the rectangle -- which is
// associative and commutative, so it is np.argmax's first maximum whatever the order.
//
// Parallelism is over pixels; no atomics, no waiting between workgroups, and every loop bound is
// a descriptor field smi_lite_measure_* validated on the host (check_plan).  The reduction's
// scratch (4 wavefronts x 10 values) takes the place of the halo in LDS after a barrier, so the
// LDS budget -- and with it which stamps the device takes -- is that of reweight.hip.
#include <cmath>
#include <cstdint>

#include "reweight_device.h"

namespace smi {
namespace {

using namespace reweight_tile;

constexpr int kSums = 8;
constexpr int kRecord = SMI_LITE_MEASURE_RECORD;  // the sums, the peak value, its position
static_assert(kRecord == kSums + 2, "record layout");
constexpr int kWaves = kThreads / 64;
constexpr int kNoPixel = INT32_MAX;  // position of "no pixel yet": loses every tie

template <typename T>
struct MeasureArgs {
    ReweightArgs<T> r;  // r.out == nullptr: the cubes are not stored
    double *partial;    // [workgroup][band][kRecord]
};

template <typename T>
__global__ __launch_bounds__(kThreads) void measure_totals_kernel(const ReweightArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    tile_pass<T, false>(a, lds_raw);
}

__device__ __forceinline__ void take_peak(double &v, int &at, double ov, int oat) {
    if (ov > v || (ov == v && oat < at)) v = ov, at = oat;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void measure_sources_kernel(const MeasureArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    Tile t;
    T m[kPerThread];
    tile_model<T, true>(a.r, lds_raw, t, m);

    double s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0;
    double peak = -INFINITY;
    int peak_at = kNoPixel;  // oy * kTileX + ox: row-major inside the tile
    if (t.active) {
        const double y = t.ty0 + t.oy;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            if (t.ox + j >= t.tw) continue;
            const int64_t at = frame_at(t, j);
            const T flux = source_flux(m[j], a.r.total[at], a.r.images[at]);
            if (a.r.out) a.r.out[cube_at(t, j)] = flux;
            const double M = m[j], f = flux, x = t.tx0 + t.ox + j;
            s[0] += M;
            s[1] += M * M;
            s[2] += f;
            s[3] += y * f;
            s[4] += x * f;
            s[5] += (y * y) * f;
            s[6] += (y * x) * f;
            s[7] += (x * x) * f;
            take_peak(peak, peak_at, f, t.oy * kTileX + t.ox + j);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) s[k] += __shfl_down(s[k], off, 64);
        const double ov = __shfl_down(peak, off, 64);
        const int oat = __shfl_down(peak_at, off, 64);
        take_peak(peak, peak_at, ov, oat);
    }

    __syncthreads();  // every tap loop has read the halo: its place is free
    double *scratch = reinterpret_cast<double *>(lds_raw);  // [kWaves][kSums + 1], then positions
    int *scratch_at = reinterpret_cast<int *>(scratch + kWaves * (kSums + 1));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) scratch[wave * (kSums + 1) + k] = s[k];
        scratch[wave * (kSums + 1) + kSums] = peak;
        scratch_at[wave] = peak_at;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; ++w) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) s[k] += scratch[w * (kSums + 1) + k];
        take_peak(peak, peak_at, scratch[w * (kSums + 1) + kSums], scratch_at[w]);
    }
    double *rec = a.partial + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * kRecord;
#pragma unroll
    for (int k = 0; k < kSums; ++k) rec[k] = s[k];
    rec[kSums] = peak;
    // position in the source's rectangle (exact in a double: below 2^48); -1: no pixel compared
    // greater than -inf (not-a-number fluxes, outside the contract)
    rec[kSums + 1] = peak_at == kNoPixel
                         ? -1.0
                         : (double)((int64_t)(t.ty0 + peak_at / kTileX) * t.rw + t.tx0 +
                                    peak_at % kTileX);
}

// first[s] .. first[s + 1]: the workgroups (tiles, in row-major order) of source s
__global__ void measure_combine_kernel(const int32_t *first, int32_t n_sources, int32_t C,
                                       const double *partial, double *records) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_sources * C) return;
    const int32_t src = (int32_t)(i / C), band = (int32_t)(i % C);
    double s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0;
    double peak = -INFINITY, peak_at = -1;
    for (int32_t w = first[src]; w < first[src + 1]; ++w) {
        const double *p = partial + ((int64_t)w * C + band) * kRecord;
#pragma unroll
        for (int k = 0; k < kSums; ++k) s[k] += p[k];
        const double ov = p[kSums], oat = p[kSums + 1];
        if (oat >= 0 && (ov > peak || (ov == peak && oat < peak_at))) peak = ov, peak_at = oat;
    }
    double *rec = records + i * kRecord;
#pragma unroll
    for (int k = 0; k < kSums; ++k) rec[k] = s[k];
    rec[kSums] = peak;
    rec[kSums + 1] = peak_at;
}

// milliseconds the three launches of this host thread's last call took on the device
thread_local double g_last_launch_ms = 0;

struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
};

template <typename T>
int measure(const Plan<T> &p, int32_t device, T *out, int64_t n_out, double *records,
            int64_t n_record) {
    SMI_REQUIRE(out || n_out == 0, "a cube buffer size without a cube buffer");
    SMI_REQUIRE(n_record >= 0 && (records || !n_record), "null record buffer");
    std::vector<int32_t> work_total, work_src;
    size_t lds = 0;
    int rc = check_plan(p, out != nullptr, n_out, &work_total, &work_src, &lds);
    if (rc) return rc;
    const int64_t need = (int64_t)p.n_sources * p.C * kRecord;
    SMI_REQUIRE(n_record >= need, "record buffer too small");
    static_assert(kWaves * (kSums + 1) * sizeof(double) + kWaves * sizeof(int) <=
                      (size_t)kTileY * kTileX * sizeof(float), "scratch beyond the smallest halo");
    std::vector<int32_t> first(p.n_sources + 1, 0);
    for (size_t w = 0; w < work_src.size() / 2; ++w) ++first[work_src[2 * w] + 1];
    for (int32_t s = 0; s < p.n_sources; ++s) first[s + 1] += first[s];
    if ((rc = check_device(device))) return rc;
    if (work_src.empty()) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    Uploaded<T> dev;
    MeasureArgs<T> a;
    if ((rc = dev.upload(p, work_total, work_src, out ? n_out : -1, &a.r))) return rc;
    DevBuf<int32_t> d_first;
    DevBuf<double> d_partial, d_records;
    const size_t n_tiles = work_src.size() / 2;
    SMI_HIP(d_first.upload(first.data(), first.size()));
    SMI_HIP(d_partial.alloc(n_tiles * p.C * kRecord));
    SMI_HIP(d_records.alloc((size_t)need));
    a.partial = d_partial.p;

    Event begin, end;
    SMI_HIP(hipEventCreate(&begin.e));
    SMI_HIP(hipEventCreate(&end.e));
    SMI_HIP(hipEventRecord(begin.e, 0));
    a.r.work = dev.work_total.p;
    hipLaunchKernelGGL((measure_totals_kernel<T>), dim3((unsigned)(work_total.size() / 2), p.C),
                       dim3(kThreads), lds, 0, a.r);
    SMI_HIP(hipGetLastError());
    a.r.work = dev.work_src.p;
    hipLaunchKernelGGL((measure_sources_kernel<T>), dim3((unsigned)n_tiles, p.C), dim3(kThreads),
                       lds, 0, a);
    SMI_HIP(hipGetLastError());
    const int64_t n_rows = (int64_t)p.n_sources * p.C;
    hipLaunchKernelGGL(measure_combine_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                       0, d_first.p, p.n_sources, p.C, d_partial.p, d_records.p);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipEventRecord(end.e, 0));
    SMI_HIP(hipMemcpy(records, d_records.p, (size_t)need * sizeof(double), hipMemcpyDeviceToHost));
    if (out) SMI_HIP(hipMemcpy(out, dev.out.p, (size_t)n_out * sizeof(T), hipMemcpyDeviceToHost));
    float ms = 0;
    SMI_HIP(hipEventSynchronize(end.e));
    SMI_HIP(hipEventElapsedTime(&ms, begin.e, end.e));
    g_last_launch_ms = ms;
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_lite_measure_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_reweight_blend *blends, int32_t n_sources,
                         const smi_reweight_source *sources, int32_t n_components,
                         const smi_reweight_component *components, const float *images,
                         int64_t n_image, const float *stamps, int64_t n_stamp, const float *seds,
                         int64_t n_sed, const float *morphs, int64_t n_morph, float *out,
                         int64_t n_out, double *records, int64_t n_record) {
    const smi::reweight_tile::Plan<float> p = {C, kh, kw, n_blends, blends, n_sources, sources,
        n_components, components, images, n_image, stamps, n_stamp, seds, n_sed, morphs, n_morph};
    return smi::measure<float>(p, device, out, n_out, records, n_record);
}
int smi_lite_measure_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_reweight_blend *blends, int32_t n_sources,
                         const smi_reweight_source *sources, int32_t n_components,
                         const smi_reweight_component *components, const double *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp, const double *seds,
                         int64_t n_sed, const double *morphs, int64_t n_morph, double *out,
                         int64_t n_out, double *records, int64_t n_record) {
    const smi::reweight_tile::Plan<double> p = {C, kh, kw, n_blends, blends, n_sources, sources,
        n_components, components, images, n_image, stamps, n_stamp, seds, n_sed, morphs, n_morph};
    return smi::measure<double>(p, device, out, n_out, records, n_record);
}

int smi_lite_measure_last_launch_ms(double *ms) {
    if (!ms) {
        smi::set_error("null output");
        return SMI_ERR_INVALID;
    }
    *ms = smi::g_last_launch_ms;
    return SMI_OK;
}

}  // extern "C"
