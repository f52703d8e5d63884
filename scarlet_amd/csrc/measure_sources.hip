// measure_blends: the sums a row of scarlet.measure is made of -- a source's fluxes, first and
// second moments and brightest pixel, and per observed band the sums of its model alone rendered
// into that band -- for the sources of a catalogue of blends, three launches per chunk.
//
//   model    one workgroup per (source, model band).  Thread t takes the pixels t, t + 256, ... of
//            the source's box (row-major), forms each model pixel m -- the rounded products
//            sed[band] * morph[y, x] of the components whose box holds it, added to +0 in
//            component order, in float64 -- and adds m, y m, x m, (y y) m, (y x) m, (x x) m to
//            its own sums (integer y, x from the box corner: the coordinate products are exact,
//            each term has one rounded multiplication); it keeps its first largest m.  Then the
//            wavefront (lane l adds lane l + 32, then l + 16, 8, 4, 2, 1), then wavefront 0 + 1,
//            + 2, + 3.  The peak compares (value, pixel index) pairs -- larger value, or equal
//            value and lower index --, which is associative and commutative: np.argmax's first
//            maximum whatever the order.
//   render   one workgroup of 256 threads per (source, 16 x 16 tile, observed band).  The tiles
//            cover the REGION: the source's box grown by the stamp's half and clipped to the
//            frame.  The window of the band's model channel under the tile's taps is staged in LDS
//            as float64 (window_device.h), zero outside the box and outside the frame; one thread
//            per pixel runs the tap loop, R; then R, R R and (R R) (1 / W) of the 256 pixels
//            (+0 for those outside the region) are summed per segment of 32 pixels in pixel order
//            by 8 consecutive lanes, and the 8 are joined by a fixed butterfly.
//   reduce   one thread per (source, observed band, quantity) adds its tiles in tile order.
//
// The columns of the segment sums are 256 doubles with one double of padding after every 32 (2
// banks per segment): the 3 x 8 lanes that add them read 24 different bank pairs.
//
// No atomics, no workgroup waits for another, the order of every sum is a function of the
// source's box, its frame and the stamp shape alone, and every loop bound is a descriptor field
// smi_measure_sources_f32 validated on the host before anything is launched (check_plan).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "window_device.h"

namespace smi {
namespace {

using window::kTile;
using window::tap_range;
using window::tap_sum;
using window::window_pitch;

constexpr int kThreads = kTile * kTile;
constexpr int kWaves = kThreads / 64;
constexpr int kSegs = 8, kSegLen = kThreads / kSegs;  // 8 x 32 pixels
constexpr int kCol = kThreads + kSegs;                // doubles of a column in LDS
constexpr int kSums = 6;
constexpr int kRecord = SMI_MEASURE_SOURCES_RECORD;   // the sums, the peak value, its position
static_assert(kRecord == kSums + 2, "record layout");
constexpr int kRendered = 3;                          // sum R, sum R^2, sum R^2 / W
constexpr int kMaxStamp = 63;                         // side: a window of 78 x 80 doubles, 49 KiB
constexpr int32_t kMaxExtent = 1 << 14;               // sides of a box
constexpr int32_t kMaxCoord = 1 << 24;                // |origins| and frame sides
constexpr int kNoPixel = INT32_MAX;                   // position of "no pixel yet": loses every tie

struct Rect {
    int y0, x0, h, w;
};

// the part of the source's box that lies in the frame: what of its model is rendered
__host__ __device__ inline Rect in_frame(const smi_measure_source &s) {
    Rect r;
    r.y0 = s.y0 > 0 ? s.y0 : 0, r.x0 = s.x0 > 0 ? s.x0 : 0;
    const int y1 = s.y0 + s.h < s.fh ? s.y0 + s.h : s.fh;
    const int x1 = s.x0 + s.w < s.fw ? s.x0 + s.w : s.fw;
    r.h = y1 > r.y0 ? y1 - r.y0 : 0, r.w = x1 > r.x0 ? x1 - r.x0 : 0;
    return r;
}

// the frame pixels the rendered model can reach: the box grown by the stamp's half, clipped
__host__ __device__ inline Rect region_of(const smi_measure_source &s, int kh, int kw) {
    Rect r;
    r.y0 = s.y0 - kh / 2 > 0 ? s.y0 - kh / 2 : 0, r.x0 = s.x0 - kw / 2 > 0 ? s.x0 - kw / 2 : 0;
    const int y1 = s.y0 + s.h + kh / 2 < s.fh ? s.y0 + s.h + kh / 2 : s.fh;
    const int x1 = s.x0 + s.w + kw / 2 < s.fw ? s.x0 + s.w + kw / 2 : s.fw;
    r.h = y1 > r.y0 ? y1 - r.y0 : 0, r.w = x1 > r.x0 ? x1 - r.x0 : 0;
    return r;
}

__host__ __device__ inline int tiles_of(const Rect &r) {
    return ((r.h + kTile - 1) / kTile) * ((r.w + kTile - 1) / kTile);
}

struct MeasureArgs {
    const smi_measure_source *sources;
    const smi_measure_component *comps;
    const smi_measure_band *bands;
    const double *seds, *morphs;
    const float *stamps, *weights;
    const int32_t *work;  // per workgroup of the render launch: (source, tile, band of the source)
    const int64_t *rows;  // per (source, band): its first workgroup, its tiles
    double *records, *part, *rendered;
    int64_t n_rows;
    int32_t kh, kw, C;
};

// model pixel (y, x), frame coordinates, of band `band`
__device__ __forceinline__ double model_pixel(const MeasureArgs &a, const smi_measure_source &s,
                                              int band, int y, int x) {
    double acc = 0;
    for (int k = 0; k < s.n_comp; ++k) {
        const smi_measure_component d = a.comps[s.comp0 + k];
        const int yy = y - d.y0, xx = x - d.x0;
        if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w)
            acc += a.seds[d.sed_off + band] * a.morphs[d.morph_off + (int64_t)yy * d.w + xx];
    }
    return acc;
}

__device__ __forceinline__ void take_peak(double &v, int &at, double ov, int oat) {
    if (ov > v || (ov == v && oat < at)) v = ov, at = oat;
}

__global__ __launch_bounds__(kThreads) void measure_model_kernel(const MeasureArgs a) {
    __shared__ double scratch[kWaves][kSums + 1];
    __shared__ int scratch_at[kWaves];
    const smi_measure_source s = a.sources[blockIdx.x];
    const int band = blockIdx.y;
    const int n = s.h * s.w;  // <= 2^28

    double sum[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = 0;
    double peak = -INFINITY;
    int peak_at = kNoPixel;
    for (int e = threadIdx.x; e < n; e += kThreads) {
        const int iy = e / s.w, ix = e - iy * s.w;
        const double m = model_pixel(a, s, band, s.y0 + iy, s.x0 + ix);
        const double y = iy, x = ix;
        sum[0] += m;
        sum[1] += y * m;
        sum[2] += x * m;
        sum[3] += (y * y) * m;
        sum[4] += (y * x) * m;
        sum[5] += (x * x) * m;
        if (m > peak) peak = m, peak_at = e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sum[k] += __shfl_down(sum[k], off, 64);
        const double ov = __shfl_down(peak, off, 64);
        const int oat = __shfl_down(peak_at, off, 64);
        take_peak(peak, peak_at, ov, oat);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) scratch[wave][k] = sum[k];
        scratch[wave][kSums] = peak;
        scratch_at[wave] = peak_at;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; ++w) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sum[k] += scratch[w][k];
        take_peak(peak, peak_at, scratch[w][kSums], scratch_at[w]);
    }
    double *rec = a.records + ((int64_t)blockIdx.x * a.C + band) * kRecord;
#pragma unroll
    for (int k = 0; k < kSums; ++k) rec[k] = sum[k];
    rec[kSums] = peak;
    // -1: no pixel compared greater than -inf (not-a-number models: the caller's fallback)
    rec[kSums + 1] = peak_at == kNoPixel ? -1.0 : (double)peak_at;
}

__global__ __launch_bounds__(kThreads) void measure_render_kernel(const MeasureArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int kh = a.kh, kw = a.kw;
    const int wh = kTile + kh - 1, ww = kTile + kw - 1, wp = window_pitch(kw);
    double *win = reinterpret_cast<double *>(lds_raw);  // the model under the tile's taps
    double *col = win + wh * wp;                        // [kRendered][kCol]

    const int tid = threadIdx.x;
    const int32_t *work = a.work + 3 * (int64_t)blockIdx.x;
    const smi_measure_source s = a.sources[work[0]];
    const int tile = work[1];
    const smi_measure_band bd = a.bands[s.band0 + work[2]];
    const Rect g = region_of(s, kh, kw), box = in_frame(s);
    const int tiles_x = (g.w + kTile - 1) / kTile;
    const int ty0 = g.y0 + (tile / tiles_x) * kTile, tx0 = g.x0 + (tile % tiles_x) * kTile;
    const int th = min(kTile, g.y0 + g.h - ty0), tw = min(kTile, g.x0 + g.w - tx0);

    // window (r, c) is frame pixel (ty0 - kh / 2 + r, tx0 - kw / 2 + c)
    const int wy0 = ty0 - kh / 2, wx0 = tx0 - kw / 2;
    for (int e = tid; e < wh * ww; e += kThreads) {
        const int r = e / ww, c = e - r * ww;
        const int y = wy0 + r, x = wx0 + c;
        const bool lit = y >= box.y0 && y < box.y0 + box.h && x >= box.x0 && x < box.x0 + box.w;
        win[r * wp + c] = lit ? model_pixel(a, s, bd.channel, y, x) : 0.0;
    }
    __syncthreads();

    const int i = tid / kTile, j = tid % kTile;
    const bool inside = i < th && j < tw;
    int ky_lo, ky_hi, kx_lo, kx_hi;
    tap_range(kh, box.y0 - wy0, box.h, &ky_lo, &ky_hi);
    tap_range(kw, box.x0 - wx0, box.w, &kx_lo, &kx_hi);
    const double acc = tap_sum(win, wp, i, j, kh, kw, a.stamps + bd.stamp_off, ky_lo, ky_hi, kx_lo,
                               kx_hi);
    {
        const double R = inside ? acc : 0.0;
        const double W =
            inside ? (double)a.weights[bd.weight_off + (int64_t)(ty0 + i) * s.fw + tx0 + j] : 1.0;
        const int at = tid + tid / kSegLen;
        col[at] = R;
        col[kCol + at] = R * R;
        col[2 * kCol + at] = (R * R) * (1.0 / W);
    }
    __syncthreads();
    if (tid >= 64) return;  // (one wavefront: every lane of it shuffles)
    const int q = tid / kSegs, seg = tid % kSegs;
    const bool active = q < kRendered;
    double sum = 0;
    if (active) {
        const double *u = col + q * kCol + seg * (kSegLen + 1);
        for (int e = 0; e < kSegLen; ++e) sum += u[e];
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    if (active && seg == 0) a.part[(int64_t)blockIdx.x * kRendered + q] = sum;
}

__global__ void measure_reduce_kernel(const MeasureArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rows * kRendered) return;
    const int64_t row = i / kRendered;
    const int q = (int)(i % kRendered);
    const int64_t first = a.rows[2 * row], n = a.rows[2 * row + 1];
    double sum = 0;
    for (int64_t t = 0; t < n; ++t) sum += a.part[(first + t) * kRendered + q];
    a.rendered[i] = sum;
}

struct Plan {
    int32_t C, kh, kw;
    int32_t n_sources;
    const smi_measure_source *sources;
    int32_t n_components;
    const smi_measure_component *comps;
    int32_t n_bands;
    const smi_measure_band *bands;
    const double *seds;
    int64_t n_sed;
    const double *morphs;
    int64_t n_morph;
    const float *stamps;
    int64_t n_stamp;
    const float *weights;
    int64_t n_weight;
};

// Everything a kernel's loop bounds and addresses are made of, before anything is launched.
// work: (source, tile, band) per workgroup of the render launch -- a source's bands one after
// the other, each with its tiles in order --; rows: per (source, band) its first workgroup and
// its number of tiles.
int check_plan(const Plan &p, int64_t n_record, int64_t n_rendered, std::vector<int32_t> *work,
               std::vector<int64_t> *rows) {
    SMI_REQUIRE(p.C > 0 && p.C <= 65535, "bands");
    SMI_REQUIRE(p.kh > 0 && p.kw > 0 && p.kh % 2 == 1 && p.kw % 2 == 1,
                "the stamp must have odd height and width");
    SMI_REQUIRE(p.kh <= kMaxStamp && p.kw <= kMaxStamp, "stamp beyond the kernel's limit");
    SMI_REQUIRE(p.n_sources >= 0 && p.n_components >= 0 && p.n_bands >= 0, "negative count");
    SMI_REQUIRE(p.n_sed >= 0 && p.n_morph >= 0 && p.n_stamp >= 0 && p.n_weight >= 0 &&
                    n_record >= 0 && n_rendered >= 0, "negative buffer size");
    SMI_REQUIRE((p.sources || !p.n_sources) && (p.comps || !p.n_components) &&
                    (p.bands || !p.n_bands), "null descriptor table");
    SMI_REQUIRE((p.seds || !p.n_sed) && (p.morphs || !p.n_morph) && (p.stamps || !p.n_stamp) &&
                    (p.weights || !p.n_weight), "null buffer");
    for (int32_t c = 0; c < p.n_components; ++c) {
        const smi_measure_component &d = p.comps[c];
        SMI_REQUIRE(d.h > 0 && d.w > 0 && d.h <= kMaxExtent && d.w <= kMaxExtent,
                    "component extent");
        SMI_REQUIRE(d.y0 >= -kMaxCoord && d.y0 <= kMaxCoord && d.x0 >= -kMaxCoord &&
                        d.x0 <= kMaxCoord, "component origin");
        SMI_REQUIRE(in_buffer(d.sed_off, p.C, p.n_sed), "spectrum outside its buffer");
        SMI_REQUIRE(in_buffer(d.morph_off, (int64_t)d.h * d.w, p.n_morph),
                    "morphology outside its buffer");
    }
    for (int32_t b = 0; b < p.n_bands; ++b) {
        const smi_measure_band &bd = p.bands[b];
        SMI_REQUIRE(bd.channel >= 0 && bd.channel < p.C, "model band of an observed band");
        SMI_REQUIRE(in_buffer(bd.stamp_off, (int64_t)p.kh * p.kw, p.n_stamp),
                    "stamp outside its buffer");
    }
    int64_t n_rows = 0;
    for (int32_t i = 0; i < p.n_sources; ++i) {
        const smi_measure_source &s = p.sources[i];
        SMI_REQUIRE(s.fh > 0 && s.fw > 0 && s.fh <= kMaxCoord && s.fw <= kMaxCoord, "frame extent");
        SMI_REQUIRE(s.h > 0 && s.w > 0 && s.h <= kMaxExtent && s.w <= kMaxExtent, "box extent");
        SMI_REQUIRE(s.y0 >= -kMaxCoord && s.y0 <= kMaxCoord && s.x0 >= -kMaxCoord &&
                        s.x0 <= kMaxCoord, "box origin");
        SMI_REQUIRE(s.n_comp >= 1 && s.comp0 >= 0 && s.n_comp <= p.n_components - s.comp0,
                    "component range");
        SMI_REQUIRE(s.n_band >= 0 && s.band0 >= 0 && s.n_band <= p.n_bands - s.band0,
                    "band range");
        for (int32_t c = s.comp0; c < s.comp0 + s.n_comp; ++c) {
            const smi_measure_component &d = p.comps[c];
            SMI_REQUIRE(d.y0 >= s.y0 && d.x0 >= s.x0 && d.h <= s.h - (d.y0 - s.y0) &&
                            d.w <= s.w - (d.x0 - s.x0), "a component's box leaves its source's");
        }
        for (int32_t b = s.band0; b < s.band0 + s.n_band; ++b)
            SMI_REQUIRE(in_buffer(p.bands[b].weight_off, (int64_t)s.fh * s.fw, p.n_weight),
                        "weights outside their buffer");
        const int tiles = tiles_of(region_of(s, p.kh, p.kw));
        for (int32_t b = 0; b < s.n_band; ++b) {
            rows->push_back((int64_t)(work->size() / 3));
            rows->push_back(tiles);
            for (int t = 0; t < tiles; ++t) work->push_back(i), work->push_back(t), work->push_back(b);
            SMI_REQUIRE(work->size() / 3 <= (size_t)INT32_MAX, "too many tiles for one launch");
        }
        n_rows += s.n_band;
    }
    SMI_REQUIRE((int64_t)p.n_sources * p.C * kRecord <= n_record, "record buffer too small");
    SMI_REQUIRE(n_rows * kRendered <= n_rendered, "rendered buffer too small");
    return SMI_OK;
}

// milliseconds the three launches of this host thread's last call took on the device
thread_local double g_last_launch_ms[3] = {0, 0, 0};

int measure_sources(const Plan &p, int32_t device, double *records, int64_t n_record,
                    double *rendered, int64_t n_rendered) {
    SMI_REQUIRE((records || !n_record) && (rendered || !n_rendered), "null output buffer");
    std::vector<int32_t> work;
    std::vector<int64_t> rows;
    int rc = check_plan(p, n_record, n_rendered, &work, &rows);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available");
        return SMI_ERR_NO_DEVICE;
    }
    SMI_REQUIRE(device >= 0 && device < ndev, "device index");
    if (p.n_sources == 0) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    const size_t n_work = work.size() / 3, n_rows = rows.size() / 2;
    const size_t need_record = (size_t)p.n_sources * p.C * kRecord;
    DevBuf<smi_measure_source> d_sources;
    DevBuf<smi_measure_component> d_comps;
    DevBuf<smi_measure_band> d_bands;
    DevBuf<double> d_seds, d_morphs, d_records, d_part, d_rendered;
    DevBuf<float> d_stamps, d_weights;
    DevBuf<int32_t> d_work;
    DevBuf<int64_t> d_rows;
    SMI_HIP(d_sources.upload(p.sources, p.n_sources));
    SMI_HIP(d_comps.upload(p.comps, p.n_components));
    SMI_HIP(d_bands.upload(p.bands, p.n_bands));
    SMI_HIP(d_seds.upload(p.seds, p.n_sed));
    SMI_HIP(d_morphs.upload(p.morphs, p.n_morph));
    SMI_HIP(d_stamps.upload(p.stamps, p.n_stamp));
    SMI_HIP(d_weights.upload(p.weights, p.n_weight));
    SMI_HIP(d_work.upload(work.data(), work.size()));
    SMI_HIP(d_rows.upload(rows.data(), rows.size()));
    SMI_HIP(d_records.alloc(need_record));
    SMI_HIP(d_part.alloc(n_work * kRendered));
    SMI_HIP(d_rendered.alloc(n_rows * kRendered));

    MeasureArgs a;
    a.sources = d_sources.p, a.comps = d_comps.p, a.bands = d_bands.p;
    a.seds = d_seds.p, a.morphs = d_morphs.p, a.stamps = d_stamps.p, a.weights = d_weights.p;
    a.work = d_work.p, a.rows = d_rows.p;
    a.records = d_records.p, a.part = d_part.p, a.rendered = d_rendered.p;
    a.n_rows = (int64_t)n_rows, a.kh = p.kh, a.kw = p.kw, a.C = p.C;

    const size_t lds = ((size_t)(kTile + p.kh - 1) * window_pitch(p.kw) + kRendered * kCol) *
                       sizeof(double);
    static size_t configured[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(measure_render_kernel), lds,
                                 configured)))
        return rc;

    Events ev;
    for (hipEvent_t &e : ev.e) SMI_HIP(hipEventCreate(&e));
    SMI_HIP(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(measure_model_kernel, dim3((unsigned)p.n_sources, (unsigned)p.C),
                       dim3(kThreads), 0, 0, a);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipEventRecord(ev.e[1], 0));
    if (n_work) {
        hipLaunchKernelGGL(measure_render_kernel, dim3((unsigned)n_work), dim3(kThreads), lds, 0, a);
        SMI_HIP(hipGetLastError());
    }
    SMI_HIP(hipEventRecord(ev.e[2], 0));
    if (n_rows) {
        hipLaunchKernelGGL(measure_reduce_kernel,
                           dim3((unsigned)((n_rows * kRendered + 255) / 256)), dim3(256), 0, 0, a);
        SMI_HIP(hipGetLastError());
    }
    SMI_HIP(hipEventRecord(ev.e[3], 0));
    // (into buffers of the host's own first: the outputs stay untouched if a copy fails)
    std::vector<double> h_records(need_record), h_rendered(n_rows * kRendered);
    SMI_HIP(hipMemcpy(h_records.data(), d_records.p, need_record * sizeof(double),
                      hipMemcpyDeviceToHost));
    if (n_rows)
        SMI_HIP(hipMemcpy(h_rendered.data(), d_rendered.p, n_rows * kRendered * sizeof(double),
                          hipMemcpyDeviceToHost));
    SMI_HIP(hipEventSynchronize(ev.e[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        SMI_HIP(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
        g_last_launch_ms[k] = ms;
    }
    std::copy(h_records.begin(), h_records.end(), records);
    std::copy(h_rendered.begin(), h_rendered.end(), rendered);
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_measure_sources_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_sources,
                            const smi_measure_source *sources, int32_t n_components,
                            const smi_measure_component *components, int32_t n_bands,
                            const smi_measure_band *bands, const double *seds, int64_t n_sed,
                            const double *morphs, int64_t n_morph, const float *stamps,
                            int64_t n_stamp, const float *weights, int64_t n_weight,
                            double *records, int64_t n_record, double *rendered,
                            int64_t n_rendered) {
    const smi::Plan p = {C, kh, kw, n_sources, sources, n_components, components, n_bands, bands,
                         seds, n_sed, morphs, n_morph, stamps, n_stamp, weights, n_weight};
    return smi::measure_sources(p, device, records, n_record, rendered, n_rendered);
}

int smi_measure_sources_last_launch_ms(double *ms) {
    if (!ms) {
        smi::set_error("null output");
        return SMI_ERR_INVALID;
    }
    for (int k = 0; k < 3; ++k) ms[k] = smi::g_last_launch_ms[k];
    return SMI_OK;
}

}  // extern "C"
