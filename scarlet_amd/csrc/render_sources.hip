// render_blends: the images of a catalogue of blends -- per blend the scene as every observed band
// sees it, the residual and chi^2, per source its own rendering and the flux of the data shared
// out among the sources (reference scarlet/lite/measure.py:65-90) --, three launches per chunk.
//
//   scene    one workgroup of 256 threads per (blend, 16 x 16 tile of its frame, observed band).
//            The window of the band's model channel under the tile's taps is staged in LDS as
//            float64 (window_device.h): every window pixel inside the frame is the sum of the
//            rounded products sed[channel] * morph[y, x] of the blend's components whose box holds
//            it, added to +0 in component order, and zero outside the frame.  Components whose box
//            misses the window and taps that meet no row or column of the frame add exact zeros
//            and are skipped.  Thread (i, j) = (t / 16, t % 16) owns pixel (i, j) of the tile -- a
//            tile row of 16 floats is one 64-byte segment of a store -- and runs the tap loop, R:
//            it writes float32(R), data - float32(R), R itself when the fluxes are asked for, and
//            W (R - D)^2 (D, W widened) into a column of LDS that is summed per segment of 32
//            pixels in pixel order by 8 consecutive lanes, joined by a fixed butterfly: the column
//            sum of measure_sources.hip's render launch.
//   sources  one workgroup per (source, tile of its REGION, observed band): the source's box grown
//            by the stamp's half and clipped to the frame.  Window and tap loop are those of
//            measure_sources.hip's render launch, so R_k has the bits measure_blends sums.  It
//            writes float32(R_k) and, when asked, the flux
//            float32(min(max(R_k, 0) / max(R_tot, 0), 1) * image), 0 where max(R_tot, 0) == 0,
//            with R_tot the float64 scene of the first launch and image = data, or data * (W > 0).
//   reduce   one thread per (blend, observed band) adds the chi^2 of its tiles in tile order.
//
// No atomics, no workgroup waits for another, the order of every sum is a function of the frame,
// the boxes and the stamp shape alone, and every loop bound is a descriptor field
// smi_render_sources_f32 validated on the host before anything is launched (check_plan).
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
constexpr int kSegs = 8, kSegLen = kThreads / kSegs;  // 8 x 32 pixels
constexpr int kCol = kThreads + kSegs;                // doubles of the column in LDS
constexpr int kMaxStamp = 63;                         // side: a window of 78 x 80 doubles, 49 KiB
constexpr int32_t kMaxExtent = 1 << 14;               // sides of a box
constexpr int32_t kMaxCoord = 1 << 24;                // |origins| and frame sides

struct Rect {
    int y0, x0, h, w;
};

// the part of a box that lies in the frame: what of its model is rendered
__host__ __device__ inline Rect in_frame(int y0, int x0, int h, int w, int fh, int fw) {
    Rect r;
    r.y0 = y0 > 0 ? y0 : 0, r.x0 = x0 > 0 ? x0 : 0;
    const int y1 = y0 + h < fh ? y0 + h : fh;
    const int x1 = x0 + w < fw ? x0 + w : fw;
    r.h = y1 > r.y0 ? y1 - r.y0 : 0, r.w = x1 > r.x0 ? x1 - r.x0 : 0;
    return r;
}

// the frame pixels the rendered model can reach: the box grown by the stamp's half, clipped
__host__ __device__ inline Rect region_of(const smi_render_source &s, int fh, int fw, int kh,
                                          int kw) {
    Rect r;
    r.y0 = s.y0 - kh / 2 > 0 ? s.y0 - kh / 2 : 0, r.x0 = s.x0 - kw / 2 > 0 ? s.x0 - kw / 2 : 0;
    const int y1 = s.y0 + s.h + kh / 2 < fh ? s.y0 + s.h + kh / 2 : fh;
    const int x1 = s.x0 + s.w + kw / 2 < fw ? s.x0 + s.w + kw / 2 : fw;
    r.h = y1 > r.y0 ? y1 - r.y0 : 0, r.w = x1 > r.x0 ? x1 - r.x0 : 0;
    return r;
}

__host__ __device__ inline int64_t tiles_of(int h, int w) {
    return (int64_t)((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
}

struct RenderArgs {
    const smi_render_blend *blends;
    const smi_render_source *sources;
    const smi_measure_component *comps;
    const smi_measure_band *bands;
    const double *seds, *morphs;
    const float *stamps, *data, *weights;
    const int32_t *scene_work;   // per workgroup of the scene launch: (blend, tile, band of it)
    const int32_t *source_work;  // per workgroup of the sources launch: (source, tile, band)
    const int64_t *rows;         // per band of the band table: its first workgroup, its tiles
    float *rendered, *residual, *src_rendered, *flux;  // flux: nullptr unless asked for
    double *total;                                     // the float64 scene: nullptr likewise
    double *part, *chi2;
    int64_t n_rows;
    int32_t kh, kw, mask;
};

// model pixel (y, x), frame coordinates, of band `band`: components [comp0, comp0 + n_comp)
__device__ __forceinline__ double model_pixel(const RenderArgs &a, int comp0, int n_comp, int band,
                                              int y, int x) {
    double acc = 0;
    for (int k = 0; k < n_comp; ++k) {
        const smi_measure_component d = a.comps[comp0 + k];
        const int yy = y - d.y0, xx = x - d.x0;
        if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w)
            acc += a.seds[d.sed_off + band] * a.morphs[d.morph_off + (int64_t)yy * d.w + xx];
    }
    return acc;
}

__global__ __launch_bounds__(kThreads) void render_scene_kernel(const RenderArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int kh = a.kh, kw = a.kw;
    const int wh = kTile + kh - 1, ww = kTile + kw - 1, wp = window_pitch(kw);
    double *win = reinterpret_cast<double *>(lds_raw);  // the scene under the tile's taps
    double *col = win + wh * wp;                        // [kCol]

    const int tid = threadIdx.x;
    const int32_t *work = a.scene_work + 3 * (int64_t)blockIdx.x;
    const smi_render_blend bl = a.blends[work[0]];
    const int tile = work[1], b = work[2];
    const smi_measure_band bd = a.bands[bl.band0 + b];
    const int fh = bl.fh, fw = bl.fw;
    const int tiles_x = (fw + kTile - 1) / kTile;
    const int ty0 = (tile / tiles_x) * kTile, tx0 = (tile % tiles_x) * kTile;
    const int th = min(kTile, fh - ty0), tw = min(kTile, fw - tx0);

    // window (r, c) is frame pixel (ty0 - kh / 2 + r, tx0 - kw / 2 + c)
    const int wy0 = ty0 - kh / 2, wx0 = tx0 - kw / 2;
    for (int e = tid; e < wh * ww; e += kThreads) {
        const int r = e / ww, c = e - r * ww;
        const int y = wy0 + r, x = wx0 + c;
        double acc = 0;
        if (y >= 0 && y < fh && x >= 0 && x < fw) {
            for (int k = 0; k < bl.n_comp; ++k) {
                const smi_measure_component d = a.comps[bl.comp0 + k];
                // (the same for every thread: a box that misses the window holds none of its pixels)
                if (d.y0 >= wy0 + wh || d.y0 + d.h <= wy0 || d.x0 >= wx0 + ww || d.x0 + d.w <= wx0)
                    continue;
                const int yy = y - d.y0, xx = x - d.x0;
                if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w)
                    acc += a.seds[d.sed_off + bd.channel] *
                           a.morphs[d.morph_off + (int64_t)yy * d.w + xx];
            }
        }
        win[r * wp + c] = acc;
    }
    __syncthreads();

    const int i = tid / kTile, j = tid % kTile;
    const bool inside = i < th && j < tw;
    int ky_lo, ky_hi, kx_lo, kx_hi;
    tap_range(kh, -wy0, fh, &ky_lo, &ky_hi);
    tap_range(kw, -wx0, fw, &kx_lo, &kx_hi);
    const double R = tap_sum(win, wp, i, j, kh, kw, a.stamps + bd.stamp_off, ky_lo, ky_hi, kx_lo,
                             kx_hi);
    double term = 0;
    if (inside) {
        const int64_t px = (int64_t)(ty0 + i) * fw + tx0 + j;
        const int64_t at = bl.out_off + (int64_t)b * fh * fw + px;
        const float D = a.data[bd.weight_off + px], W = a.weights[bd.weight_off + px];
        const float r32 = (float)R;
        a.rendered[at] = r32;
        a.residual[at] = D - r32;
        if (a.total) a.total[at] = R;
        const double diff = R - (double)D;
        term = (double)W * (diff * diff);
    }
    col[tid + tid / kSegLen] = term;
    __syncthreads();
    if (tid >= 64) return;  // (one wavefront: every lane of it shuffles)
    double sum = 0;
    if (tid < kSegs) {
        const double *u = col + tid * (kSegLen + 1);
        for (int e = 0; e < kSegLen; ++e) sum += u[e];
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    if (tid == 0) a.part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void render_sources_kernel(const RenderArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int kh = a.kh, kw = a.kw;
    const int wh = kTile + kh - 1, ww = kTile + kw - 1, wp = window_pitch(kw);
    double *win = reinterpret_cast<double *>(lds_raw);  // the model under the tile's taps

    const int tid = threadIdx.x;
    const int32_t *work = a.source_work + 3 * (int64_t)blockIdx.x;
    const smi_render_source s = a.sources[work[0]];
    const smi_render_blend bl = a.blends[s.blend];
    const int tile = work[1], b = work[2];
    const smi_measure_band bd = a.bands[bl.band0 + b];
    const int fh = bl.fh, fw = bl.fw;
    const Rect g = region_of(s, fh, fw, kh, kw), box = in_frame(s.y0, s.x0, s.h, s.w, fh, fw);
    const int tiles_x = (g.w + kTile - 1) / kTile;
    const int ty0 = g.y0 + (tile / tiles_x) * kTile, tx0 = g.x0 + (tile % tiles_x) * kTile;
    const int th = min(kTile, g.y0 + g.h - ty0), tw = min(kTile, g.x0 + g.w - tx0);

    const int wy0 = ty0 - kh / 2, wx0 = tx0 - kw / 2;
    for (int e = tid; e < wh * ww; e += kThreads) {
        const int r = e / ww, c = e - r * ww;
        const int y = wy0 + r, x = wx0 + c;
        const bool lit = y >= box.y0 && y < box.y0 + box.h && x >= box.x0 && x < box.x0 + box.w;
        win[r * wp + c] = lit ? model_pixel(a, s.comp0, s.n_comp, bd.channel, y, x) : 0.0;
    }
    __syncthreads();

    const int i = tid / kTile, j = tid % kTile;
    int ky_lo, ky_hi, kx_lo, kx_hi;
    tap_range(kh, box.y0 - wy0, box.h, &ky_lo, &ky_hi);
    tap_range(kw, box.x0 - wx0, box.w, &kx_lo, &kx_hi);
    const double R = tap_sum(win, wp, i, j, kh, kw, a.stamps + bd.stamp_off, ky_lo, ky_hi, kx_lo,
                             kx_hi);
    if (!(i < th && j < tw)) return;
    const int y = ty0 + i, x = tx0 + j;
    const int64_t at = s.out_off + ((int64_t)b * g.h + (y - g.y0)) * g.w + (x - g.x0);
    a.src_rendered[at] = (float)R;
    if (!a.flux) return;
    const int64_t px = (int64_t)y * fw + x;
    const double T = a.total[bl.out_off + (int64_t)b * fh * fw + px];
    const float D = a.data[bd.weight_off + px], W = a.weights[bd.weight_off + px];
    const float image = a.mask ? D * (W > 0.0f ? 1.0f : 0.0f) : D;
    const double num = R < 0 ? 0.0 : R, den = T < 0 ? 0.0 : T;
    double ratio = num / den;
    if (den == 0) ratio = 0;
    if (ratio > 1) ratio = 1;
    a.flux[at] = (float)(ratio * (double)image);
}

__global__ void render_reduce_kernel(const RenderArgs a) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n_rows) return;
    const int64_t first = a.rows[2 * row], n = a.rows[2 * row + 1];
    double sum = 0;
    for (int64_t t = 0; t < n; ++t) sum += a.part[first + t];
    a.chi2[row] = sum;
}

struct Plan {
    int32_t C, kh, kw, flags;
    int32_t n_blends;
    const smi_render_blend *blends;
    int32_t n_sources;
    const smi_render_source *sources;
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
    const float *data;
    int64_t n_data;
    const float *weights;
    int64_t n_weight;
    int64_t n_rendered, n_residual, n_chi2, n_src_rendered, n_flux;
};

// `count` planes of `plane` elements at `off` lie in a buffer of `size` elements
inline bool planes_in_buffer(int64_t off, int64_t count, int64_t plane, int64_t size) {
    if (off < 0 || count < 0 || plane < 0 || off > size) return false;
    return plane == 0 || count <= (size - off) / plane;
}

// Everything a kernel's loop bounds and addresses are made of, before anything is launched.
// scene_work: (blend, tile, band) per workgroup of the scene launch -- a blend's bands one after
// the other, each with its tiles in order --; rows: per band of the table its first workgroup and
// its number of tiles; source_work: (source, tile, band) of the sources launch; n_total: elements
// of the scene cubes of all blends.
int check_plan(const Plan &p, std::vector<int32_t> *scene_work, std::vector<int64_t> *rows,
               std::vector<int32_t> *source_work, int64_t *n_total) {
    const bool want_flux = p.flags & SMI_RENDER_REWEIGHT;
    const bool want_sources = want_flux || (p.flags & SMI_RENDER_SOURCES);
    SMI_REQUIRE(p.C > 0 && p.C <= 65535, "bands");
    SMI_REQUIRE(p.kh > 0 && p.kw > 0 && p.kh % 2 == 1 && p.kw % 2 == 1,
                "the stamp must have odd height and width");
    SMI_REQUIRE(p.kh <= kMaxStamp && p.kw <= kMaxStamp, "stamp beyond the kernel's limit");
    SMI_REQUIRE((p.flags & ~(SMI_RENDER_SOURCES | SMI_RENDER_REWEIGHT | SMI_RENDER_MASK)) == 0,
                "unknown flag");
    SMI_REQUIRE(p.n_blends >= 0 && p.n_sources >= 0 && p.n_components >= 0 && p.n_bands >= 0,
                "negative count");
    SMI_REQUIRE(want_sources || p.n_sources == 0, "sources without SMI_RENDER_SOURCES");
    SMI_REQUIRE(p.n_sed >= 0 && p.n_morph >= 0 && p.n_stamp >= 0 && p.n_data >= 0 &&
                    p.n_weight >= 0 && p.n_rendered >= 0 && p.n_residual >= 0 && p.n_chi2 >= 0 &&
                    p.n_src_rendered >= 0 && p.n_flux >= 0, "negative buffer size");
    SMI_REQUIRE((p.blends || !p.n_blends) && (p.sources || !p.n_sources) &&
                    (p.comps || !p.n_components) && (p.bands || !p.n_bands),
                "null descriptor table");
    SMI_REQUIRE((p.seds || !p.n_sed) && (p.morphs || !p.n_morph) && (p.stamps || !p.n_stamp) &&
                    (p.data || !p.n_data) && (p.weights || !p.n_weight), "null buffer");
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
    SMI_REQUIRE(p.n_bands <= p.n_chi2, "chi2 buffer too small");
    int64_t n_scene = 0, bands_seen = 0;
    *n_total = 0;
    for (int32_t i = 0; i < p.n_blends; ++i) {
        const smi_render_blend &bl = p.blends[i];
        SMI_REQUIRE(bl.fh > 0 && bl.fw > 0 && bl.fh <= kMaxCoord && bl.fw <= kMaxCoord,
                    "frame extent");
        SMI_REQUIRE(bl.n_comp >= 0 && bl.comp0 >= 0 && bl.n_comp <= p.n_components - bl.comp0,
                    "component range");
        // (the bands of the blends tile the band table: chi2 has one entry per band)
        SMI_REQUIRE(bl.n_band >= 0 && bl.band0 == bands_seen && bl.n_band <= p.n_bands - bl.band0,
                    "band range");
        bands_seen += bl.n_band;
        const int64_t plane = (int64_t)bl.fh * bl.fw;
        for (int32_t b = bl.band0; b < bl.band0 + bl.n_band; ++b) {
            SMI_REQUIRE(in_buffer(p.bands[b].weight_off, plane, p.n_weight),
                        "weights outside their buffer");
            SMI_REQUIRE(in_buffer(p.bands[b].weight_off, plane, p.n_data),
                        "data outside their buffer");
        }
        SMI_REQUIRE(planes_in_buffer(bl.out_off, bl.n_band, plane, p.n_rendered),
                    "rendered buffer too small");
        SMI_REQUIRE(planes_in_buffer(bl.out_off, bl.n_band, plane, p.n_residual),
                    "residual buffer too small");
        *n_total = std::max(*n_total, bl.out_off + bl.n_band * plane);
        const int64_t tiles = tiles_of(bl.fh, bl.fw);
        SMI_REQUIRE(tiles <= INT32_MAX && n_scene + tiles * bl.n_band <= INT32_MAX,
                    "too many tiles for one launch");
        for (int32_t b = 0; b < bl.n_band; ++b) {
            rows->push_back(n_scene);
            rows->push_back(tiles);
            for (int32_t t = 0; t < (int32_t)tiles; ++t)
                scene_work->push_back(i), scene_work->push_back(t), scene_work->push_back(b);
            n_scene += tiles;
        }
    }
    SMI_REQUIRE(bands_seen == p.n_bands, "bands that belong to no blend");
    int64_t n_source_work = 0;
    for (int32_t i = 0; i < p.n_sources; ++i) {
        const smi_render_source &s = p.sources[i];
        SMI_REQUIRE(s.blend >= 0 && s.blend < p.n_blends, "blend of a source");
        const smi_render_blend &bl = p.blends[s.blend];
        SMI_REQUIRE(s.h > 0 && s.w > 0 && s.h <= kMaxExtent && s.w <= kMaxExtent, "box extent");
        SMI_REQUIRE(s.y0 >= -kMaxCoord && s.y0 <= kMaxCoord && s.x0 >= -kMaxCoord &&
                        s.x0 <= kMaxCoord, "box origin");
        SMI_REQUIRE(s.n_comp >= 1 && s.comp0 >= bl.comp0 &&
                        s.n_comp <= bl.n_comp - (s.comp0 - bl.comp0),
                    "component range of a source");
        for (int32_t c = s.comp0; c < s.comp0 + s.n_comp; ++c) {
            const smi_measure_component &d = p.comps[c];
            SMI_REQUIRE(d.y0 >= s.y0 && d.x0 >= s.x0 && d.h <= s.h - (d.y0 - s.y0) &&
                            d.w <= s.w - (d.x0 - s.x0), "a component's box leaves its source's");
        }
        const Rect g = region_of(s, bl.fh, bl.fw, p.kh, p.kw);
        const int64_t plane = (int64_t)g.h * g.w;
        SMI_REQUIRE(planes_in_buffer(s.out_off, bl.n_band, plane, p.n_src_rendered),
                    "source rendering outside its buffer");
        SMI_REQUIRE(!want_flux || planes_in_buffer(s.out_off, bl.n_band, plane, p.n_flux),
                    "flux outside its buffer");
        const int64_t tiles = plane ? tiles_of(g.h, g.w) : 0;
        SMI_REQUIRE(n_source_work + tiles * bl.n_band <= INT32_MAX,
                    "too many tiles for one launch");
        for (int32_t b = 0; b < bl.n_band; ++b)
            for (int32_t t = 0; t < (int32_t)tiles; ++t)
                source_work->push_back(i), source_work->push_back(t), source_work->push_back(b);
        n_source_work += tiles * bl.n_band;
    }
    return SMI_OK;
}

int render_sources(const Plan &p, int32_t device, float *rendered, float *residual, double *chi2,
                   float *src_rendered, float *flux, double *launch_ms) {
    const bool want_flux = p.flags & SMI_RENDER_REWEIGHT;
    SMI_REQUIRE((rendered || !p.n_rendered) && (residual || !p.n_residual) &&
                    (chi2 || !p.n_chi2) && (src_rendered || !p.n_src_rendered) &&
                    (flux || !p.n_flux), "null output buffer");
    std::vector<int32_t> scene_work, source_work;
    std::vector<int64_t> rows;
    int64_t n_total = 0;
    int rc = check_plan(p, &scene_work, &rows, &source_work, &n_total);
    if (rc) return rc;
    if ((rc = have_device())) return rc;
    int ndev = 0;
    SMI_HIP(hipGetDeviceCount(&ndev));
    SMI_REQUIRE(device >= 0 && device < ndev, "device index");
    if (launch_ms) launch_ms[0] = launch_ms[1] = launch_ms[2] = 0;
    if (p.n_blends == 0) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    const size_t n_scene = scene_work.size() / 3, n_source = source_work.size() / 3;
    const size_t n_rows = rows.size() / 2;
    // elements of the per-source outputs the plan addresses
    size_t n_src_out = 0;
    for (int32_t i = 0; i < p.n_sources; ++i) {
        const smi_render_source &s = p.sources[i];
        const smi_render_blend &bl = p.blends[s.blend];
        const Rect g = region_of(s, bl.fh, bl.fw, p.kh, p.kw);
        n_src_out = std::max(n_src_out, (size_t)(s.out_off + (int64_t)bl.n_band * g.h * g.w));
    }
    DevBuf<smi_render_blend> d_blends;
    DevBuf<smi_render_source> d_sources;
    DevBuf<smi_measure_component> d_comps;
    DevBuf<smi_measure_band> d_bands;
    DevBuf<double> d_seds, d_morphs, d_total, d_part, d_chi2;
    DevBuf<float> d_stamps, d_data, d_weights, d_rendered, d_residual, d_src, d_flux;
    DevBuf<int32_t> d_scene_work, d_source_work;
    DevBuf<int64_t> d_rows;
    SMI_HIP(d_blends.upload(p.blends, p.n_blends));
    SMI_HIP(d_sources.upload(p.sources, p.n_sources));
    SMI_HIP(d_comps.upload(p.comps, p.n_components));
    SMI_HIP(d_bands.upload(p.bands, p.n_bands));
    SMI_HIP(d_seds.upload(p.seds, p.n_sed));
    SMI_HIP(d_morphs.upload(p.morphs, p.n_morph));
    SMI_HIP(d_stamps.upload(p.stamps, p.n_stamp));
    SMI_HIP(d_data.upload(p.data, p.n_data));
    SMI_HIP(d_weights.upload(p.weights, p.n_weight));
    SMI_HIP(d_scene_work.upload(scene_work.data(), scene_work.size()));
    SMI_HIP(d_source_work.upload(source_work.data(), source_work.size()));
    SMI_HIP(d_rows.upload(rows.data(), rows.size()));
    SMI_HIP(d_rendered.alloc(n_total));
    SMI_HIP(d_residual.alloc(n_total));
    SMI_HIP(d_part.alloc(n_scene));
    SMI_HIP(d_chi2.alloc(n_rows));
    SMI_HIP(d_src.alloc(n_src_out));
    if (want_flux) {
        SMI_HIP(d_total.alloc(n_total));
        SMI_HIP(d_flux.alloc(n_src_out));
        if (n_src_out) SMI_HIP(hipMemsetAsync(d_flux.p, 0, n_src_out * sizeof(float), 0));
    }
    // (elements between the cubes the tables address, if any, come back as zeros)
    if (n_total) {
        SMI_HIP(hipMemsetAsync(d_rendered.p, 0, n_total * sizeof(float), 0));
        SMI_HIP(hipMemsetAsync(d_residual.p, 0, n_total * sizeof(float), 0));
    }
    if (n_src_out) SMI_HIP(hipMemsetAsync(d_src.p, 0, n_src_out * sizeof(float), 0));

    RenderArgs a;
    a.blends = d_blends.p, a.sources = d_sources.p, a.comps = d_comps.p, a.bands = d_bands.p;
    a.seds = d_seds.p, a.morphs = d_morphs.p, a.stamps = d_stamps.p;
    a.data = d_data.p, a.weights = d_weights.p;
    a.scene_work = d_scene_work.p, a.source_work = d_source_work.p, a.rows = d_rows.p;
    a.rendered = d_rendered.p, a.residual = d_residual.p, a.src_rendered = d_src.p;
    a.flux = d_flux.p, a.total = d_total.p;  // (nullptr unless the fluxes are asked for)
    a.part = d_part.p, a.chi2 = d_chi2.p;
    a.n_rows = (int64_t)n_rows, a.kh = p.kh, a.kw = p.kw;
    a.mask = (p.flags & SMI_RENDER_MASK) ? 1 : 0;

    const size_t lds =
        ((size_t)(kTile + p.kh - 1) * window_pitch(p.kw) + kCol) * sizeof(double);
    static size_t scene_configured[kMaxDevices] = {}, sources_configured[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(render_scene_kernel), lds,
                                 scene_configured)))
        return rc;
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(render_sources_kernel), lds,
                                 sources_configured)))
        return rc;

    Events ev;
    for (hipEvent_t &e : ev.e) SMI_HIP(hipEventCreate(&e));
    SMI_HIP(hipEventRecord(ev.e[0], 0));
    if (n_scene) {
        hipLaunchKernelGGL(render_scene_kernel, dim3((unsigned)n_scene), dim3(kThreads), lds, 0, a);
        SMI_HIP(hipGetLastError());
    }
    SMI_HIP(hipEventRecord(ev.e[1], 0));
    if (n_source) {
        hipLaunchKernelGGL(render_sources_kernel, dim3((unsigned)n_source), dim3(kThreads), lds, 0,
                           a);
        SMI_HIP(hipGetLastError());
    }
    SMI_HIP(hipEventRecord(ev.e[2], 0));
    if (n_rows) {
        hipLaunchKernelGGL(render_reduce_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256),
                           0, 0, a);
        SMI_HIP(hipGetLastError());
    }
    SMI_HIP(hipEventRecord(ev.e[3], 0));
    SMI_HIP(hipEventSynchronize(ev.e[3]));
    if (launch_ms)
        for (int k = 0; k < 3; ++k) {
            float ms = 0;
            SMI_HIP(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
            launch_ms[k] = ms;
        }
    // (the launches are over and sound: from here on the outputs are written)
    if (n_total) {
        SMI_HIP(hipMemcpy(rendered, d_rendered.p, n_total * sizeof(float), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(residual, d_residual.p, n_total * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (n_rows) SMI_HIP(hipMemcpy(chi2, d_chi2.p, n_rows * sizeof(double), hipMemcpyDeviceToHost));
    if (n_src_out) {
        SMI_HIP(hipMemcpy(src_rendered, d_src.p, n_src_out * sizeof(float), hipMemcpyDeviceToHost));
        if (want_flux)
            SMI_HIP(hipMemcpy(flux, d_flux.p, n_src_out * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_render_sources_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t flags,
                           int32_t n_blends, const smi_render_blend *blends, int32_t n_sources,
                           const smi_render_source *sources, int32_t n_components,
                           const smi_measure_component *components, int32_t n_bands,
                           const smi_measure_band *bands, const double *seds, int64_t n_sed,
                           const double *morphs, int64_t n_morph, const float *stamps,
                           int64_t n_stamp, const float *data, int64_t n_data,
                           const float *weights, int64_t n_weight, float *rendered,
                           int64_t n_rendered, float *residual, int64_t n_residual, double *chi2,
                           int64_t n_chi2, float *source_rendered, int64_t n_source_rendered,
                           float *flux, int64_t n_flux, double *launch_ms) {
    const smi::Plan p = {C, kh, kw, flags, n_blends, blends, n_sources, sources, n_components,
                         components, n_bands, bands, seds, n_sed, morphs, n_morph, stamps, n_stamp,
                         data, n_data, weights, n_weight, n_rendered, n_residual, n_chi2,
                         n_source_rendered, n_flux};
    return smi::render_sources(p, device, rendered, residual, chi2, source_rendered, flux,
                               launch_ms);
}

}  // extern "C"
