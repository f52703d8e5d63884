// The tile of lite.weight_blends, shared by reweight.hip (the fluxes) and lite_measure.hip (the
// fluxes' sums): a workgroup renders one tile of a rectangle plus the (kh - 1, kw - 1) halo of
// the stamp into LDS -- every pixel starts at 0 and adds sed[band] * morph of the components
// whose rectangle holds it, in order -- and runs the tap loop of the reference's apply_filter
// (operators_pybind11.cc:39-56) from there: accumulator from 0, taps in row-major order, one
// rounded multiply and one rounded add per tap.  A halo pixel no component covers is an exact 0,
// and `acc + (+-0) == acc` for an accumulator that started at +0, so the zero-filled halo gives
// the bits the reference gets by skipping taps that leave its array (finite stamps).
//
//   totals   rectangle = the frame of a blend, components = the blend's, clipped to the
//            frame by the plan; result max(.., 0) -> `total`
//   sources  rectangle = the part of the source's grown box inside the frame, components =
//            the source's, unclipped; result max(.., 0) / total with the two ratio rules,
//            times the masked image
//
// Also the host side both entry points share: the validation of a plan (every loop bound and
// offset of the kernels is a descriptor field checked here) and the upload of its buffers.
#pragma once

#include <algorithm>

#include "common.h"
#include "rounded_math.h"

namespace smi {
namespace reweight_tile {

constexpr int kTileY = 32, kTileX = 32;  // outputs of a workgroup: 256 threads x 4 along x
constexpr int kPerThread = 4;
constexpr int kThreads = 256;
// Dynamic LDS a launch may ask for without hipFuncSetAttribute.  Halo + stamp of the largest
// difference kernel of the reference's scenes (43 x 43) in float64 take 58 KiB; stamps beyond
// the budget are refused here and take the per-blend path in lite/measure.py.
constexpr size_t kLdsBudget = 64 * 1024;

// row pitch of the halo in elements: odd, so that the 8 rows x 8 four-pixel groups of a
// wavefront fall on different LDS banks (row r shifts the group addresses 4 t by r * pitch)
__host__ __device__ inline int halo_pitch(int kw) { return (kTileX + kw - 1) | 1; }
inline size_t lds_elems(int kh, int kw) {
    return (size_t)(kTileY + kh - 1) * halo_pitch(kw) + (size_t)kh * kw;
}

template <typename T>
struct ReweightArgs {
    const smi_reweight_blend *blends;
    const smi_reweight_source *sources;
    const smi_reweight_component *comps;
    const int32_t *work;  // per workgroup (item, tile): item = blend (totals) or source
    const T *images, *stamps, *seds, *morphs;
    T *total;  // laid out like `images`
    T *out;
    int32_t kh, kw;
};

// what a thread knows about its workgroup's tile and its own four pixels in it
struct Tile {
    smi_reweight_blend bl;
    int ry0, rx0, rh, rw;  // rectangle of the item in frame coordinates
    int ty0, tx0, th, tw;  // the tile inside the rectangle
    int oy, ox;            // the thread's row and first column inside the tile
    int band;
    int64_t out_off;       // sources: the item's cube in `out`
    bool active;           // the thread has a pixel inside the tile
};

// Stages halo and stamp of the workgroup's tile in `lds` and runs the tap loop: m[j] =
// max(model, 0) at (oy, ox + j).  Every thread of the workgroup calls it (it holds a barrier);
// the m of a thread that is not `active`, and m[j] at ox + j >= tw, are not set.
template <typename T, bool kSources>
__device__ __forceinline__ void tile_model(const ReweightArgs<T> &a, unsigned char *lds, Tile &t,
                                           T (&m)[kPerThread]) {
    T *halo = reinterpret_cast<T *>(lds);
    const int kh = a.kh, kw = a.kw, pitch = halo_pitch(kw);
    T *stamp = halo + (kTileY + kh - 1) * pitch;

    const int tid = threadIdx.x;
    const int item = a.work[2 * blockIdx.x], tile = a.work[2 * blockIdx.x + 1];
    const int band = blockIdx.y;
    // rectangle of this launch's item in frame coordinates, and its components
    int b = item, ry0 = 0, rx0 = 0, rh = 0, rw = 0, c0 = 0, nc = 0;
    int64_t out_off = 0;
    if (kSources) {
        const smi_reweight_source s = a.sources[item];
        b = s.blend, ry0 = s.y0, rx0 = s.x0, rh = s.h, rw = s.w, c0 = s.comp0, nc = s.n_comp;
        out_off = s.out_off;
    }
    const smi_reweight_blend bl = a.blends[b];
    if (!kSources) rh = bl.h, rw = bl.w, c0 = bl.comp0, nc = bl.n_comp;

    const int tiles_x = (rw + kTileX - 1) / kTileX;
    const int ty0 = (tile / tiles_x) * kTileY, tx0 = (tile % tiles_x) * kTileX;
    const int th = min(kTileY, rh - ty0), tw = min(kTileX, rw - tx0);
    // staged part of the halo: the rows the tile's outputs read, the columns its threads read
    const int hh = th + kh - 1;
    const int hw = ((tw + kPerThread - 1) & ~(kPerThread - 1)) + kw - 1;

    const T *kern = a.stamps + bl.stamp_off + (int64_t)band * kh * kw;
    for (int i = tid; i < kh * kw; i += kThreads) stamp[i] = kern[i];

    const int fy0 = ry0 + ty0 - kh / 2, fx0 = rx0 + tx0 - kw / 2;  // frame position of halo[0][0]
    for (int idx = tid; idx < hh * hw; idx += kThreads) {
        const int i = idx / hw, j = idx - i * hw;
        const int y = fy0 + i, x = fx0 + j;
        T v = 0;
        for (int c = c0; c < c0 + nc; ++c) {
            const smi_reweight_component d = a.comps[c];  // wave-uniform: scalar loads
            const int yy = y - d.y0, xx = x - d.x0;
            if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w)
                v = add_rn(v, mul_rn(a.seds[d.sed_off + band],
                                     a.morphs[d.morph_off + (int64_t)yy * d.stride + xx]));
        }
        halo[i * pitch + j] = v;
    }
    __syncthreads();

    const int oy = tid >> 3, ox = (tid & 7) * kPerThread;
    t.bl = bl;
    t.ry0 = ry0, t.rx0 = rx0, t.rh = rh, t.rw = rw;
    t.ty0 = ty0, t.tx0 = tx0, t.th = th, t.tw = tw;
    t.oy = oy, t.ox = ox, t.band = band, t.out_off = out_off;
    t.active = oy < th && ox < tw;
    if (!t.active) return;
    // result[y][x] = sum over (ky, kx) ascending of K[ky][kx] * image[y - (ky - kh / 2)][x - (kx -
    // kw / 2)]: halo row oy + (kh - 1 - ky), column ox + j + (kw - 1 - kx)
    T acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    for (int ky = 0; ky < kh; ++ky) {
        const T *row = halo + (oy + kh - 1 - ky) * pitch + ox + (kw - 1);
        const T *k = stamp + ky * kw;
        T w1 = row[1], w2 = row[2], w3 = row[3];
#pragma unroll 4
        for (int kx = 0; kx < kw; ++kx) {
            const T w0 = row[-kx], kv = k[kx];
            acc0 = add_rn(acc0, mul_rn(kv, w0));
            acc1 = add_rn(acc1, mul_rn(kv, w1));
            acc2 = add_rn(acc2, mul_rn(kv, w2));
            acc3 = add_rn(acc3, mul_rn(kv, w3));
            w3 = w2, w2 = w1, w1 = w0;
        }
    }
    m[0] = acc0 < 0 ? (T)0 : acc0;
    m[1] = acc1 < 0 ? (T)0 : acc1;
    m[2] = acc2 < 0 ? (T)0 : acc2;
    m[3] = acc3 < 0 ? (T)0 : acc3;
}

// position of pixel j of an active thread in the [C][h][w] planes of its blend
__device__ __forceinline__ int64_t frame_at(const Tile &t, int j) {
    return t.bl.image_off + ((int64_t)t.band * t.bl.h + (t.ry0 + t.ty0 + t.oy)) * t.bl.w + t.rx0 +
           t.tx0 + t.ox + j;
}
// ... and in the [C][h][w] cube of its source
__device__ __forceinline__ int64_t cube_at(const Tile &t, int j) {
    return t.out_off + ((int64_t)t.band * t.rh + (t.ty0 + t.oy)) * t.rw + t.tx0 + t.ox + j;
}

// the share of the image a source gets at a pixel: model / total with the two ratio rules
template <typename T>
__device__ __forceinline__ T source_flux(T m, T total, T image) {
    T r = div_rn(m, total);
    if (total == 0) r = 0;
    if (r > 1) r = 1;
    return mul_rn(r, image);
}

// the whole pass of one workgroup: totals -> a.total, sources -> a.out
template <typename T, bool kSources>
__device__ __forceinline__ void tile_pass(const ReweightArgs<T> &a, unsigned char *lds) {
    Tile t;
    T m[kPerThread];
    tile_model<T, kSources>(a, lds, t, m);
    if (!t.active) return;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (t.ox + j >= t.tw) continue;
        const int64_t at = frame_at(t, j);
        if (!kSources)
            a.total[at] = m[j];
        else
            a.out[cube_at(t, j)] = source_flux(m[j], a.total[at], a.images[at]);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int32_t kMaxCoord = 1 << 24;  // |origins| and extents: sums of a few stay in int32

// every component of [comp0, comp0 + n): inside the table, and its rectangle inside its buffers
inline int check_components(const smi_reweight_component *comps, int32_t n_components,
                            int32_t comp0, int32_t n, int32_t C, int64_t n_sed, int64_t n_morph) {
    SMI_REQUIRE(comp0 >= 0 && n >= 0 && n <= n_components - comp0, "component range");
    for (int32_t c = comp0; c < comp0 + n; ++c) {
        const smi_reweight_component &d = comps[c];
        SMI_REQUIRE(d.h >= 0 && d.w >= 0 && d.h <= kMaxCoord && d.w <= kMaxCoord && d.stride >= d.w,
                    "component extent");
        SMI_REQUIRE(d.y0 >= -kMaxCoord && d.y0 <= kMaxCoord && d.x0 >= -kMaxCoord &&
                        d.x0 <= kMaxCoord, "component origin");
        SMI_REQUIRE(d.sed_off >= 0 && d.sed_off <= n_sed - C, "spectrum outside its buffer");
        if (d.h > 0 && d.w > 0)
            SMI_REQUIRE(d.morph_off >= 0 && d.morph_off <= n_morph &&
                            (int64_t)(d.h - 1) * d.stride + d.w <= n_morph - d.morph_off,
                        "morphology outside its buffer");
    }
    return SMI_OK;
}

// The plan of smi_reweight_* / smi_lite_measure_*: the tables and the input buffers.
template <typename T>
struct Plan {
    int32_t C, kh, kw;
    int32_t n_blends;
    const smi_reweight_blend *blends;
    int32_t n_sources;
    const smi_reweight_source *sources;
    int32_t n_components;
    const smi_reweight_component *comps;
    const T *images;
    int64_t n_image;
    const T *stamps;
    int64_t n_stamp;
    const T *seds;
    int64_t n_sed;
    const T *morphs;
    int64_t n_morph;
};

// Validates a plan and lists the (item, tile) pairs of the two launches.  `cubes`: every
// source's [C][h][w] result must lie inside a buffer of n_out elements.
template <typename T>
int check_plan(const Plan<T> &p, bool cubes, int64_t n_out, std::vector<int32_t> *work_total,
               std::vector<int32_t> *work_src, size_t *lds_bytes) {
    const int32_t C = p.C, kh = p.kh, kw = p.kw;
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_REQUIRE(kh > 0 && kw > 0 && kh % 2 == 1 && kw % 2 == 1 && kh <= 4095 && kw <= 4095,
                "the stamp must have odd height and width");
    const size_t lds = lds_elems(kh, kw) * sizeof(T);
    SMI_REQUIRE(lds <= kLdsBudget, "stamp too large for the LDS tile");
    *lds_bytes = lds;
    SMI_REQUIRE(p.n_blends >= 0 && p.n_sources >= 0 && p.n_components >= 0, "negative count");
    SMI_REQUIRE(p.n_image >= 0 && p.n_stamp >= 0 && p.n_sed >= 0 && p.n_morph >= 0 && n_out >= 0,
                "negative buffer size");
    SMI_REQUIRE((p.blends || !p.n_blends) && (p.sources || !p.n_sources) &&
                    (p.comps || !p.n_components), "null descriptor table");
    SMI_REQUIRE((p.images || !p.n_image) && (p.stamps || !p.n_stamp) && (p.seds || !p.n_sed) &&
                    (p.morphs || !p.n_morph), "null buffer");
    const int64_t stamp_elems = (int64_t)C * kh * kw;
    for (int32_t b = 0; b < p.n_blends; ++b) {
        const smi_reweight_blend &bl = p.blends[b];
        SMI_REQUIRE(bl.h > 0 && bl.w > 0 && bl.h <= kMaxCoord && bl.w <= kMaxCoord, "frame extent");
        const int64_t cube = (int64_t)C * bl.h * bl.w;
        SMI_REQUIRE(bl.image_off >= 0 && bl.image_off <= p.n_image &&
                        cube <= p.n_image - bl.image_off, "frame outside the image buffer");
        SMI_REQUIRE(bl.stamp_off >= 0 && bl.stamp_off <= p.n_stamp &&
                        stamp_elems <= p.n_stamp - bl.stamp_off, "stamp outside its buffer");
        int rc = check_components(p.comps, p.n_components, bl.comp0, bl.n_comp, C, p.n_sed,
                                  p.n_morph);
        if (rc) return rc;
        for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c) {
            const smi_reweight_component &d = p.comps[c];
            SMI_REQUIRE(d.h == 0 || d.w == 0 || (d.y0 >= 0 && d.x0 >= 0 && d.y0 + d.h <= bl.h &&
                                                 d.x0 + d.w <= bl.w),
                        "a blend's component rectangle leaves the frame");
        }
        const int32_t tiles = ((bl.h + kTileY - 1) / kTileY) * ((bl.w + kTileX - 1) / kTileX);
        for (int32_t t = 0; t < tiles; ++t) work_total->push_back(b), work_total->push_back(t);
    }
    for (int32_t s = 0; s < p.n_sources; ++s) {
        const smi_reweight_source &sr = p.sources[s];
        SMI_REQUIRE(sr.blend >= 0 && sr.blend < p.n_blends, "source of an unknown blend");
        const smi_reweight_blend &bl = p.blends[sr.blend];
        SMI_REQUIRE(sr.h > 0 && sr.w > 0 && sr.y0 >= 0 && sr.x0 >= 0 && sr.h <= bl.h - sr.y0 &&
                        sr.w <= bl.w - sr.x0, "a source's rectangle leaves the frame");
        const int64_t cube = (int64_t)C * sr.h * sr.w;
        if (cubes)
            SMI_REQUIRE(sr.out_off >= 0 && sr.out_off <= n_out && cube <= n_out - sr.out_off,
                        "a source's result outside the output buffer");
        int rc = check_components(p.comps, p.n_components, sr.comp0, sr.n_comp, C, p.n_sed,
                                  p.n_morph);
        if (rc) return rc;
        const int32_t tiles = ((sr.h + kTileY - 1) / kTileY) * ((sr.w + kTileX - 1) / kTileX);
        for (int32_t t = 0; t < tiles; ++t) work_src->push_back(s), work_src->push_back(t);
    }
    SMI_REQUIRE(work_total->size() / 2 <= (size_t)INT32_MAX &&
                    work_src->size() / 2 <= (size_t)INT32_MAX, "too many tiles for one launch");
    return SMI_OK;
}

inline int check_device(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available");
        return SMI_ERR_NO_DEVICE;
    }
    SMI_REQUIRE(device >= 0 && device < ndev, "device index");
    return SMI_OK;
}

// A validated plan on the current device: tables, work lists, inputs, `total`; `out` of n_out
// elements, zeroed, when n_out >= 0.
template <typename T>
struct Uploaded {
    DevBuf<smi_reweight_blend> blends;
    DevBuf<smi_reweight_source> sources;
    DevBuf<smi_reweight_component> comps;
    DevBuf<int32_t> work_total, work_src;
    DevBuf<T> images, stamps, seds, morphs, total, out;

    int upload(const Plan<T> &p, const std::vector<int32_t> &wt, const std::vector<int32_t> &ws,
               int64_t n_out, ReweightArgs<T> *a) {
        SMI_HIP(blends.upload(p.blends, p.n_blends));
        SMI_HIP(sources.upload(p.sources, p.n_sources));
        SMI_HIP(comps.upload(p.comps, p.n_components));
        SMI_HIP(work_total.upload(wt.data(), wt.size()));
        SMI_HIP(work_src.upload(ws.data(), ws.size()));
        SMI_HIP(images.upload(p.images, p.n_image));
        SMI_HIP(stamps.upload(p.stamps, p.n_stamp));
        SMI_HIP(seds.upload(p.seds, p.n_sed));
        SMI_HIP(morphs.upload(p.morphs, p.n_morph));
        SMI_HIP(total.alloc(p.n_image));
        if (n_out >= 0) {
            SMI_HIP(out.alloc(n_out));
            // (every element of a validated plan's output is written by exactly one thread; the
            // plan of lite/measure.py packs the results back to back)
            SMI_HIP(hipMemset(out.p, 0, (size_t)std::max<int64_t>(n_out, 1) * sizeof(T)));
        }
        a->blends = blends.p, a->sources = sources.p, a->comps = comps.p;
        a->images = images.p, a->stamps = stamps.p, a->seds = seds.p, a->morphs = morphs.p;
        a->total = total.p, a->out = out.p, a->kh = p.kh, a->kw = p.kw;
        a->work = nullptr;
        return SMI_OK;
    }
};

}  // namespace reweight_tile
}  // namespace smi
