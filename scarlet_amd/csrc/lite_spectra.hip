// lite.fit_spectra_blends: the normal equations of scarlet.lite's joint spectrum fit
// (reference scarlet/lite/initialization.py:140-186, multifit_seds) for a catalogue of blends,
// two launches per chunk.
//
// Per blend and band the design has one column per component: its morphology, zero outside its
// own box, convolved ("same", evaluated on the union box of all component boxes) with the
// band's stamp.  The data is the image on the union box, zero outside the frame.  The launches
// give G = A^T A (K x K) and r = A^T d in float64; the minimum-norm solve is the host's.
//
//   tiles   one workgroup per (blend, 16 x 16 tile of the union box, band).  A component is
//           PRESENT on a tile when its box grown by the stamp's half meets the tile: only then
//           can its column be non-zero there.  The workgroup keeps the columns of the present
//           components and the data column in LDS.  A column is made with one thread per
//           pixel: the part of the morphology under the tile's taps is staged in LDS as
//           float64, zeros around it, and every thread runs the tap loop over it, the taps
//           themselves read at wave-uniform addresses.  Then the sums of every pair of
//           columns: 8 consecutive lanes take the 8 segments of 32 pixels of one pair, each
//           adds its segment in pixel order, and the 8 are added by a fixed butterfly.  It
//           writes the tile's full G and r, zeros for what is not present, so a pair whose
//           grown boxes never share a pixel is an exact 0 and nothing has to be cleared first.
//   reduce  one thread per entry adds the tiles of its blend in tile order.
//
// A column is 256 doubles with one double of padding after every 32: 264 doubles, i.e.
// 16 (mod 64) LDS banks per column and 2 per segment, so the 4 pairs x 8 segments of a
// half-wavefront read 32 different 8-byte bank pairs (or the same address).
//
// No atomics, no workgroup waits for another, every sum has a fixed order that depends on the
// blend alone, and every loop bound is a descriptor field smi_lite_spectra_* validated on the
// host before anything is launched.
#include <algorithm>

#include "common.h"
#include "window_device.h"

namespace smi {
namespace {

using window::kTile;  // the tile, its window and the tap loop: window_device.h
using window::tap_range;
using window::tap_sum;
using window::uniform;
using window::window_pitch;
constexpr int kThreads = kTile * kTile;
constexpr int kSegs = 8, kSegLen = kThreads / kSegs;  // 8 x 32 pixels
constexpr int kPitch = kThreads + kSegs;              // doubles of a column in LDS
constexpr int kMaxComponents = 64;                    // of a blend: one wavefront finds the present
constexpr int kMaxPresent = 32;                       // on one tile: 33 columns, 68 KiB
constexpr int kMaxStamp = 63;                         // side: a window of 78 x 80 doubles, 49 KiB
constexpr int32_t kMaxExtent = 4096;                  // sides of a union box and of a morphology
constexpr int32_t kMaxCoord = 1 << 24;                // |origins| and frame sides
constexpr size_t kLdsLimit = 160 * 1024 - 1024;       // of a CU, less the static arrays below

struct Tile {
    int y0, x0, h, w;  // in union-box coordinates
};

__host__ __device__ inline Tile tile_of(const smi_lite_spectra_blend &bl, int tile) {
    const int tiles_x = (bl.fw + kTile - 1) / kTile;
    Tile t;
    t.y0 = (tile / tiles_x) * kTile, t.x0 = (tile % tiles_x) * kTile;
    t.h = bl.fh - t.y0 < kTile ? bl.fh - t.y0 : kTile;
    t.w = bl.fw - t.x0 < kTile ? bl.fw - t.x0 : kTile;
    return t;
}

inline int32_t tiles_of(const smi_lite_spectra_blend &bl) {
    return ((bl.fh + kTile - 1) / kTile) * ((bl.fw + kTile - 1) / kTile);
}

// does the component's box, grown by the stamp's half, meet the tile?
__host__ __device__ inline bool present_on(const smi_lite_spectra_blend &bl,
                                           const smi_lite_spectra_component &d, const Tile &t,
                                           int kh, int kw) {
    if (d.h <= 0 || d.w <= 0) return false;
    const int cy = d.y0 - bl.y0, cx = d.x0 - bl.x0;
    return cy - kh / 2 < t.y0 + t.h && cy + d.h + kh / 2 > t.y0 && cx - kw / 2 < t.x0 + t.w &&
           cx + d.w + kw / 2 > t.x0;
}

template <typename T>
struct SpectraArgs {
    const smi_lite_spectra_blend *blends;
    const smi_lite_spectra_component *comps;
    const int32_t *work;      // per workgroup (blend, tile)
    const int64_t *part_off;  // per blend: its tiles' sums in `part`, [tile][band][K K + K]
    const T *images, *morphs;
    const double *stamps;
    double *part, *out;
    int32_t kh, kw, C;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void spectra_tile_kernel(const SpectraArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int slot_of[kMaxComponents];  // component -> its column, -1: not present
    __shared__ int comp_of[kMaxComponents];  // column -> component
    __shared__ int n_present;
    const int kh = a.kh, kw = a.kw;
    const int wh = kTile + kh - 1, ww = kTile + kw - 1, wp = window_pitch(kw);
    double *win = reinterpret_cast<double *>(lds_raw);  // a morphology under the tile's taps
    double *col = win + wh * wp;

    const int tid = threadIdx.x, band = blockIdx.y;
    const int b = a.work[2 * blockIdx.x], tile = a.work[2 * blockIdx.x + 1];
    const smi_lite_spectra_blend bl = a.blends[b];
    const int K = bl.n_comp;
    const Tile t = tile_of(bl, tile);

    // (taps are read at wave-uniform addresses, before the kernel's first store)
    const double *kern = a.stamps + bl.stamp_off + (int64_t)band * kh * kw;
    if (tid < 64) {  // the first wavefront: present components keep their order
        bool hit = false;
        if (tid < K) hit = present_on(bl, a.comps[bl.comp0 + tid], t, kh, kw);
        const unsigned long long mask = __ballot(hit);
        const int slot = __popcll(mask & ((1ull << tid) - 1ull));
        if (tid < K) slot_of[tid] = hit ? slot : -1;
        if (hit) comp_of[slot] = tid;
        if (tid == 0) n_present = __popcll(mask);
    }
    __syncthreads();
    // (read from LDS: made wave-uniform for the compiler, so that what follows from them --
    // descriptors, tap ranges, the taps themselves -- stays in scalar registers)
    const int P = uniform(n_present);  // <= kMaxPresent: the host walked the same tiles

    // ---- the columns: thread = pixel
    {
        const int i = tid / kTile, j = tid % kTile;
        const bool inside = i < t.h && j < t.w;
        const int at = tid + tid / kSegLen;
        const int uy = t.y0 + i, ux = t.x0 + j;
        for (int s = 0; s < P; ++s) {
            const smi_lite_spectra_component d =
                a.comps[bl.comp0 + uniform(comp_of[s])];
            // the morphology on the window of the tile: window (r, c) is union-box pixel
            // (t.y0 - kh / 2 + r, t.x0 - kw / 2 + c), 0 outside the morphology's box
            const int r0 = d.y0 - bl.y0 - (t.y0 - kh / 2), c0 = d.x0 - bl.x0 - (t.x0 - kw / 2);
            const T *m = a.morphs + d.morph_off;
            for (int e = tid; e < wh * ww; e += kThreads) {
                const int r = e / ww, c = e - r * ww;
                const int yy = r - r0, xx = c - c0;
                win[r * wp + c] = (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w)
                                      ? (double)m[(int64_t)yy * d.w + xx] : 0.0;
            }
            __syncthreads();
            // pixel (i, j) = sum over the taps, rows then columns ascending, of K[ky][kx] *
            // window[i + kh - 1 - ky][j + kw - 1 - kx]; the taps under which no pixel of the
            // tile meets the morphology's rows [r0, r0 + h) and columns add exact zeros (finite
            // stamps): skipped
            int ky_lo, ky_hi, kx_lo, kx_hi;
            tap_range(kh, r0, d.h, &ky_lo, &ky_hi);
            tap_range(kw, c0, d.w, &kx_lo, &kx_hi);
            const double acc = tap_sum(win, wp, i, j, kh, kw, kern, ky_lo, ky_hi, kx_lo, kx_hi);
            col[s * kPitch + at] = inside ? acc : 0.0;
            __syncthreads();  // (the window is staged again)
        }
        const int y = bl.y0 + uy, x = bl.x0 + ux;
        double v = 0;
        if (inside && y >= 0 && y < bl.h && x >= 0 && x < bl.w)
            v = (double)a.images[bl.image_off + ((int64_t)band * bl.h + y) * bl.w + x];
        col[P * kPitch + at] = v;
    }
    __syncthreads();

    const int E = K * K + K;
    double *dst = a.part + a.part_off[b] + ((int64_t)tile * a.C + band) * E;
    // ---- exact zeros for what is not present on this tile
    for (int e = tid; e < E; e += kThreads) {
        const bool absent = e < K * K ? (slot_of[e / K] < 0 || slot_of[e % K] < 0)
                                      : slot_of[e - K * K] < 0;
        if (absent) dst[e] = 0.0;
    }
    // ---- the pair sums: item = (column sp, column sq >= sp or the data, segment)
    const int n_items = P * (P + 1) * kSegs;
    for (int base = 0; base < n_items; base += kThreads) {  // (uniform: every lane shuffles)
        const int item = base + tid;
        const int seg = item % kSegs, pair = item / kSegs;
        const int sp = pair / (P + 1), sq = pair % (P + 1);
        const bool active = item < n_items && sq >= sp;
        double acc = 0;
        if (active) {
            const double *u = col + sp * kPitch + seg * (kSegLen + 1);
            const double *v = col + sq * kPitch + seg * (kSegLen + 1);
            for (int i = 0; i < kSegLen; ++i) acc += u[i] * v[i];
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (active && seg == 0) {
            const int gp = comp_of[sp];
            if (sq == P) {
                dst[K * K + gp] = acc;
            } else {
                const int gq = comp_of[sq];
                dst[gp * K + gq] = acc;
                dst[gq * K + gp] = acc;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void spectra_reduce_kernel(const SpectraArgs<T> a) {
    const int b = blockIdx.x, band = blockIdx.y;
    const smi_lite_spectra_blend bl = a.blends[b];
    const int E = bl.n_comp * bl.n_comp + bl.n_comp;
    const int n_tiles = ((bl.fh + kTile - 1) / kTile) * ((bl.fw + kTile - 1) / kTile);
    const double *src = a.part + a.part_off[b] + (int64_t)band * E;
    for (int e = threadIdx.x; e < E; e += kThreads) {
        double s = 0;
        for (int t = 0; t < n_tiles; ++t) s += src[(int64_t)t * a.C * E + e];
        a.out[bl.out_off + (int64_t)band * E + e] = s;
    }
}

template <typename T>
int lite_spectra(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                 const smi_lite_spectra_blend *blends, int32_t n_components,
                 const smi_lite_spectra_component *comps, const T *images, int64_t n_image,
                 const double *stamps, int64_t n_stamp, const T *morphs, int64_t n_morph,
                 double *out, int64_t n_out) {
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_REQUIRE(kh > 0 && kw > 0 && kh % 2 == 1 && kw % 2 == 1,
                "the stamp must have odd height and width");
    SMI_REQUIRE(kh <= kMaxStamp && kw <= kMaxStamp, "stamp beyond the kernel's limit");
    SMI_REQUIRE(n_blends >= 0 && n_components >= 0, "negative count");
    SMI_REQUIRE(n_image >= 0 && n_stamp >= 0 && n_morph >= 0 && n_out >= 0, "negative buffer size");
    SMI_REQUIRE((blends || !n_blends) && (comps || !n_components), "null descriptor table");
    SMI_REQUIRE((images || !n_image) && (stamps || !n_stamp) && (morphs || !n_morph) &&
                    (out || !n_out), "null buffer");
    const int64_t stamp_elems = (int64_t)C * kh * kw;
    std::vector<int32_t> work;
    std::vector<int64_t> part_off(n_blends);
    int64_t n_part = 0;
    int max_present = 0;
    for (int32_t b = 0; b < n_blends; ++b) {
        const smi_lite_spectra_blend &bl = blends[b];
        SMI_REQUIRE(bl.h > 0 && bl.w > 0 && bl.h <= kMaxCoord && bl.w <= kMaxCoord, "frame extent");
        SMI_REQUIRE(bl.fh > 0 && bl.fw > 0 && bl.fh <= kMaxExtent && bl.fw <= kMaxExtent,
                    "union box beyond the extent limit");
        SMI_REQUIRE(bl.y0 >= -kMaxCoord && bl.y0 <= kMaxCoord && bl.x0 >= -kMaxCoord &&
                        bl.x0 <= kMaxCoord, "union box origin");
        SMI_REQUIRE(in_buffer(bl.image_off, (int64_t)C * bl.h * bl.w, n_image),
                    "frame outside the image buffer");
        SMI_REQUIRE(in_buffer(bl.stamp_off, stamp_elems, n_stamp), "stamp outside its buffer");
        SMI_REQUIRE(bl.n_comp >= 1 && bl.n_comp <= kMaxComponents, "components of a blend");
        SMI_REQUIRE(bl.comp0 >= 0 && bl.n_comp <= n_components - bl.comp0, "component range");
        const int64_t E = (int64_t)bl.n_comp * bl.n_comp + bl.n_comp;
        SMI_REQUIRE(in_buffer(bl.out_off, C * E, n_out), "a blend's sums outside the output buffer");
        for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c) {
            const smi_lite_spectra_component &d = comps[c];
            SMI_REQUIRE(d.h >= 0 && d.w >= 0 && d.h <= kMaxExtent && d.w <= kMaxExtent,
                        "component extent");
            SMI_REQUIRE(d.y0 >= -kMaxCoord && d.y0 <= 2 * kMaxCoord && d.x0 >= -kMaxCoord &&
                            d.x0 <= 2 * kMaxCoord, "component origin");
            if (d.h == 0 || d.w == 0) continue;
            SMI_REQUIRE(d.y0 >= bl.y0 && d.x0 >= bl.x0 && d.h <= bl.fh - (d.y0 - bl.y0) &&
                            d.w <= bl.fw - (d.x0 - bl.x0), "a component's box leaves the union box");
            SMI_REQUIRE(in_buffer(d.morph_off, (int64_t)d.h * d.w, n_morph),
                        "morphology outside its buffer");
        }
        const int32_t tiles = tiles_of(bl);
        for (int32_t t = 0; t < tiles; ++t) {
            const Tile tl = tile_of(bl, t);
            int present = 0;
            for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c)
                present += present_on(bl, comps[c], tl, kh, kw);
            SMI_REQUIRE(present <= kMaxPresent, "components present on one tile");
            max_present = std::max(max_present, present);
            work.push_back(b), work.push_back(t);
        }
        part_off[b] = n_part;
        n_part += (int64_t)tiles * C * E;
    }
    SMI_REQUIRE(work.size() / 2 <= (size_t)INT32_MAX, "too many tiles for one launch");
    const size_t lds = ((size_t)(max_present + 1) * kPitch +
                        (size_t)(kTile + kh - 1) * window_pitch(kw)) * sizeof(double);
    SMI_REQUIRE(lds <= kLdsLimit, "columns and window beyond the LDS of a CU");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available");
        return SMI_ERR_NO_DEVICE;
    }
    SMI_REQUIRE(device >= 0 && device < ndev, "device index");
    if (n_blends == 0) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    DevBuf<smi_lite_spectra_blend> d_blends;
    DevBuf<smi_lite_spectra_component> d_comps;
    DevBuf<int32_t> d_work;
    DevBuf<int64_t> d_part_off;
    DevBuf<T> d_images, d_morphs;
    DevBuf<double> d_stamps, d_part, d_out;
    SMI_HIP(d_blends.upload(blends, n_blends));
    SMI_HIP(d_comps.upload(comps, n_components));
    SMI_HIP(d_work.upload(work.data(), work.size()));
    SMI_HIP(d_part_off.upload(part_off.data(), part_off.size()));
    SMI_HIP(d_images.upload(images, n_image));
    SMI_HIP(d_stamps.upload(stamps, n_stamp));
    SMI_HIP(d_morphs.upload(morphs, n_morph));
    SMI_HIP(d_part.alloc(n_part));
    SMI_HIP(d_out.alloc(n_out));
    // (every entry of a blend is written by exactly one thread; the plan of lite/spectra.py
    // packs the blends back to back)
    SMI_HIP(hipMemset(d_out.p, 0, (size_t)std::max<int64_t>(n_out, 1) * sizeof(double)));

    SpectraArgs<T> a;
    a.blends = d_blends.p, a.comps = d_comps.p, a.work = d_work.p, a.part_off = d_part_off.p;
    a.images = d_images.p, a.morphs = d_morphs.p, a.stamps = d_stamps.p;
    a.part = d_part.p, a.out = d_out.p, a.kh = kh, a.kw = kw, a.C = C;
    auto kern = spectra_tile_kernel<T>;
    SMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(work.size() / 2), C), dim3(kThreads), lds, 0, a);
    SMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(spectra_reduce_kernel<T>, dim3(n_blends, C), dim3(kThreads), 0, 0, a);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipMemcpy(out, d_out.p, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost));
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_lite_spectra_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_lite_spectra_blend *blends, int32_t n_components,
                         const smi_lite_spectra_component *components, const float *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp,
                         const float *morphs, int64_t n_morph, double *out, int64_t n_out) {
    return smi::lite_spectra<float>(device, C, kh, kw, n_blends, blends, n_components, components,
                                    images, n_image, stamps, n_stamp, morphs, n_morph, out, n_out);
}
int smi_lite_spectra_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_lite_spectra_blend *blends, int32_t n_components,
                         const smi_lite_spectra_component *components, const double *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp,
                         const double *morphs, int64_t n_morph, double *out, int64_t n_out) {
    return smi::lite_spectra<double>(device, C, kh, kw, n_blends, blends, n_components, components,
                                     images, n_image, stamps, n_stamp, morphs, n_morph, out, n_out);
}

}  // extern "C"
