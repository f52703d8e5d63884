// lite.weight_blends: the flux-conserving reweighting of scarlet.lite (reference
// scarlet/lite/measure.py:39-91) for a catalogue of blends, two launches per chunk.
//
// Both launches run the same kernel: a workgroup renders one tile of a rectangle plus the
// (kh - 1, kw - 1) halo of the stamp into LDS -- every pixel starts at 0 and adds
// sed[band] * morph of the components whose rectangle holds it, in order -- and runs the tap
// loop of the reference's apply_filter (operators_pybind11.cc:39-56) from there: accumulator
// from 0, taps in row-major order, one rounded multiply and one rounded add per tap.  A halo
// pixel no component covers is an exact 0, and `acc + (+-0) == acc` for an accumulator that
// started at +0, so the zero-filled halo gives the bits the reference gets by skipping taps
// that leave its array (finite stamps).
//
//   totals   rectangle = the frame of a blend, components = the blend's, clipped to the
//            frame by the plan; result max(.., 0) -> `total`
//   sources  rectangle = the part of the source's grown box inside the frame, components =
//            the source's, unclipped; result max(.., 0) / total with the two ratio rules,
//            times the masked image -> the packed output
//
// Parallelism is over pixels only; no atomics, no waiting between workgroups, and every loop
// bound is a descriptor field smi_reweight_* validated on the host.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "rounded_math.h"

namespace smi {
namespace {

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

template <typename T, bool kSources>
__global__ __launch_bounds__(kThreads) void reweight_kernel(const ReweightArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T *halo = reinterpret_cast<T *>(lds_raw);
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
    if (oy >= th || ox >= tw) return;
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
    const T acc[kPerThread] = {acc0, acc1, acc2, acc3};
    const int y = ry0 + ty0 + oy;  // frame row
    const int64_t plane = bl.image_off + (int64_t)band * bl.h * bl.w;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (ox + j >= tw) continue;
        const int x = rx0 + tx0 + ox + j;
        const T m = acc[j] < 0 ? (T)0 : acc[j];
        const int64_t at = plane + (int64_t)y * bl.w + x;
        if (!kSources) {
            a.total[at] = m;
        } else {
            const T t = a.total[at];
            T r = div_rn(m, t);
            if (t == 0) r = 0;
            if (r > 1) r = 1;
            a.out[out_off + ((int64_t)band * rh + (ty0 + oy)) * rw + tx0 + ox + j] =
                mul_rn(r, a.images[at]);
        }
    }
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) {
        return hipMalloc(reinterpret_cast<void **>(&p), (n ? n : 1) * sizeof(T));
    }
    hipError_t upload(const T *h, size_t n) {
        hipError_t e = alloc(n);
        if (e != hipSuccess || n == 0) return e;
        return hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice);
    }
};

constexpr int32_t kMaxCoord = 1 << 24;  // |origins| and extents: sums of a few stay in int32

// every component of [comp0, comp0 + n): inside the table, and its rectangle inside its buffers
int check_components(const smi_reweight_component *comps, int32_t n_components, int32_t comp0,
                     int32_t n, int32_t C, int64_t n_sed, int64_t n_morph) {
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

template <typename T>
int reweight(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
             const smi_reweight_blend *blends, int32_t n_sources,
             const smi_reweight_source *sources, int32_t n_components,
             const smi_reweight_component *comps, const T *images, int64_t n_image,
             const T *stamps, int64_t n_stamp, const T *seds, int64_t n_sed, const T *morphs,
             int64_t n_morph, T *out, int64_t n_out) {
    SMI_REQUIRE(C > 0 && C <= 65535, "bands");
    SMI_REQUIRE(kh > 0 && kw > 0 && kh % 2 == 1 && kw % 2 == 1 && kh <= 4095 && kw <= 4095,
                "the stamp must have odd height and width");
    const size_t lds = lds_elems(kh, kw) * sizeof(T);
    SMI_REQUIRE(lds <= kLdsBudget, "stamp too large for the LDS tile");
    SMI_REQUIRE(n_blends >= 0 && n_sources >= 0 && n_components >= 0, "negative count");
    SMI_REQUIRE(n_image >= 0 && n_stamp >= 0 && n_sed >= 0 && n_morph >= 0 && n_out >= 0,
                "negative buffer size");
    SMI_REQUIRE((blends || !n_blends) && (sources || !n_sources) && (comps || !n_components),
                "null descriptor table");
    SMI_REQUIRE((images || !n_image) && (stamps || !n_stamp) && (seds || !n_sed) &&
                    (morphs || !n_morph) && (out || !n_out), "null buffer");
    const int64_t stamp_elems = (int64_t)C * kh * kw;
    std::vector<int32_t> work_total, work_src;
    for (int32_t b = 0; b < n_blends; ++b) {
        const smi_reweight_blend &bl = blends[b];
        SMI_REQUIRE(bl.h > 0 && bl.w > 0 && bl.h <= kMaxCoord && bl.w <= kMaxCoord, "frame extent");
        const int64_t cube = (int64_t)C * bl.h * bl.w;
        SMI_REQUIRE(bl.image_off >= 0 && bl.image_off <= n_image && cube <= n_image - bl.image_off,
                    "frame outside the image buffer");
        SMI_REQUIRE(bl.stamp_off >= 0 && bl.stamp_off <= n_stamp &&
                        stamp_elems <= n_stamp - bl.stamp_off, "stamp outside its buffer");
        int rc = check_components(comps, n_components, bl.comp0, bl.n_comp, C, n_sed, n_morph);
        if (rc) return rc;
        for (int32_t c = bl.comp0; c < bl.comp0 + bl.n_comp; ++c) {
            const smi_reweight_component &d = comps[c];
            SMI_REQUIRE(d.h == 0 || d.w == 0 || (d.y0 >= 0 && d.x0 >= 0 && d.y0 + d.h <= bl.h &&
                                                 d.x0 + d.w <= bl.w),
                        "a blend's component rectangle leaves the frame");
        }
        const int32_t tiles = ((bl.h + kTileY - 1) / kTileY) * ((bl.w + kTileX - 1) / kTileX);
        for (int32_t t = 0; t < tiles; ++t) work_total.push_back(b), work_total.push_back(t);
    }
    for (int32_t s = 0; s < n_sources; ++s) {
        const smi_reweight_source &sr = sources[s];
        SMI_REQUIRE(sr.blend >= 0 && sr.blend < n_blends, "source of an unknown blend");
        const smi_reweight_blend &bl = blends[sr.blend];
        SMI_REQUIRE(sr.h > 0 && sr.w > 0 && sr.y0 >= 0 && sr.x0 >= 0 && sr.h <= bl.h - sr.y0 &&
                        sr.w <= bl.w - sr.x0, "a source's rectangle leaves the frame");
        const int64_t cube = (int64_t)C * sr.h * sr.w;
        SMI_REQUIRE(sr.out_off >= 0 && sr.out_off <= n_out && cube <= n_out - sr.out_off,
                    "a source's result outside the output buffer");
        int rc = check_components(comps, n_components, sr.comp0, sr.n_comp, C, n_sed, n_morph);
        if (rc) return rc;
        const int32_t tiles = ((sr.h + kTileY - 1) / kTileY) * ((sr.w + kTileX - 1) / kTileX);
        for (int32_t t = 0; t < tiles; ++t) work_src.push_back(s), work_src.push_back(t);
    }
    SMI_REQUIRE(work_total.size() / 2 <= (size_t)INT32_MAX && work_src.size() / 2 <= (size_t)INT32_MAX,
                "too many tiles for one launch");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available");
        return SMI_ERR_NO_DEVICE;
    }
    SMI_REQUIRE(device >= 0 && device < ndev, "device index");
    if (work_src.empty()) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    DevBuf<smi_reweight_blend> d_blends;
    DevBuf<smi_reweight_source> d_sources;
    DevBuf<smi_reweight_component> d_comps;
    DevBuf<int32_t> d_work_total, d_work_src;
    DevBuf<T> d_images, d_stamps, d_seds, d_morphs, d_total, d_out;
    SMI_HIP(d_blends.upload(blends, n_blends));
    SMI_HIP(d_sources.upload(sources, n_sources));
    SMI_HIP(d_comps.upload(comps, n_components));
    SMI_HIP(d_work_total.upload(work_total.data(), work_total.size()));
    SMI_HIP(d_work_src.upload(work_src.data(), work_src.size()));
    SMI_HIP(d_images.upload(images, n_image));
    SMI_HIP(d_stamps.upload(stamps, n_stamp));
    SMI_HIP(d_seds.upload(seds, n_sed));
    SMI_HIP(d_morphs.upload(morphs, n_morph));
    SMI_HIP(d_total.alloc(n_image));
    SMI_HIP(d_out.alloc(n_out));
    // (every element of a validated plan's output is written by exactly one thread; the plan of
    // lite/measure.py packs the results back to back)
    SMI_HIP(hipMemset(d_out.p, 0, (size_t)std::max<int64_t>(n_out, 1) * sizeof(T)));

    ReweightArgs<T> a;
    a.blends = d_blends.p, a.sources = d_sources.p, a.comps = d_comps.p;
    a.images = d_images.p, a.stamps = d_stamps.p, a.seds = d_seds.p, a.morphs = d_morphs.p;
    a.total = d_total.p, a.out = d_out.p, a.kh = kh, a.kw = kw;
    a.work = d_work_total.p;
    hipLaunchKernelGGL((reweight_kernel<T, false>), dim3((unsigned)(work_total.size() / 2), C),
                       dim3(kThreads), lds, 0, a);
    SMI_HIP(hipGetLastError());
    a.work = d_work_src.p;
    hipLaunchKernelGGL((reweight_kernel<T, true>), dim3((unsigned)(work_src.size() / 2), C),
                       dim3(kThreads), lds, 0, a);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipMemcpy(out, d_out.p, (size_t)n_out * sizeof(T), hipMemcpyDeviceToHost));
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_reweight_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                     const smi_reweight_blend *blends, int32_t n_sources,
                     const smi_reweight_source *sources, int32_t n_components,
                     const smi_reweight_component *components, const float *images,
                     int64_t n_image, const float *stamps, int64_t n_stamp, const float *seds,
                     int64_t n_sed, const float *morphs, int64_t n_morph, float *out,
                     int64_t n_out) {
    return smi::reweight<float>(device, C, kh, kw, n_blends, blends, n_sources, sources,
                                n_components, components, images, n_image, stamps, n_stamp, seds,
                                n_sed, morphs, n_morph, out, n_out);
}
int smi_reweight_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                     const smi_reweight_blend *blends, int32_t n_sources,
                     const smi_reweight_source *sources, int32_t n_components,
                     const smi_reweight_component *components, const double *images,
                     int64_t n_image, const double *stamps, int64_t n_stamp, const double *seds,
                     int64_t n_sed, const double *morphs, int64_t n_morph, double *out,
                     int64_t n_out) {
    return smi::reweight<double>(device, C, kh, kw, n_blends, blends, n_sources, sources,
                                 n_components, components, images, n_image, stamps, n_stamp, seds,
                                 n_sed, morphs, n_morph, out, n_out);
}

}  // extern "C"
