// lite.weight_blends: the flux-conserving reweighting of scarlet.lite (reference
// scarlet/lite/measure.py:39-91) for a catalogue of blends, two launches per chunk.
//
// Both launches run the same kernel, the tile of reweight_device.h (halo staging and tap loop,
// shared with lite_measure.hip): first the totals of every blend's frame -> `total`, then every
// source's model / total with the two ratio rules, times the masked image -> the packed output.
//
// Parallelism is over pixels only; no atomics, no waiting between workgroups, and every loop
// bound is a descriptor field smi_reweight_* validated on the host (check_plan).
#include "reweight_device.h"

namespace smi {
namespace {

using namespace reweight_tile;

template <typename T, bool kSources>
__global__ __launch_bounds__(kThreads) void reweight_kernel(const ReweightArgs<T> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    tile_pass<T, kSources>(a, lds_raw);
}

template <typename T>
int reweight(const Plan<T> &p, int32_t device, T *out, int64_t n_out) {
    SMI_REQUIRE(out || n_out <= 0, "null buffer");
    std::vector<int32_t> work_total, work_src;
    size_t lds = 0;
    int rc = check_plan(p, true, n_out, &work_total, &work_src, &lds);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    if (work_src.empty()) return SMI_OK;  // nothing to write
    SMI_HIP(hipSetDevice(device));

    Uploaded<T> dev;
    ReweightArgs<T> a;
    if ((rc = dev.upload(p, work_total, work_src, n_out, &a))) return rc;
    a.work = dev.work_total.p;
    hipLaunchKernelGGL((reweight_kernel<T, false>), dim3((unsigned)(work_total.size() / 2), p.C),
                       dim3(kThreads), lds, 0, a);
    SMI_HIP(hipGetLastError());
    a.work = dev.work_src.p;
    hipLaunchKernelGGL((reweight_kernel<T, true>), dim3((unsigned)(work_src.size() / 2), p.C),
                       dim3(kThreads), lds, 0, a);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipMemcpy(out, dev.out.p, (size_t)n_out * sizeof(T), hipMemcpyDeviceToHost));
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
    const smi::reweight_tile::Plan<float> p = {C, kh, kw, n_blends, blends, n_sources, sources,
        n_components, components, images, n_image, stamps, n_stamp, seds, n_sed, morphs, n_morph};
    return smi::reweight<float>(p, device, out, n_out);
}
int smi_reweight_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                     const smi_reweight_blend *blends, int32_t n_sources,
                     const smi_reweight_source *sources, int32_t n_components,
                     const smi_reweight_component *components, const double *images,
                     int64_t n_image, const double *stamps, int64_t n_stamp, const double *seds,
                     int64_t n_sed, const double *morphs, int64_t n_morph, double *out,
                     int64_t n_out) {
    const smi::reweight_tile::Plan<double> p = {C, kh, kw, n_blends, blends, n_sources, sources,
        n_components, components, images, n_image, stamps, n_stamp, seds, n_sed, morphs, n_morph};
    return smi::reweight<double>(p, device, out, n_out);
}

}  // extern "C"
