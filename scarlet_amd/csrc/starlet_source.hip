// StarletSource: a morphology whose parameter is the starlet coefficients of its image
// (StarletMorphology, reference morphology.py:516-604; StarletSource, source.py:525-612).
//
// The model is the generation-2 reconstruction (wavelet.py:284-311) of the coefficients
// c[0 .. S], S = planes - 1:
//     x_S = c[S],   x_j = B_j x_{j+1} + c[j]  (j = S-1 .. 0),   image = x_0
// with B_j the separable 5-tap B-spline (1/16, 1/4, 3/8, 1/4, 1/16) at spacing 2^j whose taps
// outside the box are dropped (wavelet.py:154-191).  B_j is symmetric under that boundary, so the
// gradient needs no autograd: with g = sum_c sed_c G_c on the box,
//     a_0 = g,   a_{j+1} = B_j a_j,   d(-logL)/dc[j] = a_j (j < S),   d(-logL)/dc[S] = a_S.
//
// Per iteration and starlet component, where the shift kernels sit for shifting components:
//   starlet_step_kernel     the box gradient and the cascade a_1 .. a_S, then AMSGrad on all
//                           planes * h * w coefficients as ONE parameter (one max(psi)) and the
//                           proximal sub-iterations z <- prox(z - psi / max(psi) (z - x)), prox =
//                           max(., floor) then |.| < t_plane -> 0, stopped on the device by
//                           ||z' - z||^2 <= e_rel^2 ||z||^2 over all planes
//                           (oracle.pgm.adaprox_update); for a component of
//                           StarletMorphology(monotonic=True) prox is prox_monotonic_mask on
//                           every plane instead (mask_device.h), see below;
//   starlet_forward_kernel  the reconstruction of the coefficients into the component's `morph`
//                           slot, which the render stage and the spectrum's gradient read.
// The spectrum is stepped by the ordinary update kernel in between: it sees the component as an
// image that is held fixed and has no constraint, so it leaves the `morph` slot as it is.
//
// One workgroup of 1024 threads per component; all arithmetic in float32 like every other
// parameter of the batch (the float64 bit-exact transforms of starlet.hip keep serving detection
// and construction).  The two work planes of the passes live in LDS while they fit (boxes up to
// kStarLdsPixels pixels, ~138^2), in global memory beyond; coefficients, moments and the cascade
// are streamed from global memory (L2-resident between the phases of one workgroup).
#include <algorithm>

#include "common.h"
#include "mask_device.h"
#include "starlet_device.h"

namespace smi {
namespace {

constexpr int kT = kMaskT;
constexpr int kWaves = kT / 64;
// reduction scratch in front of the work planes: kWaves doubles x 2 + kWaves floats, then the
// shared words of the monotonic mask operator, padded
constexpr int kRedBytes = 512;
constexpr int kMaskSharedAt = 2 * kWaves * sizeof(double) + kWaves * sizeof(float);
static_assert(kMaskSharedAt % 8 == 0 && kMaskSharedAt + sizeof(MaskShared) <= kRedBytes, "");

extern __shared__ __attribute__((aligned(16))) unsigned char star_lds[];

struct Red {
    double *d0, *d1;
    float *f;
};

__device__ __forceinline__ Red red_scratch() {
    Red r;
    r.d0 = reinterpret_cast<double *>(star_lds);
    r.d1 = r.d0 + kWaves;
    r.f = reinterpret_cast<float *>(r.d1 + kWaves);
    return r;
}

__device__ float block_max(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sh[0];
    for (int w = 1; w < kWaves; ++w) t = fmaxf(t, sh[w]);
    return t;
}

// sums of two values over the block, in a fixed order
__device__ void block_sum2(double &a, double &b, const Red &r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        r.d0[threadIdx.x >> 6] = a;
        r.d1[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = b = 0.0;
    for (int w = 0; w < kWaves; ++w) {
        a += r.d0[w];
        b += r.d1[w];
    }
}

// One 1-D pass of B_j at spacing d along AXIS (0: rows y +- d, 1: columns x +- d) over an
// (h, w) plane; out = conv (+ addend).  `in` never aliases `out`.  Ends with a barrier.
template <int AXIS>
__device__ void bspline_pass(const float *in, float *out, const float *addend, int h, int w,
                             int d) {
    const int N = h * w;
    for (int i = threadIdx.x; i < N; i += kT) {
        const int y = i / w, x = i - y * w;
        const float acc = bspline_tap<AXIS, float, int>(in + i, y, x, h, w, d);
        out[i] = addend ? acc + addend[i] : acc;
    }
    __syncthreads();
}

struct StarCtx {
    int k, b, h, w, N, P;
    int64_t coff;
    float *work0, *work1;
};

__device__ __forceinline__ StarCtx star_ctx(const BatchView &v, const StarletView &sv) {
    StarCtx c;
    const int s = blockIdx.x;
    c.k = sv.comp[s];
    c.b = v.c_blend[c.k];
    c.h = v.c_h[c.k];
    c.w = v.c_w[c.k];
    c.N = c.h * c.w;
    c.P = sv.planes[s];
    c.coff = sv.coff[s];
    if (sv.work) {  // work planes in global memory: 2 N floats per component
        c.work0 = sv.work + 2 * v.c_moff[c.k];
        c.work1 = c.work0 + c.N;
    } else {
        c.work0 = reinterpret_cast<float *>(star_lds + kRedBytes);
        c.work1 = c.work0 + ((sv.max_pixels + 3) & ~3);
    }
    return c;
}

// The monotonic mask operator on the P planes of a stack, one after the other.  Its state lives
// in the two work planes, which the B-spline passes have left by then: `visited` in the first,
// the three byte maps in the second (3 N of its 4 N bytes) -- in LDS or in the global scratch,
// wherever the work planes are.
struct MonoRule {
    int cy, cx, radius, max_iter;
    double variance;
};

__device__ __forceinline__ void mono_plane(float *plane, const StarCtx &c, const MonoRule &r) {
    monotonic_mask_plane(plane, c.h, c.w, r.cy, r.cx, r.radius, r.variance, r.max_iter,
                         reinterpret_cast<int32_t *>(c.work0),
                         reinterpret_cast<uint8_t *>(c.work1),
                         reinterpret_cast<MaskShared *>(star_lds + kMaskSharedAt));
}

// MONO: the batch holds monotonic components (sv.mono); the instance without is the kernel as
// it was before they existed, and batches without them keep launching it.
template <bool MONO>
__global__ __launch_bounds__(kT) void starlet_step_kernel(BatchView v, StarletView sv,
                                                          const float *G, int it, float e_rel,
                                                          int prox_max_iter, int grad_only) {
    const StarCtx c = star_ctx(v, sv);
    if (!grad_only && v.state[c.b] >= 2) return;
    const int tid = threadIdx.x, N = c.N, S = c.P - 1, C = v.C;
    const int oy = v.c_oy[c.k], ox = v.c_ox[c.k];
    const float *sed = v.sed + (int64_t)c.k * C;
    float *grad = sv.grad + c.coff;
    // the blend's own frame (smi_batch_set_frame_extents): a wave-uniform read
    const int Hb = v.frame_h(c.b), Wb = v.frame_w(c.b);

    // 1. a_0 = sum_c sed_c G_c over the box, zero outside the frame (blend.py:30-46)
    for (int i = tid; i < N; i += kT) {
        const int y = i / c.w, x = i - y * c.w;
        const int fy = y + oy, fx = x + ox;
        float acc = 0.f;
        if ((unsigned)fy < (unsigned)Hb && (unsigned)fx < (unsigned)Wb) {
            const float *g = G + ((int64_t)c.b * C * v.Fy + fy) * v.Fx + fx;
            for (int ch = 0; ch < C; ++ch) acc = fmaf(sed[ch], g[(int64_t)ch * v.Fy * v.Fx], acc);
        }
        grad[i] = acc;
    }
    __syncthreads();
    // 2. the cascade: plane j + 1 = B_j plane j
    for (int j = 0; j < S; ++j) {
        const int d = bspline_spacing(j, c.h, c.w);
        bspline_pass<0>(grad + (int64_t)j * N, c.work0, nullptr, c.h, c.w, d);
        bspline_pass<1>(c.work0, grad + (int64_t)(j + 1) * N, nullptr, c.h, c.w, d);
    }
    if (grad_only) return;

    // 3. AMSGrad on all planes as one parameter (proxmin's amsgrad: no bias correction,
    //    vhat = v and a tenth of the step at it = 0); x goes where the gradient was
    const Red red = red_scratch();
    float *x = sv.coeffs + c.coff, *m = sv.m + c.coff, *vv = sv.v + c.coff, *vh = sv.vh + c.coff;
    const float *thr = sv.thresh + sv.toff[blockIdx.x];
    const float floor_ = v.c_pos_floor[c.k];
    const bool fixed = sv.fixed[blockIdx.x] != 0;
    const int lit = v.local_it(c.b, it);
    const float alpha = v.c_morph_step[c.k];
    const float b1 = v.b1, b2 = v.b2, eps = v.eps;
    // a monotonic component takes its moments with the constants as the caller gave them
    // (float32(0.999) alone puts 1.3e-5 on v); the others keep the batch's float32 ones
    const bool exact = MONO && sv.mono[blockIdx.x];
    float max_psi = 0.f;
    int bad = 0;
    for (int p = 0; p < c.P; ++p)
        for (int q = tid; q < N; q += kT) {
            const int64_t i = (int64_t)p * N + q;
            const float g = fixed ? 0.f : grad[i];
            float mi, vi;
            if (MONO && exact) {
                const double gd = (double)g;
                mi = (float)((1.0 - sv.b1) * gd + sv.b1 * (double)m[i]);
                vi = (float)((1.0 - sv.b2) * (gd * gd) + sv.b2 * (double)vv[i]);
            } else {
                mi = (1.f - b1) * g + b1 * m[i];
                vi = (1.f - b2) * (g * g) + b2 * vv[i];
            }
            const float vhi = lit == 0 ? vi : fmaxf(vh[i], vi);
            const float psi = eps > 0.f ? sqrtf(fmaxf(vhi, eps)) : sqrtf(vhi);
            float upd = alpha * mi / psi;
            if (lit == 0) upd = upd / 10.f;
            const float xi = x[i] - upd;
            m[i] = mi;
            vv[i] = vi;
            vh[i] = vhi;
            grad[i] = xi;
            if (prox_max_iter <= 0) {
                x[i] = xi;
                bad |= !isfinite(xi);
            }
            max_psi = fmaxf(max_psi, psi);
        }
    max_psi = block_max(max_psi, red.f);
    // 4. proximal sub-iterations in the metric psi; z lives in the coefficient array.  The
    //    first one starts at z = x, where z - psi / max(psi) (z - x) is x itself.
    const float e2 = e_rel * e_rel;
    if (MONO && sv.mono[blockIdx.x]) {
        // prox = prox_monotonic_mask per plane (MonotonicMaskConstraint.__call__ on a stack): the
        // candidate y goes into the coefficient plane, the operator works on it in place with
        // the whole workgroup, and z waits in the component's plane of sv.zsave for the norm
        MonoRule rule;
        rule.cy = c.h / 2;
        rule.cx = c.w / 2;
        rule.radius = sv.mono_radius[blockIdx.x];
        rule.max_iter = sv.mono_max_iter[blockIdx.x];
        rule.variance = sv.mono_variance[blockIdx.x];
        float *zs = sv.zsave + v.c_moff[c.k];
        for (int t = 1; t <= prox_max_iter; ++t) {
            double d2 = 0.0, n2 = 0.0;
            bad = 0;
            for (int p = 0; p < c.P; ++p) {
                float *plane = x + (int64_t)p * N;
                for (int q = tid; q < N; q += kT) {
                    const int64_t i = (int64_t)p * N + q;
                    const float xi = grad[i];
                    float z, y;
                    if (t == 1) {
                        z = y = xi;
                    } else {
                        z = plane[q];
                        const float psi = eps > 0.f ? sqrtf(fmaxf(vh[i], eps)) : sqrtf(vh[i]);
                        y = z - psi / max_psi * (z - xi);
                    }
                    bad |= !isfinite(y) || !isfinite(xi);
                    zs[q] = z;
                    plane[q] = y;
                    n2 += (double)z * (double)z;
                }
                __syncthreads();
                mono_plane(plane, c, rule);
                for (int q = tid; q < N; q += kT) {
                    const float dz = plane[q] - zs[q];
                    d2 += (double)dz * (double)dz;
                }
            }
            block_sum2(d2, n2, red);
            if (d2 <= (double)e2 * n2) break;
        }
        if (__syncthreads_or(bad) && tid == 0) atomicExch(&v.state[c.b], v.fail_code);
        return;
    }
    for (int t = 1; t <= prox_max_iter; ++t) {
        double d2 = 0.0, n2 = 0.0;
        bad = 0;
        for (int p = 0; p < c.P; ++p) {
            const float tp = thr[p];
            for (int q = tid; q < N; q += kT) {
                const int64_t i = (int64_t)p * N + q;
                const float xi = grad[i];
                float z, y;
                if (t == 1) {
                    z = y = xi;
                } else {
                    z = x[i];
                    const float psi = eps > 0.f ? sqrtf(fmaxf(vh[i], eps)) : sqrtf(vh[i]);
                    y = z - psi / max_psi * (z - xi);
                }
                y = fmaxf(y, floor_);
                if (fabsf(y) < tp) y = 0.f;
                // (fmaxf drops a NaN: look at the unconstrained value as well)
                bad |= !isfinite(y) || !isfinite(xi);
                x[i] = y;
                const float dz = y - z;
                d2 += (double)dz * (double)dz;
                n2 += (double)z * (double)z;
            }
        }
        block_sum2(d2, n2, red);
        if (d2 <= (double)e2 * n2) break;
    }
    if (__syncthreads_or(bad) && tid == 0) atomicExch(&v.state[c.b], v.fail_code);
}

__global__ __launch_bounds__(kT) void starlet_forward_kernel(BatchView v, StarletView sv,
                                                             int respect_state) {
    const StarCtx c = star_ctx(v, sv);
    if (respect_state && v.state[c.b] >= 2) return;
    const int N = c.N, S = c.P - 1;
    const float *coeffs = sv.coeffs + c.coff;
    float *out = v.morph + v.c_moff[c.k];
    const float *cur = coeffs + (int64_t)S * N;
    if (S == 0)
        for (int i = threadIdx.x; i < N; i += kT) out[i] = cur[i];
    for (int j = S - 1; j >= 0; --j) {
        const int d = bspline_spacing(j, c.h, c.w);
        float *dst = j == 0 ? out : c.work0;
        bspline_pass<0>(cur, c.work1, nullptr, c.h, c.w, d);
        bspline_pass<1>(c.work1, dst, coeffs + (int64_t)j * N, c.h, c.w, d);
        cur = dst;
    }
    __syncthreads();
    int bad = 0;
    for (int i = threadIdx.x; i < N; i += kT) bad |= !isfinite(out[i]);
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicExch(&v.state[c.b], v.fail_code);
}

// prox_monotonic_mask once on every plane of a [planes][h][w] stack: the operator of the step
// kernel on its own, with the work planes where a component of that box would have them
__global__ __launch_bounds__(kT) void starlet_mono_kernel(float *stack, int planes, int h, int w,
                                                          MonoRule rule, float *work) {
    StarCtx c;
    c.h = h;
    c.w = w;
    c.N = h * w;
    c.P = planes;
    c.work0 = work ? work : reinterpret_cast<float *>(star_lds + kRedBytes);
    c.work1 = c.work0 + ((c.N + 3) & ~3);
    for (int p = 0; p < planes; ++p) mono_plane(stack + (int64_t)p * c.N, c, rule);
}

size_t star_lds_bytes(const StarletView &sv) {
    return kRedBytes + (sv.work ? 0 : 2 * (size_t)((sv.max_pixels + 3) & ~3) * sizeof(float));
}

int configure_starlet_kernels(size_t lds) {
    static size_t cfg_step[kMaxDevices] = {}, cfg_forward[kMaxDevices] = {};
    static size_t cfg_mono[kMaxDevices] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(starlet_step_kernel<false>), lds,
                                    cfg_step))
        return rc;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(starlet_step_kernel<true>), lds,
                                    cfg_mono))
        return rc;
    return ensure_dynamic_lds(reinterpret_cast<const void *>(starlet_forward_kernel), lds,
                              cfg_forward);
}

}  // namespace

bool starlet_needs_scratch(int max_pixels) { return max_pixels > kStarLdsPixels; }

int launch_starlet_step(const BatchView &v, const StarletView &sv, const float *G, int32_t it,
                        float e_rel, int32_t prox_max_iter, int32_t grad_only, hipStream_t s) {
    if (sv.n_star == 0) return SMI_OK;
    const size_t lds = star_lds_bytes(sv);
    SMI_REQUIRE(lds <= 160 * 1024, "starlet component box too large for the LDS");
    if (int rc = configure_starlet_kernels(lds)) return rc;
    if (sv.mono)
        hipLaunchKernelGGL(starlet_step_kernel<true>, dim3(sv.n_star), dim3(kT), lds, s, v, sv, G,
                           it, e_rel, prox_max_iter, grad_only);
    else
        hipLaunchKernelGGL(starlet_step_kernel<false>, dim3(sv.n_star), dim3(kT), lds, s, v, sv, G,
                           it, e_rel, prox_max_iter, grad_only);
    return SMI_OK;
}

int starlet_monotonic_mask_host(float *stack, int32_t planes, int32_t h, int32_t w,
                                int32_t center_radius, double variance, int32_t max_iter) {
    const size_t N = (size_t)h * w, bytes = (size_t)planes * N * sizeof(float);
    const bool scratch = starlet_needs_scratch((int)N);
    float *d_stack = nullptr, *d_work = nullptr;
    int rc = SMI_OK;
    const size_t lds = kRedBytes + (scratch ? 0 : 2 * ((N + 3) & ~(size_t)3) * sizeof(float));
    static size_t cfg[kMaxDevices] = {};
    if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(starlet_mono_kernel), lds, cfg)))
        return rc;
    SMI_HIP(hipMalloc(reinterpret_cast<void **>(&d_stack), bytes));
    hipError_t e = scratch ? hipMalloc(reinterpret_cast<void **>(&d_work),
                                       2 * ((N + 3) & ~(size_t)3) * sizeof(float))
                           : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(d_stack, stack, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        MonoRule rule;
        rule.cy = h / 2;
        rule.cx = w / 2;
        rule.radius = center_radius;
        rule.max_iter = max_iter;
        rule.variance = variance;
        hipLaunchKernelGGL(starlet_mono_kernel, dim3(1), dim3(kT), lds, 0, d_stack, planes, h, w,
                           rule, d_work);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(stack, d_stack, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_stack);
    if (d_work) (void)hipFree(d_work);
    SMI_HIP(e);
    return rc;
}

int launch_starlet_forward(const BatchView &v, const StarletView &sv, int32_t respect_state,
                           hipStream_t s) {
    if (sv.n_star == 0) return SMI_OK;
    const size_t lds = star_lds_bytes(sv);
    SMI_REQUIRE(lds <= 160 * 1024, "starlet component box too large for the LDS");
    if (int rc = configure_starlet_kernels(lds)) return rc;
    hipLaunchKernelGGL(starlet_forward_kernel, dim3(sv.n_star), dim3(kT), lds, s, v, sv,
                       respect_state);
    return SMI_OK;
}

}  // namespace smi
