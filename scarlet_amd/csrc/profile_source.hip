// GaussianSource / SpergelSource: a morphology that is a closed-form radial profile of a handful
// of float64 parameters (ProfileMorphology, reference morphology.py:210-473; the sources,
// source.py:131-246):
//     x = X - cx, y = Y - cy on the integer pixel grid of the box,  s = 1 / sqrt(1 - |e|^2),
//     X' = s ((1 - e1) x - e2 y),  Y' = s (-e2 x + (1 + e1) y),  R2 = (X'^2 + Y'^2) / radius^2,
//     Gaussian: exp(-R2 / 2);  Spergel: f_nu(c_nu sqrt(R2 + 1e-4)),
//     f_nu(u) = (u / 2)^nu K_nu(u) / Gamma(nu + 1)
// (profile_math.h).  The morphology is not normalised.  The parameters -- centre (2), radius (1),
// ellipticity (2) and, for Spergel, nu (1) -- live with their AMSGrad moments as six doubles per
// component in arrays of their own; the component's `morph` slot holds the float32 image the
// render stage and the spectrum's gradient read.
//
// Per iteration and profile component, where the starlet kernels sit for starlet components:
//   profile_step_kernel     one pass over the box clipped to the frame: g = sum_c sed_c G_c, the
//                           profile and its partials once in double, six sums; then, each
//                           parameter by itself like the reference's Parameters, the AMSGrad step
//                           (a tenth of it and vhat = v on the first iteration) and the proximal
//                           sub-iterations with the exit test of oracle.pgm.adaprox_update --
//                           radius >= 1e-2, ellipticity pulled to |e| = 1 / 1.1 when |e|^2 > 1,
//                           nu clipped to [-0.85, 4], no constraint on the centre.  With
//                           `grad_only` the six sums are stored and nothing moves.
//   profile_forward_kernel  the float32 morphology at the current parameters into the `morph`
//                           slot (every pixel of the box, also where it overhangs the frame).
// The spectrum is stepped by the ordinary update kernel in between, which sees an image that is
// held fixed and has no constraint -- the arrangement of the starlet components.
//
// One workgroup per component and strided loops: any box from 15^2 to the whole frame.  Every
// lane sums its own pixels in index order, lanes are combined by a butterfly within the
// wavefront and the wavefronts in index order through LDS: the sums depend on nothing but the
// component, so a batch gives the bits of a fit by itself.  No atomics on parameters.
#include <algorithm>

#include "common.h"
#include "profile_math.h"

namespace smi {
namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;

// sum of NV values per thread over the block in a fixed order; every thread gets the result
template <int NV>
__device__ void block_sum(double (&a)[NV], double *sh) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[i] += __shfl_xor(a[i], o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) sh[(threadIdx.x >> 6) * NV + i] = a[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = sh[i];
        for (int w = 1; w < kWaves; ++w) t += sh[w * NV + i];
        a[i] = t;
    }
}

// The proximal operator of parameter group `grp` on z[0 .. n): 0 centre (none), 1 radius,
// 2 ellipticity, 3 nu.
__device__ __forceinline__ void profile_prox(int grp, double *z) {
    if (grp == 1) {
        z[0] = fmax(z[0], 1e-2);  // morphology.py:319-320
    } else if (grp == 2) {
        const double n2 = z[0] * z[0] + z[1] * z[1];  // morphology.py:322-326
        if (n2 > 1.0) {
            const double d = sqrt(n2) * 1.1;
            z[0] /= d;
            z[1] /= d;
        }
    } else if (grp == 3) {
        z[0] = fmax(fmin(4.0, z[0]), -0.85);  // morphology.py:472-473
    }
}

template <int KIND>
__device__ void profile_step(const BatchView &v, const ProfileView &pv, const float *G, int it,
                             float e_rel, int prox_max_iter, int grad_only) {
    const int s = blockIdx.x, k = pv.comp[s], b = v.c_blend[k];
    const int tid = threadIdx.x, C = v.C;
    const int h = v.c_h[k], w = v.c_w[k], oy = v.c_oy[k], ox = v.c_ox[k];
    __shared__ double sh[kWaves * kProfileDoubles];
    double *par = pv.par + (int64_t)s * kProfileDoubles;
    const ProfileConsts pc = profile_consts(par, KIND);
    // the box clipped to the blend's own frame (smi_batch_set_frame_extents: a wave-uniform
    // read): the gradient is zero where it overhangs (blend.py:30-46)
    const int y_lo = max(oy, 0), y_hi = min(oy + h, v.frame_h(b));
    const int x_lo = max(ox, 0), x_hi = min(ox + w, v.frame_w(b));
    const int cw = max(x_hi - x_lo, 0), n = max(y_hi - y_lo, 0) * cw;
    const float *sed = v.sed + (int64_t)k * C;
    const int64_t plane = (int64_t)v.Fy * v.Fx;
    double acc[kProfileDoubles] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kT) {
        const int fy = y_lo + i / cw, fx = x_lo + i % cw;
        const float *g = G + ((int64_t)b * C * v.Fy + fy) * v.Fx + fx;
        double gm = 0.0;
        for (int ch = 0; ch < C; ++ch) gm += (double)sed[ch] * (double)g[ch * plane];
        double d[kProfileDoubles];
        profile_at<KIND>(pc, (double)fy, (double)fx, d);
#pragma unroll
        for (int j = 0; j < kProfileDoubles; ++j) acc[j] += gm * d[j];
    }
    block_sum<kProfileDoubles>(acc, sh);
    if (tid != 0) return;
    double *grad = pv.grad + (int64_t)s * kProfileDoubles;
    for (int j = 0; j < kProfileDoubles; ++j) grad[j] = acc[j];
    if (grad_only) return;

    double *m = pv.m + (int64_t)s * kProfileDoubles, *vv = pv.v + (int64_t)s * kProfileDoubles;
    double *vh = pv.vh + (int64_t)s * kProfileDoubles;
    const double *step = pv.step + 4 * s, *rel = pv.rel + 4 * s;
    const int fixed = pv.fixed[s];
    const int lit = v.local_it(b, it);
    const double b1 = v.b1, b2 = v.b2, eps = v.eps, e2 = (double)e_rel * (double)e_rel;
    // groups: centre, radius, ellipticity, nu -- first entry and length in the six doubles
    const int first[4] = {kPcy, kPradius, kPe1, kPnu}, len[4] = {2, 1, 2, 1};
    int bad = 0;
    for (int grp = 0; grp < (KIND == kProfileSpergel ? 4 : 3); ++grp) {
        const int o = first[grp], L = len[grp];
        // relative_step (parameter.py:126-129) on the pre-update value: max(minimum, factor mean)
        double mean = 0.0;
        for (int j = 0; j < L; ++j) mean += par[o + j];
        mean /= L;
        const double alpha = rel[grp] != 0.0 ? fmax(step[grp], rel[grp] * mean) : step[grp];
        double x[2] = {0.0, 0.0}, psi[2] = {0.0, 0.0}, max_psi = 0.0;
        for (int j = 0; j < L; ++j) {
            // Parameter(fixed=True): a zero gradient, everything else as usual (blend.py:107-115)
            const double g = (fixed >> grp) & 1 ? 0.0 : acc[o + j];
            const double mi = (1.0 - b1) * g + b1 * m[o + j];
            const double vi = (1.0 - b2) * (g * g) + b2 * vv[o + j];
            const double vhi = lit == 0 ? vi : fmax(vh[o + j], vi);
            psi[j] = eps > 0.0 ? sqrt(fmax(vhi, eps)) : sqrt(vhi);
            double upd = alpha * mi / psi[j];
            if (lit == 0) upd = upd / 10.0;
            x[j] = par[o + j] - upd;
            m[o + j] = mi;
            vv[o + j] = vi;
            vh[o + j] = vhi;
            max_psi = fmax(max_psi, psi[j]);
        }
        double z[2] = {x[0], x[1]};
        if (grp != 0)
            for (int t = 1; t <= prox_max_iter; ++t) {
                double zn[2];
                for (int j = 0; j < L; ++j) zn[j] = z[j] - psi[j] / max_psi * (z[j] - x[j]);
                profile_prox(grp, zn);
                double d2 = 0.0, n2 = 0.0;
                for (int j = 0; j < L; ++j) {
                    d2 += (zn[j] - z[j]) * (zn[j] - z[j]);
                    n2 += z[j] * z[j];
                    z[j] = zn[j];
                }
                if (d2 <= e2 * n2) break;
            }
        for (int j = 0; j < L; ++j) {
            par[o + j] = z[j];
            bad |= !isfinite(z[j]);
        }
    }
    if (bad) atomicExch(&v.state[b], v.fail_code);
}

__global__ __launch_bounds__(kT) void profile_step_kernel(BatchView v, ProfileView pv,
                                                          const float *G, int it, float e_rel,
                                                          int prox_max_iter, int grad_only) {
    const int s = blockIdx.x;
    if (!grad_only && v.state[v.c_blend[pv.comp[s]]] >= 2) return;
    if (pv.kind[s] == kProfileSpergel)
        profile_step<kProfileSpergel>(v, pv, G, it, e_rel, prox_max_iter, grad_only);
    else
        profile_step<kProfileGaussian>(v, pv, G, it, e_rel, prox_max_iter, grad_only);
}

template <int KIND>
__device__ int profile_write(const ProfileConsts &pc, float *out, int h, int w, int oy, int ox) {
    int bad = 0;
    for (int i = threadIdx.x; i < h * w; i += kT) {
        const int y = i / w, x = i - y * w;
        const float z = (float)profile_at<KIND>(pc, (double)(y + oy), (double)(x + ox), nullptr);
        out[i] = z;
        bad |= !isfinite(z);
    }
    return bad;
}

__global__ __launch_bounds__(kT) void profile_forward_kernel(BatchView v, ProfileView pv,
                                                             int respect_state) {
    const int s = blockIdx.x, k = pv.comp[s], b = v.c_blend[k];
    if (respect_state && v.state[b] >= 2) return;
    const int kind = pv.kind[s];
    const ProfileConsts pc = profile_consts(pv.par + (int64_t)s * kProfileDoubles, kind);
    float *out = v.morph + v.c_moff[k];
    const int bad = kind == kProfileSpergel
                        ? profile_write<kProfileSpergel>(pc, out, v.c_h[k], v.c_w[k], v.c_oy[k], v.c_ox[k])
                        : profile_write<kProfileGaussian>(pc, out, v.c_h[k], v.c_w[k], v.c_oy[k], v.c_ox[k]);
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicExch(&v.state[b], v.fail_code);
}

// smi_profile_probe: value and the six partials at every pixel of a box, [7][h][w]
template <int KIND>
__device__ void probe_box(const double *par, int h, int w, int oy, int ox, double *out) {
    const ProfileConsts pc = profile_consts(par, KIND);
    const int N = h * w;
    for (int i = blockIdx.x * kT + threadIdx.x; i < N; i += gridDim.x * kT) {
        const int y = i / w, x = i - y * w;
        double d[kProfileDoubles];
        out[i] = profile_at<KIND>(pc, (double)(y + oy), (double)(x + ox), d);
        for (int j = 0; j < kProfileDoubles; ++j) out[(int64_t)(j + 1) * N + i] = d[j];
    }
}

__global__ __launch_bounds__(kT) void profile_probe_kernel(int kind, const double *par, int h,
                                                           int w, int oy, int ox, double *out) {
    if (kind == kProfileSpergel)
        probe_box<kProfileSpergel>(par, h, w, oy, ox, out);
    else
        probe_box<kProfileGaussian>(par, h, w, oy, ox, out);
}

}  // namespace

int launch_profile_step(const BatchView &v, const ProfileView &pv, const float *G, int32_t it,
                        float e_rel, int32_t prox_max_iter, int32_t grad_only, hipStream_t s) {
    if (pv.n_prof == 0) return SMI_OK;
    hipLaunchKernelGGL(profile_step_kernel, dim3(pv.n_prof), dim3(kT), 0, s, v, pv, G, it, e_rel,
                       prox_max_iter, grad_only);
    return SMI_OK;
}

int launch_profile_forward(const BatchView &v, const ProfileView &pv, int32_t respect_state,
                           hipStream_t s) {
    if (pv.n_prof == 0) return SMI_OK;
    hipLaunchKernelGGL(profile_forward_kernel, dim3(pv.n_prof), dim3(kT), 0, s, v, pv,
                       respect_state);
    return SMI_OK;
}

void launch_profile_probe(int32_t kind, const double *par, int32_t h, int32_t w, int32_t oy,
                          int32_t ox, double *out, hipStream_t s) {
    const int blocks = std::min((h * w + kT - 1) / kT, 1024);
    hipLaunchKernelGGL(profile_probe_kernel, dim3(blocks), dim3(kT), 0, s, kind, par, h, w, oy, ox,
                       out);
}

}  // namespace smi
