// Device code of the footprint rules (see the header comment of footprints.hip) shared by the
// kernels of footprints.hip -- planes [P][H][W] of one frame -- and of footprints_batch.hip --
// a ragged list of planes.  A kernel of either file finds its plane, then calls these with the
// plane's own image, label and record arrays: labels are indices inside the plane's frame, so
// both files give the same footprints, ranks and peaks.  The host code that orders and filters
// the peaks the fetch kernels emit is here too, once.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace smi {
namespace {

constexpr int kTile = 64;           // tile side = wavefront width
constexpr int kRows = 4;            // wavefronts per workgroup
constexpr int kT = 64 * kRows;      // threads per workgroup
constexpr int kChunk = kT * 8;      // pixels per scan chunk
constexpr int kMaxGrid = 65535;
constexpr int kRec = 7;             // int32 arrays per plane beside the labels
enum { R_Y0 = 0, R_Y1, R_X0, R_X1, R_AREA, R_RANK, R_MOFF };

__host__ __device__ inline int64_t nchunks(int64_t N) { return (N + kChunk - 1) / kChunk; }
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

__device__ __forceinline__ int ld_agent(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of i on the global parent array: parents are strictly smaller, a root is its own
__device__ __forceinline__ int find_global(const int32_t *par, int i) {
    int p;
    while ((p = ld_agent(par + i)) != i) i = p;
    return i;
}

// unite the sets of a and b; the larger root is hung under the smaller.  When the atomic min
// returns something other than the root we held, another union got there first and its value
// still has to be united with ours: max(a, b) is smaller at every retry.
__device__ inline void union_global(int32_t *par, int a, int b) {
    for (;;) {
        a = find_global(par, a);
        b = find_global(par, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int ld_lds(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int find_lds(int *lab, int i) {
    const int start = i;
    int p;
    while ((p = ld_lds(lab + i)) != i) i = p;
    // shorten the next walk; a min, so that a concurrent union's smaller parent stays
    if (start != i) atomicMin(lab + start, i);
    return i;
}

__device__ inline void union_lds(int *lab, int a, int b) {
    for (;;) {
        a = find_lds(lab, a);
        b = find_lds(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

// pass 1 for tile (tx, ty) of the plane im[H][W]: block (64, kRows), lab = kTile * kTile ints
// of LDS.  Ends with a barrier, so the next tile may follow at once.
template <typename T>
__device__ __forceinline__ void label_tile(const T *im, int32_t *par, int H, int W, double th,
                                           int tx, int ty, int *lab) {
    const int lane = threadIdx.x, wy = threadIdx.y;
    const int x = tx * kTile + lane, ybase = ty * kTile;
    constexpr int kPer = kTile / kRows;
    for (int r = 0; r < kPer; ++r) {
        const int ly = wy * kPer + r, y = ybase + ly;
        const bool fg = x < W && y < H && ((double)im[(int64_t)y * W + x] > th);
        const unsigned long long m = __ballot(fg);
        // first pixel of this lane's horizontal run: one past the highest clear bit below
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);
        const int s = below ? 64 - __clzll((long long)below) : 0;
        lab[ly * kTile + lane] = fg ? ly * kTile + s : -1;
    }
    __syncthreads();
    for (int r = 0; r < kPer; ++r) {
        const int ly = wy * kPer + r, i = ly * kTile + lane;
        if (ly == 0) continue;
        // the sign of a label never changes, so these reads need no ordering
        const bool fg = ld_lds(lab + i) >= 0, up = ld_lds(lab + i - kTile) >= 0;
        const bool left = lane > 0 && ld_lds(lab + i - 1) >= 0 &&
                          ld_lds(lab + i - kTile - 1) >= 0;
        if (fg && up && !left) union_lds(lab, i, i - kTile);
    }
    __syncthreads();
    for (int r = 0; r < kPer; ++r) {
        const int ly = wy * kPer + r, y = ybase + ly, i = ly * kTile + lane;
        if (x >= W || y >= H) continue;
        int out = -1;
        if (lab[i] >= 0) {
            int root = i, p;
            while ((p = lab[root]) != root) root = p;
            out = (ybase + root / kTile) * W + tx * kTile + root % kTile;
        }
        par[(int64_t)y * W + x] = out;
    }
    __syncthreads();
}

// Border pixels of a plane: first the (tiles_x - 1) * H pixels left of which a tile ends, then
// the (tiles_y - 1) * W pixels above which one ends
__host__ __device__ inline int64_t border_pixels(int H, int W) {
    const int64_t tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    return (tiles_x - 1) * H + (tiles_y - 1) * W;
}

// pass 2 for border pixel k of the plane; nv = (tiles_x - 1) * H
__device__ __forceinline__ void merge_border_pixel(int32_t *par, int H, int W, int64_t nv,
                                                   int64_t k) {
    int x, y, q;
    bool first;
    if (k < nv) {
        x = (int)(k / H + 1) * kTile;
        y = (int)(k % H);
        q = y * W + x - 1;
        // the pixel above belongs to the same two tiles unless a tile row starts here
        first = y % kTile == 0 || ld_agent(par + q + 1 - W) < 0 || ld_agent(par + q - W) < 0;
    } else {
        const int64_t j = k - nv;
        y = (int)(j / W + 1) * kTile;
        x = (int)(j % W);
        q = (y - 1) * W + x;
        first = x % kTile == 0 || ld_agent(par + y * W + x - 1) < 0 || ld_agent(par + q - 1) < 0;
    }
    const int p = y * W + x;
    if (first && ld_agent(par + p) >= 0 && ld_agent(par + q) >= 0) union_global(par, p, q);
}

// pass 3 for pixel p = y * W + x; rc = the plane's [kRec][N] records
__device__ __forceinline__ void flatten_pixel(int32_t *lab, int32_t *rc, int64_t N, int H, int W,
                                              int p) {
    if (ld_agent(lab + p) < 0) return;
    const int root = find_global(lab, p);
    // any value a concurrent find reads here, old or new, is an ancestor of p
    __hip_atomic_store(lab + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (root == p) {
        rc[R_Y0 * N + p] = H;
        rc[R_Y1 * N + p] = -1;
        rc[R_X0 * N + p] = W;
        rc[R_X1 * N + p] = -1;
        rc[R_AREA * N + p] = 0;
        rc[R_RANK * N + p] = -1;
        rc[R_MOFF * N + p] = 0;
    }
}

// pass 4 for the 64 pixels (y, xbase ..) a wavefront holds.  The whole wavefront calls it: the
// lanes that share a label are a bit mask, and one lane per distinct label sends the record
__device__ __forceinline__ void record_row(const int32_t *lab, int32_t *rc, int64_t N, int W,
                                           int y, int xbase) {
    const int lane = threadIdx.x, x = xbase + lane;
    const int L = x < W ? lab[(int64_t)y * W + x] : -1;
    unsigned long long rem = __ballot(L >= 0);
    while (rem) {  // one round per distinct label of the wavefront
        const int leader = __ffsll((long long)rem) - 1;
        const int Ll = __shfl(L, leader, 64);
        const unsigned long long m = __ballot(L == Ll);
        if (lane == leader) {
            atomicMin(rc + R_Y0 * N + Ll, y);
            atomicMax(rc + R_Y1 * N + Ll, y);
            atomicMin(rc + R_X0 * N + Ll, xbase + leader);
            atomicMax(rc + R_X1 * N + Ll, xbase + 63 - __clzll((long long)m));
            atomicAdd(rc + R_AREA * N + Ll, __popcll(m));
        }
        rem &= ~m;
    }
}

__device__ __forceinline__ bool kept_root(const int32_t *rc, int64_t N, int p, int min_area,
                                          long long *box) {
    const long long h = rc[R_Y1 * N + p] - rc[R_Y0 * N + p] + 1;
    const long long w = rc[R_X1 * N + p] - rc[R_X0 * N + p] + 1;
    *box = h * w;
    return h * w > (long long)min_area && rc[R_AREA * N + p] >= min_area;
}

// exclusive scan of one value per thread over the workgroup (kT threads, 1-D), in thread
// order; *total = the sum
__device__ inline long long block_scan(long long v, long long *sh, long long *total) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int k = 0; k < kT / 64; ++k) {
        if (k < wave) base += sh[k];
        tot += sh[k];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// passes 5 and 7 for scan chunk `chunk` of a plane, block kT (1-D); thread t owns 8 consecutive
// pixels, pt = the chunk's two sums.  FINAL 0: pt = (kept roots, their box pixels).  FINAL 1: pt
// holds the exclusive prefixes; rank and mask offset of every kept root.
template <int FINAL>
__device__ __forceinline__ void rank_chunk(const int32_t *lab, int32_t *rc, int64_t N,
                                           int min_area, long long *pt, int64_t chunk,
                                           long long *sh) {
    const int64_t p0 = chunk * kChunk + threadIdx.x * 8;
    long long cnt = 0, pix = 0, box[8];
    bool keep[8];
    for (int k = 0; k < 8; ++k) {
        const int64_t p = p0 + k;
        keep[k] = p < N && lab[p] == (int)p && kept_root(rc, N, (int)p, min_area, &box[k]);
        if (keep[k]) {
            ++cnt;
            pix += box[k];
        }
    }
    long long tc, tp;
    long long ec = block_scan(cnt, sh, &tc);
    long long ep = block_scan(pix, sh, &tp);
    if (!FINAL) {
        if (threadIdx.x == 0) {
            pt[0] = tc;
            pt[1] = tp;
        }
        return;
    }
    ec += pt[0];
    ep += pt[1];
    for (int k = 0; k < 8; ++k)
        if (keep[k]) {
            rc[R_RANK * N + p0 + k] = (int32_t)ec++;
            // wraps only when the plane's total does, which the caller refuses
            rc[R_MOFF * N + p0 + k] = (int32_t)(uint32_t)ep;
            ep += box[k];
        }
}

// pass 6 for one plane, one workgroup of kT threads: the chunk sums pt[nchunk][2] become
// exclusive prefixes, the totals go to tot[0..1]; tot[2] (peaks) is zeroed for pass 8
__device__ __forceinline__ void scan_chunk_sums(long long *pt, int64_t nchunk, long long *tot,
                                                long long *sh) {
    const int64_t seg = (nchunk + kT - 1) / kT;
    int64_t a = threadIdx.x * seg, b = a + seg;
    if (a > nchunk) a = nchunk;
    if (b > nchunk) b = nchunk;
    long long cnt = 0, pix = 0;
    for (int64_t c = a; c < b; ++c) {
        cnt += pt[2 * c];
        pix += pt[2 * c + 1];
    }
    long long tc, tp;
    long long ec = block_scan(cnt, sh, &tc);
    long long ep = block_scan(pix, sh, &tp);
    for (int64_t c = a; c < b; ++c) {
        const long long vc = pt[2 * c], vp = pt[2 * c + 1];
        pt[2 * c] = ec;
        pt[2 * c + 1] = ep;
        ec += vc;
        ep += vp;
    }
    if (threadIdx.x == 0) {
        tot[0] = tc;
        tot[1] = tp;
        tot[2] = 0;
    }
}

// the peak rule for pixel (y, x) of footprint L (a kept root)
template <typename T>
__device__ __forceinline__ bool is_peak(const T *im, const int32_t *lab, const int32_t *rc,
                                        int64_t N, int W, int y, int x, int L, T v) {
    const int y0 = rc[R_Y0 * N + L], y1 = rc[R_Y1 * N + L];
    const int x0 = rc[R_X0 * N + L], x1 = rc[R_X1 * N + L];
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            if (!dy && !dx) continue;
            const int a = y + dy, b = x + dx;
            if (a < y0 || a > y1 || b < x0 || b > x1) continue;  // the box lies in the image
            const int64_t q = (int64_t)a * W + b;
            const T n = lab[q] == L ? im[q] : T(0);
            if (!(v > n)) return false;
        }
    return true;
}

// is pixel (y, x), x < W, a peak of a kept footprint?  *rank = its footprint's, *v = its value
template <typename T>
__device__ __forceinline__ bool peak_at(const T *im, const int32_t *lab, const int32_t *rc,
                                        int64_t N, int W, int y, int x, int *rank, T *v) {
    const int64_t p = (int64_t)y * W + x;
    const int L = lab[p];
    if (L < 0 || (*rank = rc[R_RANK * N + L]) < 0) return false;
    *v = im[p];
    return is_peak<T>(im, lab, rc, N, W, y, x, L, *v);
}

// one mask byte: pixel j of the box (bounds[4]) of the footprint with root `root`
__device__ __forceinline__ uint8_t mask_byte(const int32_t *lab, int W, const int32_t *bounds,
                                             int root, int64_t j) {
    const int y0 = bounds[0], x0 = bounds[2];
    const int w = bounds[3] - x0 + 1;
    const int y = y0 + (int)(j / w), x = x0 + (int)(j % w);
    return lab[(int64_t)y * W + x] == root ? 1 : 0;
}

// The order of detect.cpp inside a footprint: brightest first, equal fluxes in raster order
template <typename Rec>
inline bool peak_before(const Rec &a, const Rec &b) {
    if (a.flux != b.flux) return a.flux > b.flux;
    return a.lin < b.lin;
}

// The sequential min_separation filter of detect.cpp per footprint.  pk: the peak records of
// footprints 0 .. n - 1, sorted by footprint and then by peak_before; fp(rec) = the footprint
// of a record, width(rec) = the width of its plane (lin = y * width + x).  Fills
// peak_start[n + 1], peak_yx and peak_flux with the peaks kept.
template <typename Rec, typename Fp, typename Width>
inline void select_peaks(const std::vector<Rec> &pk, int32_t n, Fp fp, Width width,
                         double min_separation, int32_t *peak_start, int32_t *peak_yx,
                         double *peak_flux) {
    const double min2 = min_separation * min_separation;
    int32_t k = 0;
    size_t i = 0;
    for (int32_t f = 0; f < n; ++f) {
        peak_start[f] = k;
        size_t e = i;
        while (e < pk.size() && fp(pk[e]) == f) ++e;
        const bool filter = min_separation > 0 && e - i > 1;
        for (; i < e; ++i) {
            const int32_t W = width(pk[i]);
            const int32_t y = pk[i].lin / W, x = pk[i].lin - y * W;
            bool ok = true;
            if (filter)
                for (int32_t j = peak_start[f]; j < k && ok; ++j) {
                    const double dy = (double)peak_yx[2 * j] - y, dx = (double)peak_yx[2 * j + 1] - x;
                    if (dy * dy + dx * dx < min2) ok = false;
                }
            if (!ok) continue;
            peak_yx[2 * k] = y;
            peak_yx[2 * k + 1] = x;
            peak_flux[k] = pk[i].flux;
            ++k;
        }
    }
    peak_start[n] = k;
}

}  // namespace
}  // namespace smi
