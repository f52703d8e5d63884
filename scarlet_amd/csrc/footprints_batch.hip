// Footprints and peaks of a ragged list of device-resident planes: the rules of footprints.hip
// (its header comment; the device code of both files is footprints_device.h) for planes whose
// frames differ and that may lie anywhere in device memory, in one chain of launches whatever
// the number of planes.  Labels stay indices inside the plane's own frame, so the ranks are the
// host's seed order per plane and every result equals footprints.hip's for that plane alone.
//
// The plane table (smi_footprint_plane, one record per plane, uploaded once per call into the
// work buffer) carries the address of the plane's first pixel, h, w and three exclusive
// prefixes over the planes: pixels (the plane's place in the flat label / record arrays), 64 x 64
// tiles and scan chunks of kChunk pixels.  The host adds a fourth, blocks of kT border pixels.
// A kernel launches over all tiles, chunks or border blocks of all planes; a workgroup finds
// its plane by a binary search of the prefix column -- uniform per workgroup, so scalar work --
// and a tile, chunk or border block never spans two planes.  A plane of one tile has no border
// block: a zero entry of that prefix, which the search steps over.
//
// Label chain, as label_planes of footprints.hip: 1 tile label, 2 border merge (launched only
// when some plane has more than one tile), 3 flatten, 4 records, 5 keep flags and chunk sums,
// 6 scan of the chunk sums (one workgroup per plane, grid-strided beyond 65535 planes), 7 rank
// and mask offset, 8 peak count; then one download of the per-plane totals.  Passes 3, 4 and 8
// map a workgroup to a tile, a wavefront to 64 pixels of one row.
// Fetch chain, once for all planes: the host turns the totals into exclusive offsets over the
// planes; the kept records go out in (plane, rank) order, then all mask bytes (one thread per
// byte, a binary search of the box offsets), then all peak records, which carry their plane;
// one download, one wait.  The host sorts the peaks by (plane, rank, flux descending, index
// ascending) and filters them per footprint (select_peaks).
// No workgroup waits for another, and parent words are read and written with agent-scope
// atomics in passes 2 and 3, as in footprints.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "footprints_device.h"

namespace smi {
namespace {

constexpr int64_t kGridCap = 1 << 20;  // workgroups of a launch; the kernels stride beyond

struct PeakBatchDev {
    int32_t plane, rank, lin, pad;
    double flux;
};

// the work buffer, as the kernels see it
struct BatchWork {
    const smi_footprint_plane *tb;  // [n]
    const int64_t *border0;         // [n + 1]: first border block of every plane
    int32_t *label;                 // plane p at tb[p].pixel_off
    int32_t *rec;                   // plane p: [kRec][h * w] at kRec * tb[p].pixel_off
    long long *part;                // chunk c of plane p at 2 * (tb[p].chunk0 + c)
    long long *tot;                 // [n][4]: kept, mask bytes, peaks
    int32_t n;
};

struct BatchLayout {
    int64_t pixels, tiles, chunks, border_blocks;  // totals over the planes
    int64_t table, border, label, rec, part, tot, total;  // byte offsets
};

// the table's prefixes are checked against the shapes, so that no kernel indexes outside the
// work buffer whatever the caller wrote
int batch_layout(const smi_footprint_plane *tb, int32_t n, BatchLayout *l,
                 std::vector<int64_t> *border0) {
    SMI_REQUIRE(tb, "footprints batch: null plane table");
    SMI_REQUIRE(n > 0, "footprints batch: no planes");
    int64_t pix = 0, tiles = 0, chunks = 0, border = 0;
    if (border0) border0->assign((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int64_t h = tb[i].h, w = tb[i].w;
        SMI_REQUIRE(h > 0 && w > 0, "footprints batch: empty plane");
        SMI_REQUIRE(h * w <= INT32_MAX, "footprints batch: more than 2^31 - 1 pixels in a plane");
        SMI_REQUIRE(tb[i].pixel_off == pix && tb[i].tile0 == tiles && tb[i].chunk0 == chunks,
                    "footprints batch: the table's prefixes do not fit its shapes");
        if (border0) (*border0)[i] = border;
        pix += h * w;
        tiles += ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
        chunks += nchunks(h * w);
        border += (border_pixels((int)h, (int)w) + kT - 1) / kT;
    }
    if (border0) (*border0)[n] = border;
    SMI_REQUIRE(tiles <= INT32_MAX && chunks <= INT32_MAX && border <= INT32_MAX,
                "footprints batch: more than 2^31 - 1 tiles");
    l->pixels = pix;
    l->tiles = tiles;
    l->chunks = chunks;
    l->border_blocks = border;
    l->table = 0;
    l->border = l->table + align16((int64_t)n * (int64_t)sizeof(smi_footprint_plane));
    l->label = l->border + align16(((int64_t)n + 1) * 8);
    l->rec = l->label + align16(pix * 4);
    l->part = l->rec + align16(pix * kRec * 4);
    l->tot = l->part + align16(chunks * 16);
    l->total = l->tot + (int64_t)n * 32;
    return SMI_OK;
}

BatchWork carve(void *d_work, const BatchLayout &l, int32_t n) {
    char *p = (char *)d_work;
    BatchWork w;
    w.tb = (const smi_footprint_plane *)(p + l.table);
    w.border0 = (const int64_t *)(p + l.border);
    w.label = (int32_t *)(p + l.label);
    w.rec = (int32_t *)(p + l.rec);
    w.part = (long long *)(p + l.part);
    w.tot = (long long *)(p + l.tot);
    w.n = n;
    return w;
}

// the last i of [0, n) with at(i) <= v; at() ascending, at(0) = 0 <= v
template <typename F>
__device__ __forceinline__ int last_not_above(int n, int64_t v, F at) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (at(mid) <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the plane of tile t, and the tile's place in it
struct TileOf {
    smi_footprint_plane p;
    int pl, tx, ty;
};
__device__ __forceinline__ TileOf tile_of(const BatchWork &b, int64_t t) {
    TileOf o;
    o.pl = last_not_above(b.n, t, [&](int i) { return b.tb[i].tile0; });
    o.p = b.tb[o.pl];
    const int tiles_x = (o.p.w + kTile - 1) / kTile, local = (int)(t - o.p.tile0);
    o.ty = local / tiles_x;
    o.tx = local - o.ty * tiles_x;
    return o;
}
__device__ __forceinline__ int plane_of_chunk(const BatchWork &b, int64_t c) {
    return last_not_above(b.n, c, [&](int i) { return b.tb[i].chunk0; });
}

// pass 1.  grid min(tiles, kGridCap), block (64, kRows) -- as are passes 3, 4, 8 and the peaks
template <typename T>
__global__ __launch_bounds__(kT) void tile_label_batch(BatchWork b, double th, int64_t n_tiles) {
    __shared__ int lab[kTile * kTile];
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileOf o = tile_of(b, t);
        label_tile<T>((const T *)o.p.address, b.label + o.p.pixel_off, o.p.h, o.p.w, th, o.tx,
                      o.ty, lab);
    }
}

// pass 2.  grid min(border blocks, kGridCap), block kT: block j of a plane holds its border
// pixels [j * kT, (j + 1) * kT)
__global__ __launch_bounds__(kT) void merge_borders_batch(BatchWork b, int64_t n_blocks) {
    for (int64_t g = blockIdx.x; g < n_blocks; g += gridDim.x) {
        const int pl = last_not_above(b.n, g, [&](int i) { return b.border0[i]; });
        const smi_footprint_plane p = b.tb[pl];
        const int64_t tiles_x = (p.w + kTile - 1) / kTile;
        const int64_t nv = (tiles_x - 1) * p.h, k = (g - b.border0[pl]) * kT + threadIdx.x;
        if (k < border_pixels(p.h, p.w)) merge_border_pixel(b.label + p.pixel_off, p.h, p.w, nv, k);
    }
}

// pass 3
__global__ __launch_bounds__(kT) void flatten_batch(BatchWork b, int64_t n_tiles) {
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileOf o = tile_of(b, t);
        const int H = o.p.h, W = o.p.w, x = o.tx * kTile + threadIdx.x;
        if (x >= W) continue;
        const int64_t N = (int64_t)H * W;
        for (int r = 0; r < kTile / kRows; ++r) {
            const int y = o.ty * kTile + r * kRows + threadIdx.y;
            if (y < H)
                flatten_pixel(b.label + o.p.pixel_off, b.rec + kRec * o.p.pixel_off, N, H, W,
                              y * W + x);
        }
    }
}

// pass 4
__global__ __launch_bounds__(kT) void records_batch(BatchWork b, int64_t n_tiles) {
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileOf o = tile_of(b, t);
        const int H = o.p.h, W = o.p.w;
        const int64_t N = (int64_t)H * W;
        for (int r = 0; r < kTile / kRows; ++r) {
            const int y = o.ty * kTile + r * kRows + threadIdx.y;  // one row per wavefront
            if (y < H)
                record_row(b.label + o.p.pixel_off, b.rec + kRec * o.p.pixel_off, N, W, y,
                           o.tx * kTile);
        }
    }
}

// passes 5 and 7.  grid min(chunks, kGridCap), block kT
template <int FINAL>
__global__ __launch_bounds__(kT) void rank_batch(BatchWork b, int min_area, int64_t n_chunks) {
    __shared__ long long sh[kT / 64];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const smi_footprint_plane p = b.tb[plane_of_chunk(b, c)];
        rank_chunk<FINAL>(b.label + p.pixel_off, b.rec + kRec * p.pixel_off,
                          (int64_t)p.h * p.w, min_area, b.part + 2 * c, c - p.chunk0, sh);
    }
}

// pass 6.  One workgroup per plane; grid min(n, kMaxGrid), block kT
__global__ __launch_bounds__(kT) void chunk_scan_batch(BatchWork b) {
    __shared__ long long sh[kT / 64];
    for (int pl = blockIdx.x; pl < b.n; pl += gridDim.x) {
        const smi_footprint_plane p = b.tb[pl];
        scan_chunk_sums(b.part + 2 * p.chunk0, nchunks((int64_t)p.h * p.w), b.tot + 4 * pl, sh);
    }
}

// pass 8 (EMIT 0): tot[plane][2] += peaks, one add per wavefront.  Fetch (EMIT 1): the peaks of
// all planes go to out[] in arrival order, slots from *counter; a slot beyond `cap` (the sum of
// the counts of pass 8) is not written
template <typename T, int EMIT>
__global__ __launch_bounds__(kT) void peaks_batch(BatchWork b, int64_t n_tiles, PeakBatchDev *out,
                                                  unsigned int *counter, unsigned int cap) {
    const int lane = threadIdx.x;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileOf o = tile_of(b, t);
        const int H = o.p.h, W = o.p.w, x = o.tx * kTile + lane;
        const int64_t N = (int64_t)H * W;
        const T *im = (const T *)o.p.address;
        const int32_t *lab = b.label + o.p.pixel_off, *rc = b.rec + kRec * o.p.pixel_off;
        for (int r = 0; r < kTile / kRows; ++r) {
            const int y = o.ty * kTile + r * kRows + threadIdx.y;
            if (y >= H) continue;  // the whole wavefront
            int rank = -1;
            T v = T(0);
            const bool peak = x < W && peak_at<T>(im, lab, rc, N, W, y, x, &rank, &v);
            const unsigned long long m = __ballot(peak);
            if (!m) continue;
            const int leader = __ffsll((long long)m) - 1;
            if (!EMIT) {
                if (lane == leader)
                    atomicAdd((unsigned long long *)(b.tot + 4 * o.pl + 2),
                              (unsigned long long)__popcll(m));
            } else {
                unsigned int base = 0;
                if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(m));
                base = __shfl(base, leader, 64);
                const unsigned int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                if (peak && slot < cap) {
                    out[slot].plane = o.pl;
                    out[slot].rank = rank;
                    out[slot].lin = y * W + x;
                    out[slot].pad = 0;
                    out[slot].flux = (double)v;
                }
            }
        }
    }
}

// what the fetch kernels write: footprint f = fp0[plane] + rank
struct FetchDev {
    const int32_t *fp0, *m0;  // [n + 1]: first footprint and first mask byte of every plane
    int32_t *bounds;          // [f][4]
    int32_t *moff, *roots, *plane;  // [f]: first mask byte, root and plane
};

// fetch.  grid min(chunks, kGridCap), block kT
__global__ __launch_bounds__(kT) void compact_batch(BatchWork b, FetchDev f, int64_t n_chunks) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int pl = plane_of_chunk(b, c);
        const smi_footprint_plane p = b.tb[pl];
        const int64_t N = (int64_t)p.h * p.w;
        const int32_t *lab = b.label + p.pixel_off, *rc = b.rec + kRec * p.pixel_off;
        for (int k = 0; k < kChunk / kT; ++k) {
            const int64_t q = (c - p.chunk0) * kChunk + k * kT + threadIdx.x;
            if (q >= N || lab[q] != (int)q) continue;
            const int r = rc[R_RANK * N + q];
            // (a rank beyond the caller's count of this plane has no slot)
            if (r < 0 || r >= f.fp0[pl + 1] - f.fp0[pl]) continue;
            const int g = f.fp0[pl] + r;
            f.bounds[4 * g] = rc[R_Y0 * N + q];
            f.bounds[4 * g + 1] = rc[R_Y1 * N + q];
            f.bounds[4 * g + 2] = rc[R_X0 * N + q];
            f.bounds[4 * g + 3] = rc[R_X1 * N + q];
            f.moff[g] = f.m0[pl] + rc[R_MOFF * N + q];
            f.roots[g] = (int)q;
            f.plane[g] = pl;
        }
    }
}

// fetch: one thread per mask byte of all planes; its footprint is the last with moff <= byte
__global__ __launch_bounds__(kT) void masks_batch(BatchWork b, FetchDev f, int n_fp,
                                                  int64_t n_bytes, uint8_t *masks) {
    for (int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x; k < n_bytes;
         k += (int64_t)gridDim.x * kT) {
        const int g = last_not_above(n_fp, k, [&](int i) { return (int64_t)f.moff[i]; });
        const smi_footprint_plane p = b.tb[f.plane[g]];
        masks[k] = mask_byte(b.label + p.pixel_off, p.w, f.bounds + 4 * g, f.roots[g],
                             k - f.moff[g]);
    }
}

struct Stats {
    int32_t launches = 0, syncs = 0;
    void report(int32_t *out) const {
        if (out) {
            out[0] = launches;
            out[1] = syncs;
        }
    }
};

unsigned grid_of(int64_t n) { return (unsigned)std::min<int64_t>(n, kGridCap); }

template <typename T>
int check_addresses(const smi_footprint_plane *tb, int32_t n) {
    for (int32_t i = 0; i < n; ++i)
        SMI_REQUIRE(tb[i].address != 0 && tb[i].address % sizeof(T) == 0,
                    "footprints batch: null or misaligned plane address");
    return SMI_OK;
}

template <typename T>
int label_batch(const smi_footprint_plane *tb, int32_t n, int32_t min_area, int32_t thresh,
                void *d_work, int64_t work_size, int32_t *counts, int32_t *stats, void *stream) {
    BatchLayout l;
    std::vector<int64_t> border0;
    int rc = batch_layout(tb, n, &l, &border0);
    if (rc) return rc;
    rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_work && counts, "null argument");
    SMI_REQUIRE(work_size >= l.total, "work buffer too small");
    rc = check_addresses<T>(tb, n);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BatchWork w = carve(d_work, l, n);
    Stats s;

    // the table and the border prefix, one upload (the label array follows them)
    std::vector<char> up((size_t)l.label, 0);
    std::memcpy(up.data() + l.table, tb, (size_t)n * sizeof(smi_footprint_plane));
    std::memcpy(up.data() + l.border, border0.data(), border0.size() * 8);
    SMI_HIP(hipMemcpyAsync(d_work, up.data(), up.size(), hipMemcpyHostToDevice, st));

    const dim3 block2(64, kRows);
    const unsigned gt = grid_of(l.tiles), gc = grid_of(l.chunks);
    hipLaunchKernelGGL(tile_label_batch<T>, dim3(gt), block2, 0, st, w, (double)thresh, l.tiles);
    ++s.launches;
    if (l.border_blocks > 0) {
        hipLaunchKernelGGL(merge_borders_batch, dim3(grid_of(l.border_blocks)), dim3(kT), 0, st, w,
                           l.border_blocks);
        ++s.launches;
    }
    hipLaunchKernelGGL(flatten_batch, dim3(gt), block2, 0, st, w, l.tiles);
    hipLaunchKernelGGL(records_batch, dim3(gt), block2, 0, st, w, l.tiles);
    hipLaunchKernelGGL(rank_batch<0>, dim3(gc), dim3(kT), 0, st, w, min_area, l.chunks);
    hipLaunchKernelGGL(chunk_scan_batch, dim3((unsigned)std::min<int32_t>(n, kMaxGrid)), dim3(kT),
                       0, st, w);
    hipLaunchKernelGGL(rank_batch<1>, dim3(gc), dim3(kT), 0, st, w, min_area, l.chunks);
    hipLaunchKernelGGL((peaks_batch<T, 0>), dim3(gt), block2, 0, st, w, l.tiles,
                       (PeakBatchDev *)nullptr, (unsigned int *)nullptr, 0u);
    s.launches += 6;
    SMI_HIP(hipGetLastError());
    std::vector<long long> tot((size_t)n * 4);
    SMI_HIP(hipMemcpyAsync(tot.data(), w.tot, tot.size() * sizeof(long long),
                           hipMemcpyDeviceToHost, st));
    SMI_HIP(hipStreamSynchronize(st));
    ++s.syncs;
    s.report(stats);
    long long sum[3] = {0, 0, 0};
    for (int32_t pl = 0; pl < n; ++pl)
        for (int k = 0; k < 3; ++k) {
            sum[k] += tot[4 * (size_t)pl + k];
            if (sum[k] > INT32_MAX) {
                set_error("footprints batch: more than 2^31 - 1 footprints, mask pixels or peaks");
                return SMI_ERR_INVALID;
            }
        }
    for (int32_t pl = 0; pl < n; ++pl)
        for (int k = 0; k < 3; ++k) counts[3 * (size_t)pl + k] = (int32_t)tot[4 * (size_t)pl + k];
    return SMI_OK;
}

// layout of the fetch scratch for counts[n][3] = (footprints, mask bytes, peaks) per plane
struct BatchScratch {
    int64_t n_fp, n_mask, n_peak;                 // totals
    int64_t fp0, m0, moff, roots, plane;          // byte offsets: what only the device reads
    int64_t out, bounds, counter, peaks, masks;   // ... and the block that is downloaded whole
    int64_t total;
};
int scratch_layout(int32_t n, const int32_t *counts, BatchScratch *s) {
    SMI_REQUIRE(n > 0 && counts, "footprints batch: no counts");
    int64_t sum[3] = {0, 0, 0};
    for (int32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            SMI_REQUIRE(counts[3 * (size_t)i + k] >= 0, "bad counts");
            sum[k] += counts[3 * (size_t)i + k];
        }
    SMI_REQUIRE(sum[0] <= INT32_MAX && sum[1] <= INT32_MAX && sum[2] <= INT32_MAX,
                "footprints batch: more than 2^31 - 1 footprints, mask pixels or peaks");
    s->n_fp = sum[0];
    s->n_mask = sum[1];
    s->n_peak = sum[2];
    s->fp0 = 0;
    s->m0 = s->fp0 + align16(4 * ((int64_t)n + 1));
    s->moff = s->m0 + align16(4 * ((int64_t)n + 1));
    s->roots = s->moff + align16(4 * sum[0]);
    s->plane = s->roots + align16(4 * sum[0]);
    s->out = s->plane + align16(4 * sum[0]);
    s->bounds = s->out;
    s->counter = s->bounds + 16 * sum[0];
    s->peaks = s->counter + 16;
    s->masks = s->peaks + (int64_t)sizeof(PeakBatchDev) * sum[2];
    s->total = s->masks + align16(sum[1]);
    return SMI_OK;
}

template <typename T>
int fetch_batch(const smi_footprint_plane *tb, int32_t n, double min_separation,
                const int32_t *counts, const void *d_work, void *d_scratch, int64_t scratch_size,
                int32_t *bounds, uint8_t *masks, int32_t *fp_start, int32_t *peak_start,
                int32_t *peak_yx, double *peak_flux, int32_t *stats, void *stream) {
    BatchLayout l;
    int rc = batch_layout(tb, n, &l, nullptr);
    if (rc) return rc;
    BatchScratch sl;
    rc = scratch_layout(n, counts, &sl);
    if (rc) return rc;
    rc = have_device();
    if (rc) return rc;
    SMI_REQUIRE(d_work && fp_start && peak_start, "null argument");
    Stats s;
    // first footprint and first mask byte of every plane
    std::vector<int32_t> off(2 * ((size_t)n + 1) + 8, 0);
    int32_t *fp0 = off.data(), *m0 = off.data() + (sl.m0 - sl.fp0) / 4;
    for (int32_t i = 0; i < n; ++i) {
        fp0[i + 1] = fp0[i] + counts[3 * (size_t)i];
        m0[i + 1] = m0[i] + counts[3 * (size_t)i + 1];
    }
    std::memcpy(fp_start, fp0, ((size_t)n + 1) * 4);
    const int32_t n_fp = (int32_t)sl.n_fp, np = (int32_t)sl.n_peak;
    if (n_fp == 0) {
        peak_start[0] = 0;
        s.report(stats);
        return SMI_OK;
    }
    SMI_REQUIRE(bounds && masks, "null argument");
    SMI_REQUIRE((peak_yx && peak_flux) || np == 0, "null peak arrays");
    SMI_REQUIRE(d_scratch && scratch_size >= sl.total, "scratch buffer too small");
    rc = check_addresses<T>(tb, n);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BatchWork w = carve(const_cast<void *>(d_work), l, n);
    char *sc = (char *)d_scratch;
    FetchDev f;
    f.fp0 = (const int32_t *)(sc + sl.fp0);
    f.m0 = (const int32_t *)(sc + sl.m0);
    f.bounds = (int32_t *)(sc + sl.bounds);
    f.moff = (int32_t *)(sc + sl.moff);
    f.roots = (int32_t *)(sc + sl.roots);
    f.plane = (int32_t *)(sc + sl.plane);
    unsigned int *d_counter = (unsigned int *)(sc + sl.counter);
    PeakBatchDev *d_peaks = (PeakBatchDev *)(sc + sl.peaks);

    SMI_HIP(hipMemcpyAsync(sc + sl.fp0, off.data(), (size_t)(sl.moff - sl.fp0),
                           hipMemcpyHostToDevice, st));
    SMI_HIP(hipMemsetAsync(d_counter, 0, 16, st));
    hipLaunchKernelGGL(compact_batch, dim3(grid_of(l.chunks)), dim3(kT), 0, st, w, f, l.chunks);
    hipLaunchKernelGGL(masks_batch, dim3(grid_of((sl.n_mask + kT - 1) / kT)), dim3(kT), 0, st, w,
                       f, n_fp, sl.n_mask, (uint8_t *)(sc + sl.masks));
    s.launches += 2;
    if (np > 0) {
        hipLaunchKernelGGL((peaks_batch<T, 1>), dim3(grid_of(l.tiles)), dim3(64, kRows), 0, st, w,
                           l.tiles, d_peaks, d_counter, (unsigned int)np);
        ++s.launches;
    }
    SMI_HIP(hipGetLastError());
    // bounds, the counter, the peak records and the mask bytes lie one after another
    std::vector<char> host((size_t)(sl.masks + sl.n_mask - sl.out));
    SMI_HIP(hipMemcpyAsync(host.data(), sc + sl.out, host.size(), hipMemcpyDeviceToHost, st));
    SMI_HIP(hipStreamSynchronize(st));
    ++s.syncs;
    s.report(stats);
    unsigned int emitted = 0;
    std::memcpy(&emitted, host.data() + (sl.counter - sl.out), sizeof(emitted));
    SMI_REQUIRE(emitted == (unsigned int)np,
                "footprints batch: the images changed since they were labelled");
    std::memcpy(bounds, host.data() + (sl.bounds - sl.out), 16 * (size_t)n_fp);
    std::memcpy(masks, host.data() + (sl.masks - sl.out), (size_t)sl.n_mask);
    std::vector<PeakBatchDev> pk((size_t)np);
    if (np > 0)
        std::memcpy(pk.data(), host.data() + (sl.peaks - sl.out), sizeof(PeakBatchDev) * (size_t)np);

    std::sort(pk.begin(), pk.end(), [](const PeakBatchDev &a, const PeakBatchDev &b) {
        if (a.plane != b.plane) return a.plane < b.plane;
        if (a.rank != b.rank) return a.rank < b.rank;
        return peak_before(a, b);
    });
    select_peaks(
        pk, n_fp, [fp0](const PeakBatchDev &p) { return fp0[p.plane] + p.rank; },
        [tb](const PeakBatchDev &p) { return tb[p.plane].w; }, min_separation, peak_start,
        peak_yx, peak_flux);
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_footprints_batch_work_bytes(int32_t n_planes, const smi_footprint_plane *table,
                                    int64_t *bytes) {
    SMI_REQUIRE(bytes, "null argument");
    smi::BatchLayout l;
    int rc = smi::batch_layout(table, n_planes, &l, nullptr);
    if (rc) return rc;
    *bytes = l.total;
    return SMI_OK;
}
int smi_footprints_batch_fetch_bytes(int32_t n_planes, const int32_t *counts, int64_t *bytes) {
    SMI_REQUIRE(bytes, "null argument");
    smi::BatchScratch s;
    int rc = smi::scratch_layout(n_planes, counts, &s);
    if (rc) return rc;
    *bytes = s.total;
    return SMI_OK;
}
int smi_footprints_batch_label_f32(const smi_footprint_plane *table, int32_t n_planes,
                                   int32_t min_area, int32_t thresh, void *d_work,
                                   int64_t work_bytes, int32_t *counts, int32_t *stats,
                                   void *stream) {
    return smi::label_batch<float>(table, n_planes, min_area, thresh, d_work, work_bytes, counts,
                                   stats, stream);
}
int smi_footprints_batch_label_f64(const smi_footprint_plane *table, int32_t n_planes,
                                   int32_t min_area, int32_t thresh, void *d_work,
                                   int64_t work_bytes, int32_t *counts, int32_t *stats,
                                   void *stream) {
    return smi::label_batch<double>(table, n_planes, min_area, thresh, d_work, work_bytes, counts,
                                    stats, stream);
}
int smi_footprints_batch_fetch_f32(const smi_footprint_plane *table, int32_t n_planes,
                                   double min_separation, const int32_t *counts,
                                   const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                   int32_t *bounds, uint8_t *masks, int32_t *fp_start,
                                   int32_t *peak_start, int32_t *peak_yx, double *peak_flux,
                                   int32_t *stats, void *stream) {
    return smi::fetch_batch<float>(table, n_planes, min_separation, counts, d_work, d_scratch,
                                   scratch_bytes, bounds, masks, fp_start, peak_start, peak_yx,
                                   peak_flux, stats, stream);
}
int smi_footprints_batch_fetch_f64(const smi_footprint_plane *table, int32_t n_planes,
                                   double min_separation, const int32_t *counts,
                                   const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                   int32_t *bounds, uint8_t *masks, int32_t *fp_start,
                                   int32_t *peak_start, int32_t *peak_yx, double *peak_flux,
                                   int32_t *stats, void *stream) {
    return smi::fetch_batch<double>(table, n_planes, min_separation, counts, d_work, d_scratch,
                                    scratch_bytes, bounds, masks, fp_start, peak_start, peak_yx,
                                    peak_flux, stats, stream);
}

}  // extern "C"
