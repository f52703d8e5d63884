// Footprints and peaks of a detection image, the behaviour of the reference's
// scarlet.detect_pybind11.get_footprints (used by detect.get_blend_structures).
//
// A footprint is a 4-connected set of pixels > thresh (an integer threshold, as the
// reference's `const int thresh`), found from seeds in raster order, with inclusive bounds
// (y0, y1, x0, x1).  It is kept when its box has more than min_area pixels and it has at least
// min_area pixels of its own.  Its peaks are the strict maxima over the existing 8 neighbours
// in the box, with the pixels outside the footprint set to 0, brightest first (a stable sort:
// equal fluxes keep raster order); with min_separation > 0 a peak closer than that to a
// brighter kept one is dropped.  A footprint without a strict maximum (a plateau) keeps an
// empty peak list.
//
// Host code: a labelling pass with branches at every pixel, O(H W), and the results are
// needed on the host.  The fill keeps its own stack, so a footprint of any size works.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace smi {
namespace {

struct PeakRec {
    int32_t y, x;
    double flux;
};

struct FootprintRec {
    int32_t bounds[4];
    std::vector<uint8_t> mask;  // (y1-y0+1) x (x1-x0+1)
    std::vector<PeakRec> peaks;
};

// the result of the last smi_get_footprints_* call on this thread, until it is fetched
thread_local std::vector<FootprintRec> g_footprints;

template <typename T>
std::vector<PeakRec> patch_peaks(const std::vector<T> &patch, int h, int w, int y0, int x0,
                                 double min_separation) {
    std::vector<PeakRec> peaks;
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const T v = patch[(size_t)i * w + j];
            bool peak = true;
            for (int di = -1; di <= 1 && peak; ++di)
                for (int dj = -1; dj <= 1; ++dj) {
                    if (!di && !dj) continue;
                    const int a = i + di, b = j + dj;
                    if (a < 0 || a >= h || b < 0 || b >= w) continue;
                    if (v <= patch[(size_t)a * w + b]) {
                        peak = false;
                        break;
                    }
                }
            if (peak) peaks.push_back({i + y0, j + x0, (double)v});
        }
    std::stable_sort(peaks.begin(), peaks.end(),
                     [](const PeakRec &a, const PeakRec &b) { return a.flux > b.flux; });
    if (min_separation > 0 && peaks.size() > 1) {
        const double min2 = min_separation * min_separation;
        std::vector<PeakRec> kept;
        for (const PeakRec &p : peaks) {
            bool ok = true;
            for (const PeakRec &k : kept) {
                const double dy = (double)k.y - p.y, dx = (double)k.x - p.x;
                if (dy * dy + dx * dx < min2) {
                    ok = false;
                    break;
                }
            }
            if (ok) kept.push_back(p);
        }
        peaks.swap(kept);
    }
    return peaks;
}

template <typename T>
int get_footprints(const T *image, int32_t H, int32_t W, double min_separation,
                   int32_t min_area, int32_t thresh, int32_t *counts) {
    SMI_REQUIRE(image && counts, "null argument");
    SMI_REQUIRE(H > 0 && W > 0, "bad sizes");
    g_footprints.clear();
    const size_t N = (size_t)H * W;
    const double th = (double)thresh;
    std::vector<uint8_t> seen(N, 0);
    std::vector<int32_t> stack, members;
    int64_t mask_bytes = 0, n_peaks = 0;
    for (int32_t i = 0; i < H; ++i)
        for (int32_t j = 0; j < W; ++j) {
            const size_t s = (size_t)i * W + j;
            if (seen[s] || !((double)image[s] > th)) continue;
            int32_t b[4] = {i, i, j, j};
            members.clear();
            stack.assign(1, (int32_t)s);
            seen[s] = 1;
            while (!stack.empty()) {
                const int32_t p = stack.back();
                stack.pop_back();
                members.push_back(p);
                const int32_t y = p / W, x = p - y * W;
                b[0] = std::min(b[0], y);
                b[1] = std::max(b[1], y);
                b[2] = std::min(b[2], x);
                b[3] = std::max(b[3], x);
                const int32_t nb[4] = {y > 0 ? p - W : -1, y < H - 1 ? p + W : -1,
                                       x > 0 ? p - 1 : -1, x < W - 1 ? p + 1 : -1};
                for (int k = 0; k < 4; ++k) {
                    const int32_t q = nb[k];
                    if (q < 0 || seen[q] || !((double)image[q] > th)) continue;
                    seen[q] = 1;
                    stack.push_back(q);
                }
            }
            const int h = b[1] - b[0] + 1, w = b[3] - b[2] + 1;
            if (!((int64_t)h * w > min_area) || !((int64_t)members.size() >= min_area)) continue;
            FootprintRec fp;
            std::copy(b, b + 4, fp.bounds);
            fp.mask.assign((size_t)h * w, 0);
            std::vector<T> patch((size_t)h * w, T(0));
            for (int32_t p : members) {
                const int32_t y = p / W - b[0], x = p % W - b[2];
                fp.mask[(size_t)y * w + x] = 1;
                patch[(size_t)y * w + x] = image[p];
            }
            fp.peaks = patch_peaks<T>(patch, h, w, b[0], b[2], min_separation);
            mask_bytes += (int64_t)h * w;
            n_peaks += (int64_t)fp.peaks.size();
            g_footprints.push_back(std::move(fp));
        }
    if (mask_bytes > INT32_MAX || n_peaks > INT32_MAX) {
        g_footprints.clear();
        set_error("footprints: more than 2^31 mask pixels or peaks");
        return SMI_ERR_INVALID;
    }
    counts[0] = (int32_t)g_footprints.size();
    counts[1] = (int32_t)mask_bytes;
    counts[2] = (int32_t)n_peaks;
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_get_footprints_f32(const float *image, int32_t H, int32_t W, double min_separation,
                           int32_t min_area, int32_t thresh, int32_t *counts) {
    return smi::get_footprints<float>(image, H, W, min_separation, min_area, thresh, counts);
}
int smi_get_footprints_f64(const double *image, int32_t H, int32_t W, double min_separation,
                           int32_t min_area, int32_t thresh, int32_t *counts) {
    return smi::get_footprints<double>(image, H, W, min_separation, min_area, thresh, counts);
}

int smi_footprints_fetch(int32_t *bounds, uint8_t *masks, int32_t *peak_start, int32_t *peak_yx,
                         double *peak_flux) {
    auto &fps = smi::g_footprints;
    int64_t npk = 0;
    for (const auto &fp : fps) npk += (int64_t)fp.peaks.size();
    SMI_REQUIRE((bounds && masks && peak_start) || fps.empty(), "null argument");
    SMI_REQUIRE((peak_yx && peak_flux) || npk == 0, "null peak arrays");
    size_t m = 0;
    int32_t k = 0;
    for (size_t f = 0; f < fps.size(); ++f) {
        const auto &fp = fps[f];
        std::copy(fp.bounds, fp.bounds + 4, bounds + 4 * f);
        std::copy(fp.mask.begin(), fp.mask.end(), masks + m);
        m += fp.mask.size();
        peak_start[f] = k;
        for (const auto &p : fp.peaks) {
            peak_yx[2 * k] = p.y;
            peak_yx[2 * k + 1] = p.x;
            peak_flux[k] = p.flux;
            ++k;
        }
    }
    if (peak_start) peak_start[fps.size()] = k;
    fps.clear();
    return SMI_OK;
}

}  // extern "C"
