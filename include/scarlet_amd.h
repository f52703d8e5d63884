/*
 * scarlet_amd.h -- C ABI of libscarlet_amd.so, the MI355X (gfx950) back end for
 * the proximal-gradient fitting loop of pmelchior/scarlet.
 *
 * Plain C: pointers, sizes, POD structs.  All functions return 0 on success or a
 * negative smi_status; smi_last_error() gives the message of the last failure on
 * the calling thread.  Host pointers unless a parameter is named d_* (device).
 * Handles are not thread-safe; one smi_batch lives on one GPU.
 *
 * The entry points replace these reference interfaces (paths relative to the
 * reference checkout):
 *
 *   seam 1  scarlet/operators_pybind11.cc:234-260  (pybind11 module
 *           `scarlet.operators_pybind11`, called from scarlet/operator.py:54-58
 *           and scarlet/renderer.py:108-116)
 *             prox_weighted_monotonic  -> smi_prox_weighted_monotonic_{f32,f64}
 *             apply_filter             -> smi_apply_filter_{f32,f64}
 *
 *   seam 2  the optimizer call in scarlet/blend.py:165-180
 *           (proxmin.adaprox(X, grad, step, prox=..., scheme="amsgrad",
 *           prox_max_iter=10, M=, V=, Vhat=) together with the closures it is
 *           given: Blend._loss_func blend.py:259-274, Blend.get_model
 *           blend.py:200-244, Observation.get_log_likelihood
 *           observation.py:147-170, ConvolutionRenderer renderer.py:247-259,
 *           ConstraintChain constraint.py:76-80)
 *             -> smi_batch_* : the same loop for a batch of independent blends,
 *                resident on the device.
 */
#ifndef SCARLET_AMD_H
#define SCARLET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum smi_status {
    SMI_OK = 0,
    SMI_ERR_INVALID = -1,   /* bad argument (shape, NULL, out of range)            */
    SMI_ERR_HIP = -2,       /* HIP runtime / rocFFT failure                        */
    SMI_ERR_NO_DEVICE = -3, /* no usable GPU                                       */
    SMI_ERR_ARITHMETIC = -4 /* a parameter became non-finite (model.py:153-165)    */
} smi_status;

const char *smi_last_error(void);
int smi_device_count(void);
/* "scarlet_amd <version> gfx950" */
const char *smi_version(void);

/* ------------------------------------------------------------------------- *
 * Seam 1: operators_pybind11 drop-ins.  Caller owns all buffers; flat_img and
 * result are modified in place, like the Eigen::Ref arguments of the reference.
 * ------------------------------------------------------------------------- */

/* operators_pybind11.cc:14-36.  flat_img[n_pix]; weights[n_off][n_pix] row major;
 * offsets[n_off]; dist_idx[n_idx] = sweep order (peak excluded).  Sequential
 * (Gauss-Seidel) semantics are preserved exactly: the device kernel walks the
 * levels of the dependency graph, which yields bit-identical results. */
int smi_prox_weighted_monotonic_f32(float *flat_img, const float *weights,
                                    const int32_t *offsets, int32_t n_off,
                                    const int32_t *dist_idx, int32_t n_idx,
                                    int32_t n_pix, float min_gradient);
int smi_prox_weighted_monotonic_f64(double *flat_img, const double *weights,
                                    const int32_t *offsets, int32_t n_off,
                                    const int32_t *dist_idx, int32_t n_idx,
                                    int32_t n_pix, double min_gradient);

/* The same sweep for n_img independent images of n_pix pixels, every one with tables of its
 * own, in ONE launch (one workgroup per image): what the initialisation of a scene needs --
 * each source's detection image made monotonic about that source's centre (source.py:312-333
 * calls operators_pybind11.cc:14-36 once per source; initialization.py:287-363 loops over the
 * sources).  images[n_img][n_pix] in place; weights[n_img][n_off][n_pix]; dist_idx[n_img][n_idx];
 * offsets[n_off] shared.  Image i comes out bit for bit as smi_prox_weighted_monotonic_*(
 * images[i], weights[i], offsets, n_off, dist_idx[i], n_idx, n_pix, min_gradient) leaves it. */
int smi_prox_weighted_monotonic_many_f32(int32_t n_img, float *images, int32_t n_pix,
                                         const float *weights, const int32_t *offsets,
                                         int32_t n_off, const int32_t *dist_idx, int32_t n_idx,
                                         float min_gradient);
int smi_prox_weighted_monotonic_many_f64(int32_t n_img, double *images, int32_t n_pix,
                                         const double *weights, const int32_t *offsets,
                                         int32_t n_off, const int32_t *dist_idx, int32_t n_idx,
                                         double min_gradient);

/* operators_pybind11.cc:39-56.  image[H][W], result[H][W]; taps given as in the
 * reference: values[n_taps] and the four slice-bound vectors. */
int smi_apply_filter_f32(const float *image, int32_t H, int32_t W,
                         const float *values, int32_t n_taps,
                         const int32_t *y_start, const int32_t *y_end,
                         const int32_t *x_start, const int32_t *x_end,
                         float *result);
int smi_apply_filter_f64(const double *image, int32_t H, int32_t W,
                         const double *values, int32_t n_taps,
                         const int32_t *y_start, const int32_t *y_end,
                         const int32_t *x_start, const int32_t *x_end,
                         double *result);

/* scarlet/lite/measure.py:39-91 (weight_sources) for a catalogue of blends that share the
 * number of bands C and the (kh, kw) difference-kernel stamp: per blend the frame-clipped
 * scene, per source its own model, both convolved with the tap loop of apply_filter above
 * and clamped at 0; then out = min(model / total, 1) (0 where total == 0) * images on the
 * part of every source's grown box that lies in the frame.  Host buffers in, host buffer out;
 * all coordinates relative to the frame's corner; offsets and sizes count elements.
 *
 *   images[blend.image_off .. + C h w]   the (masked) images the ratio multiplies
 *   stamps[blend.stamp_off .. + C kh kw] the blend's stamp, one per band
 *   seds[component.sed_off .. + C], morphs[component.morph_off + y stride + x]
 *   out[source.out_off .. + C h w]       the source's result, [C][h][w]
 *
 * A blend's components [comp0, comp0 + n_comp) make its scene and must lie inside its frame
 * (the caller clips them: y0 / x0 / h / w describe the clipped rectangle, morph_off its first
 * pixel, stride the row length of the morphology); a source's components make its model
 * and may overhang.  The plan is validated before anything is launched: a bad one returns
 * SMI_ERR_INVALID.  Bit-identical to the per-band apply_filter chain of the reference. */
typedef struct smi_reweight_blend {
    int32_t h, w;           /* frame */
    int32_t comp0, n_comp;  /* components of the scene, in the order they are added */
    int64_t image_off, stamp_off;
} smi_reweight_blend;
typedef struct smi_reweight_source {
    int32_t blend;
    int32_t comp0, n_comp;  /* components of the source, in the order they are added */
    int32_t y0, x0, h, w;   /* output rectangle, inside the frame, not empty */
    int32_t reserved;
    int64_t out_off;
} smi_reweight_source;
typedef struct smi_reweight_component {
    int32_t y0, x0, h, w;   /* rectangle the component covers */
    int32_t stride, reserved;
    int64_t sed_off, morph_off;
} smi_reweight_component;
int smi_reweight_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                     const smi_reweight_blend *blends, int32_t n_sources,
                     const smi_reweight_source *sources, int32_t n_components,
                     const smi_reweight_component *components, const float *images,
                     int64_t n_image, const float *stamps, int64_t n_stamp, const float *seds,
                     int64_t n_sed, const float *morphs, int64_t n_morph, float *out,
                     int64_t n_out);
int smi_reweight_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                     const smi_reweight_blend *blends, int32_t n_sources,
                     const smi_reweight_source *sources, int32_t n_components,
                     const smi_reweight_component *components, const double *images,
                     int64_t n_image, const double *stamps, int64_t n_stamp, const double *seds,
                     int64_t n_sed, const double *morphs, int64_t n_morph, double *out,
                     int64_t n_out);

/* lite.measure_blends: the sums of a catalogue row over the flux cubes of smi_reweight_* above,
 * without the cubes having to leave the device.  Tables and input buffers are those of
 * smi_reweight_*, validated the same way (a bad plan returns SMI_ERR_INVALID before anything is
 * launched).  `out` may be NULL (then n_out must be 0 and out_off is ignored): no cube is
 * stored, allocated or copied; otherwise it receives bit for bit what smi_reweight_* writes.
 * records[(source * C + band) * SMI_LITE_MEASURE_RECORD + k], n_record >= n_sources * C *
 * SMI_LITE_MEASURE_RECORD, in float64, with f the source's flux, M its convolved model clipped
 * at 0, and y, x integers counted from the corner of the source's rectangle:
 *
 *   k = 0 sum M      2 sum f      4 sum x f      6 sum y x f    8 the largest f
 *       1 sum M^2    3 sum y f    5 sum y^2 f    7 sum x^2 f    9 y * w + x of its first pixel
 *
 * (row-major first, as np.argmax; -1 when no f compares: not-a-number data).  The order of
 * every sum depends on the (h, w) of the source's rectangle alone, so a source's record has the
 * same bits wherever it stands in the tables. */
#define SMI_LITE_MEASURE_RECORD 10
int smi_lite_measure_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_reweight_blend *blends, int32_t n_sources,
                         const smi_reweight_source *sources, int32_t n_components,
                         const smi_reweight_component *components, const float *images,
                         int64_t n_image, const float *stamps, int64_t n_stamp, const float *seds,
                         int64_t n_sed, const float *morphs, int64_t n_morph, float *out,
                         int64_t n_out, double *records, int64_t n_record);
int smi_lite_measure_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_reweight_blend *blends, int32_t n_sources,
                         const smi_reweight_source *sources, int32_t n_components,
                         const smi_reweight_component *components, const double *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp, const double *seds,
                         int64_t n_sed, const double *morphs, int64_t n_morph, double *out,
                         int64_t n_out, double *records, int64_t n_record);
/* milliseconds the three launches of the calling thread's last smi_lite_measure_* call took on
 * the device (events around them), for tools/lite_measure_time.py */
int smi_lite_measure_last_launch_ms(double *ms);

/* lite.fit_spectra_blends: the normal equations of multifit_seds (reference
 * scarlet/lite/initialization.py:140-186) for a catalogue of blends that share the number of
 * bands C and the (kh, kw) difference-kernel stamp.  Per blend and band, with one column per
 * component -- its morphology, zero outside its own box, convolved ("same") with the band's
 * stamp on the union box of all component boxes -- and d the image on the union box, zero
 * outside the frame:
 *
 *   out[blend.out_off + band (K K + K) + p K + q] = sum of column p x column q   (G, symmetric)
 *   out[blend.out_off + band (K K + K) + K K + p] = sum of column p x d          (r)
 *
 * in float64, K = n_comp.  Host buffers in, host buffer out; coordinates relative to the
 * frame's corner; offsets and sizes count elements.  images[blend.image_off .. + C h w];
 * stamps[blend.stamp_off .. + C kh kw] in float64; morphs[component.morph_off .. + h w], rows of
 * w.  The union box (y0, x0, fh, fw) must hold every component box.  Limits: stamp sides
 * <= 63, 1 .. 64 components per blend, at most 32 components whose box grown by the stamp's half
 * meets one 16 x 16 tile of the union box, union box and morphology sides <= 4096.  The plan
 * is validated before anything is launched: a bad one returns SMI_ERR_INVALID and leaves
 * `out` alone.  The sums of a blend have the same bits wherever it stands in the tables. */
typedef struct smi_lite_spectra_blend {
    int32_t h, w;            /* frame */
    int32_t y0, x0, fh, fw;  /* union box of the components, may leave the frame */
    int32_t comp0, n_comp;
    int64_t image_off, stamp_off, out_off;
} smi_lite_spectra_blend;
typedef struct smi_lite_spectra_component {
    int32_t y0, x0, h, w;    /* box of the morphology */
    int64_t morph_off;
} smi_lite_spectra_component;
int smi_lite_spectra_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_lite_spectra_blend *blends, int32_t n_components,
                         const smi_lite_spectra_component *components, const float *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp,
                         const float *morphs, int64_t n_morph, double *out, int64_t n_out);
int smi_lite_spectra_f64(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_blends,
                         const smi_lite_spectra_blend *blends, int32_t n_components,
                         const smi_lite_spectra_component *components, const double *images,
                         int64_t n_image, const double *stamps, int64_t n_stamp,
                         const double *morphs, int64_t n_morph, double *out, int64_t n_out);

/* measure_blends: the sums a catalogue row of scarlet.measure is made of, for the sources of
 * many blends that share the number of model bands C and the (kh, kw) stamp shape; three
 * launches.  Host buffers in, host buffers out; coordinates relative to the corner of the
 * source's frame; offsets and sizes count elements.
 *
 * A model pixel of band c is the sum over the source's components, in table order and in float64,
 * of the rounded products seds[sed_off + c] * morphs[morph_off + y w + x], zero outside a
 * component's box.
 *
 *   records[(source * C + c) * SMI_MEASURE_SOURCES_RECORD + k] over the source's box, y and x
 *   integers counted from its corner:
 *     k = 0 sum m    2 sum x m      4 sum y x m    6 the largest m
 *         1 sum y m  3 sum y^2 m    5 sum x^2 m    7 y * w + x of its first pixel (-1: none)
 *   rendered[(row + b) * 3 + q], row = the bands of all sources before this one, b the source's
 *   band (source.band0 + b of the band table): with R the model of bands[..].channel, what of it
 *   lies in the frame, convolved ("same", zero boundary, float64 over the float32 taps
 *   stamps[stamp_off .. + kh kw]) and W = weights[weight_off .. + fh fw], over the frame's
 *   pixels the source's box grown by the stamp's half reaches:
 *     q = 0 sum R    1 sum R^2    2 sum R^2 (1 / W)
 *
 * Limits: odd stamp sides <= 63, box and morphology sides <= 16384, a component's box inside its
 * source's.  Every table is validated before anything is launched: a bad one returns
 * SMI_ERR_INVALID and leaves the outputs alone.  The order of every sum depends on the source's
 * box, its frame and the stamp shape alone: a source's sums have the same bits wherever it
 * stands in the tables. */
typedef struct smi_measure_source {
    int32_t y0, x0, h, w;   /* box of the source's model, may leave the frame */
    int32_t fh, fw;         /* frame */
    int32_t comp0, n_comp;  /* its components, in the order they are added */
    int32_t band0, n_band;  /* the observed bands of its blend in the band table */
} smi_measure_source;
typedef struct smi_measure_component {
    int32_t y0, x0, h, w;   /* box of the morphology, inside the source's */
    int64_t sed_off, morph_off;
} smi_measure_component;
typedef struct smi_measure_band {
    int32_t channel, reserved;  /* model band this observed band renders */
    int64_t stamp_off, weight_off;
} smi_measure_band;
#define SMI_MEASURE_SOURCES_RECORD 8
int smi_measure_sources_f32(int32_t device, int32_t C, int32_t kh, int32_t kw, int32_t n_sources,
                            const smi_measure_source *sources, int32_t n_components,
                            const smi_measure_component *components, int32_t n_bands,
                            const smi_measure_band *bands, const double *seds, int64_t n_sed,
                            const double *morphs, int64_t n_morph, const float *stamps,
                            int64_t n_stamp, const float *weights, int64_t n_weight,
                            double *records, int64_t n_record, double *rendered,
                            int64_t n_rendered);
/* ms[0 .. 2]: milliseconds the model, render and reduce launches of the calling thread's last
 * smi_measure_sources_f32 call took on the device (events around them), for
 * tools/measure_blends_time.py */
int smi_measure_sources_last_launch_ms(double *ms);

/* render_blends: the images of many blends that share the number of model bands C and the
 * (kh, kw) stamp shape; three launches.  Host buffers in, host buffers out; coordinates relative
 * to the corner of the blend's frame; offsets and sizes count elements.  Components and bands are
 * those of smi_measure_sources_f32; data[weight_off .. + fh fw] is the band's image beside its
 * weights.  The bands of the blends tile the band table in order (blend.band0 = the bands of the
 * blends before it), the components of a source are among its blend's.
 *
 * With R the blend's scene -- every model pixel of bands[..].channel the sum over the blend's
 * components, in table order and in float64, of the rounded products seds[sed_off + c] *
 * morphs[morph_off + y w + x], zero outside the frame -- convolved ("same", zero boundary, float64
 * over the float32 taps), D the data and W the weights of observed band b of the blend:
 *
 *   rendered[blend.out_off + (b fh + y) fw + x] = float32(R)
 *   residual[the same]                          = D - float32(R)           (in float32)
 *   chi2[blend.band0 + b]                       = sum W (R - D)^2          (in float64)
 *
 * chi2 is summed per 16 x 16 tile (segments of 32 pixels in pixel order, the 8 segments joined
 * by a butterfly), then over the tiles in tile order.  With SMI_RENDER_SOURCES, per source, R_k
 * being its components alone rendered as smi_measure_sources_f32 renders them (the same bits) on
 * its region (gy0, gx0, gh, gw) -- its box grown by the stamp's half, clipped to the frame --:
 *
 *   source_rendered[source.out_off + (b gh + y - gy0) gw + x - gx0] = float32(R_k)
 *
 * and with SMI_RENDER_REWEIGHT (which implies the former) the rules of scarlet/lite/measure.py:
 *
 *   flux[the same] = float32(ratio * image), ratio = max(R_k, 0) / max(R, 0), 0 where the
 *   denominator is 0 and 1 where it exceeds 1; image = D, or D * (W > 0) with SMI_RENDER_MASK.
 *
 * Without SMI_RENDER_SOURCES n_sources must be 0; without SMI_RENDER_REWEIGHT `flux` is not
 * written and may be NULL with n_flux 0.  launch_ms (may be NULL) receives the milliseconds the
 * scene, sources and reduce launches took on the device (events around them).
 *
 * Limits: odd stamp sides <= 63, box and morphology sides <= 16384, a component's box inside its
 * source's.  Every table is validated before anything is launched: a bad one returns
 * SMI_ERR_INVALID and leaves the outputs alone.  The order of every sum depends on the frame, the
 * boxes and the stamp shape alone: a blend's outputs have the same bits wherever it stands in the
 * tables. */
typedef struct smi_render_blend {
    int32_t fh, fw;         /* frame */
    int32_t comp0, n_comp;  /* its components, sources in a row, in the order they are added */
    int32_t band0, n_band;  /* its observed bands in the band table */
    int64_t out_off;        /* its [n_band][fh][fw] cubes in rendered and residual */
} smi_render_blend;
typedef struct smi_render_source {
    int32_t y0, x0, h, w;   /* box of the source's model, may leave the frame */
    int32_t blend;
    int32_t comp0, n_comp;  /* its components, among its blend's */
    int32_t reserved;
    int64_t out_off;        /* its [n_band][gh][gw] cubes in source_rendered and flux */
} smi_render_source;
#define SMI_RENDER_SOURCES 1
#define SMI_RENDER_REWEIGHT 2
#define SMI_RENDER_MASK 4
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
                           float *flux, int64_t n_flux, double *launch_ms);

/* lite.init_blends: the wavelet initialisation of scarlet.lite (reference
 * lite/initialization.py:422-605) for a catalogue of blends.  Six steps, each one launch
 * over a table of tasks; the caller owns every buffer (`d_*`: device memory) and orders the
 * calls on `stream`.  A table is passed twice: in host memory, where it is validated before
 * anything is launched (a bad one returns SMI_ERR_INVALID), and as the copy on the device the
 * kernel reads.  Offsets and sizes count elements of the buffer they refer to.
 *   coadd  three sums of clipped wavelet planes per blend (detectlets, bulgelets, disklets):
 *          planes first[k], first[k] + step[k], ... (count[k] of them) added in that order
 *   snr    per source the two float64 sums of calculate_snr, PSF stamp on the centre
 *   taps   per task the centre pixel of apply_filter in every band (C values) and the plane's
 *          value at the centre (one more), bit-identical to the reference's tap loop
 *   masks  prox_monotonic_mask(X, 0, centre, max_iter=0): valid map, bounds (min row, max
 *          row, min col, max col), and per task the value at the seed
 *   crop   where(valid, plane, 0) on a box that may leave the frame, divided by its maximum
 *   fit    per source and band a.a, a.b, b.b, a.img, b.img over the union box of two
 *          morphologies (a, b: the morphologies convolved with the band's stamp) */
typedef struct smi_lite_init_coadd {
    int32_t n_planes;
    int32_t first[3], count[3], step[3];
    int32_t reserved[2];
    int64_t n_pix, wavelet_off, coadd_off;  /* coadds: 3 planes of n_pix */
} smi_lite_init_coadd;
typedef struct smi_lite_init_snr {
    int32_t h, w, cy, cx, ph, pw;
    int64_t image_off, psf_off;
} smi_lite_init_snr;
typedef struct smi_lite_init_taps {
    int32_t h, w, cy, cx, kh, kw;
    int64_t plane_off, stamp_off, out_off;  /* out: C + 1 values */
} smi_lite_init_taps;
typedef struct smi_lite_init_mask {
    int32_t h, w, cy, cx;
    int64_t plane_off, pix_off, valid_off;  /* pix_off: the task's h * w of the scratch */
} smi_lite_init_mask;
typedef struct smi_lite_init_crop {
    int32_t h, w;            /* plane */
    int32_t y0, x0, bh, bw;  /* box, in plane coordinates */
    int64_t plane_off, valid_off, out_off;
} smi_lite_init_crop;
typedef struct smi_lite_init_fit {
    int32_t h, w;                    /* frame */
    int32_t y0, x0, fh, fw;          /* union box, in frame coordinates */
    int32_t a_y0, a_x0, a_h, a_w;    /* boxes of the two morphologies, inside the union */
    int32_t b_y0, b_x0, b_h, b_w;
    int32_t kh, kw;
    int64_t image_off, stamp_off, a_off, b_off;
} smi_lite_init_fit;
int smi_lite_init_coadd_f32(int32_t n, const smi_lite_init_coadd *tasks, const void *d_tasks,
                            const float *d_wavelets, int64_t n_wavelets, float *d_coadds,
                            int64_t n_coadds, void *stream);
int smi_lite_init_snr_f32(int32_t C, int32_t n, const smi_lite_init_snr *tasks, const void *d_tasks,
                          const float *d_images, const float *d_variance, int64_t n_image,
                          const float *d_psfs, int64_t n_psf, double *d_out, int64_t n_out,
                          void *stream);
int smi_lite_init_taps_f32(int32_t C, int32_t n, const smi_lite_init_taps *tasks,
                           const void *d_tasks, const float *d_planes, int64_t n_plane,
                           const float *d_stamps, int64_t n_stamp, float *d_out, int64_t n_out,
                           void *stream);
int smi_lite_init_masks_f32(int32_t n, const smi_lite_init_mask *tasks, const void *d_tasks,
                            const float *d_planes, int64_t n_plane, int32_t *d_visited,
                            uint8_t *d_unchecked, uint8_t *d_orphans, int64_t n_scratch,
                            uint8_t *d_valid, int64_t n_valid, int32_t *d_bounds, float *d_values,
                            int64_t n_results, void *stream);
int smi_lite_init_crop_f32(int32_t n, const smi_lite_init_crop *tasks, const void *d_tasks,
                           const float *d_planes, int64_t n_plane, const uint8_t *d_valid,
                           int64_t n_valid, float *d_out, int64_t n_out, void *stream);
int smi_lite_init_fit_f32(int32_t C, int32_t n, const smi_lite_init_fit *tasks, const void *d_tasks,
                          const float *d_morphs, int64_t n_morph, const void *d_images,
                          int32_t images_f64, int64_t n_image, const double *d_stamps,
                          int64_t n_stamp, double *d_out, int64_t n_out, void *stream);
int smi_lite_init_coadd_f64(int32_t n, const smi_lite_init_coadd *tasks, const void *d_tasks,
                            const double *d_wavelets, int64_t n_wavelets, double *d_coadds,
                            int64_t n_coadds, void *stream);
int smi_lite_init_snr_f64(int32_t C, int32_t n, const smi_lite_init_snr *tasks, const void *d_tasks,
                          const double *d_images, const double *d_variance, int64_t n_image,
                          const double *d_psfs, int64_t n_psf, double *d_out, int64_t n_out,
                          void *stream);
int smi_lite_init_taps_f64(int32_t C, int32_t n, const smi_lite_init_taps *tasks,
                           const void *d_tasks, const double *d_planes, int64_t n_plane,
                           const double *d_stamps, int64_t n_stamp, double *d_out, int64_t n_out,
                           void *stream);
int smi_lite_init_masks_f64(int32_t n, const smi_lite_init_mask *tasks, const void *d_tasks,
                            const double *d_planes, int64_t n_plane, int32_t *d_visited,
                            uint8_t *d_unchecked, uint8_t *d_orphans, int64_t n_scratch,
                            uint8_t *d_valid, int64_t n_valid, int32_t *d_bounds, double *d_values,
                            int64_t n_results, void *stream);
int smi_lite_init_crop_f64(int32_t n, const smi_lite_init_crop *tasks, const void *d_tasks,
                           const double *d_planes, int64_t n_plane, const uint8_t *d_valid,
                           int64_t n_valid, double *d_out, int64_t n_out, void *stream);
int smi_lite_init_fit_f64(int32_t C, int32_t n, const smi_lite_init_fit *tasks, const void *d_tasks,
                          const double *d_morphs, int64_t n_morph, const void *d_images,
                          int32_t images_f64, int64_t n_image, const double *d_stamps,
                          int64_t n_stamp, double *d_out, int64_t n_out, void *stream);

/* lite.init_blends_main: the scarlet-main initialisation of scarlet.lite (reference
 * lite/initialization.py:188-247, 321-419 with use_mask=False) for a catalogue of blends, with
 * the conventions of smi_lite_init_* above, whose snr, taps, crop and fit entries it shares.  A
 * chunk takes at most eight launches, whatever its blends and sources: main_coadd, snr, taps of
 * the detection images, taps of the model PSFs, main_sweep, crop, main_split, fit.
 *   main_coadd  detect[p] = sum over the bands, in order, of images[c][p] / nr2[c], all in the
 *               data type (np.sum(images / noise_rms**2, axis=0))
 *   main_sweep  per source, one workgroup with the frame in LDS (at most (160 KiB - 1 KiB) /
 *               sizeof(T) pixels): prox_uncentered_symmetry(X, 0, centre, "sdss"), then
 *               prox_weighted_monotonic(shape, "angle", min_gradient=0, centre), then
 *               X[~(X > thresh)] = 0, compared in double.  d_cos is the table of
 *               cos(arctan2(-Y, -X) - arctan2(dy_i, dx_i)) over the offsets |Y| <= ry, |X| <= rx
 *               from the centre, [2 ry + 1][2 rx + 1][8] doubles in the reference's neighbour
 *               order, which covers every frame of the table (h - 1 <= ry, w - 1 <= rx).  Per
 *               task the swept plane, the bounds (min row, max row, min col, max col) of its
 *               pixels > 0 -- (0, -1, 0, -1) without any -- and its maximum
 *   main_split  of a cut-out normalised to maximum 1: bulge = max(morph - level, 0) and
 *               disk = min(morph, level), level cast to the data type, each divided by its own
 *               maximum; all three live in d_morphs */
typedef struct smi_lite_init_main_coadd {
    int32_t bands, reserved;
    int64_t n_pix, image_off, nr2_off, detect_off;
} smi_lite_init_main_coadd;
typedef struct smi_lite_init_main_sweep {
    int32_t h, w, cy, cx;
    int64_t plane_off, out_off;
    double thresh;
} smi_lite_init_main_sweep;
typedef struct smi_lite_init_main_split {
    int32_t bh, bw;
    int64_t morph_off, bulge_off, disk_off;
} smi_lite_init_main_split;
int smi_lite_init_main_coadd_f32(int32_t n, const smi_lite_init_main_coadd *tasks,
                                 const void *d_tasks, const float *d_images, int64_t n_image,
                                 const float *d_nr2, int64_t n_nr2, float *d_detect,
                                 int64_t n_detect, void *stream);
int smi_lite_init_main_sweep_f32(int32_t n, const smi_lite_init_main_sweep *tasks,
                                 const void *d_tasks, const float *d_planes, int64_t n_plane,
                                 const double *d_cos, int64_t n_cos, int32_t ry, int32_t rx,
                                 float *d_out, int64_t n_out, int32_t *d_bounds, float *d_peaks,
                                 int64_t n_results, void *stream);
int smi_lite_init_main_split_f32(int32_t n, const smi_lite_init_main_split *tasks,
                                 const void *d_tasks, float *d_morphs, int64_t n_morph,
                                 double level, void *stream);
int smi_lite_init_main_coadd_f64(int32_t n, const smi_lite_init_main_coadd *tasks,
                                 const void *d_tasks, const double *d_images, int64_t n_image,
                                 const double *d_nr2, int64_t n_nr2, double *d_detect,
                                 int64_t n_detect, void *stream);
int smi_lite_init_main_sweep_f64(int32_t n, const smi_lite_init_main_sweep *tasks,
                                 const void *d_tasks, const double *d_planes, int64_t n_plane,
                                 const double *d_cos, int64_t n_cos, int32_t ry, int32_t rx,
                                 double *d_out, int64_t n_out, int32_t *d_bounds, double *d_peaks,
                                 int64_t n_results, void *stream);
int smi_lite_init_main_split_f64(int32_t n, const smi_lite_init_main_split *tasks,
                                 const void *d_tasks, double *d_morphs, int64_t n_morph,
                                 double level, void *stream);

/* initialization.init_blends: the morphologies and the normal equations of the spectra of
 * initialization.init_all_sources (reference initialization.py:30-170, 287-363, 493-588;
 * source.py:249-522) for a catalogue of float32 blends, with the conventions of smi_lite_init_*
 * above.  A chunk takes five launches, whatever its blends and sources.  d_data and d_var hold the cubes of build_initialization_image (data and
 * noise_rms**2 on the model frame, (bands, h, w) per blend) at the same offsets; the variance
 * is positive, and negated where the pixel has no weight: psf_snr leaves those pixels out and
 * sweep reads the magnitude, as the coadd of the reference does.
 *   psf_snr  per source and band the three float64 sums of get_psf_spectrum over the box of the
 *            (ph, pw) PSF stamp on the pixel: sum d p, sum p p, sum p var p.  Pixels beyond the
 *            frame hold zero data and zero noise; pixels with var <= 0 are left out.  out: 3
 *            doubles per band
 *   sweep    per source, one workgroup with the frame in LDS as float64 (at most (160 KiB -
 *            1 KiB) / 8 pixels): the coadd weighted with the source's spectrum (bands doubles at
 *            spec_off), prox_uncentered_symmetry(X, 0, centre, "sdss"),
 *            prox_weighted_monotonic(shape, "flat", min_gradient=0, centre), then
 *            X[~(X > thresh * std)] = 0.  Per task the plane, the bounds (min row, max row, min
 *            col, max col) of its pixels > 0 -- (0, -1, 0, -1) without any -- and its maximum
 *   crop     per source the (side, side) cut-out at (y0, x0), zeros beyond the frame, divided by
 *            its maximum (one lit pixel in the middle where nothing is left), np.maximum with
 *            the side * side doubles at floor_off; with layers == 2 split at percentile / 100 of
 *            the peak as MultiExtendedSource.init_morphs does, each layer divided by its own
 *            maximum.  out: layers * side * side doubles; flags: bit 0 where one is not
 *            finite, bit 1 where the cut-out held no pixel > 0
 *   spectra_tiles, spectra_reduce  the weighted normal equations of set_spectra_to_match.  A
 *            blend names its (h, w) frame, the (fh, fw) region at (y0, x0) inside it that its
 *            convolved models can reach, its float32 data and weight cubes at cube_off, its
 *            (bands, kh, kw) float64 stamps (odd sides of at most 63; 1 x 1 for the identity) and
 *            n_comp <= 64 components from comp0: float64 (h, w) morphologies with their origin
 *            in frame coordinates, zero outside the box and outside the frame.  `work` lists
 *            (blend, tile) of every 16 x 16 tile of every region, in order; at most 32 components
 *            may reach one tile.  Per tile and band K K + 3 K doubles at part_off: G = A^T W A,
 *            r = A^T W d, sum a w and sum a of the convolved columns a; reduce adds a blend's
 *            tiles in order into out_off, [band][K K + 3 K] */
typedef struct smi_init_sources_psf_snr {
    int32_t h, w, cy, cx, ph, pw, bands, reserved;
    int64_t cube_off, psf_off, out_off;
} smi_init_sources_psf_snr;
typedef struct smi_init_sources_sweep {
    int32_t h, w, cy, cx, bands, reserved;
    int64_t cube_off, spec_off, out_off;
    double thresh;
} smi_init_sources_sweep;
typedef struct smi_init_sources_crop {
    int32_t h, w;           /* plane */
    int32_t y0, x0, side;   /* box, in plane coordinates */
    int32_t layers;
    int64_t plane_off, floor_off, out_off;
    double percentile;
} smi_init_sources_crop;
typedef struct smi_init_sources_spectra_blend {
    int32_t h, w;            /* frame */
    int32_t y0, x0, fh, fw;  /* region, in frame coordinates */
    int32_t bands, kh, kw;
    int32_t n_comp, comp0, reserved;
    int64_t cube_off, stamp_off, part_off, out_off;
} smi_init_sources_spectra_blend;
typedef struct smi_init_sources_spectra_component {
    int32_t y0, x0, h, w;    /* box, in frame coordinates */
    int64_t morph_off;
} smi_init_sources_spectra_component;
int smi_init_sources_psf_snr_f32(int32_t n, const smi_init_sources_psf_snr *tasks, const void *d_tasks,
                             const float *d_data, const float *d_var, int64_t n_cube,
                             const double *d_psfs, int64_t n_psf, double *d_out, int64_t n_out,
                             void *stream);
int smi_init_sources_sweep_f32(int32_t n, const smi_init_sources_sweep *tasks, const void *d_tasks,
                           const float *d_data, const float *d_var, int64_t n_cube,
                           const double *d_spectra, int64_t n_spectra, double *d_out,
                           int64_t n_out, int32_t *d_bounds, double *d_peaks, int64_t n_results,
                           void *stream);
int smi_init_sources_crop_f32(int32_t n, const smi_init_sources_crop *tasks, const void *d_tasks,
                          const double *d_planes, int64_t n_plane, const double *d_floors,
                          int64_t n_floor, double *d_out, int64_t n_out, int32_t *d_flags,
                          int64_t n_flags, void *stream);
int smi_init_sources_spectra_tiles_f32(
    int32_t n, const smi_init_sources_spectra_blend *blends, const void *d_blends, int32_t n_comps,
    const smi_init_sources_spectra_component *comps, const void *d_comps, int32_t n_work,
    const int32_t *work, const void *d_work, const float *d_data, const float *d_weights,
    int64_t n_cube, const double *d_stamps, int64_t n_stamp, const double *d_morphs,
    int64_t n_morph, double *d_part, int64_t n_part, int64_t n_out, void *stream);
int smi_init_sources_spectra_reduce_f32(int32_t n, const smi_init_sources_spectra_blend *blends,
                                        const void *d_blends, const double *d_part, int64_t n_part,
                                        double *d_out, int64_t n_out, void *stream);

/* get_valid_monotonic_pixels / linear_interpolate_invalid_pixels
 * (operators_pybind11.cc:61-232, float32 and float64 overload sets; callers
 * operator.py:155-176).  Row-major (rows, cols) images; `unchecked` / `orphans` are the
 * NumPy bool maps as bytes; `bounds` = (min row, max row, min col, max col); all updated
 * in place like the Eigen::Ref arguments of the reference.  Bit-identical maps and
 * values to the C++ recursion (tests: test_mask_operators_bit_exact). */
int smi_get_valid_monotonic_pixels_f32(int32_t i, int32_t j, const float *image, int32_t rows,
                                       int32_t cols, uint8_t *unchecked, uint8_t *orphans,
                                       double variance, int32_t *bounds, double thresh);
int smi_get_valid_monotonic_pixels_f64(int32_t i, int32_t j, const double *image, int32_t rows,
                                       int32_t cols, uint8_t *unchecked, uint8_t *orphans,
                                       double variance, int32_t *bounds, double thresh);
int smi_linear_interpolate_invalid_pixels_f32(const int32_t *row_indices,
                                              const int32_t *column_indices, int32_t n_indices,
                                              uint8_t *unchecked, float *model, int32_t rows,
                                              int32_t cols, uint8_t *orphans, double variance,
                                              int32_t recursive, int32_t *bounds);
int smi_linear_interpolate_invalid_pixels_f64(const int32_t *row_indices,
                                              const int32_t *column_indices, int32_t n_indices,
                                              uint8_t *unchecked, double *model, int32_t rows,
                                              int32_t cols, uint8_t *orphans, double variance,
                                              int32_t recursive, int32_t *bounds);

/* ------------------------------------------------------------------------- *
 * Seam 2: batched proximal-gradient fit.
 * ------------------------------------------------------------------------- */

typedef struct smi_batch smi_batch;

/* prox chain of a morphology (morphology.py:644-670): bit flags */
enum {
    SMI_PROX_MONOTONIC = 1,  /* MonotonicityConstraint (constraint.py:183-234)  */
    SMI_PROX_SYMMETRY = 2,   /* SymmetryConstraint (constraint.py:262-273)      */
    SMI_PROX_POSITIVE = 4,   /* PositivityConstraint (constraint.py:83-92)      */
    SMI_PROX_CENTER_ON = 8,  /* CenterOnConstraint (constraint.py:276-287)      */
    SMI_PROX_NORM_MAX = 16,  /* NormalizationConstraint("max") (95-114)         */
    SMI_PROX_NORM_SUM = 32,  /* NormalizationConstraint("sum")                  */
    SMI_PROX_L1 = 64,        /* L1Constraint -> proxmin prox_soft (134-145)     */
    SMI_PROX_L0 = 128,       /* L0Constraint -> proxmin prox_hard (117-130)     */
    /* MonotonicityConstraint(fit_center_radius=1) (constraint.py:203-208,
     * operator.py:99-129): the sweep starts at the brightest pixel of the 3x3 block
     * around the box centre; `sweep_plan` is the first of 9 consecutive plans built
     * for the centres (cy-1..cy+1) x (cx-1..cx+1), row major */
    SMI_PROX_FIT_CENTER = 256,
    /* scarlet.lite background threshold (lite/models.py:222-228): a pixel is set to 0
     * when sed[c] * morph < bg_level[c] in every band (new sed); replaces positivity */
    SMI_PROX_BG_THRESH = 512,
    /* l_thresh of SMI_PROX_L1 / L0 is relative: multiplied by the step of the proximal
     * sub-iteration, gamma = alpha / max(psi) (type="relative", the reference's default,
     * constraint.py:117-145; lite/parameters.py:296-299) */
    SMI_PROX_L_RELATIVE = 1024,
    /* MonotonicityConstraint(use_mask=True) (constraint.py:228-232): pixels that a
     * strictly decreasing, positive 4-neighbour path connects to the centre
     * (get_valid_monotonic_pixels, operators_pybind11.cc:61-125, variance 0) keep their
     * value from before the sweep; needs SMI_PROX_MONOTONIC */
    SMI_PROX_MONO_MASK = 2048,
    /* not a constraint: the component is a PointSource (source.py:92-128) whose
     * morphology is the model PSF evaluated at a free sub-pixel centre
     * (PointSourceMorphology, morphology.py:476-513; GaussianPSF, psf.py:80-142) */
    SMI_COMPONENT_POINT_SOURCE = 1 << 16,
    /* the image morphology is moved by a free sub-pixel Fourier shift
     * (ExtendedSource(shifting=True): morphology.py:124-130, 673-676; fft.shift,
     * fft.py:399-428): `center` holds the initial shift (y, x), `shift_step` its step */
    SMI_COMPONENT_SHIFTING = 1 << 17,
    /* Parameter(fixed=True) (parameter.py:38-39, blend.py:107-115): the parameter stays in
     * X but its gradient is taken as zero; the step (nothing) and the proximal operator
     * are still applied, as proxmin does with the expanded zero gradient.  FIXED_MORPH
     * fixes the image of an extended source or the centre of a point source. */
    SMI_COMPONENT_FIXED_SED = 1 << 18,
    SMI_COMPONENT_FIXED_MORPH = 1 << 19,
    /* the morphology is the reconstruction of starlet coefficients, which are the parameter
     * (StarletSource, source.py:525-612; StarletMorphology, morphology.py:516-604): see the
     * star_* fields of smi_components.  SMI_COMPONENT_FIXED_MORPH fixes the coefficients.
     * No other prox flag: the constraint is PositivityConstraint(pos_floor) followed by the
     * per-plane hard threshold star_thresh, or -- StarletMorphology(monotonic=True), marked in
     * star_monotonic -- MonotonicMaskConstraint about the middle of the box on every plane. */
    SMI_COMPONENT_STARLET = 1 << 20,
    /* the morphology is a radial profile of a few float64 numbers, which are the parameters
     * (GaussianSource / SpergelSource, source.py:131-246; ProfileMorphology, morphology.py:210-473):
     * see the prof_* fields of smi_components.  The only other flag it takes is
     * SMI_COMPONENT_FIXED_SED; its parameters are fixed one by one through prof_fixed. */
    SMI_COMPONENT_PROFILE = 1 << 21
};
enum { SMI_PROFILE_GAUSSIAN = 0, SMI_PROFILE_SPERGEL = 1 };
/* bits of prof_fixed and order of the four entries of prof_step / prof_rel_step */
enum { SMI_PROFILE_CENTER = 0, SMI_PROFILE_RADIUS = 1, SMI_PROFILE_ELLIPTICITY = 2, SMI_PROFILE_NU = 3 };
#define SMI_PROX_EXTENDED_SOURCE \
    (SMI_PROX_MONOTONIC | SMI_PROX_POSITIVE | SMI_PROX_CENTER_ON | SMI_PROX_NORM_MAX)

typedef struct smi_batch_desc {
    int32_t n_blends;     /* independent scenes in the batch                       */
    int32_t C, H, W;      /* model frame = observed frame (bands, rows, columns)   */
    int32_t n_components; /* total over all blends                                 */
    int32_t kernel_h;     /* difference-kernel stamp; 0 => NullRenderer            */
    int32_t kernel_w;
    int32_t kernel_bands; /* 1 (band shared) or C                                  */
    int32_t kernel_per_blend; /* 0: one kernel set for the whole batch, 1: per blend */
    int32_t fft_h;        /* FFT shape; 0 => reference rule fft.py:116-167         */
    int32_t fft_w;
    int32_t max_iter;     /* capacity of the per-blend loss history                */
    int32_t conv_path;    /* 0 auto: LDS-resident fused convolution kernel when the  */
                          /*   padded band fits the LDS, else rocFFT;                */
                          /* 1 rocFFT pipeline (reference FFT shape by default);     */
                          /* 2 fused kernel or fail                                  */
} smi_batch_desc;

/* per component, all arrays of length n_components unless noted */
typedef struct smi_components {
    const int32_t *blend;       /* owning blend, non-decreasing                     */
    const int32_t *origin_y;    /* box origin in frame pixels (may be negative)     */
    const int32_t *origin_x;
    const int32_t *box_h;
    const int32_t *box_w;
    const float *sed;           /* [n_components][C]                                */
    const float *morph;         /* boxes packed back to back, row major             */
    const float *sed_min_step;  /* [n_components][C]  (spectrum.py:56)              */
    const float *sed_rel_step;  /* relative_step factor, 1e-2 in the reference      */
    const float *morph_step;    /* constant step, 1e-2 (morphology.py:670)          */
    const int32_t *prox_flags;  /* SMI_PROX_* of the morphology                     */
    const int32_t *sweep_plan;  /* index into the plans added with                  */
                                /* smi_batch_add_sweep_plan, -1 if not monotonic    */
    const float *min_gradient;  /* MonotonicityConstraint.min_gradient              */
    const float *l_thresh;      /* threshold for SMI_PROX_L1/L0 (absolute unless     */
                                /* SMI_PROX_L_RELATIVE)                              */
    const float *morph_rel_step;/* step = max(morph_step, rel * mean(morph)); NULL=0 */
                                /* (relative_step, parameter.py:126-129)            */
    /* point sources (SMI_COMPONENT_POINT_SOURCE in prox_flags); both NULL if none.
     * For such a component the box is the PSF box at the rounded initial centre
     * (morphology.py:494-497), its `morph` input is ignored (the library evaluates
     * the pixel-integrated Gaussian), and `morph_step` is the step of the centre
     * (3e-2, source.py:115). */
    const double *center;       /* [n_components][2] (y, x) in frame pixels; for     */
                                /* SMI_COMPONENT_SHIFTING entries: the shift (y, x)  */
    const float *psf_sigma;     /* [n_components] model PSF sigma (all bands alike)  */
    const float *shift_step;    /* [n_components] step of a free shift (1e-1,        */
                                /* morphology.py:675); NULL = 1e-1                   */
    const float *center_floor;  /* [n_components] floor of the centre pixel for      */
                                /* SMI_PROX_CENTER_ON: 1e-6 (CenterOnConstraint,     */
                                /* constraint.py:276-287) or the `floor` of a lite   */
                                /* component (lite/models.py:233-236); NULL = 1e-6   */
    const float *bg_level;      /* [n_components][C] bg_rms * bg_thresh for          */
                                /* SMI_PROX_BG_THRESH; NULL if unused                */
    const float *fista_step;    /* [n_components] FistaParameter.step                */
                                /* (lite/initialization.py:308-312); NULL unless the */
                                /* batch runs SMI_SCHEME_FISTA                       */
    const float *sym_strength;  /* [n_components] strength of SMI_PROX_SYMMETRY         */
                                /* (SymmetryConstraint(strength), constraint.py:262-273,*/
                                /* operator.py:274-293); NULL = 1                        */
    const float *pos_floor;     /* [n_components] PositivityConstraint(zero) of the       */
                                /* morphology (constraint.py:83-92); NULL = 0              */
    const int32_t *chain_repeat;/* [n_components] ConstraintChain(repeat) (constraint.py:  */
                                /* 60-80): the whole chain applied that many times per     */
                                /* proximal evaluation; NULL = 1                           */
    const float *shift_rel_step;/* [n_components] relative_step of a free shift             */
                                /* (parameter.py:126-129): step = max(shift_step, rel *     */
                                /* mean(shift)); NULL = 0.  (The centre of a point source   */
                                /* takes its rule from morph_step / morph_rel_step: step =  */
                                /* max(morph_step, rel * mean(centre in frame pixels)).)    */
    const float *psf_beta;      /* [n_components] point sources on a MoffatPSF model PSF     */
                                /* (psf.py:145-202): (1 + r^2 / alpha^2)^-beta sampled at    */
                                /* the pixel centres, alpha in psf_sigma; 0 or NULL = the    */
                                /* pixel-integrated Gaussian of width psf_sigma              */
    /* starlet components (SMI_COMPONENT_STARLET in prox_flags); all NULL if none.  For such a
     * component `morph` is ignored (the library reconstructs the image from the coefficients),
     * `morph_step` is the constant step of the coefficients (1e-2, morphology.py:564) and
     * `pos_floor` the floor of their PositivityConstraint. */
    const int32_t *star_planes; /* [n_components] coefficient planes, scales + 1 (<= 31); 0   */
                                /* for other components                                       */
    const float *star_coeffs;   /* the [planes][box_h][box_w] stacks of the starlet           */
                                /* components, back to back in component order                */
    const float *star_thresh;   /* their per-plane absolute thresholds of the L0Constraint,   */
                                /* planes entries each, back to back (last plane: 0)          */
    const float *sed_floor;     /* [n_components] PositivityConstraint(zero) of the spectrum: */
                                /* 1e-20 (spectrum.py:54-56) or 0 (RandomSource,              */
                                /* source.py:81-86); NULL = 1e-20                             */
    /* profile components (SMI_COMPONENT_PROFILE in prox_flags); all NULL if none, entries of
     * other components are ignored.  `morph` is ignored for such a component (the library
     * evaluates exp(-R2 / 2) or the Spergel profile on the box, unnormalised, in double). */
    const int32_t *prof_kind;    /* [n_components] SMI_PROFILE_*                              */
    const double *prof_params;   /* [n_components][6] centre y, x (model-frame pixels),       */
                                 /* radius, e1, e2, nu (ignored by a Gaussian)                */
    const double *prof_step;     /* [n_components][4] constant step (or the minimum of a      */
                                 /* relative step) of centre, radius, ellipticity, nu         */
    const double *prof_rel_step; /* [n_components][4] relative_step factor (parameter.py:     */
                                 /* 126-129: max(minimum, factor * mean)); 0 = constant step  */
    const int32_t *prof_fixed;   /* [n_components] bit 1 << SMI_PROFILE_*: Parameter(fixed)   */
    /* monotonic starlet components (StarletMorphology(monotonic=True), morphology.py:549-553);
     * all NULL if none.  The constraint of such a component's coefficients is
     * MonotonicMaskConstraint((box_h / 2, box_w / 2), center_radius, variance, max_iter)
     * (constraint.py:237-259; operator.prox_monotonic_mask, operator.py:131-180) applied to
     * every plane; its star_thresh entries (still `planes` of them) and pos_floor are ignored. */
    const int32_t *star_monotonic;     /* [n_components] != 0: monotonic planes; entries of     */
                                       /* components that are no starlet are ignored            */
    const int32_t *star_center_radius; /* [n_components] half width of the window the centre is */
                                       /* looked for in (get_center); 0: the middle itself      */
    const double *star_variance;       /* [n_components] slack of the monotonicity test, >= 0   */
    const int32_t *star_max_iter;      /* [n_components] interpolation passes at the most       */
} smi_components;

int smi_batch_create(const smi_batch_desc *desc, int device, smi_batch **out);
int smi_batch_destroy(smi_batch *b);

/* Monotonic operator tables exactly as operator.prox_weighted_monotonic binds them
 * (operator.py:62-96): weights[8][h*w] (float64), offsets[8], dist_idx[n_idx].
 * Returns the plan index (>= 0) or a negative status. */
int smi_batch_add_sweep_plan(smi_batch *b, int32_t h, int32_t w,
                             const double *weights, const int32_t *offsets,
                             const int32_t *dist_idx, int32_t n_idx);

/* The ring schedule the update kernels derive from such tables when they are the radial ones
 * of operator.py:591-667 (host only, no GPU; csrc/common.h describes the schedule).  Returns
 * 1 and fills info = {planes | n_nat << 8, n_steps, n_pad, rmax, centre, perm, lanes,
 * stream_bytes} (n_nat: steps of the plain schedule; from there on the address words carry
 * flags: 0x8000 late ring, 1 axis pixel, 2 diagonal pixel) when the tables qualify, 0 when they do not (the kernels then keep the level plan), < 0 on bad
 * arguments.  stream_bytes = size of the device stream with the weights stored once per ring,
 * 0 when the octants differ (off-centre peak, even or oblong box): only tables with such a
 * stream run the ring schedule on the device.  With capacity >= lanes also wts[lanes][4]
 * (weights by role A, B, C, D) and addr[lanes] (16 + 4 * pixel | flags, 0 = idle);
 * lanes = (n_pad + 6) * planes * 64, step major. */
int smi_sweep_ring_plan(int32_t h, int32_t w, const double *weights, const int32_t *offsets,
                        const int32_t *dist_idx, int32_t n_idx, int32_t info[8], float *wts,
                        uint16_t *addr, int64_t capacity);

/* data, weights: [n_blends][C][H][W] float32 (observation.py:52-57).  The _device
 * form adopts device buffers (e.g. torch tensors) without copying them: log_norm, the loss of
 * the rocFFT path and further renderers read the caller's buffers, which must stay alive and
 * UNCHANGED while the batch uses them.  The fused convolution reads a SNAPSHOT taken by this
 * call -- data and weights interleaved by row pairs, one more copy of the observation in device
 * memory (8 bytes per pixel and band, also for adopted buffers) -- so an adopted tensor changed
 * in place is not seen by it: call smi_batch_set_observation_device again to register the new
 * contents.  The _device form waits for the whole device once (the buffers may have been
 * written on any stream); the host form only for the batch's stream. */
int smi_batch_set_observation(smi_batch *b, const float *data, const float *weights);
int smi_batch_set_observation_device(smi_batch *b, const float *d_data,
                                     const float *d_weights);
/* kernel: [kernel_per_blend ? n_blends : 1][kernel_bands][kernel_h][kernel_w] */
int smi_batch_set_kernel(smi_batch *b, const float *kernel);

/* ConvolutionRenderer(psf_shift=...) (renderer.py:175-177, 215-228): the difference kernel
 * is moved by a free sub-pixel Fourier shift (fft.shift, fft.py:399-428) that the fit
 * updates like any other parameter (no constraint, AMSGrad step `step`, 1e-2 in the
 * reference).  Call after smi_batch_set_observation and smi_batch_set_components instead
 * of smi_batch_set_kernel.
 *   kernel    [n_sets][kernel_bands][h0][w0]: the unshifted stamps as the renderer holds
 *             them (h0 <= kernel_h, w0 <= kernel_w; centred in the batch's odd stamp);
 *             n_sets = kernel_per_blend ? n_blends : 1 (a shared kernel needs n_blends = 1)
 *   fft_shape FFT lengths (y, x) fft.shift uses for an (h0, w0) image (fft.py:116-167 with
 *             padding 10): the periodic interpolation depends on them
 *   shift     [n_sets][2] initial (y, x); moments [n_sets][6] = m, v, vhat (y, x each) or NULL
 * Every smi_batch_step then evaluates d(-logL)/d(shift) = sum w (m - d) (model (*) dK/ds)
 * at the parameters of the iteration, steps the shift and rebuilds the kernel spectrum on
 * the device; smi_batch_gradient evaluates the gradient only.  smi_batch_set_kernel makes
 * the kernel fixed again. */
int smi_batch_set_kernel_shift(smi_batch *b, const float *kernel, int32_t h0, int32_t w0,
                               const int32_t *fft_shape, const double *shift,
                               const double *moments, double step);
/* shift [n_sets][2], moments [n_sets][6], gradient [n_sets][2] (last evaluation), kernel
 * [n_sets][kernel_bands][kernel_h][kernel_w] at the current shift; any may be NULL */
int smi_batch_get_kernel_shift(smi_batch *b, double *shift, double *moments, double *gradient,
                               float *kernel);
/* relative_step for the kernel shift (parameter.py:126-129): step = max(step of
 * smi_batch_set_kernel_shift, factor * mean(shift)); factor = 0 (default): constant step.
 * Call after smi_batch_set_kernel_shift. */
int smi_batch_set_kernel_shift_relative_step(smi_batch *b, double factor);
int smi_batch_set_components(smi_batch *b, const smi_components *comps);

/* AMSGrad moments (blend.py:153-163), same packing as sed / morph; NULL = zeros */
int smi_batch_set_moments(smi_batch *b, const float *m_sed, const float *v_sed,
                          const float *vhat_sed, const float *m_morph,
                          const float *v_morph, const float *vhat_morph);
int smi_batch_get_moments(smi_batch *b, float *m_sed, float *v_sed, float *vhat_sed,
                          float *m_morph, float *v_morph, float *vhat_morph);
int smi_batch_get_parameters(smi_batch *b, float *sed, float *morph);
/* point-source centres / free shifts [n_components][2] (entries of other components:
 * 0) and their AMSGrad moments; the gradient is valid after smi_batch_gradient.  Any
 * pointer may be NULL.  For a shifting component smi_batch_get_parameters returns the
 * image parameter; smi_batch_get_model_morphology returns what enters the model (the
 * shifted image; equal to the parameter for every other component). */
int smi_batch_get_centers(smi_batch *b, double *center, double *m, double *v, double *vhat,
                          double *gradient);
int smi_batch_set_center_moments(smi_batch *b, const double *m, const double *v,
                                 const double *vhat);
/* New values [n_components][2] for the point-source centres / free shifts (entries of other
 * components are ignored); the morphologies that enter the model follow.  For a 2-vector the
 * host steps itself -- a prior, a constraint or a step callable on it (blend.py:120-145 treats
 * every Parameter alike): its device step is 0, the host takes the step from the gradient of
 * smi_batch_get_centers and writes the result back here. */
int smi_batch_set_centers(smi_batch *b, const double *center);
int smi_batch_get_model_morphology(smi_batch *b, float *morph);
int smi_batch_set_parameters(smi_batch *b, const float *sed, const float *morph);
/* Starlet components: the coefficients, their AMSGrad moments and the gradient of -logL
 * w.r.t. them (valid after smi_batch_gradient), each packed like star_coeffs; any pointer may be
 * NULL.  smi_batch_get_parameters returns the reconstructed image of such a component.
 * smi_batch_set_starlet_moments: warm start (NULL = zeros).  A batch with starlet components
 * keeps one range of blends and the model cube; smi_batch_set_frame_extents,
 * smi_batch_update_components, smi_batch_set_iteration_base, SMI_SCHEME_FISTA and the
 * state-record / save-state calls refuse it. */
int smi_batch_get_starlet(smi_batch *b, float *coeffs, float *m, float *v, float *vhat,
                          float *gradient);
/* operator.prox_monotonic_mask about (h / 2, w / 2) (operator.py:131-180) on every plane of
 * the HOST stack [planes][h][w], in place: the device function the step of a monotonic starlet
 * component runs in its proximal sub-iterations, launched once on its own (one workgroup; for
 * tests and parity checks). */
int smi_starlet_monotonic_mask_f32(float *stack, int32_t planes, int32_t h, int32_t w,
                                   int32_t center_radius, double variance, int32_t max_iter);
int smi_batch_set_starlet_moments(smi_batch *b, const float *m, const float *v, const float *vhat);
/* Profile components: the six doubles {centre y, x, radius, e1, e2, nu} of every component
 * ([n_components][6], zeros for the others), their AMSGrad moments and the gradient of -logL
 * w.r.t. them (valid after smi_batch_gradient or a step); any pointer may be NULL.  The nu entry
 * of the gradient follows the reference's fit: the derivative of K_nu w.r.t. its order is left
 * out (morphology.py:380-381).  smi_batch_get_parameters returns the float32 image of such a
 * component.  smi_batch_set_profile_moments: warm start (NULL = zeros).  The calls that refuse
 * starlet components refuse profile components too. */
int smi_batch_get_profiles(smi_batch *b, double *params, double *m, double *v, double *vhat,
                           double *gradient);
int smi_batch_set_profile_moments(smi_batch *b, const double *m, const double *v,
                                  const double *vhat);
/* Probe: the profile `kind` with the six doubles `params` on the h x w box at (origin_y,
 * origin_x), evaluated on `device` in double: out[0] the values, out[1 .. 6] the partial
 * derivatives w.r.t. the six doubles (out is [7][h][w], host memory). */
int smi_profile_probe(int device, int32_t kind, const double *params, int32_t h, int32_t w,
                      int32_t origin_y, int32_t origin_x, double *out);

/* Update rule of the parameters.  SMI_SCHEME_AMSGRAD (default): proxmin.adaprox as used
 * by Blend.fit and lite's AdaproxParameter.  SMI_SCHEME_FISTA: lite's FistaParameter
 * (lite/parameters.py:92-165, Beck & Teboulle 2009): y = z - step/sum(other^2) * grad,
 * x' = prox(y), t' = (1 + sqrt(1 + 4 t^2))/2, z = x + (1 + (t-1)/t')(x' - x); the
 * proximal operator is applied once.  Call before smi_batch_set_components; the
 * state is z (same layout as sed / morph, initialised to x) and t per parameter. */
enum { SMI_SCHEME_AMSGRAD = 0, SMI_SCHEME_FISTA = 1 };
int smi_batch_set_scheme(smi_batch *b, int32_t scheme);
/* t: [n_components][2] (spectrum, morphology); any pointer may be NULL */
int smi_batch_get_fista_state(smi_batch *b, float *z_sed, float *z_morph, double *t);
int smi_batch_set_fista_state(smi_batch *b, const float *z_sed, const float *z_morph,
                              const double *t);

/* AMSGrad constants forwarded by Blend.fit(**alg_kwargs) to adaprox (blend.py:165-180);
 * defaults b1 = 0.9, b2 = 0.999, eps = 1e-8 (lite/parameters.py:194) */
int smi_batch_set_optimizer(smi_batch *b, float b1, float b2, float eps);
/* The same, with b1 and b2 kept in double as well: every kernel goes on with the float32
 * constants, but the moments of monotonic starlet components (star_monotonic) are taken with
 * the doubles -- float32(0.999) alone is 1.3e-5 of v = (1 - b2) g^2.  After
 * smi_batch_set_optimizer the doubles are the float32 values. */
int smi_batch_set_optimizer_f64(smi_batch *b, double b1, double b2, double eps);

/* scarlet.lite's loss has no normalisation term (lite/models.py:541): with
 * include = 0 the recorded loss is 1/2 sum w (m - d)^2 only (default 1: + log_norm,
 * observation.py:147-186).  Call before smi_batch_set_observation. */
int smi_batch_set_log_norm(smi_batch *b, int32_t include);

/* A further observation of every blend on the model's pixel grid: Blend._loss_func sums
 * the log-likelihoods of all observations (blend.py:264-271), so two observations that
 * share model channels are two terms of the loss and of the gradient image.  data, weights:
 * [n_blends][C][H][W] over the MODEL's channels (zero weight where this observation has
 * none); kernel: like smi_batch_set_kernel (same stamp shape / band layout as the batch's).
 * Needs the fused convolution path; call after smi_batch_set_observation / _set_kernel. */
int smi_batch_add_observation(smi_batch *b, const float *data, const float *weights,
                              const float *kernel);

/* Add a constant to the loss of every blend (on top of log_norm + chi^2 / 2).  The
 * facade uses it for the part of an observation that lies outside the model frame:
 * the reference zero-fills the model there (renderer.py:130-161, match_shape), so those
 * pixels contribute sum w d^2 / 2 and their share of log_norm to the loss
 * (observation.py:147-186) and, through |L|, to the stopping rule, but not to the
 * gradient.  Call after smi_batch_set_observation (which resets it). */
int smi_batch_add_loss_constant(smi_batch *b, const double *constant /* [n_blends] */);

/* Seed the "previous loss" of the stopping rule |L - L_prev| < e_rel |L| (same sign
 * convention as smi_batch_get_loss) for a batch that continues an earlier one, e.g.
 * after scarlet.lite resized a box: LiteBlend.fit keeps counting and compares the first
 * new loss with the last old one (lite/models.py:617-619). */
int smi_batch_set_previous_loss(smi_batch *b, const double *loss /* [n_blends] */);

/* HIP stream the batch launches on (hipStream_t as void*); NULL = default stream */
int smi_batch_set_stream(smi_batch *b, void *stream);

/* Blend.get_model + Observation.render + get_log_likelihood for every blend.
 * Any output may be NULL.  model, rendered: [n_blends][C][H][W]; logL[n_blends]
 * (includes -log_norm, observation.py:170-186). */
int smi_batch_forward(smi_batch *b, float *model, float *rendered, double *logL);

/* Gradient of the loss (-logL) w.r.t. every sed and morphology at the current
 * parameters; layout as sed / morph. */
int smi_batch_gradient(smi_batch *b, float *g_sed, float *g_morph);

/* Run `n_iter` iterations of the adaprox loop on the device without host
 * synchronisation; `it0` is the iteration counter of the first one (it = 0 takes
 * a tenth of the step and sets vhat = v).  `e_rel` is the relative tolerance of
 * the proximal sub-iterations (lite/parameters.py:297-303) and, when
 * `check_convergence` != 0, of the per-blend stopping rule evaluated on the device:
 * a blend stops after the update of the iteration in which
 *   it > min_iter && |L[it] - L[it-1]| < e_rel |L[it]|        (blend.py:294-299).
 * Asynchronous on the batch stream. */
int smi_batch_step(smi_batch *b, int32_t it0, int32_t n_iter, float e_rel,
                   int32_t min_iter, int32_t prox_max_iter, int32_t check_convergence);

/* Blends are independent, so a step can run ranges of blends on streams of their own:
 * while one range's update kernel drains, the others' next convolution fills the chip.
 * n = 0 (default): automatic (with the fused convolution 3 ranges from 128 blends on, 4 below
 * 768 blends when smi_set_hw_queues said that eight hardware queues exist; else 1);
 * point sources, free shifts and a low-resolution observation keep it at 1.  Results are
 * identical for every n.  The caller's stream (smi_batch_set_stream) still brackets the
 * step: the ranges start after its pending work and it waits for all of them. */
int smi_batch_set_sub_ranges(smi_batch *b, int32_t n);

/* Hardware queues the HIP runtime of this process maps streams onto (GPU_MAX_HW_QUEUES when
 * the runtime started; HIP's default is 4).  The library cannot see that number and does not
 * read the environment: it assumes 4 until the host says otherwise, and runs four ranges of
 * blends side by side only with n >= 8 (streams that share a queue run one after the other).
 * Process-wide; returns the previous value. */
int smi_set_hw_queues(int32_t n);
int smi_batch_get_sub_ranges(smi_batch *b, int32_t *n);

/* A batch of nothing but factorized components under one fused convolution (no point
 * sources, free shifts, further observations) needs Blend.get_model (blend.py:200-244) only
 * as the input rows of the convolution; by default (on = 1) the convolution kernel renders
 * those rows itself and smi_batch_step neither launches the render kernel nor moves a model
 * cube through HBM.  on = 0 keeps the cube (render kernel per iteration).  The rows are the
 * same bit for bit either way; boxes wider than 81 pixels always take the cube. */
int smi_batch_set_inline_render(smi_batch *b, int32_t on);

/* Blocking.  n_active: blends still iterating; error: index of the first blend
 * whose parameters became non-finite, or -1. */
int smi_batch_status(smi_batch *b, int32_t *n_active, int32_t *first_error);
/* per-blend state: 0 iterating, 1 in its last iteration, 2 converged (stopping rule),
 * 3 stopped with non-finite parameters (Model.check_parameters, model.py:153-165) */
int smi_batch_get_states(smi_batch *b, int32_t *state /* [n_blends] */);

/* Blend.fit for the whole batch: step() in chunks of `sync_every` iterations until
 * max_iter or until every blend has converged.  n_iter[n_blends] receives the
 * number of loss evaluations per blend (= len(blend.loss)). */
int smi_batch_fit(smi_batch *b, int32_t max_iter, float e_rel, int32_t min_iter,
                  int32_t prox_max_iter, int32_t sync_every, int32_t *n_iter);

/* loss history: out[n_blends][capacity] (loss = -logL, blend.py:273); entries past
 * a blend's n_iter are NaN. */
int smi_batch_get_loss(smi_batch *b, double *out, int32_t capacity, int32_t *n_iter);

/* Re-arm all blends (active, loss history cleared); parameters are kept. */
int smi_batch_reset(smi_batch *b);

/* Keep / bring back a device-side copy of everything a step changes (parameters, m / v /
 * vhat, FISTA and point-source state): the warm restart of Blend.fit (X, M, V, Vhat carried
 * into a new adaprox call, blend.py:155-170) without a round trip over the host.
 * smi_batch_restore_state also re-arms the blends like smi_batch_reset.  Both are
 * asynchronous on the batch stream. */
int smi_batch_save_state(smi_batch *b);
int smi_batch_restore_state(smi_batch *b);

/* Mean device time in milliseconds of the dominant kernel family per iteration,
 * measured with hipEvents on the batch stream during the last smi_batch_step call
 * when timing was enabled with smi_batch_enable_timing(b, 1); with several ranges of
 * blends (smi_batch_set_sub_ranges) the times are those of the first range, whose
 * kernels share the chip with the other ranges'.
 * phase: 0 render, 1 forward conv, 2 residual, 3 adjoint conv, 4 update, 5 total */
int smi_batch_enable_timing(smi_batch *b, int32_t on);
int smi_batch_get_timing(smi_batch *b, double *ms_per_phase, int32_t n_phases);

/* FFT shape actually used (fft_h, fft_w) */
int smi_batch_fft_shape(smi_batch *b, int32_t *fft_h, int32_t *fft_w);

/* ---------------------------------------------------------------------------------
 * Box resizing (ImageMorphology.update, morphology.py:132-207; Blend.fit's hook every ten
 * iterations, blend.py:284-292) for a batch that stays on the device between hooks.
 *
 * smi_batch_resize_test: the two reductions update() decides on, per component --
 *   margin[k]: width of the frame of pixels <= 0 around the image (shrink_box; INT32_MAX for
 *   an image without a pixel > 0), edge_pull[k]: the largest of the four edge means of
 *   -m / sqrt(sqrt(v)) * step * (image > 0) over the pixels with v != 0 (-inf if there is
 *   none; summed in another order than NumPy does and with the float32 step: callers treat
 *   values within 1e-6 of the threshold 0.1 as "ask the host").  Point sources and shifted
 *   images report (-1, nan).
 * State record of a component, float32: [sed C][m C][v C][vhat C][image N][m N][v N][vhat N],
 *   N = box_h * box_w.  smi_batch_get_component_states packs the records of the listed
 *   components back to back into `states`.
 * smi_batch_update_components: a new component table (same components per blend, `sed` and
 *   `morph` of *c are not read) in which the components with keep[k] != 0 keep their device-
 *   resident parameters and moments (their boxes must not have changed) and the others take
 *   theirs from `states`, records in the order of k.  The observation, the kernel, the loss
 *   histories and the per-blend states stay.  Factorized image components under AMSGrad
 *   only.  A table that fails the argument checks leaves the old one and its state in place;
 *   after an allocation or transfer error the batch is without components.
 *   keep[k] = 2 / 3: the component keeps its device-resident state and its SQUARE box is resized
 *   about its centre on the device, the way ImageMorphology.update does it on the host
 *   (morphology.py:132-207): the new side is box_h[k] = box_w[k] (sides differ by an even
 *   number, at most 1024 pixels), a smaller box takes the centred slice of image and moments, a
 *   larger one pads the moments with zeros and the image with np.pad(mode="linear_ramp") in
 *   float64 rounded to float32 -- keep 2 when the host image is float32 (the rows added along
 *   axis 0 are rounded before the ramps along axis 1), keep 3 when it is float64.  origin and
 *   morph_step of such a row are the caller's (origin -/+ the inset, step / 2).
 * smi_batch_set_states / smi_batch_get_progress: per-blend state (0 iterating, 2 finished or
 *   paused -- its workgroups return at once --, 3 failed) and number of recorded losses.
 * smi_batch_set_iteration_base: per blend, the iteration counter at which its current adaprox
 *   call began (NULL: 0 for all).  smi_batch_step(it0, n) then runs the blends of a batch at
 *   different counters in one launch: a blend takes the rules of the first step (alpha / 10,
 *   vhat = v: the restart after a box resize, blend.py:276-302) and min_iter from
 *   it - base[b].  Factorized image components under AMSGrad only.
 * --------------------------------------------------------------------------------- */
int smi_batch_resize_test(smi_batch *b, int32_t *margin, double *edge_pull);
int smi_batch_get_component_states(smi_batch *b, const int32_t *components, int32_t n,
                                   float *states);
int smi_batch_update_components(smi_batch *b, const smi_components *c, const int32_t *keep,
                                const float *states);
int smi_batch_set_states(smi_batch *b, const int32_t *state);
int smi_batch_set_iteration_base(smi_batch *b, const int32_t *base);
int smi_batch_get_progress(smi_batch *b, int32_t *state, int32_t *n_loss);
/* Per blend: the iteration counter `it` (as passed to smi_batch_step) after whose update the
 * blend pauses -- it is skipped by the rest of the call like a blend that has stopped (state 2)
 * -- or NULL: nobody pauses.  One smi_batch_step(it0, n) then takes every blend to ITS next
 * resize hook (blend.py:196-198: every ten iterations of the blend's own adaprox call) or to
 * the end of its iteration budget, instead of all blends to the nearest hook of any of them
 * (a thousand blends whose calls restarted at different times: 12 calls instead of 32).
 * smi_batch_get_converged: 1 for the blends whose stopping rule (blend.py:294-299) fired since
 * the last smi_batch_set_pause_at -- what tells a blend that stopped from one that pauses. */
int smi_batch_set_pause_at(smi_batch *b, const int32_t *it);
int smi_batch_get_converged(smi_batch *b, int32_t *flag);
/* What a round of fit_blends sends and fetches, in one call each (stream-ordered copies through
 * a pinned staging buffer: two synchronisations per round instead of eight small blocking
 * copies -- a single scene's fit has eight rounds of ~2 ms).  smi_batch_set_round = set_states +
 * set_iteration_base + set_pause_at (a NULL array is left as it is on the device);
 * smi_batch_get_round = get_progress + get_converged. */
int smi_batch_set_round(smi_batch *b, const int32_t *state, const int32_t *base,
                        const int32_t *pause_at);
int smi_batch_get_round(smi_batch *b, int32_t *state, int32_t *n_loss, int32_t *converged);

/* Number of host-to-device uploads of observation cubes (smi_batch_set_observation and
 * smi_batch_add_observation) this process has made so far: lets a caller -- and the tests --
 * check that a driver which keeps its batch alive does not ship the data again. */
int64_t smi_observation_uploads(void);

/* The convolution path the batch runs (what conv_path = 0 "auto" resolved to):
 * 0 none (NullRenderer, no difference kernel), 1 rocFFT pipeline, 2 fused_conv_kernel. */
int smi_batch_conv_path_used(smi_batch *b, int32_t *path);

/* Ragged frames: blend b's frame is the corner [0, h[b]) x [0, w[b]) of its [C][H][W] plane
 * (1 <= h[b] <= H, 1 <= w[b] <= W); component origins stay relative to that corner.  Every
 * kernel clips components to the blend's own extent instead of H x W: nothing is rendered
 * beyond it, and no gradient flows back from beyond it (lite/models.py:206-216).  The caller
 * pads data and weights beyond the extent (weights 0, data finite).  h = w = NULL gives every
 * blend the full frame again.  The normalisation term of the loss (Observation.log_norm) is
 * formed anew by the call, over every blend's own frame and in the order of a batch of that
 * frame shape, and keeps what smi_batch_add_loss_constant has added; on the fused convolution
 * path a blend's loss then has the bits it has in an unpadded batch (the rocFFT path sums
 * w (m - d)^2 in blocks of the padded plane).
 *
 * smi_batch_set_frame_extents is the call of the lite loop and keeps the contract it had:
 * image components only -- not combined with shifting components, point sources, starlet or
 * profile components, smi_batch_set_kernel_shift, smi_batch_attach_lowres,
 * smi_batch_add_observation or smi_batch_resize_test: those calls, and this one after them,
 * return an error.
 *
 * smi_batch_set_frame_extents_all is the call of the main loop (fit_blends): the same extents
 * for every component kind of the step loop -- image components, point sources, shifting
 * components (the Fourier shift acts on the box, its gradient is gathered from the extent),
 * starlet and profile components -- set before or after this call.  A box may reach beyond its
 * blend's extent into the padding, as it may overhang H x W: those pixels are parameters of
 * the component that see no data and no gradient.  smi_batch_resize_test,
 * smi_batch_update_components (keep codes 2 / 3 included), smi_batch_get_component_states and
 * the per-blend counters (smi_batch_set_round and the calls it stands for) read a component's
 * own box and state only and work as without extents.  Still not combined with
 * smi_batch_set_kernel_shift, smi_batch_attach_lowres or smi_batch_add_observation. */
int smi_batch_set_frame_extents(smi_batch *b, const int32_t *h, const int32_t *w);
int smi_batch_set_frame_extents_all(smi_batch *b, const int32_t *h, const int32_t *w);

/* The FFT shape smi_batch_create picks for a desc with fft_h = fft_w = 0 and these sizes
 * (host only, no GPU): the fused kernel's shape (fused_conv_choose) or, on the rocFFT path, the
 * reference rule fft.py:116-167; (H, W) for kernel_h = kernel_w = 0.  conv_path as in
 * smi_batch_desc (2: an error if the fused kernel cannot take the frame).  A rocFFT batch created
 * while a batch of the transposed complex shape is alive on its device steps aside to a larger
 * Fy (see smi_batch_create); this query does not know about live batches. */
int smi_fft_shape_for(int32_t H, int32_t W, int32_t kernel_h, int32_t kernel_w, int32_t conv_path,
                      int32_t *Fy, int32_t *Fx);

/* ---------------------------------------------------------------------------------
 * Multi-resolution rendering: the per-call part of ResolutionRenderer
 * (renderer.py:478-545) for unrotated pixel grids.  The host builds the two linear
 * operators once (scarlet_amd/renderer.py): A[C][n_a][Fy*Fx], the difference kernel
 * shifted along y to every low-resolution row (renderer.py:341-353), and
 * Pt[Fx][Fx*n_b], the transposed operator that shifts a padded model row to every
 * low-resolution column (renderer.py:498-505).  A rendering of a padded model cube
 * [C][Fy][Fx] is the linear map out[C][n_a][n_b] = A . (model . Pt) per band.
 *
 * The reference's shift is a phase ramp between a real transform and its inverse on the
 * padded grid (renderer.py:414-476), i.e. Pt is circulant along x: Pt[x'][x][b] =
 * s_b[(x - x') mod Fx].  smi_resampler_create checks that, and then evaluates the same map
 * through transforms along x of the model rows, the operator rows (made once, on the
 * device, in float64) and s_b -- path 1, "spectral": 1/25 of the arithmetic and 1/5 of the
 * HBM traffic of the two dense products (path 0), which stay for any other Pt.
 *
 * Between ROTATED pixel grids (renderer.py:319-363, 498-524) the reference Fourier-shifts the
 * padded difference kernel in 2-D to shifts[:, a] for every low-resolution row a (times h^2:
 * the operator) and, per call, the padded model by -other_shifts[:, b] for every column b, and
 * contracts the two over the padded grid.  smi_resampler_create_rotated takes what that needs
 * -- kernel[C][Fy][Fx], scale = h^2, shifts[2][n_a], other_shifts[2][n_b] (y row, then x row) --
 * and evaluates the same map in Fourier space, path 2:
 *
 *   out[c][a][b] = sum_{ky, kx} Re( E[c][a][ky][kx] conj( Mh[c][ky][kx] beta[b][ky][kx] ) )
 *
 * with E[c][a] = scale rfftn(kernel[c]) alpha'[a] and beta[b] = w_kx / (Fy Fx) beta'[b] made once
 * on the device in float64 and kept as float32 complex (C n_a Fy Kx and n_b Fy Kx of them,
 * Kx = Fx / 2 + 1; w = 1 for kx = 0 and the x-Nyquist term, else 2), Mh = rfftn(model) per
 * rendering.  alpha'[a] and beta'[b] are the tables exp(-2 pi i (f_y s_y + f_x s_x)), f_y =
 * fftfreq(Fy), f_x = rfftfreq(Fx), of s = shifts[:, a] and s = -other_shifts[:, b] with the
 * edge-column rule: the inverse real transform of the reference keeps only the Hermitian part
 * along y on the self-conjugate columns kx = 0 and (even Fx) kx = Fx / 2, so there t'[ky] =
 * (t[ky] + conj(t[-ky mod Fy])) / 2.  Sum order: K = Fy Kx is cut into slices of 64 terms
 * (longer where that would give more than 256 slices; a multiple of 32); inside a slice every
 * output adds e.x s.x, -e.y s.y with s = conj(Mh beta) for k ascending in one float64 fma
 * chain (s formed in float64 from the float32 operands and rounded to float32 once), the slices
 * are added in ascending order.  The transpose: Mbar[c][k] = sum_a E[c][a][k]
 * (sum_b resid[c][a][b] conj(beta[b][k])) with b ascending in chunks of 64, a = w (mod 4) per
 * wavefront w and the four sums combined (0 + 1) + (2 + 3), then the inverse transform along
 * y and along x.  Fx <= 2048 (a row and its twiddles live in LDS); Fy, n_a, n_b <= 65535.
 * smi_resampler_set_path refuses to move a rotated resampler to path 0 or 1 and any other to
 * path 2. */
typedef struct smi_resampler smi_resampler;
int smi_resampler_create(const float *A, const float *Pt, int32_t C, int32_t n_a, int32_t n_b,
                         int32_t Fy, int32_t Fx, smi_resampler **out);
int smi_resampler_create_rotated(const float *kernel, double scale, const double *shifts,
                                 const double *other_shifts, int32_t C, int32_t n_a, int32_t n_b,
                                 int32_t Fy, int32_t Fx, smi_resampler **out);
int smi_resampler_render(smi_resampler *r, const float *model, float *out);
/* mean device time (ms) of one rendering of the model last passed to smi_resampler_render,
 * over n_rep repetitions without host transfers (benchmark of BASELINE config 5) */
int smi_resampler_time(smi_resampler *r, int32_t n_rep, double *ms_per_render);
/* the same for the transposed map (smi_resampler_adjoint) of a zero residual */
int smi_resampler_time_adjoint(smi_resampler *r, int32_t n_rep, double *ms_per_call);
int smi_resampler_destroy(smi_resampler *r);
/* which evaluation the resampler uses: 0 = two dense products per band, 1 = spectral, 2 = the
 * Fourier-space contraction between rotated grids.
 * smi_resampler_set_path(r, 0) switches a spectral resampler to the dense products (the
 * parity tests compare the two); path 1 is refused for an operator that is not circulant. */
int smi_resampler_get_path(smi_resampler *r, int32_t *path);
int smi_resampler_set_path(smi_resampler *r, int32_t path);

/* Test entry points of the multi-resolution products (tests/test_resample_host.py,
 * tests/test_gpu_resample.py); not part of the rendering interface.
 *
 * smi_gemm_plan (host only, no GPU): what the matrix product behind both paths launches for
 * C[n_batch][M][N] = A[M][K] . B[K][N] with scratch_elems doubles for slice partials --
 * plan = {tm, tn, bk, kslice, n_slices}: the kernel variant (64 tm x 64 tn block tile, k
 * depth bk), the terms per slice and the number of slices of K.  A plan whose n_slices *
 * n_batch exceeds the grid's z limit of 65535 is an error (the product returns it too).
 *
 * smi_gemm_test: that product on host operands (batch strides in floats, 0 = shared).  C
 * and the scratch are filled with NaNs before the launch; 256 guard floats before and after
 * C and 256 guard doubles after the scratch must come back untouched (*guard_ok = 1).
 *
 * smi_resampler_adjoint: the transposed map of smi_resampler_render on the resampler's
 * current path, resid[C][n_a][n_b] -> gpad[C][Fy][Fx] (host pointers). */
int smi_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t n_batch, int64_t scratch_elems,
                  int32_t plan[5]);
int smi_gemm_test(const float *A, int64_t strideA, const float *B, int64_t strideB, float *C,
                  int64_t strideC, int32_t n_batch, int32_t M, int32_t N, int32_t K,
                  int64_t scratch_elems, int32_t plan[5], int32_t *guard_ok);
int smi_resampler_adjoint(smi_resampler *r, const float *resid, float *gpad);
/* Test entry point (tests/test_gpu_resolution_rot.py): rendering of model[C][Fy][Fx] and
 * transpose of resid[C][n_a][n_b] by a rotated resampler, into out[C][n_a][n_b] and
 * gpad[C][Fy][Fx] (host pointers).  Both device outputs are filled with NaNs before the
 * launches and lie between 256 guard floats; every work array of the rotated map (the two
 * transforms, Mbar, the slice partials) is followed by 256 guard elements.  *guard_ok = 1 if
 * all guards came back untouched.  The work arrays are refilled with NaNs on every call. */
int smi_resampler_rotated_test(smi_resampler *r, const float *model, const float *resid,
                               float *out, float *gpad, int32_t *guard_ok);
/* Test entry point (host only, no GPU): what a rotated resampler of these shapes launches --
 * plan = {ti, tj, tiles along a, tiles along b, terms per slice, slices of K = Fy Kx, chunks of
 * 64 columns b in the transpose}; the contraction's block tile is 16 ti x 16 tj outputs
 * (ti, tj <= 4). */
int smi_resampler_rotated_plan(int32_t n_a, int32_t n_b, int32_t Fy, int32_t Fx, int32_t plan[7]);

/* Test entry point (tests/test_gpu_update_step.py): y[i] = the square root the AMSGrad pass of
 * the update kernels takes when the batch's eps is at least 2^-96 -- the hardware root plus
 * the one-ulp correction, correctly rounded for operands from 2^-96 up, +inf -> +inf.  Host
 * pointers, n < 2^30. */
int smi_sqrt_rn_normal_test(const float *x, float *y, int64_t n);

/* Test entry point (tests/test_update_launch_plan_host.py; needs no device): the launch the
 * per-class update kernel gets for `n_items` components of size class `size_class` (0 .. 8: one
 * wavefront for boxes up to 21^2, 31^2, 41^2, 51^2, 61^2 pixels, then the four-wavefront teams)
 * on a chip of `cu_count` compute units, with `stage_bytes` of ring plan to copy into LDS (< 0:
 * the class has none), in a range of blends with `range_items` >= n_items components of all
 * classes, as one of `n_ranges` ranges that are stepped side by side
 * (smi_batch_set_sub_ranges) and, if `finalize_pending`, with the loss bookkeeping of the
 * iteration waiting for a launch to travel with.
 * plan = {wavefronts or teams per workgroup, updating workgroups, persistent (workgroup i loops
 * over share i of the list: items [i q + min(i, r), ... + q + (i < r)) with q, r = n_items / and
 * % workgroups), plan staged, dynamic LDS bytes without and with the table of gather offsets,
 * byte offset of that table or -1, bookkeeping: 0 none pending, 1 one trailing workgroup per
 * blend, 2 inside the persistent grid, 3 a kernel of its own in front}.  The kernel has 256 B
 * of static LDS per packed wavefront plus 64 B besides. */
int smi_update_launch_plan_test(int32_t n_items, int32_t size_class, int64_t stage_bytes,
                                int32_t cu_count, int32_t range_items, int32_t finalize_pending,
                                int32_t n_ranges, int64_t plan[8]);
/* Test entry point (tests/test_gpu_update_fold.py): that plan as the calling thread's last
 * update launch with a bookkeeping to place actually used it, development switches included
 * (bookkeeping 0: there has been none; the one launch for all small classes of a
 * range: 1 wavefront per workgroup, a workgroup per component, nothing staged). */
int smi_update_last_fold_plan_test(int64_t plan[8]);

/* The low-resolution observation as a further term of a fit (Blend._loss_func sums the
 * log-likelihoods of all observations, blend.py:265-271; Observation.get_log_likelihood,
 * observation.py:147-170).  `channels[C]` gives the model channel of every band of the
 * resampler, `data` / `weights` are [C][n_a][n_b], `log_norm` is Observation.log_norm of
 * that observation.  From then on every iteration renders the model cube through `r`,
 * adds log_norm + chi^2 / 2 to the loss and the transposed operator applied to
 * w (m - d) to the gradient image.  Every call adds one observation of blend 0 (at most 8 per
 * blend).  A resampler on the spectral path hands its tables over (a copy: `r` need not
 * outlive `b`) and the observation joins the pooled chain below; one on the dense path
 * (smi_resampler_set_path(r, 0), or an operator that is not circulant) or between rotated
 * grids (path 2) needs a batch of one blend and must outlive `b`. */
int smi_batch_attach_lowres(smi_batch *b, smi_resampler *r, const int32_t *channels,
                            const float *data, const float *weights, double log_norm);
/* The same for blend `blend` of a batch of any size, from the host operators themselves
 * (A[C][n_a][Fy*Fx], Pt[Fx][Fx*n_b] as for smi_resampler_create; Pt must be circulant, the
 * dense path is not batched): the batch makes the transforms E[C][n_a][Fy][Kx] and
 * beta[n_b][Kx], Kx = Fx / 2 + 1, on its own device -- C n_a Fy Kx 8 bytes per observation --
 * and keeps neither A nor Pt.  Observation i of a blend (the i-th call for it) adds its term
 * at slot i of that blend: loss_b = log_norm_b + chi2_b / 2 + sum_i term[b][i], i in the
 * order of the calls.
 *
 * The i-th observations of one shape class (C, n_a, n_b, Fy, Fx) are evaluated together,
 * nine launches per iteration and class whatever the number of blends: padding of the
 * observed bands, the transforms along x as one batched product over blends x bands,
 * G and out over (row a, band, blend) with every blend's own E and beta, residual and term by
 * one workgroup per (blend, observation), Gbar, Mbar, the transform back and the add into that
 * blend's plane of the gradient image.  A blend gets the bits of its own fit, because every sum
 * keeps its order: G[k] is sixteen fma chains over y = q (mod 16) in increasing y (terms e.x
 * m.x, e.y m.y / e.x m.y, -e.y m.x), added q = 0 .. 15; out is sixteen partials over k = part
 * (mod 16) combined by the xor butterfly 8, 4, 2, 1; Gbar runs over b in increasing order;
 * Mbar is four chains over a = w (mod 4) combined (0 + 1) + (2 + 3); and the two batched
 * products take the slices (float32 inside a slice, double across) that smi_gemm_plan gives
 * the blend's own C bands with its own scratch, whatever the batch.  The terms and renderings
 * of a blend that has stopped are not written again.  Frame extents
 * (smi_batch_set_frame_extents) and low-resolution observations do not combine. */
int smi_batch_attach_lowres_blend(smi_batch *b, int32_t blend, const float *A, const float *Pt,
                                  int32_t C, int32_t n_a, int32_t n_b, int32_t Fy, int32_t Fx,
                                  const int32_t *channels, const float *data,
                                  const float *weights, double log_norm);
/* rendering [C][n_a][n_b] of the index-th attached observation (of blend 0 / of `blend`) in
 * the last forward / gradient / step call that evaluated it */
int smi_batch_get_lowres_rendered(smi_batch *b, int32_t index, float *out);
int smi_batch_get_lowres_rendered_blend(smi_batch *b, int32_t blend, int32_t index, float *out);
/* Test entry points (tests/test_gpu_resample_batch.py, tests/test_fit_blends_multires_host.py).
 * smi_lowres_pool_test: n resamplers of one class (A[n][C][n_a][Fy*Fx], Pt[n][Fx][Fx*n_b])
 * through the pooled chain on host buffers, models[n][C][Fy][Fx] -> out[n][C][n_a][n_b] and
 * resid[n][C][n_a][n_b] -> gpad[n][C][Fy][Fx]; 256 guard floats before and after the pooled
 * out and gpad must come back untouched (*guard_ok = 1).
 * smi_lowres_gemm_plans_test (host only): {tm, tn, bk, kslice, n_slices} of the transform
 * along x (adjoint = 1: the one back) of a resampler with C bands by itself (`own`) and of
 * n_members of them in one launch (`pooled`; more products than the grid's z limit holds are
 * cut into several launches, `pooled` is the first). */
int smi_lowres_pool_test(int32_t n, const float *A, const float *Pt, int32_t C, int32_t n_a,
                         int32_t n_b, int32_t Fy, int32_t Fx, const float *models,
                         const float *resid, float *out, float *gpad, int32_t *guard_ok);
int smi_lowres_gemm_plans_test(int32_t C, int32_t Fy, int32_t Fx, int32_t n_members,
                               int32_t adjoint, int32_t own[5], int32_t pooled[5]);

/* ------------------------------------------------------------------------- *
 * Detection: starlet wavelets (scarlet/wavelet.py) and footprints
 * (scarlet/detect_pybind11.cc) for scarlet/detect.py.
 * ------------------------------------------------------------------------- */

/* starlet_transform (wavelet.py:220-266) of n images [n][H][W] at once: coefficients
 * d_coeffs[scales+1][n][H][W] in float64 whatever the input type, generation 1 or 2, bit for
 * bit the reference's.  d_work: n*H*W doubles of scratch.  Device pointers; the work is
 * enqueued on `stream` (hipStream_t, NULL = default stream) and not waited for.
 * 0 <= scales <= 30 and n*H <= INT32_MAX, whatever H and W: a spacing 2^j of max(H, W) or more
 * reaches no neighbour and leaves the centre tap. */
int smi_starlet_transform_f32(const float *d_images, int32_t n, int32_t H, int32_t W,
                              int32_t scales, int32_t generation, double *d_coeffs,
                              double *d_work, void *stream);
int smi_starlet_transform_f64(const double *d_images, int32_t n, int32_t H, int32_t W,
                              int32_t scales, int32_t generation, double *d_coeffs,
                              double *d_work, void *stream);
/* starlet_reconstruction (wavelet.py:284-311) of n images: d_coeffs[scales+1][n][H][W] ->
 * d_image[n][H][W]; d_work as above (generation 2 only). */
int smi_starlet_reconstruction_f64(const double *d_coeffs, int32_t n, int32_t H, int32_t W,
                                   int32_t scales, int32_t generation, double *d_image,
                                   double *d_work, void *stream);
/* get_multiresolution_support, "ground" branch (wavelet.py:381-407), for n independent
 * images of `planes` coefficient planes each: plane k of image b starts at
 * d_coeffs + k*plane_stride + b*image_stride (elements) and holds H*W pixels.  Host arrays
 * [n][planes]: sigma0 = the initial sigma_j, thresh0 = K*sigma_j of the first iteration (both
 * as the caller's dtype rounded them).  Later iterations use K*sigma_j, sigma_j = the standard
 * deviation of w*(|w| <= K sigma_j) over the plane, until every non-zero sigma_j moved by less
 * than epsilon (relative) or after max_iter iterations.  Outputs in the layout of d_coeffs
 * (either may be NULL): d_support = M (0/1), d_masked = M*w; iterations[n] (host, may be
 * NULL) = iterations run.  Returns when the outputs are complete. */
int smi_multiresolution_support_f64(const double *d_coeffs, int32_t n, int32_t planes,
                                    int32_t H, int32_t W, int64_t plane_stride,
                                    int64_t image_stride, const double *sigma0,
                                    const double *thresh0, double K, double epsilon,
                                    int32_t max_iter, int32_t *d_support, double *d_masked,
                                    int32_t *iterations, void *stream);
/* np.sum(images, axis=0) of bands [bands][H][W] -> d_out[H][W], summed in band order in the
 * images' own type (get_detect_wavelets, detect.py:386). */
int smi_coadd_f32(const float *d_images, int32_t bands, int32_t H, int32_t W, float *d_out,
                  void *stream);
int smi_coadd_f64(const double *d_images, int32_t bands, int32_t H, int32_t W, double *d_out,
                  void *stream);

/* get_detect_wavelets (detect.py:362-399) for a catalogue of blends whose frames, band counts
 * and scale counts differ (detect_batch.hip): coadd, starlet transform, multiresolution support
 * and M * w of every blend, each bit for bit what smi_coadd_* -> smi_starlet_transform_* ->
 * smi_multiresolution_support_f64 give for that blend alone (n = 1).  The table convention is
 * the one of smi_lite_init_*: the tasks are passed in host memory, where they are validated
 * before anything is launched (a bad table returns SMI_ERR_INVALID), and as the copy on the
 * device the kernels read; offsets and sizes count elements; the caller owns every buffer.
 * One task per blend:
 *   bands, h, w   its images [bands][h][w] at image_off of d_images
 *   scales        as given to the transform: planes = scales + 1 coefficient planes [h][w] at
 *                 coeff_off of d_coeffs, d_masked and d_support (ranges in table order, not
 *                 overlapping)
 *   work_off      its plane [h][w] of d_work (ranges in table order, not overlapping)
 *   sigma0, thresh0  the initial sigma_j and K * sigma_j of every plane, as the caller's dtype
 *                 rounded them
 * 1 <= h * w <= 65536 (one workgroup runs all support iterations of a blend; larger frames
 * belong to the per-image entry points above), 0 <= scales <= 30, n <= 65535.
 * Outputs, all in device memory: d_masked = M * w (-0.0 for a negative w outside the support),
 * d_support = M as 0 / 1 (may be NULL), d_iterations[n] = support iterations run.  d_coeffs
 * keeps the unmasked coefficients.  d_scratch: smi_detect_wavelets_scratch_bytes(n) bytes (the
 * final thresholds).  The calls allocate nothing, copy nothing and wait for nothing: they
 * enqueue 1 + 4 * S + 2 launches (generation 2; 1 + 2 * S + 2 for generation 1), S the largest
 * `scales` of the table, on `stream`, whatever n. */
typedef struct smi_detect_task {
    int32_t bands, h, w, scales;
    int64_t image_off, coeff_off, work_off;
    double sigma0, thresh0;
} smi_detect_task;
int smi_detect_wavelets_scratch_bytes(int32_t n, int64_t *bytes);
int smi_detect_wavelets_f32(int32_t n, const smi_detect_task *tasks, const void *d_tasks, double K,
                            double epsilon, int32_t max_iter, int32_t generation,
                            const float *d_images, int64_t n_images, double *d_coeffs,
                            int64_t n_coeffs, double *d_work, int64_t n_work, double *d_masked,
                            int32_t *d_support, int32_t *d_iterations, void *d_scratch,
                            int64_t scratch_bytes, void *stream);
int smi_detect_wavelets_f64(int32_t n, const smi_detect_task *tasks, const void *d_tasks, double K,
                            double epsilon, int32_t max_iter, int32_t generation,
                            const double *d_images, int64_t n_images, double *d_coeffs,
                            int64_t n_coeffs, double *d_work, int64_t n_work, double *d_masked,
                            int32_t *d_support, int32_t *d_iterations, void *d_scratch,
                            int64_t scratch_bytes, void *stream);

/* apply_wavelet_denoising (wavelet.py:424-465) for a ragged list of images, resident on the
 * device (denoise_batch.hip): image_coeffs = T(image) with all the task's scales, generation 2;
 * M = the "ground" multiresolution support of image_coeffs; x = R(image_coeffs); then max_iter
 * times x = x + R(M * (image_coeffs - T(x))) and, if `positive`, x[x < 0] = 0.  Float64 in the
 * reference's operation order: every image's x is bit for bit what smi_starlet_transform_* ->
 * smi_multiresolution_support_f64 (n = 1) -> smi_starlet_reconstruction_f64 give with the
 * element-wise steps between them.  The table convention is the one of smi_detect_wavelets_*
 * (host copy validated before anything is launched, device copy read by the kernels, offsets
 * and sizes in elements, the caller owns every buffer).  One task per image:
 *   h, w       its pixels [h][w] at image_off of d_images
 *   scales     planes = scales + 1 planes [h][w] at coeff_off of d_coeffs (image_coeffs),
 *              d_support (M as 0 / 1) and d_current (work: T(x) and what follows); ranges in
 *              table order, not overlapping
 *   plane_off  its plane [h][w] of d_x (the result) and of d_work; ranges in table order,
 *              not overlapping
 *   sigma0, thresh0  as in smi_detect_task
 * `stages` selects what runs, any union of
 *   SMI_DENOISE_TRANSFORM  d_images -> d_coeffs
 *   SMI_DENOISE_SUPPORT    d_coeffs -> d_support, d_iterations[n] (may be NULL), with max_iter
 *                          iterations at most; h * w <= 65536 (one workgroup per image), d_scratch
 *                          of smi_denoise_scratch_bytes(n) bytes
 *   SMI_DENOISE_ITERATE    d_coeffs, d_support -> d_x
 * so that an image beyond the limit of the support stage takes its support from
 * smi_multiresolution_support_f64 between two calls.  h * w <= 2^30, 0 <= scales <= 30,
 * n <= 65535, max_iter >= 1.  The calls allocate nothing, copy nothing and wait for nothing; they
 * enqueue smi_denoise_launches(S, max_iter, stages) launches on `stream`, S the largest `scales`
 * of the table, whatever n:
 *   (1 + 4 S) + 2 + (2 S + max_iter * max(6 S, 1))     for the three stages. */
enum { SMI_DENOISE_TRANSFORM = 1, SMI_DENOISE_SUPPORT = 2, SMI_DENOISE_ITERATE = 4 };
typedef struct smi_denoise_task {
    int32_t h, w, scales, reserved;
    int64_t image_off, coeff_off, plane_off;
    double sigma0, thresh0;
} smi_denoise_task;
int smi_denoise_scratch_bytes(int32_t n, int64_t *bytes);
int smi_denoise_launches(int32_t top_scales, int32_t max_iter, int32_t stages, int32_t *launches);
int smi_denoise_f32(int32_t n, const smi_denoise_task *tasks, const void *d_tasks, int32_t stages,
                    double K, double epsilon, int32_t max_iter, int32_t positive,
                    const float *d_images, int64_t n_images, double *d_coeffs, int32_t *d_support,
                    double *d_current, int64_t n_coeffs, double *d_x, double *d_work,
                    int64_t n_planes, int32_t *d_iterations, void *d_scratch,
                    int64_t scratch_bytes, void *stream);
int smi_denoise_f64(int32_t n, const smi_denoise_task *tasks, const void *d_tasks, int32_t stages,
                    double K, double epsilon, int32_t max_iter, int32_t positive,
                    const double *d_images, int64_t n_images, double *d_coeffs, int32_t *d_support,
                    double *d_current, int64_t n_coeffs, double *d_x, double *d_work,
                    int64_t n_planes, int32_t *d_iterations, void *d_scratch,
                    int64_t scratch_bytes, void *stream);

/* The resampling products of interpolate_observation (interpolation.py:427-463, 563-599) for a
 * ragged catalogue (sinc_resample.hip): out = Sy . X . Sx^T for every band X [ho][wo] (float32 or
 * float64, widened when read), Sy [hf][ho] and Sx [wf][wo] float64 sinc matrices formed on the
 * host, out [hf][wf] float64.  One task per band and blend, table convention as above:
 *   x_off            the band in d_x
 *   sy_off, sx_off   the matrices in d_mats (the bands of a blend share theirs)
 *   tmp_off          [hf][wo] of d_tmp for Sy . X; ranges in table order, not overlapping
 *   out_off          the result in d_out; ranges in table order, not overlapping
 * Every output element is one accumulator, the terms in ascending inner index, one fused
 * multiply-add per step, first for Sy . X, then for (Sy . X) . Sx^T: its bits do not depend on
 * the list or the grid.  Two launches whatever n <= 65535; nothing allocated, copied or waited
 * for.  SMI_SINC_TILE: the side of the square LDS tiles. */
#define SMI_SINC_TILE 16
typedef struct smi_sinc_task {
    int32_t ho, wo, hf, wf;
    int64_t x_off, sy_off, sx_off, tmp_off, out_off;
} smi_sinc_task;
int smi_sinc_resample_f32(int32_t n, const smi_sinc_task *tasks, const void *d_tasks,
                          const float *d_x, int64_t n_x, const double *d_mats, int64_t n_mats,
                          double *d_tmp, int64_t n_tmp, double *d_out, int64_t n_out,
                          void *stream);
int smi_sinc_resample_f64(int32_t n, const smi_sinc_task *tasks, const void *d_tasks,
                          const double *d_x, int64_t n_x, const double *d_mats, int64_t n_mats,
                          double *d_tmp, int64_t n_tmp, double *d_out, int64_t n_out,
                          void *stream);

/* get_footprints (detect_pybind11.cc) on the host, in two calls.  The first finds the
 * footprints of image[H][W] -- 4-connected pixels > thresh, seeds in raster order, kept when
 * the box has more than min_area pixels and the footprint at least min_area -- with their
 * peaks, keeps them for the calling thread and returns counts[3] = (footprints, mask bytes,
 * peaks).  smi_footprints_fetch then copies them out and forgets them: bounds[n][4] =
 * (y0, y1, x0, x1) inclusive, masks = the footprints' (y1-y0+1) x (x1-x0+1) byte masks one
 * after another, peak_start[n+1] = first peak of every footprint, peak_yx[peaks][2] and
 * peak_flux[peaks], brightest first (ties in raster order).  No GPU needed. */
int smi_get_footprints_f32(const float *image, int32_t H, int32_t W, double min_separation,
                           int32_t min_area, int32_t thresh, int32_t *counts);
int smi_get_footprints_f64(const double *image, int32_t H, int32_t W, double min_separation,
                           int32_t min_area, int32_t thresh, int32_t *counts);
int smi_footprints_fetch(int32_t *bounds, uint8_t *masks, int32_t *peak_start, int32_t *peak_yx,
                         double *peak_flux);

/* The same footprints and peaks for P planes d_images[P][H][W] that live on the device
 * (footprints.hip), in two steps; the results equal the host calls' exactly.  Device pointers
 * carry a d_ prefix, everything else is host memory; the work is enqueued on `stream`
 * (hipStream_t, NULL = default stream).  H*W <= INT32_MAX, P <= 65535.
 *
 * smi_footprints_device_label_* labels every plane (4-connected union-find, a label = the
 * smallest pixel index of its footprint), applies the keep rule and counts, then waits once for
 * counts[P][3] = per plane (footprints, mask bytes, strict maxima).  counts[..][2] counts the
 * peaks BEFORE the min_separation filter, which the fetch applies: it is the capacity the peak
 * arrays need, the number kept is peak_start[n] of the fetch.  d_work: scratch of
 * smi_footprints_device_work_bytes(P, H, W) bytes (32 bytes per pixel and a little more), which
 * holds the labels and records until the last fetch; SMI_ERR_INVALID when a plane has more than
 * 2^31 - 1 mask bytes or maxima.
 *
 * smi_footprints_device_fetch_* fills the arrays of smi_footprints_fetch for one `plane` from
 * d_work, d_images (unchanged since the labelling) and that plane's counts[3]: bounds[n][4],
 * masks[counts[1]], peak_start[n+1], peak_yx[counts[2]][2], peak_flux[counts[2]]; the peaks are
 * sorted and filtered by min_separation on the host as smi_get_footprints_* does.  d_scratch:
 * smi_footprints_device_fetch_bytes(counts) bytes.  It waits for the stream once.
 *
 * The two *_bytes functions are arithmetic and need no device; the others return
 * SMI_ERR_NO_DEVICE without one. */
int smi_footprints_device_work_bytes(int32_t P, int32_t H, int32_t W, int64_t *bytes);
int smi_footprints_device_fetch_bytes(const int32_t *counts, int64_t *bytes);
int smi_footprints_device_label_f32(const float *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t min_area, int32_t thresh, void *d_work,
                                    int64_t work_bytes, int32_t *counts, void *stream);
int smi_footprints_device_label_f64(const double *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t min_area, int32_t thresh, void *d_work,
                                    int64_t work_bytes, int32_t *counts, void *stream);
int smi_footprints_device_fetch_f32(const float *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t plane, double min_separation, const int32_t *counts,
                                    const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                    int32_t *bounds, uint8_t *masks, int32_t *peak_start,
                                    int32_t *peak_yx, double *peak_flux, void *stream);
int smi_footprints_device_fetch_f64(const double *d_images, int32_t P, int32_t H, int32_t W,
                                    int32_t plane, double min_separation, const int32_t *counts,
                                    const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                    int32_t *bounds, uint8_t *masks, int32_t *peak_start,
                                    int32_t *peak_yx, double *peak_flux, void *stream);

/* The same footprints and peaks for a ragged list of n_planes device planes whose frames differ
 * and that may lie anywhere in device memory (footprints_batch.hip): one chain of launches and
 * one wait per call, whatever n_planes; every plane's results equal those of
 * smi_footprints_device_* for that plane alone, exactly.  `table` is host memory, one record per
 * plane:
 *   address     device address of the plane's first pixel, [h][w] contiguous
 *   h, w        > 0, h * w <= INT32_MAX
 *   pixel_off   exclusive prefix over the planes of h * w
 *   tile0       ... of ceil(h / 64) * ceil(w / 64)
 *   chunk0      ... of ceil(h * w / 2048)
 * The prefixes are checked against the shapes (SMI_ERR_INVALID), so are a NULL table, an empty
 * plane and totals beyond INT32_MAX.
 *
 * smi_footprints_batch_label_*: counts[n_planes][3] = per plane (footprints, mask bytes, strict
 * maxima), as the per-frame call.  d_work: smi_footprints_batch_work_bytes(n_planes, table)
 * bytes; the call uploads the table into it, and it holds labels and records until the fetch.
 * Eight launches (seven when every plane is a single 64 x 64 tile), one wait.
 *
 * smi_footprints_batch_fetch_* fills, for all planes at once and in plane order, the arrays of
 * smi_footprints_fetch: bounds[n][4] and masks[] with n = the sum of counts[..][0];
 * fp_start[n_planes + 1] = first footprint of every plane; peak_start[n + 1] = first peak of
 * every footprint in peak_yx[..][2] / peak_flux[..] (capacity: the sum of counts[..][2];
 * peak_start[n] are kept after the min_separation filter).  d_scratch:
 * smi_footprints_batch_fetch_bytes(n_planes, counts) bytes.  Three launches, one wait.
 *
 * stats (may be NULL): stats[0] = kernel launches, stats[1] = stream synchronisations the call
 * made.  The two *_bytes functions are arithmetic and need no device; the others return
 * SMI_ERR_NO_DEVICE without one. */
typedef struct smi_footprint_plane {
    uint64_t address;
    int32_t h, w;
    int64_t pixel_off, tile0, chunk0;
} smi_footprint_plane;
int smi_footprints_batch_work_bytes(int32_t n_planes, const smi_footprint_plane *table,
                                    int64_t *bytes);
int smi_footprints_batch_fetch_bytes(int32_t n_planes, const int32_t *counts, int64_t *bytes);
int smi_footprints_batch_label_f32(const smi_footprint_plane *table, int32_t n_planes,
                                   int32_t min_area, int32_t thresh, void *d_work,
                                   int64_t work_bytes, int32_t *counts, int32_t *stats,
                                   void *stream);
int smi_footprints_batch_label_f64(const smi_footprint_plane *table, int32_t n_planes,
                                   int32_t min_area, int32_t thresh, void *d_work,
                                   int64_t work_bytes, int32_t *counts, int32_t *stats,
                                   void *stream);
int smi_footprints_batch_fetch_f32(const smi_footprint_plane *table, int32_t n_planes,
                                   double min_separation, const int32_t *counts,
                                   const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                   int32_t *bounds, uint8_t *masks, int32_t *fp_start,
                                   int32_t *peak_start, int32_t *peak_yx, double *peak_flux,
                                   int32_t *stats, void *stream);
int smi_footprints_batch_fetch_f64(const smi_footprint_plane *table, int32_t n_planes,
                                   double min_separation, const int32_t *counts,
                                   const void *d_work, void *d_scratch, int64_t scratch_bytes,
                                   int32_t *bounds, uint8_t *masks, int32_t *fp_start,
                                   int32_t *peak_start, int32_t *peak_yx, double *peak_flux,
                                   int32_t *stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SCARLET_AMD_H */
