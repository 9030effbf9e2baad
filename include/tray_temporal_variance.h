/*
 * tray_temporal_variance.h — temporal reprojection that also carries the
 * second moment: the step of tray_temporal.h with an M2 plane beside the colour,
 * so that a temporal state is at the same time a tray_adaptive_state
 * {mean = colour, m2, count = age, width, rows = height}. The variance-guided
 * filter (tray_progressive.h section 3), the selection, the pixel-list renderer
 * and the sparse fold (tray_adaptive.h) then apply to a moving camera's state
 * unchanged: fresh pixels can be given more samples, and the filter knows how
 * much to trust each pixel.
 *
 * An addition beside tray.h (ABI 6), tray_query.h, tray_shade.h, tray_aov.h,
 * tray_denoise.h, tray_progressive.h, tray_adaptive.h and tray_temporal.h
 * (version 1 each), all unchanged, under the same rules: plain C99, caller-owned
 * DEVICE buffers, tray_status / tray_last_error. Arguments are validated before
 * any device work and every call only enqueues on `stream` (a hipStream_t, or
 * NULL for the device's null stream). No call uses a launch context or a
 * library-owned workspace, so all are safe from any thread and on any stream.
 *
 * Every value below is a fixed sequence of correctly rounded FP64 + - x /
 * operations, int -> double conversions and comparisons in the stated order (no
 * FMA contraction), on top of tray_temporal.h's, so an independent
 * implementation reproduces it bit for bit (tests/temporal_variance_ref.py does,
 * in numpy). The parameters are tray_temporal_params and the record is
 * tray_temporal_record, as tray_temporal.h defines them.
 *
 * 1. THE STATE is a tray_temporal_state (tray_temporal.h section 1) plus `m2`,
 *    height x width x 3 doubles: per channel the sum of squared deviations of the
 *    `age` frames folded into the pixel from their mean `colour` (Welford's M2,
 *    tray_progressive.h section 1), so that m2 / (age - 1) is the sample variance
 *    of a frame's pixel and m2 / (age x (age - 1)) the variance of `colour`.
 *
 * 2. THE STEP is tray_temporal.h section 2 with additions that do not feed back
 *    into it: out.colour, out.age, out.index, out.depth and the record have exactly
 *    the bits tray_temporal_step_async gives for the same scene, cameras,
 *    parameters, frame and history (colour, age, index, depth). The rule for which
 *    taps are TAKEN is that section's 2d unchanged: M2 is never examined by it. An
 *    infinite or NaN m2 travels with the colour it belongs to, as infinite colours
 *    do there. With the names of that section (w, q, W, H, A, X, h, k):
 *
 *    a. Gather. Over the taken taps, in the same order as H, from M = (0.0, 0.0, 0.0):
 *         M.ch = M.ch + w * history.m2[q].ch;      then m = M / W per channel.
 *    b. Cap. With n0 = k - 1 (k of section 2e, so 1 <= n0 <= max_history - 1):
 *         if A > n0:  m = m * ((double)(n0 - 1) / (double)(A - 1))
 *       (one division, then one multiplication per channel); otherwise m is
 *       unchanged. A history pretended shorter than it is keeps its sample variance
 *       m2 / (n - 1); n0 = 1 gives 0 (times m: a NaN for an infinite m). The scaling
 *       also covers A > max_history, which a fold into the state from outside the
 *       step (section 4) can produce.
 *    c. Fold. With t = X - h per channel:
 *         out.colour = h + t / (double)k            (tray_temporal.h's expression)
 *         out.m2     = m + t * (X - out.colour)     (the new colour)
 *       which is Welford's update, tray_progressive.h section 1.
 *    d. A FRESH pixel (the first frame and max_history = 1 included): out.m2 = 0.0.
 *    e. `variance` (nullable, height x width x 3 doubles): per element
 *         out.m2 / ((double)k * (double)(k - 1)),  k = out.age,
 *       and +infinity in every element when k < 2 (a fresh pixel): the formula of
 *       tray_adaptive.h section 4, so the plane feeds tray_denoise_variance_async
 *       unchanged.
 *
 *    AN APPROXIMATION, said plainly: a bilinear gather blends the M2 of up to four
 *    history pixels of different ages with the colour's weights, and then treats
 *    the blend as the M2 of min-age A samples. A weighted mean of four estimates
 *    has a lower variance than any one of them (the resampling blur), and samples
 *    of neighbouring pixels are not samples of this pixel, so the carried M2 is a
 *    guide for a filter and for refill decisions, not an unbiased estimator. Its
 *    calibration against a converged reference is measured by
 *    tools/temporal_variance_sweep.py. Under a static camera every
 *    tap is snapped with weight 1.0 and nothing is approximated: colour and m2
 *    after K steps (max_history above K) have exactly the bits of
 *    tray_accum_fold_async over the same K frames, and `variance` those of
 *    tray_accum_fold_metric_async.
 *
 * 3. THE VARIANCE OF LISTED PIXELS. tray_temporal_var_variance_async writes
 *    formula 2e from the state's m2 and age (k = age[p]) for the pixels
 *    p = pixels[i], i < n_pixels, only; it treats the list as
 *    tray_adaptive_fold_async does: an entry >= height x width is skipped, and
 *    pixels that are not listed keep their bytes. A null list means every pixel.
 *
 * 4. THE REFILL CHAIN needs no further call. After the step, on the out state
 *    viewed as a tray_adaptive_state:
 *      tray_adaptive_select_async  (min_passes = 1 + R, max_passes = max_history, a
 *                                   tolerance so large that only the count decides,
 *                                   finite with a finite square, e.g. 1e150)
 *      a 32-byte record readback for n_active
 *      tray_render_pixels_async    (the list, R passes, a null pass_plane)
 *      tray_adaptive_fold_async
 *      tray_temporal_var_variance_async over the list (the fold changed age and m2
 *                                   of the listed pixels after the step wrote variance).
 *    Frame f owns the passes [f (1 + R), (f + 1)(1 + R)): the uniform frame is the
 *    first of them, the refill passes are the rest, so every sample of a pixel is
 *    distinct. Tracer.RenderSequence(refill=R) does this.
 */
#ifndef TRAY_TEMPORAL_VARIANCE_H
#define TRAY_TEMPORAL_VARIANCE_H

#include <stddef.h>

#include "tray.h"
#include "tray_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_TEMPORAL_VAR_VERSION 1

int32_t tray_temporal_var_version(void);

typedef struct tray_temporal_var_state {
    double *colour, *m2;  /* DEVICE, height x width x 3: the accumulated linear frame and its M2 */
    int32_t *age, *index; /* DEVICE, height x width: as tray_temporal_state */
    double *depth;        /* DEVICE, height x width: as tray_temporal_state */
    int32_t width, height;
} tray_temporal_var_state;

/* Section 2 on `stream` of the scene's device: one fused launch, the variance plane included.
 * frame_device holds the new frame of `camera`, height x width x 3 doubles, and is not written.
 * `history` and `prev_camera` may both be NULL: the first frame. `out` must not overlap `history`
 * or the frame: the step gathers. variance_device and record_device are nullable.
 *
 * Errors: as tray_temporal_step_async, with the m2 planes and the variance included:
 * TRAY_ERR_INVALID_ARGUMENT for a null scene, camera, params or out, exactly one of history and
 * prev_camera null, a negative width or height, a history whose width or height differs from out's,
 * max_history outside 1 .. 2^30, flags other than TRAY_FLAG_LINEAR_SCAN, a depth_tolerance that is
 * not finite and >= 0, a snap that is not finite, >= 0 and < 0.5, a non-zero `reserved`, and (on a
 * non-empty image) a null frame or a null plane of out or of history, the frame, a colour, m2 or
 * depth plane, the variance or the record not 8-byte aligned, an age or index plane not 4-byte
 * aligned, and a plane of out, the variance or the record overlapping the frame, a plane of history
 * or another output; TRAY_ERR_TOO_LARGE for width x height > 2^31 - 1. An empty image is TRAY_OK
 * and launches nothing; the record is then not written. */
int tray_temporal_var_step_async(tray_scene_t scene, const tray_camera *camera, const tray_camera *prev_camera,
                                 const tray_temporal_params *tp, const double *frame_device,
                                 const tray_temporal_var_state *history, const tray_temporal_var_state *out,
                                 double *variance_device, tray_temporal_record *record_device, void *stream);

/* Section 3 on `stream` of `device`: one launch. Only m2 and age of the state are read.
 * pixels_device holds n_pixels uint32, or is NULL for every pixel (n_pixels is then ignored).
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null state, a negative width or height, a negative
 * n_pixels with a list, and (on a non-empty image, and n_pixels > 0 with a list) a null m2, age or
 * variance, m2 or the variance not 8-byte aligned, age or the list not 4-byte aligned, and the
 * variance overlapping m2, age or the list; TRAY_ERR_TOO_LARGE for width x height or n_pixels
 * > 2^31 - 1. An empty image, or n_pixels == 0 with a list, is TRAY_OK and launches nothing. */
int tray_temporal_var_variance_async(const tray_temporal_var_state *state, const uint32_t *pixels_device,
                                     int64_t n_pixels, double *variance_device, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_TEMPORAL_VARIANCE_H */
