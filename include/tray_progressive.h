/*
 * tray_progressive.h — progressive rendering on the device: a running mean and
 * M2 over the pass frames of tray_render_passes_async, the per-pixel variance of
 * that mean with a convergence metric, and the a-trous filter of tray_denoise.h
 * with its colour bandwidth set per pixel from that variance. Together they
 * serve "keep rendering until the picture is good enough, and show the best
 * picture so far" without a frame leaving the device.
 *
 * An addition beside tray.h (ABI 6), tray_query.h, tray_shade.h, tray_aov.h and
 * tray_denoise.h (version 1 each), all unchanged, under the same rules: plain
 * C99, caller-owned DEVICE buffers, tray_status / tray_last_error. Arguments are
 * validated before any device work and every call only enqueues on `stream` (a
 * hipStream_t, or NULL for the device's null stream). No call uses a launch
 * context or a library-owned workspace, so all are safe from any thread and on
 * any stream, beside renders and queries.
 *
 * Every value below is a fixed sequence of correctly rounded FP64 + - x /
 * operations and comparisons (no FMA contraction, no transcendental function,
 * no sqrt), so an independent implementation reproduces it bit for bit
 * (tests/progressive_ref.py does, in numpy).
 *
 * 1. THE ACCUMULATOR. The state is two caller-owned images of rows x width x 3
 *    doubles, `mean` and `m2`, and the number of frames folded so far, `count`,
 *    which lives in the caller's tray_accum on the HOST. `mean` is an ordinary
 *    TRAY_OUT_RGB_F64 frame: it feeds tray_denoise_async,
 *    tray_linear_to_srgba_async and tray_denoise_variance_async as it stands.
 *
 *    Folding frame x (Welford's update), per element, in frame order:
 *      n = n + 1;  t = x - mean;  mean = mean + t / (double)n;
 *      m2 = m2 + t * (x - mean)            (the new mean)
 *    A state with count = 0 starts from mean = 0.0 and m2 = 0.0: the call does
 *    not read the buffers then, so the caller owes no memset and stale bytes do
 *    not matter. The fold is per element and in frame order, so folding 5 frames
 *    in one call, or as 1 + 4, or as 2 + 3, gives the same bits. A NaN or
 *    infinite sample stays in its own element.
 *
 * 2. THE VARIANCE OF THE MEAN AND THE METRIC, from the state after the fold with
 *    n = count:
 *      variance = m2 / D per element, D = (double)n * (double)(n - 1) (one
 *                 multiplication in C double); +infinity in every element when
 *                 n < 2, whatever m2 holds.
 *    Per pixel, with T = tolerance * tolerance (C double):
 *      v = (variance_r + variance_g) + variance_b
 *      e = (mean_r * mean_r + mean_g * mean_g) + mean_b * mean_b
 *      m = e if e > floor, else floor (also for a NaN e)
 *      q = v / m
 *    The pixel is CONVERGED iff n >= 2 and v <= T * m. A NaN anywhere makes the
 *    comparison false: the pixel counts as unconverged. The record receives
 *      unconverged = the number of pixels that are not converged, and
 *      max_ratio   = the largest q over the pixels whose q >= 0 (a NaN q is left
 *                    out; 0.0 when there is none). sqrt(max_ratio) is the worst
 *                    relative standard error of the frame.
 *    Both are order independent, so their bits repeat from run to run: an integer
 *    add of per-workgroup counts, and an integer maximum over the bit patterns of
 *    the non-negative doubles q (which order like the doubles).
 *
 * 3. THE VARIANCE-GUIDED FILTER is the filter of tray_denoise.h — the taps and
 *    their order, the kernel h, b(x), m(a) and its 2^-10 floor, x_n, x_z, u, the
 *    "a tap whose w is not > 0 is skipped" rule, demodulation, NaN pass-through,
 *    the size limits and the workgroup formula — with three changes.
 *
 *    a. A scalar noise plane. v_0(p) = (variance_r / (m_r * m_r) + variance_g /
 *       (m_g * m_g)) + variance_b / (m_b * m_b) with TRAY_DENOISE_DEMODULATE,
 *       m_ch = m(albedo_ch) at p; otherwise v_0(p) = (variance_r + variance_g) +
 *       variance_b.
 *
 *    b. The colour term. At level i with s = 2^i, g_i(p) is the 3 x 3 binomial
 *       mean of v_i around p at the level's own spacing: the points
 *       q = (x + s*dx, y + s*dy), dy = -1..1 in the outer loop and dx = -1..1 in
 *       the inner loop, both ascending; a point outside the image is skipped;
 *       k3 = h3[dy] * h3[dx] with h3 = (1/4, 1/2, 1/4);
 *         G = G + k3 * v_i(q) and B = B + k3, both from zero; g_i(p) = G / B.
 *       (The spacing follows the level, unlike SVGF's fixed 3 x 3, so that the
 *       prefilter reads the same sub-lattice as the taps.) Then, with the host
 *       constant S = sigma_variance * sigma_variance,
 *         den = S * g_i(p) + epsilon if g_i(p) > 0, else epsilon (zero, negative
 *               and NaN g: epsilon alone);   r_i(p) = 1.0 / den;
 *         x_c = ((d_r*d_r + d_g*d_g) + d_b*d_b) * r_i(p)
 *       replaces x_c = (...) * q_c,i. There is no per-level halving: the
 *       propagated variance shrinks instead. An infinite g (a state of fewer
 *       than 2 frames) gives r = 0 and x_c = 0 for finite colours: the colour
 *       term is off and the guides alone decide. Zero variance leaves epsilon
 *       alone: only taps with |d|^2 < epsilon are taken, so each level moves a
 *       channel by less than sqrt(epsilon).
 *
 *    c. The variance propagates. Beside acc and W, over the same taken taps in
 *       the same order, A = A + (w * w) * v_i(q) from zero;
 *         v_i+1(p) = A / (W * W) if W > 0, else v_i(p).
 *       A NaN v_i(q) therefore spreads through the noise plane to the pixels that
 *       take q as a tap (and makes them fall back to epsilon alone), but no value
 *       of the noise plane is ever added to a colour: a NaN variance reaches no
 *       colour, and a NaN colour passes through its own pixel as in tray_denoise.h.
 *       `variance_out`, when given, receives v_iterations: rows x width doubles,
 *       in the units the filter ran in (demodulated with the flag).
 */
#ifndef TRAY_PROGRESSIVE_H
#define TRAY_PROGRESSIVE_H

#include <stddef.h>

#include "tray.h"
#include "tray_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_PROGRESSIVE_VERSION 1

int32_t tray_progressive_version(void);

typedef struct tray_accum {
    double *mean;        /* DEVICE, rows x width x 3 (a TRAY_OUT_RGB_F64 frame) */
    double *m2;          /* DEVICE, rows x width x 3 */
    int32_t width, rows; /* any compact row set: the fold is per element */
    int32_t count;       /* HOST: frames folded so far; 0 = the buffers hold nothing yet. Updated by the fold calls */
    int32_t reserved;    /* 0 */
} tray_accum;

typedef struct tray_accum_metric_params {
    double tolerance; /* finite, >= 0: the relative standard error at which a pixel counts as converged */
    double floor;     /* finite, > 0: the least squared length of the mean the error is measured against */
} tray_accum_metric_params;

typedef struct tray_accum_metric { /* the DEVICE record, 16 bytes */
    uint64_t unconverged;
    double max_ratio;
} tray_accum_metric;

/* tolerance 0.05, floor 2^-10 (a mean colour of length 1/32: darker pixels are measured
 * against that length). TRAY_ERR_INVALID_ARGUMENT for a null `out`. */
int tray_accum_metric_default_params(tray_accum_metric_params *out);

/* Folds n_frames frames into `acc` in frame order, frame k at frames_device + k * rows *
 * width * 3 doubles (as tray_render_passes_async with TRAY_OUT_RGB_F64 writes them), and adds
 * n_frames to acc->count. One launch whatever n_frames is; the state is read once (not at all
 * when acc->count is 0) and written once, every frame element is read once. The buffers must
 * stay unchanged until the stream has run the call; the frames are not written.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null acc, mean, m2 or frames, a pointer that is not
 * 8-byte aligned, a negative width, rows, count or n_frames, a non-zero `reserved`, count +
 * n_frames > 2^31 - 1, and mean, m2 and the frames overlapping one another; TRAY_ERR_TOO_LARGE
 * for rows x width > 2^31 - 1. An empty image, or n_frames == 0, is TRAY_OK, launches nothing
 * and leaves acc->count as it was (the frames may then be NULL). */
int tray_accum_fold_async(tray_accum *acc, const double *frames_device, int32_t n_frames, int32_t device,
                          void *stream);

/* The same fold with section 2 fused into its launch (the state is in registers there, which
 * saves a pass over it): `variance_device` (rows x width x 3 doubles, nullable) and
 * `metric_device` (one tray_accum_metric, nullable) receive the values for the state after the
 * fold. The call zeroes the record itself, stream-ordered ahead of the launch. With
 * n_frames == 0 it evaluates the state as it stands and writes neither mean nor m2.
 *
 * Errors as for tray_accum_fold_async, and TRAY_ERR_INVALID_ARGUMENT for a null `mp`, a
 * tolerance that is not finite and >= 0, a floor that is not finite and > 0, a metric that is
 * not 8-byte aligned, acc->count + n_frames == 0 on a non-empty image (nothing to evaluate),
 * and `variance` or the record overlapping the state, the frames or each other. An empty
 * image is TRAY_OK and launches nothing; the record is then not written. */
int tray_accum_fold_metric_async(tray_accum *acc, const double *frames_device, int32_t n_frames,
                                 const tray_accum_metric_params *mp, double *variance_device,
                                 tray_accum_metric *metric_device, int32_t device, void *stream);

typedef struct tray_denoise_variance_params {
    int32_t width, rows;               /* a compact, spatially contiguous image, pitch = width */
    int32_t iterations;                /* 1..8 */
    int32_t flags;                     /* TRAY_DENOISE_DEMODULATE = 1 */
    double sigma_variance;             /* finite, > 0: colour bandwidth in standard deviations of the noise */
    double sigma_normal, sigma_depth;  /* finite, > 0, as in tray_denoise_params */
    double epsilon;                    /* finite, > 0: added to S * g (squared colour units) */
} tray_denoise_variance_params;

/* 5 iterations, TRAY_DENOISE_DEMODULATE, sigma_variance 3, sigma_normal 0.5, sigma_depth 0.0625,
 * epsilon 1e-12 (sigma_variance and epsilon chosen by a sweep on book-cover frames of 16, 64 and
 * 256 samples). TRAY_ERR_INVALID_ARGUMENT for a null `out` or a negative width
 * or rows. */
int tray_denoise_variance_default_params(int32_t width, int32_t rows, tray_denoise_variance_params *out);

/* Bytes of DEVICE workspace tray_denoise_variance_async needs for `p`: per intermediate
 * ping-pong buffer (none for 1 iteration, one for 2, two from 3 on) an image of rows x width x
 * 3 doubles and a noise plane of rows x width doubles. Validates `p` like the call. */
int tray_denoise_variance_workspace_bytes(const tray_denoise_variance_params *p, size_t *bytes);

/* Enqueues section 3 on `stream` of `device`: one launch per level; v_0, demodulation and
 * remodulation are fused into the first level's loads and the last level's store.
 * colour_device, variance_device (the per-channel variance of the mean, e.g. from
 * tray_accum_fold_metric_async) and out_device hold rows x width x 3 doubles;
 * variance_out_device (nullable) rows x width doubles. workspace_device may be NULL when
 * tray_denoise_variance_workspace_bytes is 0.
 *
 * Errors: as tray_denoise_async (null colour, guides, p or out, workspace, iterations, flags,
 * sigmas, demodulation without albedo, sizes, `out` overlapping `colour` or the workspace, the
 * workgroup limit of every level), and TRAY_ERR_INVALID_ARGUMENT for a null `variance`, a
 * sigma_variance or epsilon that is not finite and > 0, and `variance_out` overlapping
 * `colour`, `variance`, `out` or the workspace, or `out` overlapping `variance`. An empty
 * image is TRAY_OK and launches nothing. */
int tray_denoise_variance_async(const double *colour_device, const double *variance_device,
                                const tray_denoise_guides *guides, const tray_denoise_variance_params *p,
                                double *out_device, double *variance_out_device, void *workspace_device,
                                size_t workspace_bytes, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_PROGRESSIVE_H */
