/*
 * tray_adaptive.h — adaptive sampling on the device: render and fold only the
 * pixels that have not converged. Three calls close the loop that
 * tray_progressive.h leaves open: a renderer over a list of pixels, Welford's
 * fold with a count per pixel, and the step between them, which evaluates the
 * convergence metric per pixel, widens the unconverged set by one pixel and
 * compacts it into the next list.
 *
 * An addition beside tray.h (ABI 6), tray_query.h, tray_shade.h, tray_aov.h,
 * tray_denoise.h and tray_progressive.h (version 1 each), all unchanged, under
 * the same rules: plain C99, caller-owned DEVICE buffers, tray_status /
 * tray_last_error. Arguments are validated before any device work and every
 * call only enqueues on `stream` (a hipStream_t, or NULL for the device's null
 * stream). No call uses a launch context or a library-owned workspace, so all
 * are safe from any thread and on any stream, beside renders and queries.
 *
 * Every value below is a fixed sequence of correctly rounded FP64 + - x /
 * operations and comparisons in the stated order (no FMA contraction), so an
 * independent implementation reproduces it bit for bit (tests/adaptive_ref.py
 * does sections 3 and 4, in numpy; section 2 is compared with tray_render_async).
 *
 * 1. THE STATE is three caller-owned images over a compact, spatially contiguous
 *    image of rows x width pixels (as tray_denoise.h requires: the dilation of
 *    section 4 looks at neighbours): `mean` and `m2`, rows x width x 3 doubles, and
 *    `count`, rows x width int32: the passes folded into each pixel. `mean` is an
 *    ordinary TRAY_OUT_RGB_F64 frame. A state may be seeded from a tray_accum of n
 *    uniform passes (tray_progressive.h) by filling `count` with n.
 *
 * 2. THE RENDERER OVER A PIXEL LIST. `params` defines the image, the samples per
 *    pixel and pass r = rays_per_pixel, the seed and the row set exactly as for
 *    tray_render_aov_async. List entry i names the compact pixel
 *    pixels[i] = j * width + x (compact row j, column x); its image row is the
 *    row set's j-th, y, and the pixel word of its draw blocks is y * width + x in
 *    the coordinates of the whole image. For k in [0, n_passes) the pass rendered
 *    is  params->pass + (pass_plane ? pass_plane[pixels[i]] : 0) + k  (the plane
 *    is rows x width int32, typically the state's `count`); its sample words are
 *    pass * r + s, s = 0 .. r - 1, and must stay within 32 bits.
 *      out[(k * n_pixels + i) * 3 + c]
 *    (pass-major, like the frames of tray_render_passes_async) is the sum of the
 *    pixel's r sample colours from 0.0 in sample order, times the C double
 *    1.0 / r: exactly the bits of that pixel in tray_render_async with
 *    TRAY_FLAG_ORDERED_SUM and that pass, and segments[k * n_pixels + i] that
 *    render's per-pixel Scene.Hit count. The pass of a pixel does not depend on
 *    which other pixels are listed with it (the counter RNG of tray.h).
 *    An entry >= rows x width reads nothing and gets zeros (colour and segments):
 *    the host cannot validate the list, so a bad entry never faults.
 *
 * 3. THE SPARSE FOLD. For each list entry i with p = pixels[i] and n = count[p],
 *    the values x = values[(k * n_pixels + i) * 3 + c], k = 0 .. n_passes - 1, are
 *    folded per channel with the update of tray_progressive.h section 1:
 *      n = n + 1;  t = x - mean;  mean = mean + t / (double)n;
 *      m2 = m2 + t * (x - mean)            (the new mean)
 *    and then count[p] = n. A pixel whose count is 0 starts from mean = 0.0 and
 *    m2 = 0.0 without reading either buffer. An entry >= rows x width is skipped.
 *    THE ENTRIES MUST BE DISTINCT (two entries naming one pixel race); the list
 *    section 4 writes is. Pixels not listed keep their bytes. count + n_passes
 *    must stay within int32 (section 4 stops at max_passes <= 2^30). A NaN or
 *    infinite sample stays in its own element; where a NaN is the result, that it
 *    is a NaN is the contract, its sign and payload are not (IEEE 754 leaves them
 *    open, and `x - mean` with a NaN mean differs between implementations).
 *
 * 4. THE SELECTION. Per pixel p with n = count[p], T = tolerance * tolerance:
 *      variance = m2 / D per element, D = (double)n * (double)(n - 1);
 *                 +infinity in every element when n < 2, whatever m2 holds;
 *      v, e, m, q exactly as tray_progressive.h section 2, from this pixel's own
 *                 variance and mean;
 *      needs(p)  = !(n >= 2 && n >= min_passes && v <= T * m)   (a NaN anywhere
 *                 makes the comparison false: the pixel needs more);
 *      wanted(p) = needs(p), or, when `dilate` is 1, needs(q) for any of the 8
 *                 neighbours q of p that lie inside the image;
 *      active(p) = wanted(p) && n < max_passes.
 *    Outputs: `variance` (nullable, rows x width x 3 doubles: it feeds
 *    tray_denoise_variance_async unchanged); `pixels` (capacity rows x width): the
 *    compact indices of the active pixels in ascending order (entries from
 *    n_active on are not written); and the record:
 *      n_active     = the number of active pixels,
 *      unconverged  = the number of pixels with needs(p),
 *      max_ratio    = the largest q over the pixels whose q >= 0 (0.0 when none),
 *      pixel_passes = the sum of count over the image (counts must be >= 0).
 *    All four are order independent (integer adds and an integer maximum over bit
 *    patterns), so the bits repeat from run to run. With the same count n in every
 *    pixel and min_passes <= 2, unconverged and max_ratio equal the record of
 *    tray_accum_fold_metric_async for that state bit for bit.
 */
#ifndef TRAY_ADAPTIVE_H
#define TRAY_ADAPTIVE_H

#include <stddef.h>

#include "tray.h"
#include "tray_progressive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_ADAPTIVE_VERSION 1

int32_t tray_adaptive_version(void);

typedef struct tray_adaptive_state {
    double *mean, *m2;   /* DEVICE, rows x width x 3 */
    int32_t *count;      /* DEVICE, rows x width: passes folded into each pixel */
    int32_t width, rows; /* a compact, spatially contiguous image (as tray_denoise.h requires) */
} tray_adaptive_state;

typedef struct tray_adaptive_params {
    double tolerance, floor;          /* as tray_accum_metric_params */
    int32_t min_passes, max_passes;   /* 1 <= min <= max <= 2^30 */
    int32_t dilate;                   /* 0 or 1 */
    int32_t reserved;                 /* 0 */
} tray_adaptive_params;

typedef struct tray_adaptive_record {  /* DEVICE, 32 bytes */
    uint64_t n_active, unconverged;
    double max_ratio;
    uint64_t pixel_passes;
} tray_adaptive_record;

/* tolerance 0.05 and floor 2^-10 (tray_accum_metric_default_params), min_passes 8 (chosen by the
 * sweep of tools/adaptive_sweep.py), max_passes 64, dilate 1.
 * TRAY_ERR_INVALID_ARGUMENT for a null `out`. */
int tray_adaptive_default_params(tray_adaptive_params *out);

/* Section 2 on `stream` of the scene's device: one fused launch (camera ray, path and the ordered
 * per-pixel sum; nothing per sample goes to memory). pixels_device holds n_pixels uint32,
 * pass_plane_device (nullable) rows x width int32, out_device n_passes x n_pixels x 3 doubles,
 * segments_device (nullable) n_passes x n_pixels uint32. TRAY_FLAG_LINEAR_SCAN is honoured;
 * TRAY_FLAG_ORDERED_SUM is accepted and changes nothing (the sum is always ordered).
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null scene, camera or params, params that
 * tray_render_async refuses, params->output other than TRAY_OUT_RGB_F64, a negative n_pixels,
 * n_passes < 1, and (n_pixels > 0) null pixels or out; TRAY_ERR_TOO_LARGE for (pass + n_passes) x
 * rays_per_pixel beyond the 32-bit sample word, rows x width > 2^31 - 1, and n_pixels x n_passes
 * x rays_per_pixel > 2^31 - 1. n_pixels == 0 is TRAY_OK and launches nothing. */
int tray_render_pixels_async(tray_scene_t scene, const tray_camera *camera, const tray_params *params,
                             const uint32_t *pixels_device, int64_t n_pixels, const int32_t *pass_plane_device,
                             int32_t n_passes, double *out_device, uint32_t *segments_device, void *stream);

/* Section 3 on `stream` of `device`: one launch. values_device holds n_passes x n_pixels x 3
 * doubles (as tray_render_pixels_async writes them) and is not written.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null state, a negative width or rows, a negative
 * n_pixels, n_passes outside 1..65535, and (on a non-empty image with n_pixels > 0) a null mean,
 * m2, count, pixels or values, mean, m2 or values not 8-byte aligned, count or pixels not 4-byte
 * aligned, and any two of mean, m2, count, pixels and values overlapping; TRAY_ERR_TOO_LARGE for
 * rows x width or n_pixels > 2^31 - 1. An empty image or n_pixels == 0 is TRAY_OK and launches
 * nothing. */
int tray_adaptive_fold_async(const tray_adaptive_state *state, const uint32_t *pixels_device, int64_t n_pixels,
                             const double *values_device, int32_t n_passes, int32_t device, void *stream);

/* Bytes of DEVICE workspace tray_adaptive_select_async needs for a width x rows image: a flag
 * plane of one byte per pixel, padded to a multiple of 8 bytes, and one uint32 total per block of
 * 1024 pixels, padded to a multiple of 8 bytes:
 *   P = width * rows;  bytes = (P + 7) / 8 * 8 + ((P + 1023) / 1024 + 1) / 2 * 8   (0 when P == 0).
 * TRAY_ERR_INVALID_ARGUMENT for a negative width or rows or a null `bytes`, TRAY_ERR_TOO_LARGE for
 * P > 2^31 - 1. */
int tray_adaptive_workspace_bytes(int32_t width, int32_t rows, size_t *bytes);

/* Section 4 on `stream` of `device`: the metric pass, the block totals, their scan and the
 * compaction (four small launches; the call zeroes the record itself, stream-ordered, and owes
 * the workspace no initial contents). The state is not written.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null state, params, pixels or record, a negative width
 * or rows, a tolerance that is not finite and >= 0, a floor that is not finite and > 0,
 * min_passes or max_passes outside 1 <= min <= max <= 2^30, dilate other than 0 or 1, a non-zero
 * `reserved`, and (on a non-empty image) a null mean, m2 or count, a null workspace or
 * workspace_bytes below tray_adaptive_workspace_bytes, mean, m2, variance, the record or the
 * workspace not 8-byte aligned, count or pixels not 4-byte aligned, and the outputs (variance,
 * pixels, the record, the workspace) overlapping the state or one another; TRAY_ERR_TOO_LARGE for
 * rows x width > 2^31 - 1. An empty image is TRAY_OK and launches nothing; the record is then not
 * written. */
int tray_adaptive_select_async(const tray_adaptive_state *state, const tray_adaptive_params *params,
                               double *variance_device, uint32_t *pixels_device,
                               tray_adaptive_record *record_device, void *workspace_device, size_t workspace_bytes,
                               int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_ADAPTIVE_H */
