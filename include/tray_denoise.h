/*
 * tray_denoise.h — an edge-avoiding a-trous wavelet denoiser for a linear FP64
 * frame, guided by the first-hit feature buffers of tray_aov.h (albedo, normal,
 * depth). It makes a frame at r = 16 or 64 presentable without leaving the
 * device or this library.
 *
 * An addition beside tray.h (ABI 6), tray_query.h, tray_shade.h and tray_aov.h
 * (version 1 each), all unchanged, under the same rules: plain C99, caller-owned
 * DEVICE buffers, tray_status / tray_last_error. Arguments are validated before
 * any device work and the call only enqueues on `stream` (a hipStream_t, or NULL
 * for the device's null stream). It uses no launch context and no library-owned
 * workspace (the caller passes one), so it is safe from any thread and on any
 * stream, beside renders and queries.
 *
 * THE FILTER. Every value is a fixed sequence of correctly rounded FP64
 * + - x / operations and comparisons (no FMA contraction, no transcendental
 * function), so an independent implementation reproduces it bit for bit
 * (tests/denoise_ref.py does, in numpy).
 *
 *   Edge-stopping function: b(x) = (1 - x) * (1 - x) if x < 1, else 0. A NaN x
 *   gives 0 (the comparison is false).
 *
 *   Floor: m(a) = a if a > 2^-10, else 2^-10 (also for a NaN a), per channel.
 *
 *   Host constants, in C double:
 *     q_c,i = 1.0 / (s_c,i * s_c,i), where s_c,0 = sigma_color and
 *             s_c,i = s_c,i-1 * 0.5 (sigma_color * 2^-i);
 *     q_n   = 1.0 / (sigma_normal * sigma_normal);
 *     q_z   = 1.0 / (sigma_depth * sigma_depth).
 *
 *   Per pixel, once: u = 1.0 / depth if depth > 0, else 0.0.
 *
 *   Input of level 0: with TRAY_DENOISE_DEMODULATE c_0 = colour / m(albedo) per
 *   channel, otherwise c_0 = colour.
 *
 *   Level i = 0 .. iterations - 1, with s = 2^i. For pixel p = (x, y) visit the
 *   taps q = (x + s*dx, y + s*dy), dy = -2..2 in the outer loop and dx = -2..2
 *   in the inner loop, both ascending. A tap outside the image is skipped, not
 *   clamped. k = h[dy] * h[dx] with h = (1/16, 1/4, 3/8, 1/4, 1/16); the product
 *   is exact.
 *     d = c_i(p) - c_i(q);  x_c = ((d_r*d_r + d_g*d_g) + d_b*d_b) * q_c,i
 *     e = n(p) - n(q);      x_n = ((e_x*e_x + e_y*e_y) + e_z*e_z) * q_n
 *     t = (z_p - z_q) * (z_p >= z_q ? u_p : u_q);  x_z = (t*t) * q_z
 *   A null `normal` (`depth`) makes b(x_n) (b(x_z)) the factor 1. Sky against a
 *   sphere gives x_z = q_z: that tap is rejected when sigma_depth < 1.
 *     w = ((k * b(x_c)) * b(x_n)) * b(x_z)
 *   A tap whose w is not > 0 is skipped like one outside the image (for finite
 *   colours this gives the bits of adding w * c_i(q) = 0; it keeps a NaN or
 *   infinite c_i(q) with zero weight out of the sums). Otherwise
 *     acc_ch = acc_ch + w * c_i(q)_ch   and   W = W + w,
 *   both from zero, in tap order. c_i+1(p) = acc / W if W > 0, else c_i(p).
 *
 *   Output: with the flag c_n * m(albedo), otherwise c_n.
 *
 * A NaN colour therefore passes through its own pixel (every w is 0 there) and
 * reaches no neighbour; a NaN or infinite guide value only removes taps.
 */
#ifndef TRAY_DENOISE_H
#define TRAY_DENOISE_H

#include <stddef.h>

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_DENOISE_VERSION 1

#define TRAY_DENOISE_DEMODULATE 1 /* tray_denoise_params.flags: filter colour / m(albedo) */
#define TRAY_DENOISE_MAX_ITERATIONS 8

int32_t tray_denoise_version(void);

typedef struct tray_denoise_guides { /* DEVICE pointers, each nullable: a null guide drops its term */
    const double *albedo;            /* rows x width x 3  (tray_aov_buffers.albedo) */
    const double *normal;            /* rows x width x 3 */
    const double *depth;             /* rows x width */
} tray_denoise_guides;

typedef struct tray_denoise_params {
    int32_t width, rows;                           /* a compact, spatially contiguous image, pitch = width */
    int32_t iterations;                            /* 1..8: level i uses tap spacing 2^i */
    int32_t flags;                                 /* TRAY_DENOISE_DEMODULATE = 1 */
    double sigma_color, sigma_normal, sigma_depth; /* finite, > 0 */
} tray_denoise_params;

/* 5 iterations, TRAY_DENOISE_DEMODULATE, sigma_color 0.5, sigma_normal 0.5, sigma_depth 0.0625
 * (chosen by a sweep on book-cover frames). TRAY_ERR_INVALID_ARGUMENT for a
 * null `out` or a negative width or rows. */
int tray_denoise_default_params(int32_t width, int32_t rows, tray_denoise_params *out);

/* Bytes of DEVICE workspace tray_denoise_async needs for `p`: the intermediate levels
 * ping-pong between images of rows x width x 3 doubles (none for 1 iteration, one for 2,
 * two from 3 on). Validates `p` like tray_denoise_async. */
int tray_denoise_workspace_bytes(const tray_denoise_params *p, size_t *bytes);

/* Enqueues the filter above on `stream` of `device`: one launch per level, demodulation
 * fused into the first level's loads and remodulation into the last level's store.
 * colour_device and out_device hold rows x width x 3 doubles (TRAY_OUT_RGB_F64);
 * workspace_device may be NULL when tray_denoise_workspace_bytes is 0. The buffers must
 * stay unchanged until the stream has run the call.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null colour, guides, p or out, a workspace
 * smaller than tray_denoise_workspace_bytes (or NULL when that is > 0), iterations outside
 * 1..8, unknown flags, a non-finite or non-positive sigma, TRAY_DENOISE_DEMODULATE with a
 * null albedo, a negative width or rows, and `out` equal to or overlapping `colour` or the
 * workspace; TRAY_ERR_TOO_LARGE for rows x width > 2^31 - 1, and when a level would need more
 * than 2^24 - 1 workgroups. Level i with s = 2^i launches
 *   ceil(ceil(width / s) / 32) * ceil(ceil(rows / s) / 8) * min(s, width) * min(s, rows)
 * of them (a 32 x 8 tile of each of the s x s sub-lattices), checked for every level before the
 * first launch. Images of ordinary proportions stay far below it (1280 x 720: 16,384 at most;
 * 2^31 - 1 pixels as 46340 x 46340: 9.0 million); it is reached only by images a few pixels
 * wide or high and tens of millions long, where most of a tile is empty, e.g. width 33,
 * rows 2^25 at 8 iterations. An empty image is TRAY_OK and launches nothing. */
int tray_denoise_async(const double *colour_device, const tray_denoise_guides *guides,
                       const tray_denoise_params *p, double *out_device, void *workspace_device,
                       size_t workspace_bytes, int32_t device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_DENOISE_H */
