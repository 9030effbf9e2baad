/*
 * tray_temporal.h — temporal reprojection on the device: reuse the last frame
 * under a moving camera. One call finds, per pixel, where the surface seen
 * through the pixel's centre was in the previous frame, fetches the accumulated
 * colour from there if it is still the same surface, and folds the new frame
 * into it. The scene is static (an uploaded scene is immutable); the camera moves.
 *
 * An addition beside tray.h (ABI 6), tray_query.h, tray_shade.h, tray_aov.h,
 * tray_denoise.h, tray_progressive.h and tray_adaptive.h (version 1 each), all
 * unchanged, under the same rules: plain C99, caller-owned DEVICE buffers,
 * tray_status / tray_last_error. Arguments are validated before any device work
 * and the call only enqueues on `stream` (a hipStream_t, or NULL for the device's
 * null stream). It uses no launch context and no library-owned workspace, so it
 * is safe from any thread and on any stream, beside renders and queries.
 *
 * Every value below is a fixed sequence of correctly rounded FP64 + - x /
 * operations, fabs, floor, int <-> double conversions and comparisons in the
 * stated order (no FMA contraction, no transcendental; the one sqrt is the one
 * inside Scene.Hit), so an independent implementation that is given the centre
 * rays' hits reproduces it bit for bit (tests/temporal_ref.py does, in numpy).
 *
 * Vector operations are per component in the order written, and
 *   dot(u, v)   = (u.x * v.x + u.y * v.y) + u.z * v.z              (ray/vec3.go Dot)
 *   cross(u, v) = { u.y * v.z - u.z * v.y,  u.z * v.x - u.x * v.z,  u.x * v.y - u.y * v.x }
 *                                                                  (ray/vec3.go Cross)
 *
 * 1. THE STATE of one frame is four caller-owned planes over the FULL frame of
 *    width x height pixels, row-major, pixel p = y * width + x: `colour`, the
 *    accumulated linear frame (an ordinary TRAY_OUT_RGB_F64 frame); `age`, the
 *    frames folded into the pixel (>= 1 after a step; a value < 1 marks a pixel
 *    without history); `index`, the list index of the sphere the pixel's centre ray
 *    hits (-1: none); and `depth`, that hit's root t (+infinity: none). Row sets and
 *    tiles (tray_params' y_start, tile_rows) are NOT SUPPORTED in version 1: the
 *    gather of section 2 looks anywhere in the previous frame, so a state is always
 *    the whole image, and there is no argument that could say otherwise.
 *
 * 2. THE STEP, per pixel (x, y), with C = `camera`, P = `prev_camera`, the new
 *    frame's colour X = frame[p] (three channels) and the parameters `tp`:
 *
 *    a. Centre ray.  s = (C.pixel00 + C.pixel_x * (double)x) + C.pixel_y * (double)y
 *       (Camera.GetRay's order with zero offsets; the lens is not sampled, whatever
 *       the aperture),  o = C.position,  d = s - o,
 *         (i, t) = Scene.Hit(o, d, Interval{1e-6, +inf})
 *       exactly as tray_scene_hit_async reports it (i the list index, t the root).
 *       out.index = i (-1 for a miss), out.depth = t (+infinity for a miss).
 *
 *    b. Target.  On a hit Q = o + d * t (Ray.At) and e = Q - P.position; on a miss
 *       e = d (the sky depends on the direction alone, so the direction is what is
 *       reprojected).
 *
 *    c. Projection into P.  n = cross(P.pixel_x, P.pixel_y),  c0 = P.pixel00 - P.position,
 *         z = dot(n, e) / dot(n, c0)
 *       (P.pixel00 lies on the image plane, so z is the parameter the previous
 *       centre ray through Q would have had: the planar depth in units of the focal
 *       length, the same unit as `depth`),
 *         g = (e / z) - c0,
 *         u = dot(g, P.pixel_x) / dot(P.pixel_x, P.pixel_x),
 *         v = dot(g, P.pixel_y) / dot(P.pixel_y, P.pixel_y).
 *       IN RANGE iff  z > 0 && u > -1 && u < (double)width && v > -1 && v < (double)height
 *       (a NaN fails every test).
 *
 *    d. Taps (only when in range).  xr = floor(u + 0.5), yr = floor(v + 0.5).
 *       Snapped: if fabs(u - xr) <= snap && fabs(v - yr) <= snap, one tap at (xr, yr)
 *       with weight 1.0. Bilinear otherwise: x0 = floor(u), a = u - x0, y0 = floor(v),
 *       b = v - y0, and four taps in this order:
 *         (x0, y0)         w = (1 - a) * (1 - b)
 *         (x0 + 1, y0)     w = a * (1 - b)
 *         (x0, y0 + 1)     w = (1 - a) * b
 *         (x0 + 1, y0 + 1) w = a * b
 *       A tap at (tx, ty), history pixel q = ty * width + tx, is TAKEN iff
 *         0 <= tx < width && 0 <= ty < height,  w > 0,  history.age[q] >= 1,
 *         history.index[q] == i,
 *         i < 0  ||  fabs(history.depth[q] - z) <= depth_tolerance * z,
 *         and none of history.colour[q]'s three channels is a NaN.
 *       Over the taken taps, in order, from W = 0.0 and H = (0.0, 0.0, 0.0):
 *         W = W + w;   H.ch = H.ch + w * colour[q].ch;   A = the smallest of their ages.
 *
 *    e. Fold.  If in range and W > 0:
 *         h = H / W (per channel),  k = min(A, max_history - 1) + 1,
 *         out.colour = h + (X - h) / (double)k,   out.age = k.
 *       Otherwise the pixel is FRESH: out.colour = X, out.age = 1.
 *       With a null history (the first frame), or with max_history = 1, every
 *       pixel is fresh, and only step a. is evaluated. A NaN X goes into its own
 *       pixel only; the next step does not take that pixel, so a NaN lives for one
 *       frame. Where a NaN is the result (a NaN X, or infinite history colours of
 *       both signs), that it is a NaN is the contract, its sign and payload are not
 *       (IEEE 754 leaves them open).
 *
 *    The record (nullable) is zeroed by the call, stream-ordered ahead of the launch:
 *    `fresh` = the number of fresh pixels, `age_sum` = the sum of out.age over the
 *    image. Both are integer adds, so the bits repeat from run to run.
 *
 * 3. TWO PROPERTIES (tests/test_temporal_ref_cpu.py, tests/test_gpu_temporal.py).
 *    Static camera: with P == C the projection returns (x, y) up to a rounding
 *    error far below `snap`, so every pixel takes its own history with weight 1.0,
 *    h is the history's colour exactly, and the fold is the mean update of
 *    tray_progressive.h section 1. With max_history above the frame count
 *    out.colour after K steps has exactly the bits of tray_accum_fold_async's mean
 *    over the same K frames: an idle viewer converges as RenderProgressive does,
 *    without resampling blur (that is what `snap` is for).
 *    History cap: out.age never exceeds max_history. max_history = 1 leaves no room
 *    for history (k would be 1 and the fold h + (X - h), which is X only up to
 *    rounding), so the call then treats `history` as null whatever it holds: the
 *    step returns the frame itself, out.colour = X, out.age = 1, fresh = width x height.
 */
#ifndef TRAY_TEMPORAL_H
#define TRAY_TEMPORAL_H

#include <stddef.h>

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_TEMPORAL_VERSION 1

int32_t tray_temporal_version(void);

typedef struct tray_temporal_state {
    double *colour;  /* DEVICE, height x width x 3: the accumulated linear frame (a TRAY_OUT_RGB_F64 frame) */
    int32_t *age;    /* DEVICE, height x width: frames folded into the pixel, >= 1 after a step */
    int32_t *index;  /* DEVICE, height x width: list index of the sphere the pixel's centre ray hits, -1 none */
    double *depth;   /* DEVICE, height x width: that hit's root t, +inf for none */
    int32_t width, height;
} tray_temporal_state;

typedef struct tray_temporal_params {
    int32_t max_history;     /* 1 .. 2^30: the cap of `age` (k of section 2e never exceeds it) */
    int32_t flags;           /* 0 or TRAY_FLAG_LINEAR_SCAN (the centre ray's Scene.Hit by the scan: verification) */
    double depth_tolerance;  /* finite, >= 0: relative, section 2d */
    double snap;             /* finite, >= 0 and < 0.5, in pixels: section 2d */
    int64_t reserved;        /* 0 */
} tray_temporal_params;

typedef struct tray_temporal_record {  /* DEVICE, 16 bytes */
    uint64_t fresh, age_sum;
} tray_temporal_record;

/* depth_tolerance 0.1 (the best row of the sweep of tools/temporal_sweep.py),
 * max_history 32 (that sweep's 8-frame orbit cannot tell 8 from 64), snap 2^-20, flags 0.
 * TRAY_ERR_INVALID_ARGUMENT for a null `out`. */
int tray_temporal_default_params(tray_temporal_params *out);

/* Section 2 on `stream` of the scene's device: one fused launch (centre ray, projection, gather,
 * fold and the record's sums). frame_device holds the new frame of `camera`, height x width x 3
 * doubles, and is not written. `history` and `prev_camera` may both be NULL: the first frame.
 * `out` must not overlap `history` or the frame: the step gathers.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null scene, camera, params or out, exactly one of
 * history and prev_camera null, a negative width or height, a history whose width or height differs
 * from out's, max_history outside 1 .. 2^30, flags other than TRAY_FLAG_LINEAR_SCAN, a
 * depth_tolerance that is not finite and >= 0, a snap that is not finite, >= 0 and < 0.5, a
 * non-zero `reserved`, and (on a non-empty image) a null frame or a null plane of out or of history,
 * the frame, a colour or depth plane or the record not 8-byte aligned, an age or index plane not
 * 4-byte aligned, and a plane of out or the record overlapping the frame, a plane of history or
 * another output; TRAY_ERR_TOO_LARGE for width x height > 2^31 - 1. An empty image is TRAY_OK and
 * launches nothing; the record is then not written. */
int tray_temporal_step_async(tray_scene_t scene, const tray_camera *camera, const tray_camera *prev_camera,
                             const tray_temporal_params *tp, const double *frame_device,
                             const tray_temporal_state *history, const tray_temporal_state *out,
                             tray_temporal_record *record_device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_TEMPORAL_H */
