/*
 * tray_temporal_motion.h — temporal reprojection across scene updates: the step of
 * tray_temporal.h (and, with M2 planes, of tray_temporal_variance.h) for a scene
 * whose spheres moved since the history was made (tray_scene_update.h, or a fresh
 * upload of the new geometry). A hit on sphere i is a point of that sphere's
 * surface; where the same surface point was in the previous frame is known exactly
 * from the sphere's previous centre and radius, so the history is fetched from
 * there. The camera may move too.
 *
 * An addition beside tray.h (ABI 6) and the other feature headers (version 1
 * each), all unchanged, under the same rules: plain C99, caller-owned DEVICE
 * buffers, tray_status / tray_last_error. Arguments are validated before any device
 * work and the call only enqueues on `stream` (a hipStream_t, or NULL for the
 * device's null stream). It uses no launch context and no library-owned workspace.
 *
 * Every value below is a fixed sequence of correctly rounded FP64 + - x /
 * operations and comparisons in the stated order (no FMA contraction), on top of
 * tray_temporal.h's and tray_temporal_variance.h's, so an independent
 * implementation that is given the centre rays' hits reproduces it bit for bit
 * (tests/temporal_motion_ref.py does, in numpy). The parameters are
 * tray_temporal_params, the record is tray_temporal_record and the states are
 * tray_temporal_var_state, as those headers define them.
 *
 * 1. THE STATES. out->m2 and history->m2 (where a history is given) are either all
 *    given or all null. All given: the step of tray_temporal_variance.h section 2
 *    (M2 gather, cap scaling, Welford's fold, the variance plane). All null: the
 *    step of tray_temporal.h section 2, and `variance_device` must be null.
 *
 * 2. THE GEOMETRIES. The scene holds the CURRENT geometry already: the caller ran
 *    tray_scene_update_async, or uploaded the scene afresh, before this call, on
 *    this stream or ordered before it. The current centre c and radius R of a
 *    sphere are the scene's own, what the last upload or update wrote (the sphere
 *    record's centre, the material record's radius); the call takes no second copy
 *    of them. `prev_geometry_device` is what the scene held when `history` was
 *    made: n_spheres x {cx, cy, cz, radius} doubles in list order, the layout of
 *    tray_scene_update_async, so the tensor that was the update's argument one
 *    frame ago serves unchanged. It is not written. Sphere count, order and
 *    materials are the same in both.
 *
 * 3. THE STEP is tray_temporal.h section 2 (2a, 2c, 2d, 2e and the record word for
 *    word; with m2 also tray_temporal_variance.h section 2) with one change, in 2b,
 *    for a hit on list index i with (c', R') = prev_geometry[4i .. 4i + 3]:
 *
 *    b. Target.  Q = o + d * t (Ray.At).
 *       If c'.x == c.x && c'.y == c.y && c'.z == c.z && R' == R (four FP64
 *       comparisons: -0.0 equals 0.0, a NaN equals nothing), the sphere is UNMOVED
 *       and Q' = Q, exactly the static step. Otherwise
 *         m  = (Q - c) / R      per component: the outward normal of
 *                               ray/objects.go:100; R may be negative
 *         Q' = c' + m * R'      per component
 *       Then e = Q' - P.position. A miss keeps e = d.
 *
 *    A zero R, or a NaN or an infinity in the previous geometry, gives a
 *    non-finite projection; the in-range test of 2c then fails and the pixel is
 *    fresh. There is no special case.
 *
 *    TWO REDUCTIONS follow from the unmoved rule and hold bit for bit. With
 *    prev_geometry equal to the scene's geometry every plane and the record equal
 *    tray_temporal_var_step_async's (with m2) and tray_temporal_step_async's
 *    (without). With a partly moved scene that holds on every pixel whose sphere
 *    is unmoved and on every miss.
 *
 * 4. THE MOTION PLANE (`motion_device`, nullable, height x width x 2 doubles): per
 *    pixel (u - (double)x, v - (double)y) when the pixel is IN RANGE (2c), and a NaN
 *    in both components when it is not: the screen-space motion vector that
 *    external denoisers and temporal anti-aliasing take, pointing from the pixel to
 *    where its surface point was in the previous frame, whether or not a tap was
 *    then taken. With a null history (the first frame), or with max_history = 1,
 *    which treats the history as null (tray_temporal.h section 3), NOTHING is
 *    written to it.
 *
 * 5. A KNOWN LIMIT. History follows surfaces, not light. A static surface whose
 *    shading changes because a neighbour moved (a reflection, a refraction, bounce
 *    light, a shadow) keeps its history and converges to the new shading with the
 *    lag of max_history frames. The index and depth tests prevent GHOSTS (a moved
 *    sphere's colour left on what is behind it, or taken from what was in front of
 *    it); they do not prevent lag. A lower max_history shortens it.
 */
#ifndef TRAY_TEMPORAL_MOTION_H
#define TRAY_TEMPORAL_MOTION_H

#include <stddef.h>

#include "tray.h"
#include "tray_temporal.h"
#include "tray_temporal_variance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_TEMPORAL_MOTION_VERSION 1

int32_t tray_temporal_motion_version(void);

/* Section 3 on `stream` of the scene's device: one fused launch, the variance and motion planes
 * included. frame_device holds the new frame of `camera`, height x width x 3 doubles, and is not
 * written. `history` and `prev_camera` may both be NULL: the first frame; prev_geometry_device is
 * then ignored. `out` must not overlap `history` or the frame: the step gathers. variance_device,
 * motion_device and record_device are nullable.
 *
 * Errors: every one of tray_temporal_step_async (with m2: of tray_temporal_var_step_async), and
 * TRAY_ERR_INVALID_ARGUMENT for an n_spheres other than the scene's, m2 planes of out and history
 * partly given, a variance_device without m2, and (on a non-empty image) a null
 * prev_geometry_device when a history is given and the scene has spheres, a prev_geometry_device
 * or motion_device not 8-byte aligned, and a motion plane overlapping the frame, the previous
 * geometry, a plane of history or another output. An empty image is TRAY_OK and launches nothing. */
int tray_temporal_motion_step_async(tray_scene_t scene, const tray_camera *camera, const tray_camera *prev_camera,
                                    const double *prev_geometry_device, int32_t n_spheres,
                                    const tray_temporal_params *tp, const double *frame_device,
                                    const tray_temporal_var_state *history, const tray_temporal_var_state *out,
                                    double *variance_device, double *motion_device,
                                    tray_temporal_record *record_device, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_TEMPORAL_MOTION_H */
