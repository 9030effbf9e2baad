/* include/tray_temporal_motion.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): an animation loop that moves the spheres in place, renders the new frame and
 * folds it into the history that followed the spheres, over two ping-pong states, with the geometry
 * of the frame before as the previous geometry. Compiled with -std=c99 -Wall -Werror -pedantic by
 * tests/test_temporal_motion_abi_cpu.py and linked against the library; run only without a device
 * (argument errors). */
#include <stddef.h>

#include "tray_scene_update.h"
#include "tray_temporal_motion.h"

/* Frame k of an animation: geometries holds the frames' n x 4 doubles one after the other on the
 * device. The update's record is the caller's to read before it trusts the frame (a refused update
 * leaves the old geometry in the scene: upload geometries[k] afresh and call this with update = 0). */
int tray_temporal_motion_frame(tray_scene_t scene, const tray_camera *camera, int32_t k, int update,
                               const double *geometries, int32_t n, tray_params *params,
                               const tray_temporal_params *tp, double *frame, const tray_temporal_var_state *states,
                               double *variance, double *motion, tray_scene_update_record *update_record,
                               tray_temporal_record *record, void *stream) {
    const double *geometry = geometries + (size_t)k * (size_t)n * 4;
    int rc;
    if (tray_temporal_motion_version() != TRAY_TEMPORAL_MOTION_VERSION) return TRAY_ERR_UNSUPPORTED;
    if (!params || !tp || !states) return TRAY_ERR_INVALID_ARGUMENT;
    if (update) {
        rc = tray_scene_update_async(scene, geometry, n, update_record, stream);
        if (rc != TRAY_OK) return rc;
    }
    params->pass = k;
    rc = tray_render_async(scene, camera, params, frame, NULL, stream);
    if (rc != TRAY_OK) return rc;
    return tray_temporal_motion_step_async(scene, camera, k ? camera : NULL, k ? geometry - (size_t)n * 4 : NULL, n, tp,
                                           frame, k ? &states[(k - 1) & 1] : NULL, &states[k & 1], variance, motion,
                                           record, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_temporal_params tp;
    tray_temporal_var_state out = {NULL, NULL, NULL, NULL, NULL, 4, 4}, hist;
    tray_temporal_record rec;
    tray_camera cam[2] = {{{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}, {{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}};
    double frame[48], colour[48], m2[48], depth[16], colour2[48], m22[48], depth2[16], variance[48], motion[32];
    double geometry[12];
    int32_t age[16], index[16], age2[16], index2[16];
    int fake;
    tray_scene_t scene = (tray_scene_t)&fake; /* never looked at: validation fails first */
    if (tray_temporal_motion_version() != TRAY_TEMPORAL_MOTION_VERSION || tray_temporal_var_version() != 1) return 1;
    if (tray_temporal_default_params(&tp) != TRAY_OK) return 2;
    if (tray_temporal_motion_step_async(NULL, &cam[0], NULL, NULL, 3, &tp, frame, NULL, &out, NULL, motion, &rec,
                                        NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 3; /* null scene */
    if (!tray_last_error() || !tray_last_error()[0]) return 4;
    if (tray_temporal_motion_step_async(scene, &cam[0], NULL, NULL, 3, &tp, frame, NULL, &out, NULL, motion, &rec,
                                        NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 5; /* null planes */
    out.colour = colour;
    out.age = age;
    out.index = index;
    out.depth = depth;
    if (tray_temporal_motion_step_async(scene, &cam[0], NULL, NULL, 3, &tp, frame, NULL, &out, variance, motion, &rec,
                                        NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 6; /* a variance without m2 */
    hist = out;
    hist.colour = colour2;
    hist.m2 = m22;
    hist.age = age2;
    hist.index = index2;
    hist.depth = depth2;
    if (tray_temporal_motion_step_async(scene, &cam[1], &cam[0], geometry, 3, &tp, frame, &hist, &out, NULL, motion,
                                        &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 7; /* m2 partly given */
    out.m2 = m2;
    if (tray_temporal_motion_step_async(scene, &cam[1], &cam[0], NULL, 3, &tp, frame, &hist, &out, variance, motion,
                                        &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 8; /* a history without the previous geometry */
    if (tray_temporal_motion_step_async(scene, &cam[1], &cam[0], geometry, 3, &tp, frame, &hist, &out, variance,
                                        colour2, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 9; /* the motion plane overlaps history.colour */
    tp.max_history = 0;
    if (tray_temporal_motion_step_async(scene, &cam[1], &cam[0], geometry, 3, &tp, frame, &hist, &out, variance,
                                        motion, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 10;
    tp.max_history = 8;
    out.height = hist.height = 0; /* an empty image: TRAY_OK, nothing launched */
    if (tray_temporal_motion_step_async(scene, &cam[1], &cam[0], geometry, 3, &tp, frame, &hist, &out, variance,
                                        motion, &rec, NULL) != TRAY_OK)
        return 11;
    if (tray_temporal_motion_frame(NULL, cam, 1, 1, geometry, 3, NULL, &tp, frame, &out, variance, motion, NULL, &rec,
                                   NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 12;
    return 0;
}
