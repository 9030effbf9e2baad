/* include/tray_temporal.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): an interactive loop that renders each new frame and folds it into the
 * reprojected history, over two ping-pong states. Compiled with -std=c99 -Wall -Werror -pedantic
 * by tests/test_temporal_abi_cpu.py and linked against the library; run only without a device
 * (argument errors). */
#include <stddef.h>

#include "tray_temporal.h"

typedef char tray_temporal_state_size[sizeof(tray_temporal_state) == 4 * sizeof(void *) + 8 ? 1 : -1];
typedef char tray_temporal_params_is_32_bytes[sizeof(tray_temporal_params) == 32 ? 1 : -1];
typedef char tray_temporal_params_snap_at_16[offsetof(tray_temporal_params, snap) == 16 ? 1 : -1];
typedef char tray_temporal_record_is_16_bytes[sizeof(tray_temporal_record) == 16 ? 1 : -1];
typedef char tray_temporal_record_age_sum_at_8[offsetof(tray_temporal_record, age_sum) == 8 ? 1 : -1];

/* Frame k of a moving camera: the render, then the step from states[(k - 1) & 1] into states[k & 1]. */
int tray_temporal_frame(tray_scene_t scene, const tray_camera *cameras, int32_t k, const tray_params *params,
                        const tray_temporal_params *tp, double *frame, const tray_temporal_state *states,
                        tray_temporal_record *record, void *stream) {
    int rc;
    if (tray_temporal_version() != TRAY_TEMPORAL_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_render_async(scene, &cameras[k], params, frame, NULL, stream);
    if (rc != TRAY_OK) return rc;
    return tray_temporal_step_async(scene, &cameras[k], k ? &cameras[k - 1] : NULL, tp, frame,
                                    k ? &states[(k - 1) & 1] : NULL, &states[k & 1], record, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_temporal_params tp;
    tray_temporal_state out = {NULL, NULL, NULL, NULL, 4, 4}, hist;
    tray_temporal_record rec;
    tray_camera cam[2] = {{{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}, {{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}};
    double frame[48], colour[48], depth[16], colour2[48], depth2[16];
    int32_t age[16], index[16], age2[16], index2[16];
    int fake;
    tray_scene_t scene = (tray_scene_t)&fake; /* never looked at: validation fails first */
    if (tray_temporal_version() != TRAY_TEMPORAL_VERSION) return 1;
    if (tray_temporal_default_params(&tp) != TRAY_OK || tp.max_history < 1 || !(tp.depth_tolerance >= 0) ||
        !(tp.snap >= 0 && tp.snap < 0.5) || tp.flags != 0 || tp.reserved != 0)
        return 2;
    if (tray_temporal_default_params(NULL) != TRAY_ERR_INVALID_ARGUMENT) return 3;
    if (tray_temporal_step_async(NULL, &cam[0], NULL, &tp, frame, NULL, &out, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 4; /* null scene */
    if (!tray_last_error() || !tray_last_error()[0]) return 5;
    if (tray_temporal_step_async(scene, &cam[0], NULL, &tp, frame, NULL, &out, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 6; /* null planes */
    out.colour = colour;
    out.age = age;
    out.index = index;
    out.depth = depth;
    hist = out;
    if (tray_temporal_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 7; /* out overlaps history */
    if (tray_temporal_step_async(scene, &cam[1], &cam[0], &tp, colour, NULL, &out, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 8; /* a previous camera without a history */
    hist.colour = colour2;
    hist.age = age2;
    hist.index = index2;
    hist.depth = depth2;
    tp.snap = 0.5;
    if (tray_temporal_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 9;
    tp.snap = 0.0;
    tp.max_history = 0;
    if (tray_temporal_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 10;
    tp.max_history = 8;
    out.height = hist.height = 0; /* an empty image: TRAY_OK, nothing launched */
    if (tray_temporal_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, &rec, NULL) != TRAY_OK) return 11;
    if (tray_temporal_frame(NULL, cam, 1, NULL, &tp, frame, &out, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 12; /* null scene (tray_render_async) */
    return 0;
}
