/* include/tray_scene_update.h from C99, the way a cgo shim would use it: an
 * animation loop that moves the spheres of one uploaded scene per frame and renders it, on one stream.
 * Compiled with -std=c99 -Wall -Werror -pedantic by tests/test_scene_update_abi_cpu.py and linked
 * against the library; run only without a device (argument errors). */
#include <stddef.h>

#include "tray_scene_update.h"

typedef char tray_scene_update_record_size[sizeof(tray_scene_update_record) == 32 ? 1 : -1];
typedef char tray_scene_update_record_extent[offsetof(tray_scene_update_record, extent) == 16 ? 1 : -1];
typedef char tray_scene_update_record_bound[offsetof(tray_scene_update_record, bound) == 24 ? 1 : -1];

/* Frame k: the spheres at geometry (device memory, n x 4 doubles), then the render, both enqueued. */
int tray_scene_update_frame(tray_scene_t scene, const double *geometry, int32_t n, tray_scene_update_record *record,
                            const tray_camera *camera, tray_params *params, int32_t k, double *frame, void *stream) {
    int rc;
    if (!params) return TRAY_ERR_INVALID_ARGUMENT;
    rc = tray_scene_update_async(scene, geometry, n, record, stream);
    if (rc != TRAY_OK) return rc;
    params->pass = k;
    return tray_render_async(scene, camera, params, frame, NULL, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    double geometry[8] = {0, 0, 0, 1, 2, 0, 0, 1};
    tray_scene_update_record rec;
    int fake;
    tray_scene_t scene = (tray_scene_t)&fake; /* never looked at: validation fails first */
    if (tray_scene_update_async(NULL, geometry, 2, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 1;
    if (!tray_last_error() || !tray_last_error()[0]) return 2;
    if (tray_scene_update_async(scene, NULL, 2, &rec, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 3;
    if (tray_scene_update_async(scene, geometry, 2, NULL, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 4;
    if (tray_scene_update(NULL, geometry, 2, &rec) != TRAY_ERR_INVALID_ARGUMENT) return 5;
    if (tray_scene_update(scene, NULL, 2, &rec) != TRAY_ERR_INVALID_ARGUMENT) return 6;
    if (tray_scene_update(scene, geometry, 2, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 7;
    if (tray_scene_update_frame(NULL, geometry, 2, &rec, NULL, NULL, 0, NULL, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 8;
    return 0;
}
