/* include/tray_aov.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): the guide images of a frame beside its render. Compiled with
 * -std=c99 -Wall -Werror by tests/test_aov_abi_cpu.py and linked against the
 * library; run only without a scene (argument errors). */
#include <stddef.h>

#include "tray_aov.h"

typedef char tray_aov_buffers_is_5_pointers[sizeof(tray_aov_buffers) == 5 * sizeof(void *) ? 1 : -1];
typedef char tray_aov_buffers_index_last[offsetof(tray_aov_buffers, index) == 4 * sizeof(void *) ? 1 : -1];

int tray_aov_caller(tray_scene_t scene, const tray_camera *camera, const tray_params *params, void *frame,
                    double *albedo, double *normal, double *depth, double *coverage, int32_t *index,
                    void *stream) {
    tray_aov_buffers out;
    int rc;
    if (tray_aov_version() != TRAY_AOV_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_render_async(scene, camera, params, frame, NULL, stream);
    if (rc != TRAY_OK) return rc;
    out.albedo = albedo;
    out.normal = normal;
    out.depth = depth;
    out.coverage = coverage;
    out.index = index;
    return tray_render_aov_async(scene, camera, params, &out, stream);
}

int main(void) {
    /* Argument errors come back before any device work: no scene, so nothing runs. */
    tray_aov_buffers none = {NULL, NULL, NULL, NULL, NULL};
    if (tray_aov_version() != TRAY_AOV_VERSION) return 1;
    if (tray_render_aov_async(NULL, NULL, NULL, &none, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 2;
    if (!tray_last_error() || !tray_last_error()[0]) return 3;
    if (tray_aov_caller(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 4;
    return 0;
}
