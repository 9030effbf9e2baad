/* include/tray_denoise.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): a frame and its guide images go through the filter on the
 * stream that rendered them. Compiled with -std=c99 -Wall -Werror by
 * tests/test_denoise_abi_cpu.py and linked against the library; run only
 * without a device (argument errors). */
#include <stddef.h>

#include "tray_aov.h"
#include "tray_denoise.h"

typedef char tray_denoise_guides_is_3_pointers[sizeof(tray_denoise_guides) == 3 * sizeof(void *) ? 1 : -1];
typedef char tray_denoise_params_is_40_bytes[sizeof(tray_denoise_params) == 40 ? 1 : -1];
typedef char tray_denoise_params_sigmas_at_16[offsetof(tray_denoise_params, sigma_color) == 16 ? 1 : -1];

int tray_denoise_caller(tray_scene_t scene, const tray_camera *camera, const tray_params *params, double *frame,
                        double *albedo, double *normal, double *depth, double *out, void *workspace,
                        size_t workspace_bytes, int32_t device, void *stream) {
    tray_aov_buffers aov;
    tray_denoise_guides guides;
    tray_denoise_params dp;
    size_t need = 0;
    int rc;
    if (tray_denoise_version() != TRAY_DENOISE_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_render_async(scene, camera, params, frame, NULL, stream);
    if (rc != TRAY_OK) return rc;
    aov.albedo = albedo;
    aov.normal = normal;
    aov.depth = depth;
    aov.coverage = NULL;
    aov.index = NULL;
    rc = tray_render_aov_async(scene, camera, params, &aov, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_denoise_default_params(params->width, tray_params_rows(params), &dp);
    if (rc != TRAY_OK) return rc;
    rc = tray_denoise_workspace_bytes(&dp, &need);
    if (rc != TRAY_OK) return rc;
    if (need > workspace_bytes) return TRAY_ERR_INVALID_ARGUMENT;
    guides.albedo = albedo;
    guides.normal = normal;
    guides.depth = depth;
    return tray_denoise_async(frame, &guides, &dp, out, workspace, workspace_bytes, device, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_denoise_params dp;
    tray_denoise_guides none = {NULL, NULL, NULL};
    size_t need = 0;
    double a[3], b[3];
    if (tray_denoise_version() != TRAY_DENOISE_VERSION) return 1;
    if (tray_denoise_default_params(1280, 720, &dp) != TRAY_OK) return 2;
    if (dp.iterations != 5 || dp.flags != TRAY_DENOISE_DEMODULATE || !(dp.sigma_color > 0)) return 3;
    if (tray_denoise_workspace_bytes(&dp, &need) != TRAY_OK || need != (size_t)2 * 1280 * 720 * 3 * sizeof(double))
        return 4;
    if (tray_denoise_async(NULL, &none, &dp, b, NULL, 0, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 5;
    if (!tray_last_error() || !tray_last_error()[0]) return 6;
    dp.width = dp.rows = 1;
    dp.iterations = 1; /* no workspace; demodulation without an albedo is refused */
    if (tray_denoise_async(a, &none, &dp, b, NULL, 0, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 7;
    dp.rows = 0; /* an empty image: TRAY_OK, nothing launched */
    dp.flags = 0;
    if (tray_denoise_async(a, &none, &dp, b, NULL, 0, 0, NULL) != TRAY_OK) return 8;
    if (tray_denoise_caller(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 9;
    return 0;
}
