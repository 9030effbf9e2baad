/* include/tray_progressive.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): a batch of progressive passes is folded into the running mean on the
 * stream that rendered it, with the convergence record, and the mean goes through the
 * variance-guided filter. Compiled with -std=c99 -Wall -Werror by
 * tests/test_progressive_abi_cpu.py and linked against the library; run only without a
 * device (argument errors). */
#include <stddef.h>

#include "tray_aov.h"
#include "tray_progressive.h"

typedef char tray_accum_is_32_bytes[sizeof(tray_accum) == 2 * sizeof(void *) + 16 ? 1 : -1];
typedef char tray_accum_metric_is_16_bytes[sizeof(tray_accum_metric) == 16 ? 1 : -1];
typedef char tray_accum_metric_max_at_8[offsetof(tray_accum_metric, max_ratio) == 8 ? 1 : -1];
typedef char tray_accum_metric_params_is_16_bytes[sizeof(tray_accum_metric_params) == 16 ? 1 : -1];
typedef char tray_denoise_variance_params_is_48_bytes[sizeof(tray_denoise_variance_params) == 48 ? 1 : -1];
typedef char tray_denoise_variance_params_epsilon_at_40[offsetof(tray_denoise_variance_params, epsilon) == 40 ? 1 : -1];

int tray_progressive_caller(tray_scene_t scene, const tray_camera *camera, const tray_params *params,
                            int32_t n_passes, double *frames, tray_accum *acc, double *variance,
                            tray_accum_metric *record, const tray_denoise_guides *guides, double *out,
                            void *workspace, size_t workspace_bytes, int32_t device, void *stream) {
    tray_accum_metric_params mp;
    tray_denoise_variance_params dp;
    size_t need = 0;
    int rc;
    if (tray_progressive_version() != TRAY_PROGRESSIVE_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_render_passes_async(scene, camera, params, n_passes, frames, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_accum_metric_default_params(&mp);
    if (rc != TRAY_OK) return rc;
    rc = tray_accum_fold_metric_async(acc, frames, n_passes, &mp, variance, record, device, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_denoise_variance_default_params(acc->width, acc->rows, &dp);
    if (rc != TRAY_OK) return rc;
    rc = tray_denoise_variance_workspace_bytes(&dp, &need);
    if (rc != TRAY_OK) return rc;
    if (need > workspace_bytes) return TRAY_ERR_INVALID_ARGUMENT;
    return tray_denoise_variance_async(acc->mean, variance, guides, &dp, out, NULL, workspace, workspace_bytes,
                                       device, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_accum_metric_params mp;
    tray_denoise_variance_params dp;
    tray_denoise_guides none = {NULL, NULL, NULL};
    tray_accum acc = {NULL, NULL, 4, 4, 0, 0};
    size_t need = 0;
    double a[3], b[3], c[3];
    if (tray_progressive_version() != TRAY_PROGRESSIVE_VERSION) return 1;
    if (tray_accum_metric_default_params(&mp) != TRAY_OK || !(mp.tolerance > 0) || !(mp.floor > 0)) return 2;
    if (tray_accum_fold_async(&acc, a, 1, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 3; /* null mean */
    if (!tray_last_error() || !tray_last_error()[0]) return 4;
    if (tray_accum_fold_async(&acc, NULL, 0, 0, NULL) != TRAY_OK || acc.count != 0) return 5; /* nothing to fold */
    acc.mean = a;
    acc.m2 = a;
    acc.width = acc.rows = 1;
    if (tray_accum_fold_metric_async(&acc, b, 1, &mp, NULL, NULL, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 6;
    if (tray_denoise_variance_default_params(1280, 720, &dp) != TRAY_OK) return 7;
    if (dp.iterations != 5 || dp.flags != TRAY_DENOISE_DEMODULATE || !(dp.sigma_variance > 0) || !(dp.epsilon > 0))
        return 8;
    if (tray_denoise_variance_workspace_bytes(&dp, &need) != TRAY_OK ||
        need != (size_t)2 * 1280 * 720 * 4 * sizeof(double))
        return 9;
    dp.width = dp.rows = 1;
    dp.iterations = 1;
    if (tray_denoise_variance_async(a, NULL, &none, &dp, c, NULL, NULL, 0, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 10; /* null variance */
    if (tray_denoise_variance_async(a, b, &none, &dp, c, NULL, NULL, 0, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 11; /* demodulation without an albedo */
    dp.rows = 0; /* an empty image: TRAY_OK, nothing launched */
    dp.flags = 0;
    if (tray_denoise_variance_async(a, b, &none, &dp, c, NULL, NULL, 0, 0, NULL) != TRAY_OK) return 12;
    if (tray_progressive_caller(NULL, NULL, NULL, 1, NULL, &acc, NULL, NULL, &none, NULL, NULL, 0, 0, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 13;
    return 0;
}
