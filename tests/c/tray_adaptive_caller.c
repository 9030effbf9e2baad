/* include/tray_adaptive.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): one round of adaptive sampling on a stream. The selection step lists the
 * pixels that have not converged, the caller reads the 32-byte record back, the list is
 * rendered for `batch` more passes numbered from each pixel's own count, and the values are
 * folded into the state. Compiled with -std=c99 -Wall -Werror -pedantic by
 * tests/test_adaptive_abi_cpu.py and linked against the library; run only without a device
 * (argument errors). */
#include <stddef.h>

#include "tray_adaptive.h"

typedef char tray_adaptive_state_size[sizeof(tray_adaptive_state) == 3 * sizeof(void *) + 8 ? 1 : -1];
typedef char tray_adaptive_params_is_32_bytes[sizeof(tray_adaptive_params) == 32 ? 1 : -1];
typedef char tray_adaptive_params_dilate_at_24[offsetof(tray_adaptive_params, dilate) == 24 ? 1 : -1];
typedef char tray_adaptive_record_is_32_bytes[sizeof(tray_adaptive_record) == 32 ? 1 : -1];
typedef char tray_adaptive_record_passes_at_24[offsetof(tray_adaptive_record, pixel_passes) == 24 ? 1 : -1];

/* Select: the caller synchronises `stream` and reads record->n_active between the two halves. */
int tray_adaptive_round_select(const tray_adaptive_state *state, const tray_adaptive_params *ap, double *variance,
                               uint32_t *list, tray_adaptive_record *record, void *workspace,
                               size_t workspace_bytes, int32_t device, void *stream) {
    size_t need = 0;
    int rc;
    if (tray_adaptive_version() != TRAY_ADAPTIVE_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_adaptive_workspace_bytes(state->width, state->rows, &need);
    if (rc != TRAY_OK) return rc;
    if (need > workspace_bytes) return TRAY_ERR_INVALID_ARGUMENT;
    return tray_adaptive_select_async(state, ap, variance, list, record, workspace, workspace_bytes, device, stream);
}

int tray_adaptive_round_render(tray_scene_t scene, const tray_camera *camera, const tray_params *params,
                               const tray_adaptive_state *state, const uint32_t *list, int64_t n_active,
                               int32_t batch, double *values, int32_t device, void *stream) {
    int rc = tray_render_pixels_async(scene, camera, params, list, n_active, state->count, batch, values, NULL, stream);
    if (rc != TRAY_OK) return rc;
    return tray_adaptive_fold_async(state, list, n_active, values, batch, device, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_adaptive_params ap;
    tray_adaptive_state st = {NULL, NULL, NULL, 4, 4};
    tray_adaptive_record rec;
    uint32_t list[16];
    double a[48], b[48], values[48];
    int32_t count[16];
    size_t need = 0;
    if (tray_adaptive_version() != TRAY_ADAPTIVE_VERSION) return 1;
    if (tray_adaptive_default_params(&ap) != TRAY_OK || !(ap.tolerance > 0) || !(ap.floor > 0) || ap.dilate != 1 ||
        ap.max_passes != 64 || ap.min_passes < 1 || ap.min_passes > ap.max_passes || ap.reserved != 0)
        return 2;
    if (tray_adaptive_default_params(NULL) != TRAY_ERR_INVALID_ARGUMENT) return 3;
    if (tray_adaptive_workspace_bytes(1280, 720, &need) != TRAY_OK || need != (size_t)1280 * 720 + 900 * 4) return 4;
    if (tray_adaptive_fold_async(&st, list, 1, values, 1, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 5; /* null mean */
    if (!tray_last_error() || !tray_last_error()[0]) return 6;
    if (tray_adaptive_fold_async(&st, list, 0, values, 1, 0, NULL) != TRAY_OK) return 7; /* an empty list */
    st.mean = a;
    st.m2 = b;
    st.count = count;
    if (tray_adaptive_fold_async(&st, list, 1, values, 0, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 8;
    if (tray_adaptive_fold_async(&st, list, 1, a, 1, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 9; /* overlap */
    ap.dilate = 2;
    if (tray_adaptive_round_select(&st, &ap, NULL, list, &rec, values, sizeof values, 0, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 10;
    ap.dilate = 1;
    if (tray_adaptive_round_select(&st, &ap, NULL, list, &rec, values, 8, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 11; /* the workspace is too small */
    st.rows = 0; /* an empty image: TRAY_OK, nothing launched */
    if (tray_adaptive_round_select(&st, &ap, NULL, list, &rec, NULL, 0, 0, NULL) != TRAY_OK) return 12;
    if (tray_adaptive_round_render(NULL, NULL, NULL, &st, list, 1, 4, values, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 13; /* null scene */
    return 0;
}
