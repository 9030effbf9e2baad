/* include/tray_temporal_variance.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): an interactive loop that renders each new frame, folds it into the reprojected
 * history with its M2, and gives the fresh pixels more samples (section 4 of the header), over two
 * ping-pong states. Compiled with -std=c99 -Wall -Werror -pedantic by
 * tests/test_temporal_variance_abi_cpu.py and linked against the library; run only without a device
 * (argument errors). */
#include <stddef.h>

#include "tray_adaptive.h"
#include "tray_temporal_variance.h"

typedef char tray_temporal_var_state_size[sizeof(tray_temporal_var_state) == 5 * sizeof(void *) + 8 ? 1 : -1];
typedef char tray_temporal_var_state_m2_second[offsetof(tray_temporal_var_state, m2) == sizeof(void *) ? 1 : -1];
typedef char tray_temporal_var_state_width_after_depth[offsetof(tray_temporal_var_state, width) ==
                                                               5 * sizeof(void *)
                                                           ? 1
                                                           : -1];

/* The selection's list length, read back by the caller between the two halves of a frame. */
typedef int (*read_record_fn)(const tray_adaptive_record *device, tray_adaptive_record *host, void *stream);

/* Frame k of a moving camera with a refill of R passes: the render (pass k (1 + R)), the step from
 * states[(k - 1) & 1] into states[k & 1], and the chain on that state as a tray_adaptive_state. */
int tray_temporal_var_frame(tray_scene_t scene, const tray_camera *cameras, int32_t k, int32_t refill,
                            tray_params *params, const tray_temporal_params *tp, double *frame,
                            const tray_temporal_var_state *states, double *variance, tray_temporal_record *record,
                            uint32_t *list, tray_adaptive_record *select_record, void *workspace,
                            size_t workspace_bytes, double *values, read_record_fn read_record, int32_t device,
                            void *stream) {
    const tray_temporal_var_state *out = &states[k & 1];
    tray_adaptive_state as;
    tray_adaptive_params ap;
    tray_adaptive_record host;
    int rc;
    if (tray_temporal_var_version() != TRAY_TEMPORAL_VAR_VERSION) return TRAY_ERR_UNSUPPORTED;
    if (!params || !tp) return TRAY_ERR_INVALID_ARGUMENT;
    params->pass = k * (1 + refill);
    rc = tray_render_async(scene, &cameras[k], params, frame, NULL, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_temporal_var_step_async(scene, &cameras[k], k ? &cameras[k - 1] : NULL, tp, frame,
                                      k ? &states[(k - 1) & 1] : NULL, out, variance, record, stream);
    if (rc != TRAY_OK || refill == 0) return rc;
    as.mean = out->colour;
    as.m2 = out->m2;
    as.count = out->age;
    as.width = out->width;
    as.rows = out->height;
    rc = tray_adaptive_default_params(&ap);
    if (rc != TRAY_OK) return rc;
    ap.tolerance = 1e150; /* only the count decides */
    ap.min_passes = 1 + refill;
    ap.max_passes = tp->max_history;
    rc = tray_adaptive_select_async(&as, &ap, NULL, list, select_record, workspace, workspace_bytes, device, stream);
    if (rc != TRAY_OK) return rc;
    rc = read_record(select_record, &host, stream);
    if (rc != TRAY_OK || host.n_active == 0) return rc;
    params->pass = k * (1 + refill) + 1;
    rc = tray_render_pixels_async(scene, &cameras[k], params, list, (int64_t)host.n_active, NULL, refill, values, NULL,
                                  stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_adaptive_fold_async(&as, list, (int64_t)host.n_active, values, refill, device, stream);
    if (rc != TRAY_OK) return rc;
    return tray_temporal_var_variance_async(out, list, (int64_t)host.n_active, variance, device, stream);
}

int main(void) {
    /* Argument errors come back before any device work: nothing here needs a device. */
    tray_temporal_params tp;
    tray_temporal_var_state out = {NULL, NULL, NULL, NULL, NULL, 4, 4}, hist;
    tray_temporal_record rec;
    tray_camera cam[2] = {{{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}, {{0}, {0}, {0}, {0}, {0}, {0}, 0, 0, 0}};
    double frame[48], colour[48], m2[48], depth[16], colour2[48], m22[48], depth2[16], variance[48];
    int32_t age[16], index[16], age2[16], index2[16];
    uint32_t list[16];
    int fake;
    tray_scene_t scene = (tray_scene_t)&fake; /* never looked at: validation fails first */
    if (tray_temporal_var_version() != TRAY_TEMPORAL_VAR_VERSION || tray_temporal_version() != 1) return 1;
    if (tray_temporal_default_params(&tp) != TRAY_OK) return 2;
    if (tray_temporal_var_step_async(NULL, &cam[0], NULL, &tp, frame, NULL, &out, variance, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 3; /* null scene */
    if (!tray_last_error() || !tray_last_error()[0]) return 4;
    if (tray_temporal_var_step_async(scene, &cam[0], NULL, &tp, frame, NULL, &out, variance, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 5; /* null planes */
    out.colour = colour;
    out.m2 = m2;
    out.age = age;
    out.index = index;
    out.depth = depth;
    hist = out;
    if (tray_temporal_var_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, NULL, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 6; /* out overlaps history */
    hist.colour = colour2;
    hist.m2 = m22;
    hist.age = age2;
    hist.index = index2;
    hist.depth = depth2;
    if (tray_temporal_var_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, m22, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 7; /* the variance overlaps history.m2 */
    tp.max_history = 0;
    if (tray_temporal_var_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, variance, &rec, NULL) !=
        TRAY_ERR_INVALID_ARGUMENT)
        return 8;
    tp.max_history = 8;
    if (tray_temporal_var_variance_async(NULL, list, 4, variance, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 9;
    if (tray_temporal_var_variance_async(&out, list, -1, variance, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT) return 10;
    if (tray_temporal_var_variance_async(&out, list, 4, m2, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 11; /* the variance overlaps m2 */
    if (tray_temporal_var_variance_async(&out, list, 0, variance, 0, NULL) != TRAY_OK) return 12; /* an empty list */
    out.height = hist.height = 0; /* an empty image: TRAY_OK, nothing launched */
    if (tray_temporal_var_step_async(scene, &cam[1], &cam[0], &tp, frame, &hist, &out, variance, &rec, NULL) != TRAY_OK)
        return 13;
    if (tray_temporal_var_variance_async(&out, NULL, 0, variance, 0, NULL) != TRAY_OK) return 14;
    if (tray_temporal_var_frame(NULL, cam, 1, 3, NULL, &tp, frame, &out, variance, &rec, list, NULL, NULL, 0, NULL,
                                NULL, 0, NULL) != TRAY_ERR_INVALID_ARGUMENT)
        return 15;
    return 0;
}
