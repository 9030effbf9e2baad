/* include/tray_query.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md). Compiled with -std=c99 -Wall -Werror -fsyntax-only by
 * tests/test_query_abi_cpu.py; never run. */
#include <stddef.h>

#include "tray_query.h"

typedef char tray_ray_is_48_bytes[sizeof(tray_ray) == 48 ? 1 : -1];
typedef char tray_hit_is_64_bytes[sizeof(tray_hit) == 64 ? 1 : -1];
typedef char tray_hit_index_offset[offsetof(tray_hit, index) == 56 ? 1 : -1];

int tray_query_caller(tray_scene_t scene, const tray_camera *camera, const tray_params *params, tray_ray *rays,
                      uint32_t *ids, tray_hit *hits, double *rgb, uint32_t *segments, void *stream) {
    const int64_t n = (int64_t)tray_params_rows(params) * params->width * params->rays_per_pixel;
    int rc;
    if (tray_query_version() != TRAY_QUERY_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_camera_rays_async(camera, params, 0, rays, ids, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_scene_hit_async(scene, rays, n, 1e30, TRAY_FLAG_LINEAR_SCAN, hits, stream);
    if (rc != TRAY_OK) return rc;
    return tray_ray_color_async(scene, rays, ids, n, params->max_depth, params->seed, 0, rgb, segments, stream);
}
