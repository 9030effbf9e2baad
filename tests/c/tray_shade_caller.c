/* include/tray_shade.h from C99: every declaration used the way a cgo shim would
 * (INTEGRATION.md): one bounce of a caller's own integrator. Compiled with
 * -std=c99 -Wall -Werror -fsyntax-only by tests/test_shade_abi_cpu.py; never run. */
#include <stddef.h>

#include "tray_shade.h"

typedef char tray_scatter_is_80_bytes[sizeof(tray_scatter) == 80 ? 1 : -1];
typedef char tray_scatter_ray_offset[offsetof(tray_scatter, ray) == 24 ? 1 : -1];
typedef char tray_scatter_scattered_offset[offsetof(tray_scatter, scattered) == 72 ? 1 : -1];

int tray_shade_caller(tray_scene_t scene, const tray_background *sky, const tray_ray *rays, const uint32_t *ids,
                      int64_t n, uint32_t bounce, uint64_t seed, tray_hit *hits, tray_scatter *scattered,
                      double *sky_rgb, const double *shadow_ends, uint8_t *occluded, void *stream) {
    int rc;
    if (tray_shade_version() != TRAY_SHADE_VERSION) return TRAY_ERR_UNSUPPORTED;
    rc = tray_scene_hit_async(scene, rays, n, 1e30, 0, hits, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_scatter_async(scene, rays, hits, ids, n, bounce, seed, scattered, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_background_hit_async(sky, rays, n, sky_rgb, 0, stream);
    if (rc != TRAY_OK) return rc;
    rc = tray_scene_occluded_async(scene, rays, shadow_ends, n, 0.0, 0, occluded, stream);
    if (rc != TRAY_OK) return rc;
    return tray_scene_occluded_async(scene, rays, NULL, n, 1e30, TRAY_FLAG_LINEAR_SCAN, occluded, stream);
}
