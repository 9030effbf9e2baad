/*
 * tray_query.h — batched ray queries on an uploaded scene: the steps of the
 * render loop that the Go package exports on their own,
 *     Camera.GetRay                 (ray/camera.go:113)
 *     Scene.Hit(r, interval, hr)    (ray/objects.go:37)
 *     Scene.RayColor(r, depth)      (ray/objects.go:49)
 * for other camera models, picking, visibility and occlusion tests and callers'
 * own integrators. An addition beside tray.h (whose ABI 6 surface is unchanged):
 * same rules (plain C99, caller-owned buffers, tray_status / tray_last_error)
 * and the same arithmetic and counter-RNG contract, so every value below has
 * the bits the renderer computes for the same ray.
 *
 * All three entry points only enqueue on `stream` (a hipStream_t, or NULL for
 * the device's null stream); every buffer is DEVICE memory of the scene's (or
 * `device`'s) device. Arguments are validated before any device work. They use
 * no launch context and no per-launch global workspace, so they are safe from
 * any thread and on any stream, beside each other and beside renders of the
 * same scene. tray_scene_release does not wait for enqueued queries: the
 * caller synchronises their streams first.
 */
#ifndef TRAY_QUERY_H
#define TRAY_QUERY_H

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_QUERY_VERSION 1

/* ray.Ray (ray/ray.go): 48 bytes. */
typedef struct tray_ray {
    double origin[3];
    double direction[3];
} tray_ray;

/* ray.HitRecord (ray/objects.go:11-17) plus which sphere was hit: 64 bytes. */
typedef struct tray_hit {
    double point[3];
    double normal[3];
    double t;
    int32_t index;      /* position in the uploaded sphere list, -1: no hit */
    int32_t front_face; /* 1: the ray came from outside (SetFaceNormal, ray/objects.go:19-26) */
} tray_hit;

int32_t tray_query_version(void);

/* Camera.GetRay (ray/camera.go:113-142) for every sample of params' row set:
 * the rays Tracer.RenderLines (ray/tracer.go:130-141) would trace for pass
 * params->pass. Ray i = (j * width + x) * rays_per_pixel + s, with j the
 * COMPACT row as in tray_params; rays_device holds rows x width x
 * rays_per_pixel rays (rows = tray_params_rows(params)), at most 2^31 - 1
 * (TRAY_ERR_TOO_LARGE). ids_device (nullable) receives two words per ray, the
 * draw-block coordinates of the sample: ids[2i] = y * width + x in GLOBAL image
 * coordinates, ids[2i + 1] = pass * rays_per_pixel + s. Each ray is drawn from
 * the sample's camera block (tray.h, purpose 1) exactly as the renderer draws
 * it: no anti-aliasing disc when rays_per_pixel == 1, the lens disc only when
 * the aperture is open. Of params, max_depth, output and flags are validated
 * and otherwise unused. */
int tray_camera_rays_async(const tray_camera *camera, const tray_params *params, int32_t device,
                           tray_ray *rays_device, uint32_t *ids_device, void *stream);

/* Scene.Hit(r, Interval{1e-6, t_end}, hr) (ray/objects.go:37-46) for n rays.
 * The interval start is FrontEpsilon.Start = 1e-6 (ray/vec3.go:218), hard-wired
 * in the closest-hit arithmetic like in the renderer; t_end is Interval.End,
 * strict as Interval.Surrounds is (a root equal to t_end is no hit); +inf gives
 * RayColor's interval. A hit is Sphere.Hit's record (ray/objects.go:98-102) in
 * its operation order, with `index` the hit sphere's position in the uploaded
 * list (of equal roots, the earlier sphere, as the reference's scan keeps it);
 * a miss has index -1 and every other field zero.
 * flags: 0 or TRAY_FLAG_LINEAR_SCAN (the reference-order scan over all spheres,
 * for verification and A/B timing). Both give identical results. Without the
 * flag a ray takes the exact-culling BVH when the scene has one
 * (tray_scene_info.has_bvh), its origin lies in [-M, M]^3 (M =
 * tray_scene_info.bound) and its squared direction length lies in
 * [1e-30, 1e30]; any other ray (NaN and infinite components included) takes
 * the linear scan inside the same launch. The traversal stacks live on chip
 * (1 KB per entry of tray_scene_info.stack_depth + 3 and workgroup); a scene
 * whose stacks exceed 64 KB takes the linear scan for every query ray. */
int tray_scene_hit_async(tray_scene_t scene, const tray_ray *rays_device, int64_t n, double t_end, int32_t flags,
                         tray_hit *hits_device, void *stream);

/* Scene.RayColor(r, max_depth) (ray/objects.go:49-62) for n rays: rgb_device
 * receives 3 doubles per ray, segments_device (nullable) the path's count of
 * Scene.Hit calls. The scatter draws of ray i come from the draw blocks
 * (pixel = ids[2i], sample = ids[2i + 1], bounce, purpose 3) under the draw key
 * of `seed` (tray.h); with ids_device NULL, pixel = i and sample = 0. Fed the
 * rays and ids of tray_camera_rays_async, ray i's colour has the bits of the
 * renderer's sample i. Attenuations are multiplied outer-first like the
 * renderer's. flags as for tray_scene_hit_async. */
int tray_ray_color_async(tray_scene_t scene, const tray_ray *rays_device, const uint32_t *ids_device, int64_t n,
                         int32_t max_depth, uint64_t seed, int32_t flags, double *rgb_device,
                         uint32_t *segments_device, void *stream);

/* Errors of all three: TRAY_ERR_INVALID_ARGUMENT for a null scene, camera,
 * params, ray or result buffer (with n > 0), n < 0, max_depth <= 0, unknown
 * flags or a NaN t_end; TRAY_ERR_TOO_LARGE for n > 2^31 - 1. n == 0 is TRAY_OK
 * and launches nothing. */

#ifdef __cplusplus
}
#endif

#endif /* TRAY_QUERY_H */
