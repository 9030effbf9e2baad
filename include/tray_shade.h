/*
 * tray_shade.h — the remaining per-ray steps of the render loop as batched
 * queries, beside tray_query.h (Camera.GetRay, Scene.Hit, Scene.RayColor):
 *     Material.Scatter(r, rec)      (ray/materials.go:13-64)
 *     AmbientLight.Hit(r)           (ray/objects.go:68-73)
 * and an occlusion query (is any root in (1e-6, t_end)?). With them a caller
 * runs GetRay -> loop { Hit -> Scatter | sky } as a wavefront on the device,
 * gets Scene.RayColor's bits, and may put per-bounce outputs, termination rules,
 * shadow rays or another light between the steps.
 *
 * An addition beside tray.h (ABI 6) and tray_query.h (version 1), both
 * unchanged, under the same rules: plain C99, caller-owned DEVICE buffers,
 * tray_status / tray_last_error, the arithmetic and counter-RNG contract of
 * tray.h. All three entry points only enqueue on `stream` (a hipStream_t, or
 * NULL for the device's null stream). Arguments are validated before any device
 * work. They use no launch context and no per-launch global workspace, so they
 * are safe from any thread and on any stream, beside each other, beside the
 * queries of tray_query.h and beside renders of the same scene.
 * tray_scene_release does not wait for enqueued queries: the caller
 * synchronises their streams first.
 */
#ifndef TRAY_SHADE_H
#define TRAY_SHADE_H

#include "tray_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_SHADE_VERSION 1

int32_t tray_shade_version(void);

/* Result of Material.Scatter: 80 bytes. */
typedef struct tray_scatter {
    double attenuation[3]; /* Lambertian/Metal albedo; (1,1,1) for Dielectric */
    tray_ray ray;          /* the scattered ray: origin = rec.point */
    int32_t scattered;     /* 1: didScatter; 0: absorbed (Metal) or no hit -> every other field zero */
    int32_t reserved;      /* 0 */
} tray_scatter;

/* hits[i].Mat.Scatter(&rays[i], &hits[i]) for n rays. Point, normal, front_face
 * and index are READ FROM THE RECORD, as the Go method reads rec: they are not
 * recomputed from the sphere, so a record the caller changed is honoured. The
 * material is that of sphere `index` in the uploaded list order; an index < 0 or
 * >= the scene's sphere count gives scattered = 0 with every other field zero
 * and reads no sphere. The draws of ray i come from the draw block (pixel =
 * ids[2i], sample = ids[2i + 1], bounce, purpose 3) under the draw key of `seed`
 * (tray.h); with ids_device NULL, pixel = i and sample = 0, as
 * tray_ray_color_async. The arithmetic is the renderer's scatter step
 * (expressions and order), so fed the records of tray_scene_hit_async the
 * results have the bits of the renderer's bounce. A Metal ray with
 * Dot(scattered.Direction, rec.Normal) <= 0 is absorbed: scattered = 0, every
 * other field zero. */
int tray_scatter_async(tray_scene_t scene, const tray_ray *rays_device, const tray_hit *hits_device,
                       const uint32_t *ids_device /* nullable */, int64_t n, uint32_t bounce, uint64_t seed,
                       tray_scatter *out_device, void *stream);

/* AmbientLight.Hit(r) for n rays: rgb_device receives 3 doubles per ray,
 * Add(SMul(ColorA, 1-a), SMul(ColorB, a)) with a = 0.5 * (Unit(dir).y + 1). It
 * needs no scene, like the Go value method; `device` selects where it runs, as
 * for tray_camera_rays_async. A zero direction gives NaN, as in Go. */
int tray_background_hit_async(const tray_background *background, const tray_ray *rays_device, int64_t n,
                              double *rgb_device, int32_t device, void *stream);

/* occluded[i] = 1 iff some sphere has a root in (1e-6, end_i), else 0: by
 * definition what tray_scene_hit_async(..., end_i, flags, ...) reports as
 * index >= 0, at one byte per ray and with a traversal that stops at the first
 * accepted root. end_i = t_end_device[i] when the array is given, else the
 * scalar t_end. The interval is open (Interval.Surrounds): a root equal to
 * end_i does not occlude. A per-ray end that is NaN or <= 1e-6 is an empty
 * interval and gives 0; a NaN scalar t_end is refused. flags and the per-ray
 * choice between the BVH and the linear scan are tray_scene_hit_async's. */
int tray_scene_occluded_async(tray_scene_t scene, const tray_ray *rays_device,
                              const double *t_end_device /* nullable: per ray */, int64_t n, double t_end,
                              int32_t flags, uint8_t *occluded_device, void *stream);

/* Errors of all three: TRAY_ERR_INVALID_ARGUMENT for a null scene or
 * background, a null ray, hit or result buffer (with n > 0), n < 0, unknown
 * flags or a NaN scalar t_end; TRAY_ERR_TOO_LARGE for n > 2^31 - 1;
 * TRAY_ERR_NO_DEVICE when `device` is not a gfx950. n == 0 is TRAY_OK and
 * launches nothing. */

#ifdef __cplusplus
}
#endif

#endif /* TRAY_SHADE_H */
