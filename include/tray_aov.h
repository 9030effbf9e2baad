/*
 * tray_aov.h — per-pixel first-hit feature buffers of a frame: albedo and
 * shading normal (the guide images a denoiser takes), depth and coverage (for
 * compositing and edge detection) and an object-index image (for picking and
 * masks). One fused launch draws the frame's own camera rays, finds each
 * first hit and reduces per pixel; no per-sample data reaches memory, and the
 * number of samples rows x width x rays_per_pixel is not limited.
 *
 * An addition beside tray.h (ABI 6), tray_query.h (version 1) and tray_shade.h
 * (version 1), all unchanged, under the same rules: plain C99, caller-owned
 * DEVICE buffers, tray_status / tray_last_error, the arithmetic and counter-RNG
 * contract of tray.h. The entry point only enqueues on `stream` (a hipStream_t,
 * or NULL for the device's null stream). Arguments are validated before any
 * device work. It uses no launch context and no per-launch global workspace, so
 * it is safe from any thread and on any stream, beside renders and the queries
 * of tray_query.h and tray_shade.h of the same scene. tray_scene_release does
 * not wait for an enqueued call: the caller synchronises its stream first.
 */
#ifndef TRAY_AOV_H
#define TRAY_AOV_H

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_AOV_VERSION 1

int32_t tray_aov_version(void);

/* DEVICE pointers of the scene's device, each nullable: a null buffer is not
 * written. Rows are COMPACT as in tray_params (rows = tray_params_rows(params)),
 * pitch = width. */
typedef struct tray_aov_buffers {
    double *albedo;   /* rows x width x 3 */
    double *normal;   /* rows x width x 3 */
    double *depth;    /* rows x width */
    double *coverage; /* rows x width */
    int32_t *index;   /* rows x width */
} tray_aov_buffers;

/* For every pixel of params' row set (y_start / y_end with the interleaved
 * tiles, as tray_render_async reads them), with r = rays_per_pixel: samples
 * s = 0 .. r-1 are the rays tray_camera_rays_async (tray_query.h) produces for
 * the same camera and params (draw block (pixel = y * width + x in GLOBAL image
 * coordinates, sample word = pass * r + s, purpose 1); no anti-aliasing disc at
 * r = 1; the lens disc only with an open aperture), and h_s is the record of
 * tray_scene_hit_async for ray s with t_end = +inf, i.e. Scene.Hit(ray_s,
 * {1e-6, +inf}).
 *
 *   albedo    mean of a_s. On a hit a_s is the uploaded albedo of the hit sphere
 *             for Lambertian and Metal and (1,1,1) for Dielectric (the
 *             attenuation Material.Scatter would return; no draw is involved);
 *             on a miss a_s = AmbientLight.Hit(ray_s) (tray_background_hit_async).
 *   normal    mean of h_s.normal, the face normal after SetFaceNormal; a miss
 *             contributes zero. The mean is not renormalised.
 *   depth     the world distance h_s.t * Length(ray_s.Direction), summed over the
 *             hitting samples and divided by their count; 0 where no sample hits.
 *             Length is sqrt((x*x + y*y) + z*z) (ray/vec3.go).
 *   coverage  (number of hitting samples) * (1 / r).
 *   index     h_0.index: the sphere sample 0 hits, in uploaded list order, or -1.
 *             At r = 1 that is the pixel-centre ray.
 *
 * Every mean is formed as Tracer.RenderLines forms colorSum (ray/tracer.go:
 * 132-145): a sequential FP64 sum from zero in sample order, no FMA, then one
 * multiplication by 1.0 / r; depth takes one correctly rounded division by the
 * hit count instead. Every value is therefore a fixed sequence of correctly
 * rounded FP64 operations on values tray_query.h and tray_shade.h define bit for
 * bit, and has exactly the bits of that composition.
 *
 * flags: TRAY_FLAG_LINEAR_SCAN is honoured (same bits; the per-ray choice
 * between the BVH and the scan is tray_scene_hit_async's); TRAY_FLAG_ORDERED_SUM
 * is accepted and has no effect (the sums are always ordered). max_depth and
 * output are validated and otherwise unused. When only `index` is requested,
 * only sample 0 is traced.
 *
 * Errors: TRAY_ERR_INVALID_ARGUMENT for a null scene, camera, params or out,
 * for five null buffers, for unknown flags and for any other field of params
 * tray_render_async refuses as invalid; TRAY_ERR_TOO_LARGE for the limits of
 * the RNG counters (tray.h: width x height <= 2^32, (pass + 1) x r <= 2^32) and
 * for rows x width > 2^31 - 1. An empty row set is TRAY_OK and launches nothing. */
int tray_render_aov_async(tray_scene_t scene, const tray_camera *camera, const tray_params *params,
                          const tray_aov_buffers *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_AOV_H */
