// Internal launch interface between the C-ABI glue (tray_abi.hip) and the
// ray-query kernels (tray_query.hip: include/tray_query.h, tray_shade.h and
// tray_aov.h), the pixel-list renderer (tray_adaptive.hip) and the temporal
// step (tray_temporal.hip). Host side only:
// the device functions those units share are tray_query_device.hpp, over
// tray_device.hpp, which the megakernel (tray_kernel.hip) compiles too.
// Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tray_aov.h"
#include "../../include/tray_shade.h"  // includes tray_query.h
#include "../../include/tray_temporal.h"
#include "../../include/tray_temporal_variance.h"
#include "tray_kernel.hpp"

namespace tray {

// The queries read a scene and a camera through the megakernel's KernelParams
// (prepare_render's scene, camera, row-set and draw-key fields; the work queue,
// sample buffer and every other per-launch workspace stay null: no query
// touches one).

// Camera.GetRay for the n = p.rows x p.width x p.spp samples of p's row set,
// pass p.pass0; ids nullable.
hipError_t launch_camera_rays(KernelParams p, tray_ray* rays, uint32_t* ids, uint32_t n, hipStream_t stream);

// Scene.Hit(r, Interval{1e-6, t_end}) for n rays. use_bvh: rays whose origin
// lies in [-bound, bound]^3 traverse the BVH, the rest (and every ray without
// it) take the reference-order linear scan.
hipError_t launch_scene_hit(const KernelParams& p, bool use_bvh, double bound, const tray_ray* rays, uint32_t n,
                            double t_end, tray_hit* hits, hipStream_t stream);

// Scene.RayColor(r, p.max_depth) for n rays under p.key; ids and segments nullable.
hipError_t launch_ray_color(const KernelParams& p, bool use_bvh, double bound, const tray_ray* rays,
                            const uint32_t* ids, uint32_t n, double* rgb, uint32_t* segments, hipStream_t stream);

// include/tray_shade.h.
// Material.Scatter of n (ray, record) pairs at `bounce` under p.key (scene, material and
// draw-key fields of p); ids nullable.
hipError_t launch_scatter(const KernelParams& p, const tray_ray* rays, const tray_hit* hits, const uint32_t* ids,
                          uint32_t n, uint32_t bounce, tray_scatter* out, hipStream_t stream);

// AmbientLight{color_a, color_b}.Hit for n rays: 3 doubles per ray. Needs no scene.
hipError_t launch_background_hit(V3 color_a, V3 color_b, const tray_ray* rays, uint32_t n, double* rgb,
                                 hipStream_t stream);

// occluded[i] = launch_scene_hit(..., end_i, ...) would report a hit, with end_i =
// t_ends[i] (t_ends nullable: t_end). use_bvh and bound as for launch_scene_hit.
hipError_t launch_scene_occluded(const KernelParams& p, bool use_bvh, double bound, const tray_ray* rays,
                                 const double* t_ends, uint32_t n, double t_end, uint8_t* occluded,
                                 hipStream_t stream);

// include/tray_aov.h.
// The first-hit feature buffers of p's row set (p.rows x p.width pixels, p.spp samples
// each, pass p.pass0): p's scene, camera, image, row-set and draw-key fields. use_bvh
// and bound as for launch_scene_hit. Null buffers of `out` are not written.
hipError_t launch_render_aov(KernelParams p, bool use_bvh, double bound, const tray_aov_buffers& out,
                             hipStream_t stream);

// include/tray_adaptive.h section 2 (tray_adaptive.hip).
// The ordered-sum pixel means of n_pixels listed compact pixels of p's row set, passes
// p.pass0 + pass_plane[pixel] + k for k < n_passes, p.spp samples each: p's scene, camera,
// image, row-set and draw-key fields. n_pixels x n_passes x p.spp <= 2^31 - 1. use_bvh and
// bound as for launch_scene_hit; pass_plane and segments nullable.
hipError_t launch_render_pixels(KernelParams p, bool use_bvh, double bound, const uint32_t* pixels, uint32_t n_pixels,
                                const int32_t* pass_plane, uint32_t n_passes, double* out, uint32_t* segments,
                                hipStream_t stream);

// include/tray_temporal.h and tray_temporal_variance.h, section 2 of each (tray_temporal.hip).
// One reprojection step over the out.width x out.height frame: p's scene and camera fields and
// p.width, p.height. `history` and `prev` both null: the first frame. `record` nullable (zeroed
// on `stream` ahead of the launch). use_bvh and bound as for launch_scene_hit. out.m2 null: the
// plain step, with history's m2 and `variance` null too; else the step with the M2 planes and
// the (nullable) variance of the mean.
hipError_t launch_temporal_step(KernelParams p, bool use_bvh, double bound, const tray_camera* prev,
                                const tray_temporal_params& tp, const double* frame,
                                const tray_temporal_var_state* history, const tray_temporal_var_state& out,
                                double* variance, tray_temporal_record* record, hipStream_t stream);

// include/tray_temporal_variance.h section 3 (tray_temporal.hip): the variance of the mean of the
// n_pixels listed pixels (entries >= image_pixels skipped), or of every pixel when `pixels` is null.
hipError_t launch_temporal_variance(const double* m2, const int32_t* age, uint32_t image_pixels,
                                    const uint32_t* pixels, uint32_t n_pixels, double* variance,
                                    hipStream_t stream);

}  // namespace tray
