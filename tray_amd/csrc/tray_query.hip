// tray_query.hip — batched ray queries on an uploaded scene for gfx950
// (include/tray_query.h): Camera.GetRay (ray/camera.go:113-142), Scene.Hit
// (ray/objects.go:37-46, Sphere.Hit :81-104) and Scene.RayColor
// (ray/objects.go:49-62) as kernels of their own, one ray (sample, path) per
// lane; and (include/tray_shade.h) Material.Scatter (ray/materials.go:13-64),
// AmbientLight.Hit (ray/objects.go:68-73) and the occlusion query, the same way;
// and (include/tray_aov.h) the first-hit feature buffers of a frame, one pixel per
// lane (aov_kernel).
//
// The arithmetic is the megakernel's, not a restatement of it: tray_device.hpp
// holds the functions both compile (get_ray, camera_block, draw, quad, test_geo,
// trav_globals, trav_begin32, trav_node, trav_leaf, scene_hit_linear, unit_lsq,
// sdiv_rcp, reflect, refract, ...), and tray_query_device.hpp, over it, what one ray
// of a query needs (query_hit, query_occluded, query_shade with its scatter_step, the
// stack policy, query_args); the pixel-list renderer (tray_adaptive.hip) includes the
// same two. This file holds the query kernels and, below them, the entry points of the
// three headers: each validates, fills KernelParams and QueryArgs (the scene through
// tray_scene.hpp) and launches its kernel. Compiled with -ffp-contract=off like every other unit.

#include <string.h>

#include <algorithm>

#include "../../include/tray_aov.h"
#include "../../include/tray_debug.h"
#include "../../include/tray_shade.h"  // includes tray_query.h
#include "tray_query_device.hpp"
#include "tray_scene.hpp"

namespace tray {

// Camera.GetRay: lane i is sample s of pixel (x, compact row j), i = (j * width + x) * r + s.
__global__ __launch_bounds__(256) void camera_rays_kernel(KernelParams p, tray_ray* rays, uint32_t* ids, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t spp = (uint32_t)p.spp, width = (uint32_t)p.width;
    const uint32_t s = i % spp, q = i / spp;
    const uint32_t x = q % width, j = q / width;
    const int32_t y = row_of(p, (int32_t)j);
    const uint32_t pixel = (uint32_t)y * width + x;    // global index: the draw block's pixel word
    const uint32_t sample = p.pass0 * spp + s;          // the draw block's sample word
    D3 org, dir;
    get_ray(p, camera_block(p, pixel, sample), (double)x, (double)y, org, dir);
    tray_ray* r = rays + i;
    r->origin[0] = org.x, r->origin[1] = org.y, r->origin[2] = org.z;
    r->direction[0] = dir.x, r->direction[1] = dir.y, r->direction[2] = dir.z;
    if (ids) {
        ids[2 * (size_t)i] = pixel;
        ids[2 * (size_t)i + 1] = sample;
    }
}

// Scene.Hit: one ray per lane. The record is Sphere.Hit's (ray/objects.go:98-102):
// Point = r.At(t), the outward normal (P - C) / R as a correctly rounded quotient
// (sdiv_rcp with the host's RN(1 / R), as shade_step), SetFaceNormal.
__global__ __launch_bounds__(kQueryBlock) void scene_hit_kernel(KernelParams p, QueryArgs q) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= q.n) return;
    const SceneView sv = scene_view(p);
    const QStack S = lane_stack();
    const D3 org = ray_origin(q.rays, i), dir = ray_direction(q.rays, i);
    const QHit h = query_hit(sv, S, q, org, dir, q.t_end);
    tray_hit* o = static_cast<tray_hit*>(q.out) + i;
    if (h.ref < 0) {
        o->point[0] = o->point[1] = o->point[2] = 0.0;
        o->normal[0] = o->normal[1] = o->normal[2] = 0.0;
        o->t = 0.0;
        o->index = -1;
        o->front_face = 0;
        return;
    }
    const double4 g = h.tree ? sv.bgeo[h.ref] : sv.geo[h.ref];
    const MatRec* m = h.tree ? sv.bmat + h.ref : p.mat + h.ref;
    const double radius = m->radius, rinv = m->rinv;
    const D3 point = add(org, smul(dir, h.t));                                 // Ray.At (ray/ray.go:23-25)
    const D3 outward = sdiv_rcp(sub(point, d3(g.x, g.y, g.z)), radius, rinv);  // ray/objects.go:100
    const bool front = dot(dir, outward) < 0;                                  // SetFaceNormal (:19-26)
    const D3 normal = neg_if(outward, !front);
    o->point[0] = point.x, o->point[1] = point.y, o->point[2] = point.z;
    o->normal[0] = normal.x, o->normal[1] = normal.y, o->normal[2] = normal.z;
    o->t = h.t;
    o->index = h.tree ? sv.bidx[h.ref] : h.ref;
    o->front_face = front ? 1 : 0;
}

// Scene.RayColor: one path per lane, the recursion as the megakernel's bounce loop.
// Segments count the path's Scene.Hit calls. Five waves per SIMD: the budget of 96 VGPRs
// costs no scratch and fewer scalar spills than the compiler's own 98 at four waves, and
// measured 10 % faster on the C2 rays (DESIGN.md "Ray queries"); six waves spill to scratch.
__global__ __launch_bounds__(kQueryBlock, 5) void ray_color_kernel(KernelParams p, QueryArgs q) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= q.n) return;
    const SceneView sv = scene_view(p);
    const QStack S = lane_stack();
    D3 org = ray_origin(q.rays, i), dir = ray_direction(q.rays, i);
    const uint32_t pixel = q.ids ? q.ids[2 * (size_t)i] : i;
    const uint32_t sample = q.ids ? q.ids[2 * (size_t)i + 1] : 0u;
    D3 thr = d3(1, 1, 1), color = d3(0, 0, 0);
    uint32_t bounce = 0, segments = 0;
    bool more = true;
    while (more) {
        ++segments;
        const QHit h = query_hit(sv, S, q, org, dir, __builtin_inf());
        more = query_shade(p, sv, h, pixel, sample, bounce, org, dir, thr, color);
    }
    double* o = static_cast<double*>(q.out) + (size_t)i * 3;
    o[0] = color.x;
    o[1] = color.y;
    o[2] = color.z;
    if (q.segments) q.segments[i] = segments;
}

// Material.Scatter (include/tray_shade.h): one record per lane. Point, normal, face and
// sphere index are the RECORD's (the Go method reads rec, ray/materials.go:13-64), not
// recomputed from the sphere; the material is the list-order record of `index`. A record
// that is no hit of this scene (index outside [0, n)) reads no sphere and is not scattered.
__global__ __launch_bounds__(kQueryBlock) void scatter_kernel(KernelParams p, const tray_ray* rays,
                                                              const tray_hit* hits, const uint32_t* ids,
                                                              tray_scatter* out, uint32_t n, uint32_t bounce) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= n) return;
    const tray_hit* rec = hits + i;
    const int32_t index = rec->index;
    bool scattered = false;
    D3 point = d3(0, 0, 0), new_dir = d3(0, 0, 0), att = d3(0, 0, 0);
    if ((uint32_t)index < (uint32_t)p.n) {
        const MatRec m = p.mat[index];
        const D3 dir = ray_direction(rays, i);
        const D3 normal = d3(rec->normal[0], rec->normal[1], rec->normal[2]);
        const uint32_t pixel = ids ? ids[2 * (size_t)i] : i;
        const uint32_t sample = ids ? ids[2 * (size_t)i + 1] : 0u;
        scattered = scatter_step(p, m, pixel, sample, bounce, dir, length_sq(dir), normal, rec->front_face != 0,
                                 new_dir, att);
        point = d3(rec->point[0], rec->point[1], rec->point[2]);
    }
    if (!scattered) point = new_dir = att = d3(0, 0, 0);  // absorbed or no hit: every field zero
    tray_scatter* o = out + i;
    o->attenuation[0] = att.x, o->attenuation[1] = att.y, o->attenuation[2] = att.z;
    o->ray.origin[0] = point.x, o->ray.origin[1] = point.y, o->ray.origin[2] = point.z;
    o->ray.direction[0] = new_dir.x, o->ray.direction[1] = new_dir.y, o->ray.direction[2] = new_dir.z;
    o->scattered = scattered ? 1 : 0;
    o->reserved = 0;
}

// AmbientLight.Hit (ray/objects.go:68-73): query_shade's miss branch without the throughput.
__global__ __launch_bounds__(kQueryBlock) void background_hit_kernel(V3 a, V3 b, const tray_ray* rays, double* rgb,
                                                                     uint32_t n) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= n) return;
    const D3 dir = ray_direction(rays, i);
    const D3 ud = unit_lsq(dir, length_sq(dir));
    const double t = 0.5 * (ud.y + 1.0);
    const D3 color = add(smul(d3(a.x, a.y, a.z), 1.0 - t), smul(d3(b.x, b.y, b.z), t));
    double* o = rgb + (size_t)i * 3;
    o[0] = color.x;
    o[1] = color.y;
    o[2] = color.z;
}

// The occlusion query: one ray per lane, one byte out. t_ends (nullable) holds a
// per-ray Interval.End, else q.t_end serves every ray.
__global__ __launch_bounds__(kQueryBlock) void scene_occluded_kernel(KernelParams p, QueryArgs q,
                                                                     const double* t_ends) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= q.n) return;
    const SceneView sv = scene_view(p);
    const QStack S = lane_stack();
    const D3 org = ray_origin(q.rays, i), dir = ray_direction(q.rays, i);
    const double t_end = t_ends ? t_ends[i] : q.t_end;
    static_cast<uint8_t*>(q.out)[i] = query_occluded(sv, S, q, org, dir, t_end) ? 1 : 0;
}

// First-hit feature buffers (include/tray_aov.h): one pixel per lane and a loop over the
// pixel's samples; a wave is an 8x8 tile of pixels (of compact rows), a workgroup four
// tiles. The lanes of a wave trace one small patch of the image, so their traversals stay
// together (measured on C2 against a wave per 64-pixel row strip: 8 % faster, DESIGN.md
// 8h), every lane of a launch runs the same trip count, and the sums are the contract's by
// construction: sequential from zero in sample order, then one multiplication by 1 / r
// (ray/tracer.go:132-145). Each sample is camera_rays_kernel's ray
// (get_ray on the sample's camera block) and scene_hit_kernel's record (query_hit with
// t_end = +inf, then the same normal), reduced in registers: nothing per sample is stored.
// A miss adds +0 to the normal and depth sums, which changes no sum (none can be -0: they
// start at +0).
struct AovArgs {
    tray_aov_buffers out;
    double inv_spp;     // RN(1 / r), the host's quotient
    uint32_t tiles_x;   // 8x8 pixel tiles per row of tiles: ceil(width / 8)
    uint32_t samples;   // r, or 1 when only `index` is asked for (sample 0 decides it)
};

__global__ __launch_bounds__(kQueryBlock) void aov_kernel(KernelParams p, QueryArgs q, AovArgs a) {
    const uint32_t tile = blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t width = (uint32_t)p.width;
    const uint32_t x = (tile % a.tiles_x) * 8u + (lane & 7u), j = (tile / a.tiles_x) * 8u + (lane >> 3);
    if (x >= width || j >= (uint32_t)p.rows) return;  // the frame's right and lower edge, and tiles past the last
    const uint32_t i = j * width + x;                 // < rows x width <= 2^31 - 1
    const SceneView sv = scene_view(p);
    const QStack S = lane_stack();
    const int32_t y = row_of(p, (int32_t)j);
    const uint32_t pixel = (uint32_t)y * width + x;   // global index: the draw block's pixel word
    const uint32_t sample0 = p.pass0 * (uint32_t)p.spp;  // the draw block's sample word of s = 0
    const double px = (double)x, py = (double)y;
    D3 albedo = d3(0, 0, 0), normal = d3(0, 0, 0);
    double depth = 0.0;
    uint32_t hits = 0;
    int32_t first = -1;
    for (uint32_t s = 0; s < a.samples; ++s) {
        // The camera, draw key and background are read from the kernel arguments where they
        // are used (KernelParams is the first argument), as the megakernel reads them: held
        // in scalar registers across the traversal they spill (71 spills without this).
        const KernelParams& pk = kp_fresh();
        D3 org, dir;
        get_ray(pk, camera_block(pk, pixel, sample0 + s), px, py, org, dir);
        const QHit h = query_hit(sv, S, q, org, dir, __builtin_inf());
        D3 as, ns = d3(0, 0, 0);
        double ds = 0.0;
        if (h.ref < 0) {  // AmbientLight.Hit (ray/objects.go:68-73), as background_hit_kernel
            const KernelParams& pb = kp_fresh();
            const D3 bg_a = d3(pb.bg_a.x, pb.bg_a.y, pb.bg_a.z), bg_b = d3(pb.bg_b.x, pb.bg_b.y, pb.bg_b.z);
            const D3 ud = unit_lsq(dir, h.a);
            const double t = 0.5 * (ud.y + 1.0);
            as = add(smul(bg_a, 1.0 - t), smul(bg_b, t));
        } else {  // Sphere.Hit's record (ray/objects.go:98-102), as scene_hit_kernel
            const double4 g = h.tree ? sv.bgeo[h.ref] : sv.geo[h.ref];
            const MatRec* m = h.tree ? sv.bmat + h.ref : p.mat + h.ref;
            const bool dielectric = m->type == kDielectric;  // attenuation (1,1,1), ray/materials.go:45
            as = d3(dielectric ? 1.0 : m->albedo[0], dielectric ? 1.0 : m->albedo[1], dielectric ? 1.0 : m->albedo[2]);
            const D3 point = add(org, smul(dir, h.t));
            const D3 outward = sdiv_rcp(sub(point, d3(g.x, g.y, g.z)), m->radius, m->rinv);
            ns = neg_if(outward, !(dot(dir, outward) < 0));
            ds = h.t * sqrt_cr(h.a);  // t * Length(dir): h.a is LengthSquared's bits
            ++hits;
            if (s == 0) first = h.tree ? sv.bidx[h.ref] : h.ref;
        }
        albedo = add(albedo, as);
        normal = add(normal, ns);
        depth = depth + ds;
    }
    if (a.out.albedo) {
        double* o = a.out.albedo + (size_t)i * 3;
        o[0] = albedo.x * a.inv_spp, o[1] = albedo.y * a.inv_spp, o[2] = albedo.z * a.inv_spp;
    }
    if (a.out.normal) {
        double* o = a.out.normal + (size_t)i * 3;
        o[0] = normal.x * a.inv_spp, o[1] = normal.y * a.inv_spp, o[2] = normal.z * a.inv_spp;
    }
    if (a.out.depth) a.out.depth[i] = hits ? depth / (double)hits : 0.0;
    if (a.out.coverage) a.out.coverage[i] = (double)hits * a.inv_spp;
    if (a.out.index) a.out.index[i] = first;
}

// One ray per lane: the grid of n rays.
static dim3 ray_blocks(int64_t n) { return dim3(((uint32_t)n + kQueryBlock - 1u) / kQueryBlock); }

}  // namespace tray

using namespace tray;

// The queries read a scene and a camera through the megakernel's KernelParams (scene_params,
// frame_params, key_params; the work queue, sample buffer and every other per-launch
// workspace stay null: no query touches one). With wants_bvh, rays whose origin lies in
// [-bvh_bound, bvh_bound]^3 traverse the BVH; the rest, and every ray without it, take the
// reference-order linear scan (query_args, query_hit).
#pragma GCC visibility push(default)
extern "C" {

// ---- ray queries (include/tray_query.h) ----------------------------------------
int32_t tray_query_version(void) { return TRAY_QUERY_VERSION; }

int tray_camera_rays_async(const tray_camera* cam, const tray_params* p, int32_t device, tray_ray* rays_device,
                           uint32_t* ids_device, void* stream) {
    if (!cam) return fail(TRAY_ERR_INVALID_ARGUMENT, "null camera");
    int rc = validate_params(p);
    if (rc) return rc;
    const int64_t rows = tray_params_rows(p);
    if (rows * (int64_t)p->width > kQueryMaxRays / p->rays_per_pixel)
        return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 camera rays in one query");
    const int64_t n = rows * (int64_t)p->width * (int64_t)p->rays_per_pixel;
    if (n > 0 && !rays_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null ray buffer");
    if (n == 0) return TRAY_OK;
    rc = device_usable(device);
    if (rc) return rc;
    KernelParams k;
    memset(&k, 0, sizeof(k));
    frame_params(cam, p, (int32_t)rows, 1, k);
    k.div_tile_rows = make_fastdiv((uint32_t)std::max(k.tile_rows, 1));  // row_of
    TRAY_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(camera_rays_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0,
                       static_cast<hipStream_t>(stream), k, rays_device, ids_device, (uint32_t)n);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

int tray_scene_hit_async(tray_scene_t sc, const tray_ray* rays_device, int64_t n, double t_end, int32_t flags,
                         tray_hit* hits_device, void* stream) {
    if (t_end != t_end) return fail(TRAY_ERR_INVALID_ARGUMENT, "t_end is NaN");
    int rc = validate_query(sc, rays_device, n, flags, hits_device);
    if (rc) return rc;
    if (n == 0) return TRAY_OK;
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    size_t lds = 0;
    QueryArgs q = query_args(k, wants_bvh(sc, flags), sc->bvh_bound, rays_device, (uint32_t)n, lds);
    q.out = hits_device;
    q.t_end = t_end;
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(scene_hit_kernel, ray_blocks(n), dim3(kQueryBlock), lds, static_cast<hipStream_t>(stream), k, q);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

int tray_ray_color_async(tray_scene_t sc, const tray_ray* rays_device, const uint32_t* ids_device, int64_t n,
                         int32_t max_depth, uint64_t seed, int32_t flags, double* rgb_device,
                         uint32_t* segments_device, void* stream) {
    if (max_depth <= 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "max_depth must be > 0");
    int rc = validate_query(sc, rays_device, n, flags, rgb_device);
    if (rc) return rc;
    if (n == 0) return TRAY_OK;
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    key_params(seed, k);
    k.max_depth = max_depth;
    size_t lds = 0;
    QueryArgs q = query_args(k, wants_bvh(sc, flags), sc->bvh_bound, rays_device, (uint32_t)n, lds);
    q.ids = ids_device;
    q.out = rgb_device;
    q.segments = segments_device;
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(ray_color_kernel, ray_blocks(n), dim3(kQueryBlock), lds, static_cast<hipStream_t>(stream), k, q);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

// ---- scatter, sky and occlusion queries (include/tray_shade.h) -------------------
int32_t tray_shade_version(void) { return TRAY_SHADE_VERSION; }

int tray_scatter_async(tray_scene_t sc, const tray_ray* rays_device, const tray_hit* hits_device,
                       const uint32_t* ids_device, int64_t n, uint32_t bounce, uint64_t seed,
                       tray_scatter* out_device, void* stream) {
    int rc = validate_query(sc, rays_device, n, 0, out_device);
    if (rc) return rc;
    if (n > 0 && !hits_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null hit buffer");
    if (n == 0) return TRAY_OK;
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    key_params(seed, k);
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(scatter_kernel, ray_blocks(n), dim3(kQueryBlock), 0, static_cast<hipStream_t>(stream), k,
                       rays_device, hits_device, ids_device, out_device, (uint32_t)n, bounce);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

int tray_background_hit_async(const tray_background* bg, const tray_ray* rays_device, int64_t n, double* rgb_device,
                              int32_t device, void* stream) {
    if (n < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative ray count");
    if (n > kQueryMaxRays) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 rays in one query");
    if (n > 0 && !rays_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null ray buffer");
    if (n > 0 && !rgb_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null result buffer");
    if (!bg) return fail(TRAY_ERR_INVALID_ARGUMENT, "null background");
    if (n == 0) return TRAY_OK;
    const int rc = device_usable(device);
    if (rc) return rc;
    TRAY_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(background_hit_kernel, ray_blocks(n), dim3(kQueryBlock), 0, static_cast<hipStream_t>(stream),
                       V3{bg->color_a[0], bg->color_a[1], bg->color_a[2]},
                       V3{bg->color_b[0], bg->color_b[1], bg->color_b[2]}, rays_device, rgb_device, (uint32_t)n);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

int tray_scene_occluded_async(tray_scene_t sc, const tray_ray* rays_device, const double* t_end_device, int64_t n,
                              double t_end, int32_t flags, uint8_t* occluded_device, void* stream) {
    if (t_end != t_end) return fail(TRAY_ERR_INVALID_ARGUMENT, "t_end is NaN");
    int rc = validate_query(sc, rays_device, n, flags, occluded_device);
    if (rc) return rc;
    if (n == 0) return TRAY_OK;
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    size_t lds = 0;
    QueryArgs q = query_args(k, wants_bvh(sc, flags), sc->bvh_bound, rays_device, (uint32_t)n, lds);
    q.out = occluded_device;
    q.t_end = t_end;
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(scene_occluded_kernel, ray_blocks(n), dim3(kQueryBlock), lds, static_cast<hipStream_t>(stream),
                       k, q, t_end_device);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

// ---- first-hit feature buffers (include/tray_aov.h) -----------------------------
int32_t tray_aov_version(void) { return TRAY_AOV_VERSION; }

int tray_render_aov_async(tray_scene_t sc, const tray_camera* cam, const tray_params* p, const tray_aov_buffers* out,
                          void* stream) {
    if (!sc) return fail(TRAY_ERR_INVALID_ARGUMENT, "null scene");
    if (!cam) return fail(TRAY_ERR_INVALID_ARGUMENT, "null camera");
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null feature buffers (out)");
    int rc = validate_params(p);
    if (rc) return rc;
    if (!out->albedo && !out->normal && !out->depth && !out->coverage && !out->index)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "every feature buffer is null: nothing to write");
    const int64_t rows = tray_params_rows(p);
    if (rows * (int64_t)p->width > kQueryMaxRays)
        return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one feature-buffer call");
    if (rows == 0) return TRAY_OK;
    // One lane per pixel and a loop over its samples: rows x width x rays_per_pixel has no
    // limit here (the megakernel's 8-row band limit, band_fits, is about its item indices).
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    frame_params(cam, p, (int32_t)rows, 1, k);
    k.div_tile_rows = make_fastdiv((uint32_t)std::max(k.tile_rows, 1));  // row_of
    size_t lds = 0;
    const QueryArgs q =
        query_args(k, wants_bvh(sc, p->flags), sc->bvh_bound, nullptr, (uint32_t)k.rows * (uint32_t)k.width, lds);
    AovArgs a{};
    a.out = *out;  // null buffers are not written
    a.inv_spp = 1.0 / (double)k.spp;
    a.tiles_x = ((uint32_t)k.width + 7u) / 8u;
    a.samples = out->albedo || out->normal || out->depth || out->coverage ? (uint32_t)k.spp : 1u;
    const uint32_t tiles = a.tiles_x * (((uint32_t)k.rows + 7u) / 8u);  // a wave each: <= 2^25 + 2^28
    constexpr uint32_t kTilesPerBlock = kQueryBlock / 64;
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(aov_kernel, dim3((tiles + kTilesPerBlock - 1u) / kTilesPerBlock), dim3(kQueryBlock), lds,
                       static_cast<hipStream_t>(stream), k, q, a);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

// ---- include/tray_debug.h: which launches traverse the tree ------------------------
static_assert(TRAY_QUERY_KIND_PLAIN == kQueryPlain && TRAY_QUERY_KIND_PIXELS == kQueryPixels &&
                  TRAY_QUERY_KIND_TEMPORAL == kQueryTemporal,
              "tray_debug.h names the kinds of tray_query_device.hpp");

int tray_debug_query_traversal(int32_t kind, int32_t stack_depth, int32_t* bvh_out) {
    if (!bvh_out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null argument");
    if (kind < TRAY_QUERY_KIND_PLAIN || kind > TRAY_QUERY_KIND_TEMPORAL)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "unknown query kind");
    if (stack_depth < 0 || stack_depth > (1 << 20)) return fail(TRAY_ERR_INVALID_ARGUMENT, "stack_depth out of range");
    *bvh_out = query_takes_tree(static_cast<QueryKind>(kind), stack_depth + kStackSlack) ? 1 : 0;
    return TRAY_OK;
}

}  // extern "C"
#pragma GCC visibility pop
