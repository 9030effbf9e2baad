// tray_query_device.hpp — the device side the ray-query kernels (tray_query.hip), the
// pixel-list renderer (tray_adaptive.hip) and the temporal step (tray_temporal.hip, which
// uses query_hit and query_args) share: one ray's Scene.Hit and occlusion
// (query_hit, query_occluded) over tray_device.hpp's traversal with the queries' stack
// policy, one recursion level of RayColor on a plain path state (query_shade with its
// scatter_step), and the host-side launch arguments that go with them (query_args).
// No kernel and no entry point lives here.
//
// The arithmetic is tray_device.hpp's, the megakernel's own. The one exception is the
// scatter step (scatter_step and query_shade below), the twin of shade_step: that
// function is tied to the megakernel's lane state and pixel sums, and factoring the
// arithmetic out of it would have changed the product instances ("Ray queries").
#pragma once

#include "../../include/tray_query.h"
#include "tray_device.hpp"

namespace tray {

// Workgroup of the hit and colour kernels. The scene (nodes, leaf table, geometry,
// shading records) is read through L2, not staged: a workgroup traces 256 rays and
// ends, so a per-workgroup LDS copy of the scene is re-made every 256 rays and its
// LDS lowers the occupancy (measured on C2, DESIGN.md "Ray queries": staging the
// book cover's BVH made the hit query 1.45x and the colour query 1.57x slower).
// Only the traversal stacks live in LDS.
constexpr int kQueryBlock = 256;
static_assert(kQueryBlock % 64 == 0, "whole waves");

// The traversal stack policy of the queries (trav_node / trav_leaf take any policy
// with these two accessors): the megakernel's layout, slot i of a lane at
// base[i * lanes of the workgroup], for kQueryBlock lanes: stack_cap x 1 KB of LDS
// per workgroup. No spill area: a scene whose stack does not fit takes the linear
// scan (query_args).
struct QStack {
    static constexpr bool spill = false;
    __attribute__((address_space(3))) uint32_t* base;  // this lane's slot 0
};
__device__ __forceinline__ uint32_t stack_load(const QStack& S, int32_t i) { return S.base[i * kQueryBlock]; }
__device__ __forceinline__ void stack_store(const QStack& S, int32_t i, uint32_t v) { S.base[i * kQueryBlock] = v; }

struct QueryArgs {
    const tray_ray* rays;
    const uint32_t* ids;  // colour, nullable: (pixel, sample word) per ray
    void* out;            // tray_hit per ray / 3 doubles per ray
    uint32_t* segments;   // colour, nullable
    uint32_t n;
    int32_t use_bvh;      // 0: every ray takes the linear scan
    double bound;         // M: the BVH needs ray origins in [-M, M]^3 (tray_bvh.cpp)
    double t_end;         // hit: Interval.End
};

__device__ __forceinline__ SceneView scene_view(const KernelParams& p) {
    return SceneView{p.geo,  p.nodes, p.leaves,  p.leaf_single != 0, p.bgeo,          p.bidx,
                     p.bmat, p.n,     p.n_nodes, p.n_global,         p.n_slots - p.n_global};
}

__device__ __forceinline__ D3 ray_origin(const tray_ray* rays, uint32_t i) {
    return d3(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2]);
}
__device__ __forceinline__ D3 ray_direction(const tray_ray* rays, uint32_t i) {
    return d3(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2]);
}

// Scene.Hit(r, Interval{1e-6, t_end}): the hit's root and where its sphere's records
// are (`ref`: a leaf slot when `tree`, else the list index; -1: no hit).
struct QHit {
    double t;
    double a;  // |dir|^2 (same bits as Sphere.Hit's per sphere)
    int32_t ref;
    bool tree;
};

// Per ray: the BVH when the launch has one, the origin lies inside the bound its
// padding proof needs, and the direction is finite and of a length FP32 can carry
// (slab_dir_ok, tray_device.hpp: the one range this choice and the megakernel's camera
// rays share); any other ray takes the
// reference-order linear scan, which has no such conditions. Both give
// min over spheres of (t_i, i) with t_i in (1e-6, t_end) (the any-order rule,
// tray_device.hpp): the traversal by starting its culling distance at t_end,
// where a root equal to t_end loses because no hit is held yet; the scan by
// dropping a closest hit that is not below t_end.
__device__ __forceinline__ QHit query_hit(const SceneView& sv, const QStack& S, const QueryArgs& q, const D3& org,
                                          const D3& dir, double t_end) {
    QHit h;
    h.a = length_sq(dir);
    h.t = t_end;
    h.ref = -1;
    const double M = q.bound;
    const bool inside = __builtin_fabs(org.x) <= M && __builtin_fabs(org.y) <= M && __builtin_fabs(org.z) <= M;
    h.tree = q.use_bvh != 0 && inside && slab_dir_ok(h.a);
    if (!(t_end > 1e-6)) return h;  // an empty interval surrounds no root
    if (h.tree) {
        Trav T;
        T.tlim = __builtin_inff();
        trav_globals(T, sv, org, dir);
        if (!(T.closest < t_end)) {  // nothing closer than t_end among the out-of-tree spheres
            T.closest = t_end;
            T.slot = -1;
        }
        trav_begin32(T, sv, org, dir);
        uint32_t tested;
        while (T.cur != kBvhNone) {
            if (is_trav(T.cur)) trav_node(T, sv, S, tested);
            else trav_leaf(T, sv, S, org, dir, tested);
        }
        h.t = T.closest;
        h.ref = T.slot;
    } else {
        Stats st;
        double closest;
        const int best = scene_hit_linear<TRAY_UNROLL, false>(sv, org, dir, closest, st);
        if (best >= 0 && closest < t_end) {
            h.t = closest;
            h.ref = best;
        }
    }
    return h;
}

// "Does query_hit(..., t_end) hold a hit?" without finding the closest one: query_hit's
// algorithm, the same per-ray choice of BVH or scan included, with an early exit. Under
// the any-order rule a root is accepted only inside (1e-6, current closest), and the
// culling distance starts at t_end with no hit held, so the first accepted root already
// lies in (1e-6, t_end): the traversal stops there. What it would have gone on to find
// is a closer root of the same interval, which cannot change the answer. A hit among the
// out-of-tree spheres below t_end answers before the tree is entered.
__device__ __forceinline__ bool query_occluded(const SceneView& sv, const QStack& S, const QueryArgs& q, const D3& org,
                                               const D3& dir, double t_end) {
    const double a = length_sq(dir);
    const double M = q.bound;
    const bool inside = __builtin_fabs(org.x) <= M && __builtin_fabs(org.y) <= M && __builtin_fabs(org.z) <= M;
    const bool tree = q.use_bvh != 0 && inside && slab_dir_ok(a);
    if (!(t_end > 1e-6)) return false;  // an empty interval (a NaN end included) surrounds no root
    if (tree) {
        Trav T;
        T.tlim = __builtin_inff();
        trav_globals(T, sv, org, dir);
        if (T.closest < t_end) return true;
        T.closest = t_end;
        T.slot = -1;
        trav_begin32(T, sv, org, dir);
        uint32_t tested;
        while (T.cur != kBvhNone && T.slot < 0) {
            if (is_trav(T.cur)) trav_node(T, sv, S, tested);
            else trav_leaf(T, sv, S, org, dir, tested);
        }
        return T.slot >= 0;
    }
    Stats st;
    double closest;
    const int best = scene_hit_linear<TRAY_UNROLL, false>(sv, org, dir, closest, st);
    return best >= 0 && closest < t_end;
}

__device__ __forceinline__ QStack lane_stack() {
    extern __shared__ __attribute__((aligned(16))) uint32_t query_stacks[];
    return QStack{(__attribute__((address_space(3))) uint32_t*)query_stacks + threadIdx.x};
}

// The stacks of one workgroup; the dynamic-LDS default limit (64 KB) bounds them.
inline size_t query_stack_bytes(int32_t stack_cap) { return (size_t)stack_cap * kQueryBlock * sizeof(uint32_t); }
constexpr size_t kQueryLdsMax = 64 * 1024;

// The kernel families that find their hits through query_hit / query_occluded, by the static
// LDS their kernels hold beside the stacks (the values of TRAY_QUERY_KIND_*, include/tray_debug.h).
enum QueryKind : int32_t {
    kQueryPlain = 0,     // hit, occluded, ray colour, feature buffers: the stacks alone
    kQueryPixels = 1,    // render_pixels_kernel (tray_adaptive.hip): the parked colours
    kQueryTemporal = 2,  // temporal_step_kernel (tray_temporal.hip): the record's reduction
};
constexpr size_t kPixelStaticLds = 8 * 1024;  // an upper bound of render_pixels_kernel's static LDS (7196 bytes)
constexpr size_t kTemporalStaticLds = 64;     // temporal_step_kernel's red[2][4]

// Does a launch of `kind` on a scene with a tree traverse it (true), or does every ray take
// the linear scan because the stacks do not fit into LDS beside the kernel's own? The one
// place that decides it: query_args for every launch, tray_debug_query_traversal for tests.
inline bool query_takes_tree(QueryKind kind, int32_t stack_cap) {
    const size_t beside = kind == kQueryPixels ? kPixelStaticLds : kind == kQueryTemporal ? kTemporalStaticLds : 0;
    return query_stack_bytes(stack_cap) + beside <= kQueryLdsMax;
}

inline QueryArgs query_args(const KernelParams& p, bool use_bvh, double bound, const tray_ray* rays, uint32_t n,
                            size_t& lds, QueryKind kind = kQueryPlain) {
    QueryArgs q{};
    q.rays = rays;
    q.n = n;
    lds = query_stack_bytes(p.stack_cap);
    q.use_bvh = use_bvh && p.n_nodes > 0 && query_takes_tree(kind, p.stack_cap) ? 1 : 0;
    if (!q.use_bvh) lds = 0;
    q.bound = bound;
    q.t_end = __builtin_inf();
    return q;
}

// Material.Scatter (ray/materials.go:13-64) of a ray with direction `dir` (a = |dir|^2) at a
// hit whose record has `normal` and `front`: the draws of (pixel, sample, bounce, purpose 3),
// then Lambertian, Metal or Dielectric. Returns didScatter and leaves the scattered
// direction in `new_dir` and the attenuation in `att`; the scattered ray's origin is the
// record's point, which the caller has. THE TWIN OF the same lines of shade_step
// (tray_kernel.hip), which is tied to the megakernel's Lane: the same expressions in the
// same order, and a change to either belongs in both (tests/test_gpu_query.py compares the
// two bit for bit through query_shade, tests/test_gpu_shade.py this function with the
// oracle). The one copy on the query side: query_shade (normal computed from the sphere)
// and scatter_kernel (normal read from the caller's record) both call it.
__device__ __forceinline__ bool scatter_step(const KernelParams& p, const MatRec& m, uint32_t pixel, uint32_t sample,
                                             uint32_t bounce, const D3& dir, double a, const D3& normal, bool front,
                                             D3& new_dir, D3& att) {
    const Block w = draw(p, pixel, sample, bounce, kPurposeScatter);
    const double u0 = uniform(w.x0);
    D3 ud = d3(0, 0, 0);
    if (m.type != kLambertian) ud = unit_lsq(dir, a);
    bool scattered = true;
    att = d3(m.albedo[0], m.albedo[1], m.albedo[2]);
    const bool lambertian = m.type == kLambertian, dielectric = m.type == kDielectric;
    const double cos_theta = go_min1(dot(neg(ud), normal));
    const double z = 1.0 - 2.0 * u0;
    const double sq = sqrt_cr(dielectric ? 1.0 - cos_theta * cos_theta : 1.0 - z * z);
    D3 uv = d3(0, 0, 0);
    if (lambertian || (m.type == kMetal && m.param > 0.0)) uv = unit_vector_from(z, sq, w.x1);
    if (lambertian) {  // ray/materials.go:13-20
        new_dir = add(normal, uv);
        if (near_zero(new_dir)) new_dir = normal;
    } else if (m.type == kMetal) {  // ray/materials.go:28-37
        D3 reflected = reflect(ud, normal);
        if (m.param > 0.0) reflected = add(reflected, smul(uv, m.param));
        new_dir = reflected;
        scattered = dot(new_dir, normal) > 0;
    } else {  // Dielectric, ray/materials.go:44-64
        att = d3(1.0, 1.0, 1.0);
        const double ratio = front ? m.pinv : m.param;
        const double sin_theta = sq;
        const double r0 = front ? m.albedo[0] : m.albedo[1];
        const bool do_reflect = ratio * sin_theta > 1.0 || reflectance(cos_theta, r0) > u0;
        new_dir = do_reflect ? reflect(ud, normal) : refract(ud, normal, ratio);
    }
    return scattered;
}

// One recursion level of RayColor after Scene.Hit gave `h`: the twin of shade_step
// (tray_kernel.hip) on a plain path state instead of the megakernel's Lane / end_path,
// with the material arithmetic in scatter_step (above). Returns true when the path
// goes on with (org, dir), false when it ended with `color`.
__device__ __forceinline__ bool query_shade(const KernelParams& p, const SceneView& sv, const QHit& h, uint32_t pixel,
                                            uint32_t sample, uint32_t& bounce, D3& org, D3& dir, D3& thr, D3& color) {
    const bool hit = h.ref >= 0;
    // A hit at the last level ends the path black (RayColor(depth 0) is black).
    const bool last = bounce + 1u >= (uint32_t)p.max_depth;
    color = d3(0, 0, 0);
    if (!hit) {  // AmbientLight.Hit (ray/objects.go:68-73)
        const D3 ud = unit_lsq(dir, h.a);
        const double t = 0.5 * (ud.y + 1.0);
        const D3 bg_a = d3(p.bg_a.x, p.bg_a.y, p.bg_a.z), bg_b = d3(p.bg_b.x, p.bg_b.y, p.bg_b.z);
        color = mul(thr, add(smul(bg_a, 1.0 - t), smul(bg_b, t)));
        return false;
    }
    const bool wild = p.wild_att != 0;  // an infinite or NaN attenuation in the scene (shade_step)
    if (last && !wild) return false;
    const double4 g = h.tree ? sv.bgeo[h.ref] : sv.geo[h.ref];
    const MatRec m = h.tree ? sv.bmat[h.ref] : p.mat[h.ref];
    const D3 point = add(org, smul(dir, h.t));                                     // Ray.At (ray/ray.go:23-25)
    const D3 outward = sdiv_rcp(sub(point, d3(g.x, g.y, g.z)), m.radius, m.rinv);  // ray/objects.go:100
    const bool front = dot(dir, outward) < 0;                                      // SetFaceNormal (:19-26)
    const D3 normal = neg_if(outward, !front);
    D3 new_dir, att;
    const bool scattered = scatter_step(p, m, pixel, sample, bounce, dir, h.a, normal, front, new_dir, att);
    if (!scattered || last) {  // absorbed, or scattered into depth 0 (wild only) -> black
        if (wild) color = smul(scattered ? mul(thr, att) : thr, 0.0);
        return false;
    }
    thr = mul(thr, att);           // outer-first throughput product, as the megakernel
    org = point;
    dir = new_dir;
    ++bounce;
    return true;
}

}  // namespace tray
