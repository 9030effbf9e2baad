// tray_device.hpp — the device functions and types that more than one translation
// unit uses: the megakernel (tray_kernel.hip), the ray queries (tray_query_device.hpp,
// tray_query.hip) and the pixel-list renderer (tray_adaptive.hip) compile the same
// arithmetic from here, not restatements of it.
//
// In the order the path tracer needs them: the D3 arithmetic and the exact quotients,
// the draws and samplers, Camera.GetRay (ray/camera.go:113-142), the row set, Sphere.Hit
// and the reference-order linear scan (ray/objects.go:37-46, 81-104), and Scene.Hit
// through the exact-culling 4-wide BVH (tray_bvh.cpp): the traversal state, the stack
// policy and one node or leaf step. No kernel and no host launcher lives here; what only
// the megakernel uses (its lane state, pixel sums, shading and the kernels) stays in
// tray_kernel.hip.
// Arithmetic: FP64, reference op order; every unit is compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh.hpp"
#include "fp64.hpp"
#include "rng.hpp"
#include "tray_internal.hpp"
#include "tray_kernel.hpp"

namespace tray {

struct D3 {
    double x, y, z;
};

__device__ __forceinline__ D3 d3(double x, double y, double z) { return D3{x, y, z}; }
// Add(u,v) = {v.x+u.x, ...} (ray/vec3.go:25-27); IEEE addition commutes.
__device__ __forceinline__ D3 add(D3 u, D3 v) { return d3(v.x + u.x, v.y + u.y, v.z + u.z); }
__device__ __forceinline__ D3 sub(D3 u, D3 v) { return d3(u.x - v.x, u.y - v.y, u.z - v.z); }
__device__ __forceinline__ D3 smul(D3 v, double t) { return d3(v.x * t, v.y * t, v.z * t); }
__device__ __forceinline__ D3 mul(D3 u, D3 v) { return d3(u.x * v.x, u.y * v.y, u.z * v.z); }
__device__ __forceinline__ D3 sdiv(D3 v, double t) { return d3(v.x / t, v.y / t, v.z / t); }
__device__ __forceinline__ D3 neg(D3 v) { return d3(-v.x, -v.y, -v.z); }
// cond ? neg(v) : v as sign-bit flips (one mask, three XORs instead of six selects).
__device__ __forceinline__ double flip(double x, uint64_t m) {
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, x) ^ m);
}
__device__ __forceinline__ D3 neg_if(D3 v, bool cond) {
    const uint64_t m = (uint64_t)cond << 63;
    return d3(flip(v.x, m), flip(v.y, m), flip(v.z, m));
}

// a / b, correctly rounded, given y = RN(1/b) (exactly rounded, e.g. a full
// division or a host-side 1.0/b): q = RN(a*y) is within 1 ulp of a/b, the
// residual fma(-b, q, a) is exact, and one correction fma(r, y, q) returns
// RN(a/b) when |q| lies in [2^-960, 2^960) (Markstein 1990; Muller et al.,
// Handbook of Floating-Point Arithmetic §4.7). 3 FP64 instructions instead of
// ~10 for the generic sequence; checked on 4.3e9 pairs by tools/div_check.hip.
// The range is tested on the high word (biased exponent 63..1982; NaN and
// infinities fail); quotients outside it take the full division in a rarely
// taken branch.
//
// A vector divided by t (Unit, the normal (P - C) / R): one range check per
// component and one branch for the three. A zero component also takes that
// branch (the sign of a zero quotient needs the full division; exact zeros do
// not occur in practice), so the common path has no zero test and no select.
__device__ __forceinline__ double div_rcp_nz(double a, double b, double y, bool& ok) {
    const double q = a * y;
    const double r = __builtin_fma(-b, q, a);
    ok = ok & (((hi_word(q) & 0x7FF00000u) - (63u << 20)) < (1920u << 20));
    return __builtin_fma(r, y, q);
}
__device__ __forceinline__ D3 sdiv_rcp(D3 v, double t, double y) {
    bool ok = true;
    const D3 q = d3(div_rcp_nz(v.x, t, y, ok), div_rcp_nz(v.y, t, y, ok), div_rcp_nz(v.z, t, y, ok));
    if (__builtin_expect(!ok, 0)) return sdiv(v, t);
    return q;
}
// A root of Sphere.Hit, (h -+ sqrt(disc)) / a (ray/objects.go:91,93), is used
// only through `root > 1e-6 && root < closest` and, when that holds, as the
// value itself: a quotient below 2^-960 (or a zero of either sign) fails
// root > 1e-6 whether or not it is exact, so only the upper end of the range
// is checked (q >= 2^960, infinities and NaN take the full division): two
// integer instructions and no select.
__device__ __forceinline__ double div_root(double a, double b, double y) {
    const double q = a * y;
    const double r = __builtin_fma(-b, q, a);
    const double q1 = __builtin_fma(r, y, q);
    // biased exponent >= 1983 (one 32-bit field extract and compare)
    if (__builtin_expect(__builtin_amdgcn_ubfe(hi_word(q), 20u, 11u) >= 1983u, 0)) return a / b;
    return q1;
}
__device__ __forceinline__ double dot(D3 u, D3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
__device__ __forceinline__ double length_sq(D3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
// Unit (ray/vec3.go:116-119): each component divided by the length. `lsq` is
// length_sq(v) when the caller already has it (same bits).
__device__ __forceinline__ D3 unit_lsq(D3 v, double lsq) {
    const double l = sqrt_cr(lsq);
    return sdiv_rcp(v, l, rcp_cr(l));
}
__device__ __forceinline__ D3 unit(D3 v) { return unit_lsq(v, length_sq(v)); }
__device__ __forceinline__ bool near_zero(D3 v) {
    const double s = 1e-8;
    return (__builtin_fabs(v.x) < s) && (__builtin_fabs(v.y) < s) && (__builtin_fabs(v.z) < s);
}
// math.Min(x, 1): NaN propagates, everything else compares (no signed-zero or
// -Inf special case can change the result against the constant 1).
__device__ __forceinline__ double go_min1(double x) { return !(x >= 1.0) ? x : 1.0; }
__device__ __forceinline__ D3 reflect(D3 v, D3 n) { return sub(v, smul(n, 2 * dot(v, n))); }
__device__ __forceinline__ D3 refract(D3 uv, D3 n, double eta) {
    const double cos_theta = go_min1(dot(neg(uv), n));
    const D3 perp = smul(add(uv, smul(n, cos_theta)), eta);
    const D3 par = smul(n, -sqrt_cr(__builtin_fabs(1.0 - length_sq(perp))));
    return add(perp, par);
}
// Reflectance (ray/materials.go:66-71) given r0 = ((1 - ref_idx) / (1 + ref_idx))^2,
// precomputed per face on the host; math.Pow(x,5) == x*((x*x)*(x*x)).
__device__ __forceinline__ double reflectance(double cosine, double r0) {
    const double x = 1 - cosine;
    const double x2 = x * x;
    const double x4 = x2 * x2;
    return r0 + (1 - r0) * (x * x4);
}

// The uniform u = w 2^-32 of a 32-bit word of a draw block (include/tray.h).
__device__ __forceinline__ double uniform(uint32_t w) { return (double)w * 0x1.0p-32; }

// InDisc(radius) (ray/tracer.go:138, ray/camera.go:128): polar map of two
// uniforms: r = sqrt(ua), phi = 2 pi ub (ub given as its word).
__device__ __forceinline__ void disc(uint32_t wa, uint32_t wb, double radius, double& ox, double& oy) {
    // ua = k 2^-32: 0 or >= 2^-32, inside sqrt_core's range
    const double ua = uniform(wa);
    double r = sqrt_core(ua);
    if (wa == 0) r = ua;
    double s, c;
    sincos_2pi_word(wb, s, c);
    ox = (r * c) * radius;
    oy = (r * s) * radius;
}

// The kernel's parameters read afresh from the kernel-argument segment: a use through
// this reference reloads the fields it needs (scalar loads, cached) instead of the
// compiler keeping every parameter the loop touches in a scalar register across the
// whole loop, where the product instance spilled 20 of them to vector-register lanes.
__device__ __forceinline__ const KernelParams& kp_fresh() {
    typedef const __attribute__((address_space(4))) KernelParams* ConstParams;
    ConstParams q = (ConstParams)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));  // opaque: no load through q is hoisted above this point
    return *(const KernelParams*)q;
}

// Launch options compiled in (render_kernel's kOpt). The render loop asks questions
// whose answers are fixed for a whole launch (is there a segment buffer, is this a counting launch,
// are the rows contiguous, ...), at every use, through kp_fresh(): a scalar load, a wait, a compare
// and a branch each time. An option set answers some of them at compile time: a `true` below means
// "the launch was checked to have this property" (plain_frame_launch, tray_kernel.hip), the test
// and its dead arm are not compiled, and `false` means "ask at run time", the code as it always was.
// LaunchAsk asks everything and is the default everywhere, so code that names no option set is
// textually and in its instructions what it was.
struct LaunchAsk {
    static constexpr bool kNoSegments = false;   // KernelParams::segments is null
    static constexpr bool kNoCount = false;      // KernelParams::tile_cost is null (no counting launch)
    static constexpr bool kCand = false;         // KernelParams::cand is set (primary-ray candidates)
    static constexpr bool kMultiSample = false;  // rays per pixel > 1 (the anti-aliasing disc is drawn)
    static constexpr bool kContigRows = false;   // KernelParams::tile_rows <= 0 (no row tiles)
    static constexpr bool kOrdered = false;      // KernelParams::tile_order is set (a work order)
    static constexpr bool kOneGlobal = false;    // exactly one sphere outside the tree
    static constexpr bool kHasNodes = false;     // the tree has a root
    static constexpr bool kSingleLeaf = false;   // SceneView::single: one sphere per leaf
};
// The plain frame: every option fixed.
struct PlainFrame {
    static constexpr bool kNoSegments = true, kNoCount = true, kCand = true, kMultiSample = true, kContigRows = true,
                          kOrdered = true, kOneGlobal = true, kHasNodes = true, kSingleLeaf = true;
};
// Not a fact of the launch but the schedule measured for an instance: whether its leaf,
// shade and refill phases run by the cost rule (phase_fires, tray_kernel.hpp) or by the fixed lane
// counts. The plain-frame instance was measured; the generic instances keep their counts and code.
#ifdef TRAY_TRIGGERS_ALL  // the profile's build only: the stats instance is a generic one. Every instance then
                          // takes the rule, the linear scan's refill too (its busy lanes are its lanes in flight).
template <class Opt>
inline constexpr bool kCostTriggers = true;
#else
template <class Opt>
inline constexpr bool kCostTriggers = false;
template <>
inline constexpr bool kCostTriggers<PlainFrame> = true;
#endif

// The draw block of (pixel, sample, bounce, purpose) (include/tray.h, rng.hpp draw_block).
__device__ __forceinline__ Block draw(const KernelParams& p, uint32_t pixel, uint32_t sample, uint32_t bounce,
                                     uint32_t purpose) {
    return draw_block(p.key[0], p.key[1], p.key[2], p.key[3], pixel, sample, bounce, purpose);
}

__device__ __forceinline__ D3 ld3(const double v[3]) { return d3(v[0], v[1], v[2]); }

// RandomUnitVector (ray/rand.go:30-32): Archimedes' projection of two uniforms of
// the bounce's scatter block, z = 1 - 2 u0, r = sqrt(1 - z*z), phi = 2 pi u1.
__device__ __forceinline__ D3 unit_vector_from(double z, double r, uint32_t w1) {
    double s, c;
    sincos_2pi_word(w1, s, c);
    return d3(r * c, r * s, z);
}

// The sample's camera block (purpose 1): (pixel, sample, 0, 1).
__device__ __forceinline__ Block camera_block(const KernelParams& p, uint32_t pixel, uint32_t sample) {
    return draw(p, pixel, sample, 0u, kPurposeCamera);
}

// Camera.GetRay (ray/camera.go:113-142). The sample's camera block `u` feeds the
// anti-aliasing disc (words 0,1; ray/tracer.go:136-139, only when r > 1) and the
// lens disc (words 2,3, only when the aperture is open).
template <class Opt = LaunchAsk>
__device__ __forceinline__ void get_ray(const KernelParams& p, const Block& u, double px, double py, D3& origin,
                                        D3& dir) {
    double ox = 0.0, oy = 0.0;
    const double aperture = p.cam.aperture;
    if constexpr (Opt::kMultiSample) {
        disc(u.x0, u.x1, p.ray_radius, ox, oy);
    } else {
        if (p.spp > 1) disc(u.x0, u.x1, p.ray_radius, ox, oy);
    }
    const D3 pos = ld3(p.cam.position);
    const D3 p00 = ld3(p.cam.pixel00);
    const D3 pxv = ld3(p.cam.pixel_x);
    const D3 pyv = ld3(p.cam.pixel_y);
    const D3 sample_pt = add(add(p00, smul(pxv, px + ox)), smul(pyv, py + oy));
    origin = pos;
    dir = sub(sample_pt, pos);
    if (aperture > 0) {
        double dx, dy;
        disc(u.x2, u.x3, 1.0, dx, dy);
        const D3 du = ld3(p.cam.defocus_u);
        const D3 dv = ld3(p.cam.defocus_v);
        const D3 offset = add(smul(du, dx), smul(dv, dy));
        const D3 focus_point = add(pos, smul(dir, p.focus_time));
        origin = add(pos, offset);
        dir = sub(focus_point, origin);
    }
}

// n / d and n % d by the launch's FastDiv (tray_kernel.hpp).
__device__ __forceinline__ uint32_t udiv(uint32_t n, const FastDiv& f, uint32_t& rem) {
    const uint32_t t = __umulhi(n, f.m);
    const uint32_t q = (t + ((n - t) >> f.s1)) >> f.s2;
    rem = n - q * f.d;
    return q;
}

// Compact output row j -> image row y (see tray_params in include/tray.h).
template <class Opt = LaunchAsk>
__device__ __forceinline__ int32_t row_of(const KernelParams& p, int32_t j) {
    if constexpr (Opt::kContigRows) return p.y_start + j;
    if (p.tile_rows <= 0) return p.y_start + j;
    uint32_t within;
    const int32_t t = (int32_t)udiv((uint32_t)j, p.div_tile_rows, within);
    return p.y_start + (t * p.tile_count + p.tile_index) * p.tile_rows + (int32_t)within;
}

// Candidate root of one sphere whose discriminant is >= 0 (Sphere.Hit,
// ray/objects.go:86-94): the first root inside (1e-6, closest) wins. Used by the
// linear scan, which visits spheres in list order exactly like the reference.
__device__ __forceinline__ void candidate(double h, double disc, double a, double a_inv, int idx, double& closest,
                                          int& best) {
    if (disc >= 0) {
        const double sq = sqrt_cr(disc);
        double root = div_root(h - sq, a, a_inv);
        bool ok = root > 1e-6 && root < closest;
        if (!ok) {
            root = div_root(h + sq, a, a_inv);
            ok = root > 1e-6 && root < closest;
        }
        if (ok) {
            closest = root;
            best = idx;
        }
    }
}

// The any-order rule (test_geo). Sphere.Hit's root choice does not depend on
// the interval end: root2 >= root1, so the reference takes t = root1 if
// root1 > 1e-6, else root2, and accepts it iff t < closestSoFar. The linear
// scan therefore returns min over spheres of (t_i, i); accepting "t < closest,
// or t == closest with a lower index" reproduces it for any visiting order.

// 17 FP64 add/mul per sphere, op order of Sphere.Hit (ray/objects.go:82-86).
__device__ __forceinline__ void quad(const double4 g, const D3& org, const D3& dir, double a, double& h,
                                     double& disc) {
    const double ocx = g.x - org.x;
    const double ocy = g.y - org.y;
    const double ocz = g.z - org.z;
    h = dir.x * ocx + dir.y * ocy + dir.z * ocz;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - g.w;
    disc = h * h - a * c;
}

#ifndef TRAY_UNROLL
#define TRAY_UNROLL 8
#endif

// Instrumented launches only: per-lane counters, flushed once when the lane exits.
#ifndef TRAY_PROFILE
struct Stats {
    uint64_t segments = 0, spheres = 0, boxes = 0;
#ifdef TRAY_STATS_PRIMARY  // diagnostic: node visits, leaf visits, box tests of primary segments; all node/leaf visits
    uint64_t nodes0 = 0, leaves0 = 0, boxes0 = 0, nodes = 0, leaves = 0;
#endif
#ifdef TRAY_STATS_GROUND  // diagnostic: segments leaving an out-of-tree sphere (upward cube face / any) and their visits
    uint64_t g_seg[2] = {0, 0}, g_nodes[2] = {0, 0}, g_leaves[2] = {0, 0}, nodes = 0, leaves = 0;
#endif
};
#else  // phase profiles count in LDS; per-lane counters would cost registers
struct NoCount {
    __device__ NoCount& operator+=(uint64_t) { return *this; }
    __device__ operator unsigned long long() const { return 0ull; }
};
struct Stats {
    NoCount segments, spheres, boxes;
};
#endif

// Geometry visible to one workgroup (LDS copies, or global memory when the
// scene does not fit).
struct SceneView {
    const double4* geo;     // linear scan: list order, NaN-padded
    const Bvh4Node* nodes;  // BVH: 4-wide nodes, root first
    const int32_t* leaves;  // BVH: per leaf (first slot << 3) | count
    bool single;            // BVH: one sphere per leaf, leaf index == slot
    const double4* bgeo;    // BVH: spheres in leaf-slot order
    const int32_t* bidx;    // BVH: original list index of each slot
    const MatRec* bmat;     // BVH: shading record of each slot
    int32_t n, n_nodes;
    int32_t n_global, global_first;  // BVH: spheres tested before the tree, their first slot
};

// Scene.Hit (ray/objects.go:37-46) as the reference's linear scan over
// NaN-padded geometry (a NaN discriminant is never >= 0). Spheres are tested in
// groups of U that share one wave-level branch into the rare sqrt/div path;
// inside a group they are visited in list order.
template <int U, bool kStats>
__device__ __forceinline__ int scene_hit_linear(const SceneView& sv, const D3& org, const D3& dir, double& closest,
                                                Stats& st) {
    const double a = length_sq(dir);  // hoisted: same bits as per sphere
    const double a_inv = rcp_cr(a);
    closest = __builtin_inf();
    int best = -1;
    const int ngroups = (sv.n + U - 1) / U;
    for (int gi = 0; gi < ngroups; ++gi) {
        const int i = gi * U;
        double h[U], d[U];
#pragma unroll
        for (int k = 0; k < U; ++k) quad(sv.geo[i + k], org, dir, a, h[k], d[k]);
        double m = d[0];
#pragma unroll
        for (int k = 1; k < U; ++k) m = __builtin_fmax(m, d[k]);  // maxNum drops NaN padding
        if (m >= 0) {
#pragma unroll
            for (int k = 0; k < U; ++k) candidate(h[k], d[k], a, a_inv, i + k, closest, best);
        }
    }
    if constexpr (kStats) st.spheres += (uint64_t)sv.n;
    return best;
}

// Round a positive (or +inf) double up to a float that is >= it.
__device__ __forceinline__ float f32_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

// Per-lane traversal state of one Scene.Hit through the exact-culling 4-wide
// BVH (tray_bvh.cpp): conservative FP32 slab tests of a node's four child boxes
// (culled against the current closest hit), near-first descent with a per-lane
// stack in LDS, FP64 sphere tests with the reference's arithmetic and the
// any-order acceptance rule.
// Lane states of the BVH kernel, encoded in Trav::cur (no state register, no
// per-step state bookkeeping): an inner node (< kBvhLeafBit) = traversing; a
// leaf reference = waiting for the leaf phase; kBvhNone = traversal done,
// waiting for the shade phase (busy lane) or idle (Lane::busy false);
// kTravHit / kTravHitCam = the finished segment hit a sphere above the last level
// (Trav::slot, closest and a still describe the hit): its scatter (shade_scatter) is
// still to run, in the kernel loop's scatter step; kTravReady = the scattered ray is in
// Lane::org / dir and its setup (trav_begin) is still to run, in that step's begin part.

struct Trav {
    float ix, iy, iz, oix, oiy, oiz;  // FP32 ray: t = box * inv - org * inv
    float tlim;                       // closest rounded up to float
    int32_t near_x, near_y, near_z;   // byte offsets of the near planes in a node
    uint32_t cur;                     // child reference to visit next (kBvhNone: done)
    uint32_t top;                     // stack top: sort key (entry distance | reference)
    int32_t sp;                       // stack depth (the top included)
    double a, a_inv, closest;
    int32_t slot;  // leaf slot (geometry + shading record) of the closest hit, -1: none
};

// The BVH kernel runs one workgroup per CU by default (all its waves share one
// LDS copy of the scene); the linear scan runs 256-lane workgroups.
constexpr int kBvhBlock = TRAY_BVH_BLOCK;
static_assert(kBvhBlock <= 1024, "BVH workgroup larger than 1024 lanes");
// Traversal stack slots per lane are kept in LDS as far as the workgroup's LDS
// allows after the scene (4 KB per slot), at least kStackLdsMin of them.
constexpr int32_t kStackLdsMin = 8;
constexpr size_t kStackSlotBytes = (size_t)kBvhBlock * sizeof(uint32_t);

// Per-lane traversal stack of sort keys. The top entry lives in Trav::top and
// slot i >= 1 holds the entry below the i-th; slot 0 is a scratch slot, so
// pushes need no branches (stack_cap = depth bound + kStackSlack). Slots below `lds`
// are in LDS, slot i of the lane at base[i * kBvhBlock] (consecutive lanes,
// consecutive banks); a scene whose bound is deeper keeps the rest in a global
// overflow area (spill set: one wave-uniform branch per access otherwise).
template <bool kSpill>
struct Stack {
    static constexpr bool spill = kSpill;
    __attribute__((address_space(3))) uint32_t* base;  // this lane's slot 0
    uint32_t* ovf;     // this lane's slot `lds` in the overflow area (stride: grid lanes)
    uint32_t stride;
    int32_t lds;
};

template <class Stk>
__device__ __forceinline__ uint32_t stack_load(const Stk& S, int32_t i) {
    if constexpr (Stk::spill)
        if (i >= S.lds) return S.ovf[(size_t)(i - S.lds) * S.stride];
    return S.base[i * kBvhBlock];
}

template <class Stk>
__device__ __forceinline__ void stack_store(const Stk& S, int32_t i, uint32_t v) {
    if constexpr (Stk::spill) {
        if (i >= S.lds) {
            S.ovf[(size_t)(i - S.lds) * S.stride] = v;
            return;
        }
    }
    S.base[i * kBvhBlock] = v;
}

// Sort key of a hit child: the upper 16 bits of its entry distance (tn >= 0, so
// keys order like distances, to bf16 precision, and never exceed the true tn)
// over its 16-bit reference. ~0 = no entry.
__device__ __forceinline__ float key_tn(uint32_t key) { return __uint_as_float(key & 0xFFFF0000u); }

// Above every child reference and kBvhNone: neither is_trav nor is_leaf, not waiting
// for the shade phase (cur == kBvhNone) and not work in flight (cur < kBvhNone).
// kTravHit / kTravHitCam: marked by the shade phase / by the refill's camera-hit shading
// (told apart only by the material census of the profile build); is_marked covers both.
constexpr uint32_t kTravReady = kBvhNone + 1u, kTravHit = kBvhNone + 2u, kTravHitCam = kBvhNone + 3u;
__device__ __forceinline__ bool is_marked(uint32_t cur) { return cur > kTravReady; }
__device__ __forceinline__ bool is_trav(uint32_t cur) { return cur < kBvhLeafBit; }
__device__ __forceinline__ bool is_leaf(uint32_t cur) { return cur - kBvhLeafBit < kBvhNone - kBvhLeafBit; }

// Sphere.Hit of the sphere with geometry `g` in leaf slot `slot` under the
// any-order rule (above) with the hit kept as a slot: the
// original list index (the tie-break key, bidx) is read only on an exact tie
// t == closest, which is rare, so no index load sits on the path of every
// accepted hit (for scenes whose geometry stays in global memory it was a
// second dependent round trip after the sphere's own load).
__device__ __forceinline__ void test_geo(Trav& T, const SceneView& sv, const double4 g, int32_t slot, const D3& org,
                                         const D3& dir) {
    double h, d;
    quad(g, org, dir, T.a, h, d);
    if (d >= 0) {
        const double sq = sqrt_cr(d);
        const double r1 = div_root(h - sq, T.a, T.a_inv);
        const double t = r1 > 1e-6 ? r1 : div_root(h + sq, T.a, T.a_inv);
        // Accept with selects; only an exact tie with an earlier hit branches (to read
        // both list indices).
        const bool front = t > 1e-6;
        bool take = front & (t < T.closest);
        if (__builtin_expect(front & (t == T.closest) & (T.slot >= 0), 0)) take = sv.bidx[slot] < sv.bidx[T.slot];
        T.closest = take ? t : T.closest;
        T.slot = take ? slot : T.slot;
    }
}
__device__ __forceinline__ void test_slot(Trav& T, const SceneView& sv, int32_t slot, const D3& org, const D3& dir) {
    test_geo(T, sv, sv.bgeo[slot], slot, org, dir);
}

// Scene.Hit's FP64 setup for a new segment: a = |dir|^2 and its reciprocal,
// no hit yet, and the spheres kept out of the tree (tray_bvh.cpp, at most
// kBvhGlobals) tested first; a hit seeds the culling distance of the traversal.
template <class Opt = LaunchAsk>
__device__ __forceinline__ void trav_globals(Trav& T, const SceneView& sv, const D3& org, const D3& dir) {
    T.a = length_sq(dir);  // hoisted: same bits as per sphere
    T.a_inv = rcp_cr(T.a);
    T.closest = __builtin_inf();
    T.slot = -1;
    if constexpr (Opt::kOneGlobal) {
        test_slot(T, sv, sv.global_first, org, dir);
    } else {
#pragma unroll
        for (int32_t g = 0; g < kBvhGlobals; ++g)
            if (g < sv.n_global) test_slot(T, sv, sv.global_first + g, org, dir);
    }
}

// The direction lengths the FP32 slab test is conservative for (tray_bvh.cpp, "Range of
// the direction"): 1e-30 <= |dir|^2 <= 1e30; a NaN fails. Go sets a camera ray's length
// freely (pinhole: proportional to FocalLength; lens: about FocusDistance), and a
// caller's ray has any length. Whoever calls trav_begin32 answers for the range: the ray
// queries send any other ray through the linear scan (query_hit), the megakernel tests
// every tree sphere for such a camera ray (the refill), and the scatter step's rays are
// scattered ones, of order one (Metal and Dielectric start from Unit(direction),
// Lambertian from a unit normal plus a unit vector with NearZero replaced).
__device__ __forceinline__ bool slab_dir_ok(double a) { return a >= 1e-30 && a <= 1e30; }

// The FP32 traversal setup of a segment whose FP64 part (trav_globals) is done.
template <class Opt = LaunchAsk>
__device__ __forceinline__ void trav_begin32(Trav& T, const SceneView& sv, const D3& org, const D3& dir) {
    T.cur = Opt::kHasNodes || sv.n_nodes > 0 ? 0u : kBvhNone;  // the root
    T.sp = 0;
    T.top = ~0u;
    float dxf = (float)dir.x, dyf = (float)dir.y, dzf = (float)dir.z;
    if (__builtin_fabsf(dxf) < 1e-30f) dxf = 1e-30f;
    if (__builtin_fabsf(dyf) < 1e-30f) dyf = 1e-30f;
    if (__builtin_fabsf(dzf) < 1e-30f) dzf = 1e-30f;
    // ~1 ulp reciprocal: inside the padding's error budget (tray_bvh.cpp)
    const float ix = __builtin_amdgcn_rcpf(dxf);
    const float iy = __builtin_amdgcn_rcpf(dyf);
    const float iz = __builtin_amdgcn_rcpf(dzf);
    const float oix = (float)org.x * ix, oiy = (float)org.y * iy, oiz = (float)org.z * iz;
    T.ix = ix, T.iy = iy, T.iz = iz;
    T.oix = oix, T.oiy = oiy, T.oiz = oiz;
    // Bvh4Node::box[a][s]: the near plane is the low one when the ray runs up the axis.
    constexpr int32_t kPlane = 4 * kBvhWidth;  // bytes of one plane block (one float per child)
    T.near_x = ix < 0.0f ? kPlane : 0;
    T.near_y = 2 * kPlane + (iy < 0.0f ? kPlane : 0);
    T.near_z = 4 * kPlane + (iz < 0.0f ? kPlane : 0);
    T.tlim = f32_up(T.closest);
}

template <class Opt = LaunchAsk>
__device__ __forceinline__ void trav_begin(Trav& T, const SceneView& sv, const D3& org, const D3& dir) {
    T.tlim = __builtin_inff();
    trav_globals<Opt>(T, sv, org, dir);
    trav_begin32<Opt>(T, sv, org, dir);
}

// Push `key` if valid. The store is unconditional: with no push it writes
// slot sp, above the stack.
template <class Stk>
__device__ __forceinline__ void stack_push(Trav& T, const Stk& S, uint32_t key) {
    const bool valid = key != ~0u;
    stack_store(S, T.sp, T.top);
    T.top = valid ? key : T.top;
    T.sp += valid ? 1 : 0;
}

// Pop the next entry to visit: the top, or (when the top's box lies beyond the
// current closest hit, key_tn > tlim) the entry below it, read ahead in `below`.
// One cull at most and no further LDS round trip: an entry that is still
// beyond tlim is visited anyway, which the box tests and the any-order rule
// make harmless. Returns its reference, or kBvhNone.
template <class Stk>
__device__ __forceinline__ uint32_t stack_pop(Trav& T, const Stk& S, uint32_t below) {
    // Slot 0 always holds ~0 (written only by a push at depth 0, from the empty
    // top), so an empty stack pops ~0: key_tn(~0) is NaN (never culled) and
    // ~0 & 0xFFFF is kBvhNone. No emptiness branches: one divergent cull.
    uint32_t key = T.top;
    T.top = below;
    T.sp = max(T.sp - 1, 0);
    if (key_tn(key) > T.tlim) {
        key = T.top;
        T.sp = max(T.sp - 1, 0);
        T.top = stack_load(S, T.sp);  // the entry of depth sp sits in slot sp
        if (T.sp == 0 && key_tn(key) > T.tlim) key = ~0u;
    }
    return key & 0xFFFFu;
}


// One node visit: test the four child boxes, visit the nearest hit child next
// (an inner node or a leaf) and push the other hit children far-to-near. T.cur
// becomes the next reference (the lane's state).
template <class Stk>
__device__ __forceinline__ void trav_node(Trav& T, const SceneView& sv, const Stk& S, uint32_t& tested) {
    constexpr int32_t kPlane = 4 * kBvhWidth;  // far plane block = near ^ kPlane
    const char* nb = reinterpret_cast<const char*>(sv.nodes + T.cur);
    const uint32_t below = stack_load(S, max(T.sp - 1, 0));  // read ahead for a pop
    // Hit children: upper 16 bits of the entry distance | reference (tn >= 0, so
    // the keys order like the distances, to bf16 precision); anything else ~0.
    // An unused child's planes are (+inf, -inf): tn = +inf, never a hit.
    uint32_t key[kBvhWidth];
    tested = 0;
#pragma unroll
    for (int g = 0; g < kBvhWidth / 4; ++g) {  // four children per group of 16-B loads
        const float4 nx = *reinterpret_cast<const float4*>(nb + T.near_x + 16 * g);
        const float4 fx = *reinterpret_cast<const float4*>(nb + (T.near_x ^ kPlane) + 16 * g);
        const float4 ny = *reinterpret_cast<const float4*>(nb + T.near_y + 16 * g);
        const float4 fy = *reinterpret_cast<const float4*>(nb + (T.near_y ^ kPlane) + 16 * g);
        const float4 nz = *reinterpret_cast<const float4*>(nb + T.near_z + 16 * g);
        const float4 fz = *reinterpret_cast<const float4*>(nb + (T.near_z ^ kPlane) + 16 * g);
        const uint4 rf = *reinterpret_cast<const uint4*>(nb + 6 * kPlane + 16 * g);
        const uint32_t ref[4] = {rf.x, rf.y, rf.z, rf.w};
        const float nxa[4] = {nx.x, nx.y, nx.z, nx.w}, fxa[4] = {fx.x, fx.y, fx.z, fx.w};
        const float nya[4] = {ny.x, ny.y, ny.z, ny.w}, fya[4] = {fy.x, fy.y, fy.z, fy.w};
        const float nza[4] = {nz.x, nz.y, nz.z, nz.w}, fza[4] = {fz.x, fz.y, fz.z, fz.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // slab distances: t = plane * inv - org * inv
            const float tnx = __builtin_fmaf(nxa[k], T.ix, -T.oix), tfx = __builtin_fmaf(fxa[k], T.ix, -T.oix);
            const float tny = __builtin_fmaf(nya[k], T.iy, -T.oiy), tfy = __builtin_fmaf(fya[k], T.iy, -T.oiy);
            const float tnz = __builtin_fmaf(nza[k], T.iz, -T.oiz), tfz = __builtin_fmaf(fza[k], T.iz, -T.oiz);
            const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz), 0.0f);
            const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), T.tlim);
            key[4 * g + k] = tn <= tf ? ((__float_as_uint(tn) & 0xFFFF0000u) | ref[k]) : ~0u;
            tested += ref[k] != kBvhNone ? 1u : 0u;
        }
    }
#define TRAY_CX(i, j)                             \
    {                                             \
        const uint32_t lo_ = min(key[i], key[j]); \
        key[j] = max(key[i], key[j]);             \
        key[i] = lo_;                             \
    }
    if constexpr (kBvhWidth == 4) {
        TRAY_CX(0, 1) TRAY_CX(2, 3) TRAY_CX(0, 2) TRAY_CX(1, 3) TRAY_CX(1, 2)
    } else {  // 19-exchange network for 8
        TRAY_CX(0, 2) TRAY_CX(1, 3) TRAY_CX(4, 6) TRAY_CX(5, 7)
        TRAY_CX(0, 4) TRAY_CX(1, 5) TRAY_CX(2, 6) TRAY_CX(3, 7)
        TRAY_CX(0, 1) TRAY_CX(2, 3) TRAY_CX(4, 5) TRAY_CX(6, 7)
        TRAY_CX(2, 4) TRAY_CX(3, 5)
        TRAY_CX(1, 4) TRAY_CX(3, 6)
        TRAY_CX(1, 2) TRAY_CX(3, 4) TRAY_CX(5, 6)
    }
#undef TRAY_CX
    if (key[0] != ~0u) {
        if constexpr (kBvhWidth == 4 && !Stk::spill) {
            // Branch-free push of the hit children key[1..m] (sorted: invalid keys
            // ~0 come last) far-to-near: slots sp, sp+1, sp+2 are written
            // unconditionally; those above the new top are scratch (kStackSlack).
            const bool v1 = key[1] != ~0u, v2 = key[2] != ~0u, v3 = key[3] != ~0u;
            stack_store(S, T.sp, T.top);
            stack_store(S, T.sp + 1, v3 ? key[3] : key[2]);
            stack_store(S, T.sp + 2, key[2]);
            T.top = v1 ? key[1] : T.top;
            T.sp += (int32_t)v1 + (int32_t)v2 + (int32_t)v3;
        } else {
#pragma unroll
            for (int k = kBvhWidth - 1; k >= 1; --k) stack_push(T, S, key[k]);
        }
        T.cur = key[0] & 0xFFFFu;
    } else {
        T.cur = stack_pop(T, S, below);
    }
}

// The spheres of a multi-sphere leaf `ref` (FP64, any-order rule).
// Two spheres per step, both loads issued before either test: with the
// geometry in global memory (dense scenes) a leaf's spheres are then one
// L2 round trip, not one each. The second of an odd leaf reloads the first.
// At most kBvhLeafMax spheres per leaf: straight-line pairs (C5, 2-sphere
// leaves: -0.65 % against a counted loop).
__device__ __forceinline__ void leaf_spheres(Trav& T, const SceneView& sv, uint32_t ref, const D3& org, const D3& dir,
                                             uint32_t& tested) {
    const int32_t info = sv.leaves[ref & (kBvhLeafBit - 1u)];
    const int32_t first = info >> 3, cnt = info & 7;
#pragma unroll
    for (int32_t k = 0; k < kBvhLeafMax; k += 2) {
        if (k >= cnt) break;
        const int32_t s0 = first + k, s1 = k + 1 < cnt ? s0 + 1 : s0;
        const double4 g0 = sv.bgeo[s0], g1 = sv.bgeo[s1];
        test_geo(T, sv, g0, s0, org, dir);
        if (s1 != s0) test_geo(T, sv, g1, s1, org, dir);
        tested += s1 != s0 ? 2u : 1u;
    }
}

// Test the spheres of leaf T.cur (FP64, any-order rule), then pop the next entry.
template <class Opt = LaunchAsk, class Stk>
__device__ __forceinline__ void trav_leaf(Trav& T, const SceneView& sv, const Stk& S, const D3& org,
                                              const D3& dir, uint32_t& tested) {
    const uint32_t below = stack_load(S, max(T.sp - 1, 0));  // read ahead for the pop
    if (Opt::kSingleLeaf || sv.single) {  // one sphere per leaf: the leaf index is its slot (no leaf table, no loop)
        test_slot(T, sv, (int32_t)(T.cur & (kBvhLeafBit - 1u)), org, dir);
        tested = 1;
    } else {
        tested = 0;
        leaf_spheres(T, sv, T.cur, org, dir, tested);
    }
    T.tlim = f32_up(T.closest);
    T.cur = stack_pop(T, S, below);
}

}  // namespace tray
