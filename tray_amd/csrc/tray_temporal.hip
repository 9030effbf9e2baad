// tray_temporal.hip — include/tray_temporal.h for gfx950: the temporal reprojection
// step. One launch traces each pixel's centre ray (query_hit, the queries' Scene.Hit),
// projects the hit into the previous camera, gathers the history there, folds the new
// frame into it and counts the record's two sums.
//
// The traversal is tray_query_device.hpp's over tray_device.hpp, the megakernel's own
// arithmetic; the projection and the fold are plain FP64 in the header's order. Compiled
// with -ffp-contract=off like every other unit; the public header is the contract.
//
// A 256-lane workgroup is a 32 x 8 pixel tile (a wave: two rows of 32), not 256
// consecutive pixels: under a small camera step the taps of a wave then fall into a
// patch of about 33 x 3 history pixels, few cache lines of each plane, and the lanes'
// traversals stay together as in aov_kernel. The taps depend on the data (the hit), so
// the history is read through the caches, not staged; only the traversal stacks and the
// 64 bytes of the record's reduction live in LDS.

#include <limits>

#include "../../include/tray_temporal.h"
#include "tray_internal.hpp"
#include "tray_query_device.hpp"

namespace tray {

constexpr uint32_t kTileX = 32, kTileY = kQueryBlock / kTileX;
constexpr size_t kTemporalStaticLds = 64;  // red[2][4] below

// The previous camera as the projection needs it: what does not depend on the pixel is
// worked out once on the host (same operations, same order, no contraction there either).
struct PrevCamera {
    double position[3];
    double pixel_x[3], pixel_y[3];
    double n[3];    // cross(pixel_x, pixel_y)
    double c0[3];   // pixel00 - position
    double n_c0;    // dot(n, c0)
    double xx, yy;  // dot(pixel_x, pixel_x), dot(pixel_y, pixel_y)
};

struct TemporalArgs {
    const double* frame;
    tray_temporal_state history;  // colour null: every pixel is fresh
    tray_temporal_state out;
    tray_temporal_record* record;  // nullable
    PrevCamera prev;
    double depth_tolerance, snap;
    int32_t max_history;
    uint32_t tiles_x;  // 32 x 8 tiles per row of tiles: ceil(width / 32)
};

// The kernel's one argument: KernelParams first, where kp_fresh() reads it.
struct TemporalLaunch {
    KernelParams p;
    QueryArgs q;
    TemporalArgs a;
};
static_assert(offsetof(TemporalLaunch, p) == 0, "kp_fresh reads KernelParams at the start of the kernel arguments");

// kp_fresh for the step's arguments: read where they are used, not held across the traversal.
__device__ __forceinline__ const TemporalArgs& ta_fresh() {
    typedef const __attribute__((address_space(4))) TemporalLaunch* ConstLaunch;
    ConstLaunch l = (ConstLaunch)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(l));  // opaque: no load through l is hoisted above this point
    return ((const TemporalLaunch*)l)->a;
}

// Cross (ray/vec3.go:70-72); host and device.
__host__ __device__ inline void cross3(const double u[3], const double v[3], double out[3]) {
    out[0] = u[1] * v[2] - u[2] * v[1];
    out[1] = u[2] * v[0] - u[0] * v[2];
    out[2] = u[0] * v[1] - u[1] * v[0];
}
__host__ __device__ inline double dot3(const double u[3], const double v[3]) {
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
}

__global__ __launch_bounds__(kQueryBlock) void temporal_step_kernel(TemporalLaunch L) {
    __shared__ unsigned long long red[2][kQueryBlock / 64];
    const KernelParams& p = L.p;
    const uint32_t width = (uint32_t)p.width, height = (uint32_t)p.height;
    const uint32_t tile_y = blockIdx.x / L.a.tiles_x, tile_x = blockIdx.x - tile_y * L.a.tiles_x;
    const uint32_t x = tile_x * kTileX + (threadIdx.x & (kTileX - 1u)), y = tile_y * kTileY + threadIdx.x / kTileX;
    const bool live = x < width && y < height;  // the frame's right and lower edge
    bool fresh = false;
    int32_t age = 0;
    if (live) {
        const size_t pix = (size_t)y * width + x;  // < width x height <= 2^31 - 1
        const SceneView sv = scene_view(p);
        const QStack S = lane_stack();
        // a. the centre ray: get_ray's sample point with zero offsets, no lens
        D3 o, d;
        {
            const KernelParams& pk = kp_fresh();
            o = ld3(pk.cam.position);
            const D3 s = add(add(ld3(pk.cam.pixel00), smul(ld3(pk.cam.pixel_x), (double)x)),
                             smul(ld3(pk.cam.pixel_y), (double)y));
            d = sub(s, o);
        }
        const QHit h = query_hit(sv, S, L.q, o, d, __builtin_inf());
        const int32_t idx = h.ref < 0 ? -1 : (h.tree ? sv.bidx[h.ref] : h.ref);
        const double t = h.ref < 0 ? __builtin_inf() : h.t;
        const TemporalArgs& a = ta_fresh();
        a.out.index[pix] = idx;
        a.out.depth[pix] = t;
        const double* xin = a.frame + pix * 3;
        D3 colour = d3(xin[0], xin[1], xin[2]);
        fresh = true;
        age = 1;
        if (a.history.colour) {
            // b. the target, c. its projection into the previous camera
            const PrevCamera& P = a.prev;
            const D3 e = idx >= 0 ? sub(add(o, smul(d, t)), ld3(P.position)) : d;
            const D3 c0 = ld3(P.c0), pxv = ld3(P.pixel_x), pyv = ld3(P.pixel_y);
            const double z = dot(ld3(P.n), e) / P.n_c0;
            const D3 g = sub(sdiv(e, z), c0);
            const double u = dot(g, pxv) / P.xx, v = dot(g, pyv) / P.yy;
            if (z > 0.0 && u > -1.0 && u < (double)width && v > -1.0 && v < (double)height) {
                // d. the taps: the snapped case is the bilinear one with weights 1, 0, 0, 0 at (xr, yr)
                const double xr = __builtin_floor(u + 0.5), yr = __builtin_floor(v + 0.5);
                const bool snapped = __builtin_fabs(u - xr) <= a.snap && __builtin_fabs(v - yr) <= a.snap;
                const double x0 = snapped ? xr : __builtin_floor(u), y0 = snapped ? yr : __builtin_floor(v);
                const double fa = u - x0, fb = v - y0;
                double w[4] = {(1.0 - fa) * (1.0 - fb), fa * (1.0 - fb), (1.0 - fa) * fb, fa * fb};
                if (snapped) w[0] = 1.0, w[1] = 0.0, w[2] = 0.0, w[3] = 0.0;
                const int64_t ix0 = (int64_t)x0, iy0 = (int64_t)y0;  // in [-1, width] x [-1, height]: in range
                const double bound = a.depth_tolerance * z;
                double W = 0.0;
                D3 H = d3(0, 0, 0);
                int32_t A = std::numeric_limits<int32_t>::max();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t tx = ix0 + (j & 1), ty = iy0 + (j >> 1);
                    if (!(w[j] > 0.0) || tx < 0 || tx >= (int64_t)width || ty < 0 || ty >= (int64_t)height) continue;
                    const size_t q = (size_t)ty * width + (size_t)tx;  // inside the history planes
                    const int32_t ha = a.history.age[q];
                    if (ha < 1 || a.history.index[q] != idx) continue;
                    if (idx >= 0 && !(__builtin_fabs(a.history.depth[q] - z) <= bound)) continue;
                    const double* c = a.history.colour + q * 3;
                    const double c0x = c[0], c1 = c[1], c2 = c[2];
                    if (c0x != c0x || c1 != c1 || c2 != c2) continue;
                    W = W + w[j];
                    H = d3(H.x + w[j] * c0x, H.y + w[j] * c1, H.z + w[j] * c2);
                    A = ha < A ? ha : A;
                }
                // e. the fold
                if (W > 0.0) {
                    const D3 hm = sdiv(H, W);
                    const int32_t cap = a.max_history - 1;
                    const int32_t k = (A < cap ? A : cap) + 1;
                    const double dk = (double)k;
                    colour = d3(hm.x + (colour.x - hm.x) / dk, hm.y + (colour.y - hm.y) / dk,
                                hm.z + (colour.z - hm.z) / dk);
                    age = k;
                    fresh = false;
                }
            }
        }
        double* co = a.out.colour + pix * 3;
        co[0] = colour.x, co[1] = colour.y, co[2] = colour.z;
        a.out.age[pix] = age;
    }
    // The record: a wave reduction, then one atomic add per workgroup and sum.
    tray_temporal_record* const record = L.a.record;
    if (!record) return;  // uniform
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long n_fresh = (unsigned long long)__popcll(__ballot(fresh));
    unsigned long long ages = (unsigned long long)age;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ages += __shfl_xor(ages, off, 64);
    if (lane == 0) red[0][wave] = n_fresh, red[1][wave] = ages;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long f = 0, s = 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kQueryBlock / 64u; ++k) f += red[0][k], s += red[1][k];
        if (f) atomicAdd(reinterpret_cast<unsigned long long*>(&record->fresh), f);
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(&record->age_sum), s);
    }
}

hipError_t launch_temporal_step(KernelParams p, bool use_bvh, double bound, const tray_camera* prev,
                                const tray_temporal_params& tp, const double* frame,
                                const tray_temporal_state* history, const tray_temporal_state& out,
                                tray_temporal_record* record, hipStream_t stream) {
    if (out.width <= 0 || out.height <= 0) return hipSuccess;
    size_t lds = 0;
    QueryArgs q = query_args(p, use_bvh, bound, nullptr, 0, lds);
    if (lds + kTemporalStaticLds > kQueryLdsMax) {  // stacks that do not fit beside the reduction: the scan
        q.use_bvh = 0;
        lds = 0;
    }
    TemporalArgs a{};
    a.frame = frame;
    a.out = out;
    a.record = record;
    a.depth_tolerance = tp.depth_tolerance;
    a.snap = tp.snap;
    a.max_history = tp.max_history;
    if (history && prev && tp.max_history > 1) {  // max_history 1: the frame itself (the header, section 3)
        a.history = *history;
        PrevCamera& P = a.prev;
        for (int c = 0; c < 3; ++c) {
            P.position[c] = prev->position[c];
            P.pixel_x[c] = prev->pixel_x[c];
            P.pixel_y[c] = prev->pixel_y[c];
            P.c0[c] = prev->pixel00[c] - prev->position[c];
        }
        cross3(P.pixel_x, P.pixel_y, P.n);
        P.n_c0 = dot3(P.n, P.c0);
        P.xx = dot3(P.pixel_x, P.pixel_x);
        P.yy = dot3(P.pixel_y, P.pixel_y);
    }
    a.tiles_x = ((uint32_t)out.width + kTileX - 1u) / kTileX;
    const uint32_t tiles_y = ((uint32_t)out.height + kTileY - 1u) / kTileY;  // tiles_x x tiles_y <= 2^26 + 2^28
    hipError_t e = hipSuccess;
    if (record) e = hipMemsetAsync(record, 0, sizeof(*record), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(temporal_step_kernel, dim3(a.tiles_x * tiles_y), dim3(kQueryBlock), lds, stream,
                       TemporalLaunch{p, q, a});
    return hipGetLastError();
}

}  // namespace tray
