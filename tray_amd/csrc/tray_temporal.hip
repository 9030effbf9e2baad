// tray_temporal.hip — include/tray_temporal.h for gfx950: the temporal reprojection
// step. One launch traces each pixel's centre ray (query_hit, the queries' Scene.Hit),
// projects the hit into the previous camera, gathers the history there, folds the new
// frame into it and counts the record's two sums. A second instance of the same kernel
// (include/tray_temporal_variance.h) carries M2 with the colour and writes the variance
// of the mean in the same launch; a small streaming kernel writes that variance again
// for a list of pixels, or for the whole frame, after a fold from outside the step. A
// third and a fourth instance (include/tray_temporal_motion.h) follow a hit point with its
// sphere when the spheres have moved since the history was made, with or without M2.
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
//
// The entry points of the three headers are at the end of the file: one function
// (temporal_step) checks, fills and launches any instance of the step; the scene comes
// through tray_scene.hpp, the argument checks from tray_check.hpp.

#include <string.h>

#include <cmath>
#include <limits>

#include "../../include/tray_temporal.h"
#include "../../include/tray_temporal_motion.h"
#include "../../include/tray_temporal_variance.h"
#include "tray_query_device.hpp"
#include "tray_scene.hpp"
#include "tray_stream.hpp"

namespace tray {

constexpr uint32_t kTileX = 32, kTileY = kQueryBlock / kTileX;

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
    // The M2 instance alone (last, so that the plain instance's arguments stay where they were):
    const double* history_m2;
    double* out_m2;
    double* variance;  // nullable
    // The motion instances alone (after those, for the same reason):
    const double* prev_geometry;  // n x {cx, cy, cz, radius}, list order; null only where no ray can hit
    double* motion;               // nullable, height x width x 2
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

// kM2: the step of include/tray_temporal_variance.h. What it adds reads nothing the plain step
// decides on and feeds nothing back into it, so colour, age, index, depth and the record are
// the plain instance's.
//
// kMotion: the step of include/tray_temporal_motion.h. Section 2b alone differs: the target of
// a hit on a sphere that has moved since the history was made is the same surface point on the
// previous sphere. With both flags false the code is the plain step's, instruction for instruction.
template <bool kM2, bool kMotion>
__global__ __launch_bounds__(kQueryBlock) void temporal_step_kernel(TemporalLaunch L) {
    __shared__ unsigned long long red[2][kQueryBlock / 64];
    static_assert(sizeof(red) <= kTemporalStaticLds, "query_takes_tree counts this kernel's static LDS");
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
        D3 m2 = d3(0, 0, 0);  // kM2: out.m2, 0.0 for a fresh pixel
        fresh = true;
        age = 1;
        if (a.history.colour) {
            // b. the target, c. its projection into the previous camera
            const PrevCamera& P = a.prev;
            D3 e = d;
            if (idx >= 0) {
                D3 Q = add(o, smul(d, t));
                if constexpr (kMotion) {
                    // The hit sphere as the scene holds it now (by slot on the tree path, by list
                    // index on the scan path) and as it was, by list index: data dependent, so
                    // through the caches like the taps.
                    const KernelParams& pk = kp_fresh();
                    const double4 g = h.tree ? pk.bgeo[h.ref] : pk.geo[h.ref];
                    const double R = h.tree ? pk.bmat[h.ref].radius : pk.mat[h.ref].radius;
                    const double* pg = a.prev_geometry + (size_t)idx * 4;
                    const double pcx = pg[0], pcy = pg[1], pcz = pg[2], pR = pg[3];
                    if (!(pcx == g.x && pcy == g.y && pcz == g.z && pR == R)) {
                        const D3 m = sdiv(sub(Q, d3(g.x, g.y, g.z)), R);  // ray/objects.go:100
                        Q = add(d3(pcx, pcy, pcz), smul(m, pR));
                    }
                }
                e = sub(Q, ld3(P.position));
            }
            const D3 c0 = ld3(P.c0), pxv = ld3(P.pixel_x), pyv = ld3(P.pixel_y);
            const double z = dot(ld3(P.n), e) / P.n_c0;
            const D3 g = sub(sdiv(e, z), c0);
            const double u = dot(g, pxv) / P.xx, v = dot(g, pyv) / P.yy;
            const bool in_range = z > 0.0 && u > -1.0 && u < (double)width && v > -1.0 && v < (double)height;
            if constexpr (kMotion) {
                if (a.motion) {
                    double* mv = a.motion + pix * 2;
                    mv[0] = in_range ? u - (double)x : __builtin_nan("");
                    mv[1] = in_range ? v - (double)y : __builtin_nan("");
                }
            }
            if (in_range) {
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
                D3 H = d3(0, 0, 0), M = d3(0, 0, 0);
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
                    if constexpr (kM2) {
                        const double* m = a.history_m2 + q * 3;
                        M = d3(M.x + w[j] * m[0], M.y + w[j] * m[1], M.z + w[j] * m[2]);
                    }
                }
                // e. the fold
                if (W > 0.0) {
                    const D3 hm = sdiv(H, W);
                    const int32_t cap = a.max_history - 1;
                    const int32_t k = (A < cap ? A : cap) + 1;
                    const double dk = (double)k;
                    const D3 X = colour;
                    colour = d3(hm.x + (colour.x - hm.x) / dk, hm.y + (colour.y - hm.y) / dk,
                                hm.z + (colour.z - hm.z) / dk);
                    if constexpr (kM2) {
                        // the gathered M2, scaled to a history of n0 = k - 1 samples, then Welford's update
                        D3 m = sdiv(M, W);
                        const int32_t n0 = k - 1;
                        if (A > n0) m = smul(m, (double)(n0 - 1) / (double)(A - 1));
                        m2 = d3(m.x + (X.x - hm.x) * (X.x - colour.x), m.y + (X.y - hm.y) * (X.y - colour.y),
                                m.z + (X.z - hm.z) * (X.z - colour.z));
                    }
                    age = k;
                    fresh = false;
                }
            }
        }
        double* co = a.out.colour + pix * 3;
        co[0] = colour.x, co[1] = colour.y, co[2] = colour.z;
        a.out.age[pix] = age;
        if constexpr (kM2) {
            double* mo = a.out_m2 + pix * 3;
            mo[0] = m2.x, mo[1] = m2.y, mo[2] = m2.z;
            if (a.variance) {
                double* vo = a.variance + pix * 3;
                if (age < 2) {
                    vo[0] = vo[1] = vo[2] = __builtin_inf();
                } else {
                    const double D = (double)age * (double)(age - 1);
                    vo[0] = m2.x / D, vo[1] = m2.y / D, vo[2] = m2.z / D;
                }
            }
        }
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

static tray_temporal_state plain_state(const tray_temporal_var_state& s) {
    return tray_temporal_state{s.colour, s.age, s.index, s.depth, s.width, s.height};
}
static tray_temporal_var_state without_m2(const tray_temporal_state& s) {
    return tray_temporal_var_state{s.colour, nullptr, s.age, s.index, s.depth, s.width, s.height};
}

// What tray_temporal_motion_step_async alone takes.
struct MotionArgs {
    const double* prev_geometry;
    int32_t n_spheres;
    double* plane;  // the motion plane, nullable
};

// All steps (the plain ones without the M2 and variance rows): the states come as
// tray_temporal_var_state, a plain state widened with a null m2. One reprojection step over
// the out->width x out->height frame; `history` and `prev` both null: the first frame.
// `mo` non-null: the step of include/tray_temporal_motion.h.
static int temporal_step(tray_scene_t sc, const tray_camera* cam, const tray_camera* prev,
                         const tray_temporal_params* tp, const double* frame_device,
                         const tray_temporal_var_state* history, const tray_temporal_var_state* out, bool with_m2,
                         double* variance_device, tray_temporal_record* record_device, void* stream_arg,
                         const MotionArgs* mo = nullptr) {
    if (!sc) return fail(TRAY_ERR_INVALID_ARGUMENT, "null scene");
    if (!cam) return fail(TRAY_ERR_INVALID_ARGUMENT, "null camera");
    if (!tp) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params");
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null state (out)");
    if ((history == nullptr) != (prev == nullptr))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "history and prev_camera must both be given or both be null");
    if (out->width < 0 || out->height < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or height");
    if (history && (history->width != out->width || history->height != out->height))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "history and out differ in width or height");
    if (tp->max_history < 1 || tp->max_history > (1 << 30))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "max_history must be in 1 .. 2^30");
    if (tp->flags & ~TRAY_FLAG_LINEAR_SCAN)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "unknown flags (only TRAY_FLAG_LINEAR_SCAN applies)");
    if (!(std::isfinite(tp->depth_tolerance) && tp->depth_tolerance >= 0.0))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "depth_tolerance must be finite and >= 0");
    if (!(std::isfinite(tp->snap) && tp->snap >= 0.0 && tp->snap < 0.5))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "snap must be finite, >= 0 and < 0.5");
    if (tp->reserved != 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "reserved must be 0");
    const int64_t image = (int64_t)out->width * (int64_t)out->height;
    if (image > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one state");
    if (image == 0) return TRAY_OK;
    // The spans: outputs first (the first n_out; the variance and the record nullable), then what is only read.
    const size_t px = (size_t)image;
    Span spans[15];
    int n = 0;
    uint32_t nullable = 0;
    spans[n++] = {out->colour, px * 24, 8, "out.colour"};
    if (with_m2) spans[n++] = {out->m2, px * 24, 8, "out.m2"};
    spans[n++] = {out->age, px * 4, 4, "out.age"};
    spans[n++] = {out->index, px * 4, 4, "out.index"};
    spans[n++] = {out->depth, px * 8, 8, "out.depth"};
    if (with_m2) {
        nullable |= 1u << n;
        spans[n++] = {variance_device, px * 24, 8, "the variance"};
    }
    nullable |= 1u << n;
    spans[n++] = {record_device, sizeof(tray_temporal_record), 8, "the record"};
    if (mo) {
        nullable |= 1u << n;
        spans[n++] = {mo->plane, px * 16, 8, "the motion plane"};
    }
    const int n_out = n;
    spans[n++] = {frame_device, px * 24, 8, "the frame"};
    if (mo && history && mo->n_spheres > 0)  // ignored on the first frame; never read without a sphere to hit
        spans[n++] = {mo->prev_geometry, (size_t)mo->n_spheres * 32, 8, "the previous geometry"};
    if (history) {
        spans[n++] = {history->colour, px * 24, 8, "history.colour"};
        if (with_m2) spans[n++] = {history->m2, px * 24, 8, "history.m2"};
        spans[n++] = {history->age, px * 4, 4, "history.age"};
        spans[n++] = {history->index, px * 4, 4, "history.index"};
        spans[n++] = {history->depth, px * 8, 8, "history.depth"};
    }
    int rc = check_nulls(spans, n, nullable);
    if (!rc) rc = check_alignment(spans, n);
    if (!rc) rc = check_overlaps(spans, n, n_out);
    if (rc) return rc;
    if (mo && mo->n_spheres != sc->n)  // the first look at the scene
        return fail(TRAY_ERR_INVALID_ARGUMENT, "n_spheres differs from the scene's sphere count");
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    camera_params(cam, k);
    k.width = out->width;
    k.height = out->height;
    k.rows = out->height;
    size_t lds = 0;
    // Stacks that do not fit beside the reduction: the scan (query_takes_tree).
    const QueryArgs q = query_args(k, wants_bvh(sc, tp->flags), sc->bvh_bound, nullptr, 0, lds, kQueryTemporal);
    TemporalArgs a{};
    a.frame = frame_device;
    a.out = plain_state(*out);
    a.record = record_device;
    a.depth_tolerance = tp->depth_tolerance;
    a.snap = tp->snap;
    a.max_history = tp->max_history;
    a.out_m2 = out->m2;  // null in the plain step, as history's m2 and the variance
    a.variance = variance_device;
    if (history && tp->max_history > 1) {  // max_history 1: the frame itself (the header, section 3)
        a.history = plain_state(*history);
        a.history_m2 = history->m2;
        if (mo) a.prev_geometry = mo->prev_geometry, a.motion = mo->plane;
        // The previous camera: what does not depend on the pixel, in the header's operations and order.
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
    a.tiles_x = ((uint32_t)out->width + kTileX - 1u) / kTileX;
    const uint32_t tiles_y = ((uint32_t)out->height + kTileY - 1u) / kTileY;  // tiles_x x tiles_y <= 2^26 + 2^28
    const hipStream_t stream = static_cast<hipStream_t>(stream_arg);
    TRAY_HIP(hipSetDevice(sc->device));
    if (record_device) TRAY_HIP(hipMemsetAsync(record_device, 0, sizeof(*record_device), stream));
    const dim3 grid(a.tiles_x * tiles_y), block(kQueryBlock);
    const TemporalLaunch launch{k, q, a};
    if (mo && with_m2) hipLaunchKernelGGL((temporal_step_kernel<true, true>), grid, block, lds, stream, launch);
    else if (mo) hipLaunchKernelGGL((temporal_step_kernel<false, true>), grid, block, lds, stream, launch);
    else if (with_m2) hipLaunchKernelGGL((temporal_step_kernel<true, false>), grid, block, lds, stream, launch);
    else hipLaunchKernelGGL((temporal_step_kernel<false, false>), grid, block, lds, stream, launch);
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

// ---- include/tray_temporal_variance.h section 3: the variance of the mean from (m2, age) ----
//
// Streaming, 32 bytes read and 24 written per pixel. The whole frame is read and written in
// tray_stream.hpp's pattern (a wave covers 1 KiB of consecutive bytes per instruction), each
// element dividing by the D of pixel e / 3 from a gathered age, as the selection's metric pass
// does. A list is one entry per lane: its pixel's 3 + 1 values gathered, 3 scattered.
struct VarianceArgs {
    const double* m2;
    const int32_t* age;
    const uint32_t* pixels;  // null: every pixel
    double* variance;
    size_t elems, chunks;    // whole frame: image_pixels x 3 doubles in chunks of kBlockElems
    uint32_t n_pixels, image_pixels;
};

__device__ __forceinline__ double variance_of_mean(double m2, int32_t n) {
    if (n < 2) return __builtin_inf();
    return m2 / ((double)n * (double)(n - 1));
}

__global__ __launch_bounds__(kThreads) void temporal_variance_frame_kernel(const VarianceArgs A) {
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    for (size_t chunk = blockIdx.x; chunk < A.chunks; chunk += gridDim.x) {
        const size_t wave_base = chunk * kBlockElems + (size_t)wave * kWaveElems;
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            const size_t at = wave_base + (size_t)j * kRowElems + 2 * (size_t)lane;
            if (at >= A.elems) continue;
            double m0 = 0.0, m1 = 0.0;
            load_pair(A.m2, at, A.elems, m0, m1);
            const double v0 = variance_of_mean(m0, A.age[at / 3]);
            const double v1 = at + 1 < A.elems ? variance_of_mean(m1, A.age[(at + 1) / 3]) : 0.0;
            store_pair(A.variance, at, A.elems, v0, v1);
        }
    }
}

__global__ __launch_bounds__(kThreads) void temporal_variance_list_kernel(const VarianceArgs A) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= A.n_pixels) return;
    const uint32_t pix = A.pixels[i];
    if (pix >= A.image_pixels) return;  // a bad entry is skipped
    const int32_t n = A.age[pix];
    const double* m = A.m2 + (size_t)pix * 3;
    double* v = A.variance + (size_t)pix * 3;
    const double m0 = m[0], m1 = m[1], m2 = m[2];
    v[0] = variance_of_mean(m0, n), v[1] = variance_of_mean(m1, n), v[2] = variance_of_mean(m2, n);
}

}  // namespace tray

using namespace tray;

#pragma GCC visibility push(default)
extern "C" {

// ---- temporal reprojection (include/tray_temporal.h) -----------------------------
int32_t tray_temporal_version(void) { return TRAY_TEMPORAL_VERSION; }

int tray_temporal_default_params(tray_temporal_params* out) {
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params (out)");
    out->max_history = 32;       // tools/temporal_sweep.py, DESIGN.md 8q
    out->flags = 0;
    out->depth_tolerance = 0.1;  // the same sweep
    out->snap = 0x1.0p-20;
    out->reserved = 0;
    return TRAY_OK;
}

int tray_temporal_step_async(tray_scene_t sc, const tray_camera* cam, const tray_camera* prev,
                             const tray_temporal_params* tp, const double* frame_device,
                             const tray_temporal_state* history, const tray_temporal_state* out,
                             tray_temporal_record* record_device, void* stream) {
    tray_temporal_var_state h{}, o{};
    if (history) h = without_m2(*history);
    if (out) o = without_m2(*out);
    return temporal_step(sc, cam, prev, tp, frame_device, history ? &h : nullptr, out ? &o : nullptr, false, nullptr,
                         record_device, stream);
}

// ---- temporal reprojection with M2 (include/tray_temporal_variance.h) --------------
int32_t tray_temporal_var_version(void) { return TRAY_TEMPORAL_VAR_VERSION; }

int tray_temporal_var_step_async(tray_scene_t sc, const tray_camera* cam, const tray_camera* prev,
                                 const tray_temporal_params* tp, const double* frame_device,
                                 const tray_temporal_var_state* history, const tray_temporal_var_state* out,
                                 double* variance_device, tray_temporal_record* record_device, void* stream) {
    return temporal_step(sc, cam, prev, tp, frame_device, history, out, true, variance_device, record_device, stream);
}

// ---- temporal reprojection across scene updates (include/tray_temporal_motion.h) ----
int32_t tray_temporal_motion_version(void) { return TRAY_TEMPORAL_MOTION_VERSION; }

int tray_temporal_motion_step_async(tray_scene_t sc, const tray_camera* cam, const tray_camera* prev,
                                    const double* prev_geometry_device, int32_t n_spheres,
                                    const tray_temporal_params* tp, const double* frame_device,
                                    const tray_temporal_var_state* history, const tray_temporal_var_state* out,
                                    double* variance_device, double* motion_device,
                                    tray_temporal_record* record_device, void* stream) {
    const bool with_m2 = out && out->m2;
    if (out && history && (history->m2 != nullptr) != with_m2)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "the m2 planes of history and out must all be given or all be null");
    if (out && variance_device && !with_m2)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "a variance plane needs the m2 planes");
    const MotionArgs mo{prev_geometry_device, n_spheres, motion_device};
    return temporal_step(sc, cam, prev, tp, frame_device, history, out, with_m2, variance_device, record_device,
                         stream, &mo);
}

// Section 3: the variance of the mean of the n_pixels listed pixels (entries beyond the image
// skipped), or of every pixel when `pixels_device` is null.
int tray_temporal_var_variance_async(const tray_temporal_var_state* state, const uint32_t* pixels_device,
                                     int64_t n_pixels, double* variance_device, int32_t device, void* stream) {
    if (!state) return fail(TRAY_ERR_INVALID_ARGUMENT, "null state");
    if (state->width < 0 || state->height < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or height");
    if (pixels_device && n_pixels < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative n_pixels");
    const int64_t image = (int64_t)state->width * (int64_t)state->height;
    if (image > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one state");
    if (pixels_device && n_pixels > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "n_pixels exceeds 2^31 - 1");
    if (image == 0 || (pixels_device && n_pixels == 0)) return TRAY_OK;
    const size_t px = (size_t)image;
    const Span spans[4] = {{variance_device, px * 24, 8, "the variance"},
                           {state->m2, px * 24, 8, "m2"},
                           {state->age, px * 4, 4, "age"},
                           {pixels_device, pixels_device ? (size_t)n_pixels * 4 : 0, 4, "the pixel list"}};
    int rc = check_nulls(spans, 4, 1u << 3);
    if (!rc) rc = check_alignment(spans, 4);
    if (!rc) rc = check_overlaps(spans, 4, 1);
    if (!rc) rc = device_usable(device);
    if (rc) return rc;
    VarianceArgs a{};
    a.m2 = state->m2;
    a.age = state->age;
    a.pixels = pixels_device;
    a.variance = variance_device;
    a.image_pixels = (uint32_t)image;
    TRAY_HIP(hipSetDevice(device));
    if (pixels_device) {
        a.n_pixels = (uint32_t)n_pixels;
        const uint32_t blocks = (a.n_pixels + (uint32_t)kThreads - 1u) / (uint32_t)kThreads;  // <= 2^23
        hipLaunchKernelGGL(temporal_variance_list_kernel, dim3(blocks), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), a);
    } else {
        a.elems = (size_t)a.image_pixels * 3;
        a.chunks = (a.elems + kBlockElems - 1) / kBlockElems;
        const int64_t grid = (int64_t)a.chunks < kMaxGrid ? (int64_t)a.chunks : kMaxGrid;
        hipLaunchKernelGGL(temporal_variance_frame_kernel, dim3((uint32_t)grid), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), a);
    }
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

}  // extern "C"
#pragma GCC visibility pop
