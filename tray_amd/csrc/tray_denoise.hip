// tray_denoise.hip — include/tray_denoise.h: the edge-avoiding a-trous denoiser
// guided by the first-hit feature buffers, one gfx950 launch per level.
//
// The header is the contract: every value is a fixed sequence of correctly
// rounded FP64 operations in the header's order (the file is built with
// -ffp-contract=off like the rest of the library; `/` on doubles lowers to the
// correctly rounded v_div_scale / v_rcp / v_div_fmas / v_div_fixup sequence).
//
// Tiling. At spacing s the pixels with equal (x mod s, y mod s) form a dense
// sub-image on which the stencil is an ordinary 5x5. A workgroup of 256 lanes
// owns a 32x8 tile of one such sub-image: it stages the 36x12 points of the
// tile and its 2-point halo once into LDS (colour, normal, depth and 1/depth as
// eight planes of doubles, 27 KiB) and filters from there. A half-wave reads 32
// consecutive doubles of one plane row per ds_read_b64, which touches each of
// the 32 8-byte bank pairs once: no bank conflicts at any tap offset (and the
// counter reads 0: DESIGN.md 8i).
//
// A point outside the image is staged with a NaN in its first colour plane: its
// x_c is then NaN, b(x_c) = 0 and the tap is skipped by the same `w > 0` test
// that skips every zero-weight tap.
//
// -DTRAY_DENOISE_GLOBAL_TAPS builds the straightforward variant instead (one
// lane per pixel in image order, the 25 taps read from global memory through
// the caches); `make -C tray_amd denoise_ab` links it into a second library for
// tools/denoise_bench.py. Same bits, measured slower.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/tray_denoise.h"
#include "../../include/tray_progressive.h"
#include "tray_check.hpp"

namespace tray {
namespace {

constexpr int kTileX = 32, kTileY = 8, kHalo = 2;
constexpr int kLdsX = kTileX + 2 * kHalo, kLdsY = kTileY + 2 * kHalo;
[[maybe_unused]] constexpr int kLdsPoints = kLdsX * kLdsY;
constexpr int kThreads = kTileX * kTileY;
constexpr double kAlbedoFloor = 0.0009765625;  // 2^-10
constexpr int64_t kMaxBlocks = (1ll << 24) - 1;  // x 256 lanes: a launch stays below 2^32 work-items

struct DenoiseLevel {
    const double* in;          // rows x width x 3: the colour (level 0) or the previous level
    const double* demodulate;  // albedo when this level's loads divide by m(albedo), else null
    const double* remodulate;  // albedo when this level's store multiplies by m(albedo), else null
    const double* normal;      // nullable
    const double* depth;       // nullable
    double* out;
    int32_t width, rows, s;
    int32_t tiles_x, tiles_y, lattices_x;  // tiles per sub-image, sub-images per row of sub-images
    double q_c, q_n, q_z;
};

__device__ __forceinline__ double edge_stop(double x) {
    const double y = 1.0 - x;
    return x < 1.0 ? y * y : 0.0;
}

__device__ __forceinline__ double albedo_floor(double a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }

__device__ __forceinline__ double inv_depth(double z) { return z > 0.0 ? 1.0 / z : 0.0; }

struct Tap {
    double c0, c1, c2, n0, n1, n2, z, u;
};

// The weight of one tap of the contract: the three edge-stopping terms. q_c is the level's
// constant (tray_denoise.h) or the pixel's r_i(p) (tray_progressive.h, section 3b).
__device__ __forceinline__ double tap_weight(const DenoiseLevel& L, double q_c, double k, const Tap& p, const Tap& q) {
    const double d0 = p.c0 - q.c0, d1 = p.c1 - q.c1, d2 = p.c2 - q.c2;
    const double x_c = ((d0 * d0 + d1 * d1) + d2 * d2) * q_c;
    double w = k * edge_stop(x_c);
    if (L.normal) {
        const double e0 = p.n0 - q.n0, e1 = p.n1 - q.n1, e2 = p.n2 - q.n2;
        const double x_n = ((e0 * e0 + e1 * e1) + e2 * e2) * L.q_n;
        w = w * edge_stop(x_n);
    }
    if (L.depth) {
        const double t = (p.z - q.z) * (p.z >= q.z ? p.u : q.u);
        const double x_z = (t * t) * L.q_z;
        w = w * edge_stop(x_z);
    }
    return w;
}

// One tap of the contract: the weight, the sums.
__device__ __forceinline__ void accumulate(const DenoiseLevel& L, double k, const Tap& p, const Tap& q, double& a0,
                                           double& a1, double& a2, double& W) {
    const double w = tap_weight(L, L.q_c, k, p, q);
    if (w > 0.0) {
        a0 = a0 + w * q.c0;
        a1 = a1 + w * q.c1;
        a2 = a2 + w * q.c2;
        W = W + w;
    }
}

__device__ __forceinline__ double kernel_weight(int d) {  // h = (1/16, 1/4, 3/8, 1/4, 1/16)
    return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625;
}

// Pixel `pix` of the level's input with its guides, as the taps see it.
__device__ __forceinline__ Tap load_point(const DenoiseLevel& L, size_t pix) {
    Tap t;
    t.c0 = L.in[3 * pix];
    t.c1 = L.in[3 * pix + 1];
    t.c2 = L.in[3 * pix + 2];
    if (L.demodulate) {
        t.c0 = t.c0 / albedo_floor(L.demodulate[3 * pix]);
        t.c1 = t.c1 / albedo_floor(L.demodulate[3 * pix + 1]);
        t.c2 = t.c2 / albedo_floor(L.demodulate[3 * pix + 2]);
    }
    t.n0 = t.n1 = t.n2 = t.z = t.u = 0.0;
    if (L.normal) {
        t.n0 = L.normal[3 * pix];
        t.n1 = L.normal[3 * pix + 1];
        t.n2 = L.normal[3 * pix + 2];
    }
    if (L.depth) {
        t.z = L.depth[pix];
        t.u = inv_depth(t.z);
    }
    return t;
}

__device__ __forceinline__ void store_pixel(const DenoiseLevel& L, size_t pix, const Tap& p, double a0, double a1,
                                            double a2, double W) {
    double r0 = p.c0, r1 = p.c1, r2 = p.c2;
    if (W > 0.0) {
        r0 = a0 / W;
        r1 = a1 / W;
        r2 = a2 / W;
    }
    if (L.remodulate) {
        r0 = r0 * albedo_floor(L.remodulate[3 * pix]);
        r1 = r1 * albedo_floor(L.remodulate[3 * pix + 1]);
        r2 = r2 * albedo_floor(L.remodulate[3 * pix + 2]);
    }
    L.out[3 * pix] = r0;
    L.out[3 * pix + 1] = r1;
    L.out[3 * pix + 2] = r2;
}

#ifndef TRAY_DENOISE_GLOBAL_TAPS

// What the variance-guided level (tray_progressive.h, section 3) has beyond DenoiseLevel.
struct VarianceLevel {
    const double* variance;  // level 0: rows x width x 3, the per-channel variance of the mean; else null
    const double* plane_in;  // later levels: v_i, rows x width
    double* plane_out;       // v_i+1; null when the last level's plane is not asked for
    double S, epsilon;       // sigma_variance^2, epsilon
};

// v_0 of pixel `pix`: the scalar noise plane from the per-channel variance (in the units the
// filter runs in: divided by m(albedo)^2 at the level that demodulates).
__device__ __forceinline__ double noise_point(const DenoiseLevel& L, const VarianceLevel& V, size_t pix) {
    if (!V.variance) return V.plane_in[pix];
    double v0 = V.variance[3 * pix], v1 = V.variance[3 * pix + 1], v2 = V.variance[3 * pix + 2];
    if (L.demodulate) {
        const double m0 = albedo_floor(L.demodulate[3 * pix]), m1 = albedo_floor(L.demodulate[3 * pix + 1]),
                     m2 = albedo_floor(L.demodulate[3 * pix + 2]);
        v0 = v0 / (m0 * m0);
        v1 = v1 / (m1 * m1);
        v2 = v2 / (m2 * m2);
    }
    return (v0 + v1) + v2;
}

__device__ __forceinline__ double binomial_weight(int d) { return d == 0 ? 0.5 : 0.25; }  // h3 = (1/4, 1/2, 1/4)

// One level for one workgroup. kVariance adds a ninth LDS plane, v_i (31,104 B: still 5
// workgroups per CU). Its reads follow the other planes' pattern, a half-wave on 32 consecutive
// doubles of one plane row at every tap and prefilter offset, and its staging stores are the
// same k-indexed stores: no bank conflicts for the same reason.
template <bool kVariance>
__device__ __forceinline__ void denoise_level(const DenoiseLevel& L, const VarianceLevel& V) {
    __shared__ double lds[kVariance ? 9 : 8][kLdsPoints];
    // Block -> (sub-image, tile). Uniform per block.
    uint32_t b = blockIdx.x;
    const int32_t tile_x = (int32_t)(b % (uint32_t)L.tiles_x);
    b /= (uint32_t)L.tiles_x;
    const int32_t tile_y = (int32_t)(b % (uint32_t)L.tiles_y);
    b /= (uint32_t)L.tiles_y;
    const int32_t off_x = (int32_t)(b % (uint32_t)L.lattices_x), off_y = (int32_t)(b / (uint32_t)L.lattices_x);
    // Sub-image coordinates (i, j) <-> pixel (off_x + i * s, off_y + j * s); 64-bit: i * s may pass 2^31 in the halo.
    const int64_t i0 = (int64_t)tile_x * kTileX, j0 = (int64_t)tile_y * kTileY;
    if (off_x + i0 * L.s >= L.width || off_y + j0 * L.s >= L.rows) return;  // a shorter sub-image: no such tile

    const double nan = __builtin_nan("");
    for (int k = (int)threadIdx.x; k < kLdsPoints; k += kThreads) {
        const int ly = k / kLdsX, lx = k - ly * kLdsX;
        const int64_t x = off_x + (i0 + lx - kHalo) * L.s, y = off_y + (j0 + ly - kHalo) * L.s;
        Tap t;
        t.c0 = nan;  // outside the image: skipped through b(NaN) = 0
        t.c1 = t.c2 = t.n0 = t.n1 = t.n2 = t.z = t.u = 0.0;
        const bool inside = x >= 0 && x < L.width && y >= 0 && y < L.rows;
        if (inside) t = load_point(L, (size_t)y * (size_t)L.width + (size_t)x);
        if constexpr (kVariance)
            lds[8][k] = inside ? noise_point(L, V, (size_t)y * (size_t)L.width + (size_t)x) : 0.0;
        lds[0][k] = t.c0;
        lds[1][k] = t.c1;
        lds[2][k] = t.c2;
        lds[3][k] = t.n0;
        lds[4][k] = t.n1;
        lds[5][k] = t.n2;
        lds[6][k] = t.z;
        lds[7][k] = t.u;
    }
    __syncthreads();

    const int tx = (int)threadIdx.x % kTileX, ty = (int)threadIdx.x / kTileX;
    const int64_t x = off_x + (i0 + tx) * L.s, y = off_y + (j0 + ty) * L.s;
    if (x >= L.width || y >= L.rows) return;  // no barrier follows
    const int centre = (ty + kHalo) * kLdsX + tx + kHalo;
    Tap p;
    p.c0 = lds[0][centre], p.c1 = lds[1][centre], p.c2 = lds[2][centre];
    p.n0 = lds[3][centre], p.n1 = lds[4][centre], p.n2 = lds[5][centre];
    p.z = lds[6][centre], p.u = lds[7][centre];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, W = 0.0;
    [[maybe_unused]] double r = 0.0, A = 0.0;
    if constexpr (kVariance) {  // g_i(p): the 3 x 3 binomial mean of v_i over the in-image neighbours, then r_i(p)
        double G = 0.0, B = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int64_t qx = x + (int64_t)dx * L.s, qy = y + (int64_t)dy * L.s;
                if (qx < 0 || qx >= L.width || qy < 0 || qy >= L.rows) continue;
                const double k3 = binomial_weight(dy) * binomial_weight(dx);
                G = G + k3 * lds[8][centre + dy * kLdsX + dx];
                B = B + k3;
            }
        }
        const double g = G / B;
        r = 1.0 / (g > 0.0 ? V.S * g + V.epsilon : V.epsilon);
    }
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int at = centre + dy * kLdsX + dx;
            Tap q;
            q.c0 = lds[0][at], q.c1 = lds[1][at], q.c2 = lds[2][at];
            q.n0 = lds[3][at], q.n1 = lds[4][at], q.n2 = lds[5][at];
            q.z = lds[6][at], q.u = lds[7][at];
            const double k = kernel_weight(dy) * kernel_weight(dx);
            if constexpr (kVariance) {
                const double w = tap_weight(L, r, k, p, q);
                if (w > 0.0) {
                    a0 = a0 + w * q.c0;
                    a1 = a1 + w * q.c1;
                    a2 = a2 + w * q.c2;
                    W = W + w;
                    A = A + (w * w) * lds[8][at];
                }
            } else {
                accumulate(L, k, p, q, a0, a1, a2, W);
            }
        }
    }
    const size_t pix = (size_t)y * (size_t)L.width + (size_t)x;
    store_pixel(L, pix, p, a0, a1, a2, W);
    if constexpr (kVariance) {
        if (V.plane_out) V.plane_out[pix] = W > 0.0 ? A / (W * W) : lds[8][centre];
    }
}

__global__ __launch_bounds__(kThreads) void denoise_level_kernel(const DenoiseLevel L) {
    denoise_level<false>(L, VarianceLevel{});
}

__global__ __launch_bounds__(kThreads) void denoise_variance_level_kernel(const DenoiseLevel L,
                                                                          const VarianceLevel V) {
    denoise_level<true>(L, V);
}

// Fills the tiling fields of L and returns the workgroups of its launch.
static int64_t plan_level(DenoiseLevel& L) {
    const int64_t sub_w = ((int64_t)L.width + L.s - 1) / L.s, sub_h = ((int64_t)L.rows + L.s - 1) / L.s;
    L.tiles_x = (int32_t)((sub_w + kTileX - 1) / kTileX);
    L.tiles_y = (int32_t)((sub_h + kTileY - 1) / kTileY);
    L.lattices_x = L.s < L.width ? L.s : L.width;
    const int64_t lattices_y = L.s < L.rows ? L.s : L.rows;
    return (int64_t)L.tiles_x * L.tiles_y * L.lattices_x * lattices_y;
}

static hipError_t launch_level(DenoiseLevel& L, hipStream_t stream) {
    const int64_t blocks = plan_level(L);
    if (blocks > kMaxBlocks) return hipErrorInvalidConfiguration;  // tray_denoise_async refuses these first
    hipLaunchKernelGGL(denoise_level_kernel, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, L);
    return hipGetLastError();
}

static hipError_t launch_variance_level(DenoiseLevel& L, const VarianceLevel& V, hipStream_t stream) {
    const int64_t blocks = plan_level(L);
    if (blocks > kMaxBlocks) return hipErrorInvalidConfiguration;  // tray_denoise_variance_async refuses these first
    hipLaunchKernelGGL(denoise_variance_level_kernel, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, L, V);
    return hipGetLastError();
}

#else  // TRAY_DENOISE_GLOBAL_TAPS: the A/B baseline

__global__ __launch_bounds__(kThreads) void denoise_level_kernel(const DenoiseLevel L) {
    const size_t pix = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= (size_t)L.rows * (size_t)L.width) return;
    const int64_t y = (int64_t)(pix / (size_t)L.width), x = (int64_t)(pix - (size_t)y * (size_t)L.width);
    const Tap p = load_point(L, pix);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, W = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = y + (int64_t)dy * L.s;
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = x + (int64_t)dx * L.s;
            if (qx < 0 || qx >= L.width || qy < 0 || qy >= L.rows) continue;
            const Tap q = load_point(L, (size_t)qy * (size_t)L.width + (size_t)qx);
            accumulate(L, kernel_weight(dy) * kernel_weight(dx), p, q, a0, a1, a2, W);
        }
    }
    store_pixel(L, pix, p, a0, a1, a2, W);
}

static int64_t plan_level(DenoiseLevel& L) {
    return ((int64_t)L.rows * L.width + kThreads - 1) / kThreads;
}

static hipError_t launch_level(DenoiseLevel& L, hipStream_t stream) {
    hipLaunchKernelGGL(denoise_level_kernel, dim3((uint32_t)plan_level(L)), dim3(kThreads), 0, stream, L);
    return hipGetLastError();
}

#endif

int validate(const tray_denoise_params* p, int64_t* pixels, size_t* workspace) {
    if (!p) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params");
    if (p->width < 0 || p->rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    if (p->iterations < 1 || p->iterations > TRAY_DENOISE_MAX_ITERATIONS)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "iterations outside 1..8");
    if (p->flags & ~TRAY_DENOISE_DEMODULATE) return fail(TRAY_ERR_INVALID_ARGUMENT, "unknown flags");
    const double sigmas[3] = {p->sigma_color, p->sigma_normal, p->sigma_depth};
    static const char* const names[3] = {"sigma_color", "sigma_normal", "sigma_depth"};
    for (int i = 0; i < 3; ++i)
        if (!(std::isfinite(sigmas[i]) && sigmas[i] > 0.0))
            return fail(TRAY_ERR_INVALID_ARGUMENT, std::string(names[i]) + " must be finite and > 0");
    *pixels = (int64_t)p->width * (int64_t)p->rows;
    if (*pixels > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one denoise call");
    const size_t images = p->iterations >= 3 ? 2 : (size_t)(p->iterations - 1);
    *workspace = images * (size_t)*pixels * 3 * sizeof(double);
    return TRAY_OK;
}

#ifndef TRAY_DENOISE_GLOBAL_TAPS
// tray_denoise_variance_params through the checks of tray_denoise_params (the shared fields), then its
// own; the workspace holds a noise plane beside each intermediate image.
int validate_variance(const tray_denoise_variance_params* p, int64_t* pixels, size_t* workspace) {
    if (!p) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params");
    const tray_denoise_params shared = {p->width, p->rows, p->iterations, p->flags, 1.0, p->sigma_normal,
                                        p->sigma_depth};
    const int rc = validate(&shared, pixels, workspace);
    if (rc) return rc;
    if (!(std::isfinite(p->sigma_variance) && p->sigma_variance > 0.0))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "sigma_variance must be finite and > 0");
    if (!(std::isfinite(p->epsilon) && p->epsilon > 0.0))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "epsilon must be finite and > 0");
    *workspace = *workspace / 3 * 4;
    return TRAY_OK;
}
#endif

}  // namespace
}  // namespace tray

using namespace tray;

#pragma GCC visibility push(default)
extern "C" {

int32_t tray_denoise_version(void) { return TRAY_DENOISE_VERSION; }

int tray_denoise_default_params(int32_t width, int32_t rows, tray_denoise_params* out) {
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params (out)");
    if (width < 0 || rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    out->width = width;
    out->rows = rows;
    out->iterations = 5;
    out->flags = TRAY_DENOISE_DEMODULATE;
    out->sigma_color = 0.5;
    out->sigma_normal = 0.5;
    out->sigma_depth = 0.0625;
    return TRAY_OK;
}

int tray_denoise_workspace_bytes(const tray_denoise_params* p, size_t* bytes) {
    if (!bytes) return fail(TRAY_ERR_INVALID_ARGUMENT, "null bytes");
    int64_t pixels = 0;
    return validate(p, &pixels, bytes);
}

int tray_denoise_async(const double* colour, const tray_denoise_guides* guides, const tray_denoise_params* p,
                       double* out, void* workspace, size_t workspace_bytes, int32_t device, void* stream) {
    if (!colour) return fail(TRAY_ERR_INVALID_ARGUMENT, "null colour");
    if (!guides) return fail(TRAY_ERR_INVALID_ARGUMENT, "null guides");
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null out");
    int64_t pixels = 0;
    size_t need = 0;
    int rc = validate(p, &pixels, &need);
    if (rc) return rc;
    if ((p->flags & TRAY_DENOISE_DEMODULATE) && !guides->albedo)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "TRAY_DENOISE_DEMODULATE needs the albedo guide");
    if (need && (!workspace || workspace_bytes < need))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "workspace smaller than tray_denoise_workspace_bytes");
    const size_t image_bytes = (size_t)pixels * 3 * sizeof(double);
    const Span spans[] = {{out, image_bytes, 0, "out"},
                          {colour, image_bytes, 0, "colour"},
                          {workspace, need, 0, "the workspace"}};
    if (spans_overlap(spans[0], spans[1]))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "out overlaps colour: the filter does not run in place");
    rc = check_overlaps(spans, 3, 1);
    if (rc) return rc;
    if (pixels == 0) return TRAY_OK;

    const bool modulate = (p->flags & TRAY_DENOISE_DEMODULATE) != 0;
    double* const ping[2] = {static_cast<double*>(workspace), static_cast<double*>(workspace) + (size_t)pixels * 3};
    DenoiseLevel L;
    L.normal = guides->normal;
    L.depth = guides->depth;
    L.width = p->width;
    L.rows = p->rows;
    L.q_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    L.q_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    L.tiles_x = L.tiles_y = L.lattices_x = 0;
    for (int i = 0; i < p->iterations; ++i) {  // before any device work: all levels or none
        L.s = 1 << i;
        if (plan_level(L) > kMaxBlocks)
            return fail(TRAY_ERR_TOO_LARGE, "a level of this image needs more than 2^24 - 1 workgroups");
    }

    rc = select_device(device);
    if (rc) return rc;
    double sigma_c = p->sigma_color;
    const double* in = colour;
    for (int i = 0; i < p->iterations; ++i) {
        const bool last = i == p->iterations - 1;
        L.in = in;
        L.out = last ? out : ping[i & 1];
        L.demodulate = modulate && i == 0 ? guides->albedo : nullptr;
        L.remodulate = modulate && last ? guides->albedo : nullptr;
        L.s = 1 << i;
        L.q_c = 1.0 / (sigma_c * sigma_c);
        const hipError_t e = launch_level(L, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("denoise level: ") + hipGetErrorString(e));
        in = L.out;
        sigma_c = sigma_c * 0.5;
    }
    return TRAY_OK;
}

#ifndef TRAY_DENOISE_GLOBAL_TAPS  // include/tray_progressive.h, section 3

int tray_denoise_variance_default_params(int32_t width, int32_t rows, tray_denoise_variance_params* out) {
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params (out)");
    if (width < 0 || rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    out->width = width;
    out->rows = rows;
    out->iterations = 5;
    out->flags = TRAY_DENOISE_DEMODULATE;
    out->sigma_variance = 3.0;
    out->sigma_normal = 0.5;
    out->sigma_depth = 0.0625;
    out->epsilon = 1e-12;
    return TRAY_OK;
}

int tray_denoise_variance_workspace_bytes(const tray_denoise_variance_params* p, size_t* bytes) {
    if (!bytes) return fail(TRAY_ERR_INVALID_ARGUMENT, "null bytes");
    int64_t pixels = 0;
    return validate_variance(p, &pixels, bytes);
}

int tray_denoise_variance_async(const double* colour, const double* variance, const tray_denoise_guides* guides,
                                const tray_denoise_variance_params* p, double* out, double* variance_out,
                                void* workspace, size_t workspace_bytes, int32_t device, void* stream) {
    if (!colour) return fail(TRAY_ERR_INVALID_ARGUMENT, "null colour");
    if (!variance) return fail(TRAY_ERR_INVALID_ARGUMENT, "null variance");
    if (!guides) return fail(TRAY_ERR_INVALID_ARGUMENT, "null guides");
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null out");
    int64_t pixels = 0;
    size_t need = 0;
    int rc = validate_variance(p, &pixels, &need);
    if (rc) return rc;
    if ((p->flags & TRAY_DENOISE_DEMODULATE) && !guides->albedo)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "TRAY_DENOISE_DEMODULATE needs the albedo guide");
    if (need && (!workspace || workspace_bytes < need))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "workspace smaller than tray_denoise_variance_workspace_bytes");
    const size_t image_bytes = (size_t)pixels * 3 * sizeof(double), plane_bytes = (size_t)pixels * sizeof(double);
    const Span spans[] = {{out, image_bytes, 0, "out"},
                          {variance_out, plane_bytes, 0, "variance_out"},
                          {colour, image_bytes, 0, "colour"},
                          {variance, image_bytes, 0, "variance"},
                          {workspace, need, 0, "the workspace"}};
    if (spans_overlap(spans[0], spans[2]))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "out overlaps colour: the filter does not run in place");
    rc = check_overlaps(spans, 5, 2);
    if (rc) return rc;
    if (pixels == 0) return TRAY_OK;

    const bool modulate = (p->flags & TRAY_DENOISE_DEMODULATE) != 0;
    const size_t buffers = need / (image_bytes + plane_bytes);  // 0, 1 or 2
    double* const base = static_cast<double*>(workspace);
    double* const ping[2] = {base, base + (size_t)pixels * 3};
    double* const planes[2] = {base + buffers * (size_t)pixels * 3, base + buffers * (size_t)pixels * 3 + (size_t)pixels};
    DenoiseLevel L;
    L.normal = guides->normal;
    L.depth = guides->depth;
    L.width = p->width;
    L.rows = p->rows;
    L.q_c = 0.0;  // not used: r_i(p) takes its place
    L.q_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    L.q_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    L.tiles_x = L.tiles_y = L.lattices_x = 0;
    for (int i = 0; i < p->iterations; ++i) {  // before any device work: all levels or none
        L.s = 1 << i;
        if (plan_level(L) > kMaxBlocks)
            return fail(TRAY_ERR_TOO_LARGE, "a level of this image needs more than 2^24 - 1 workgroups");
    }

    rc = select_device(device);
    if (rc) return rc;
    VarianceLevel V;
    V.S = p->sigma_variance * p->sigma_variance;
    V.epsilon = p->epsilon;
    const double* in = colour;
    const double* plane_in = nullptr;
    for (int i = 0; i < p->iterations; ++i) {
        const bool last = i == p->iterations - 1;
        L.in = in;
        L.out = last ? out : ping[i & 1];
        L.demodulate = modulate && i == 0 ? guides->albedo : nullptr;
        L.remodulate = modulate && last ? guides->albedo : nullptr;
        L.s = 1 << i;
        V.variance = i == 0 ? variance : nullptr;
        V.plane_in = plane_in;
        V.plane_out = last ? variance_out : planes[i & 1];
        const hipError_t e = launch_variance_level(L, V, static_cast<hipStream_t>(stream));
        if (e != hipSuccess)
            return fail(TRAY_ERR_DEVICE, std::string("variance-guided denoise level: ") + hipGetErrorString(e));
        in = L.out;
        plane_in = V.plane_out;
    }
    return TRAY_OK;
}

#endif  // TRAY_DENOISE_GLOBAL_TAPS

}  // extern "C"
#pragma GCC visibility pop
