// tray_adaptive.hip — include/tray_adaptive.h for gfx950: the renderer over a pixel
// list (section 2), Welford's fold with a count per pixel (section 3) and the
// selection step (section 4: metric, dilation, ascending compaction).
//
// The renderer's arithmetic is the megakernel's and the queries': it comes from
// tray_query_device.hpp (query_hit, query_shade with its scatter_step, the stack
// policy, query_args) and, under that, tray_device.hpp (get_ray, camera_block, row_of,
// kp_fresh, ...). The metric pass streams the state the way accum_fold_kernel does,
// through tray_stream.hpp. The header's entry points are at the end of the file; the
// renderer's reaches its scene through tray_scene.hpp. Compiled with -ffp-contract=off
// like every other unit; the public header is the contract.

#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "../../include/tray_adaptive.h"
#include "tray_check.hpp"
#include "tray_query_device.hpp"
#include "tray_scene.hpp"
#include "tray_stream.hpp"

namespace tray {

// ---- section 2: the renderer over a pixel list --------------------------------------
//
// ray_color_kernel's path loop (one path per lane, 256 lanes, five waves per SIMD) with
// the camera ray in front of it and the ordered pixel sum behind it, in one launch.
// g = min(r, 256) consecutive lanes serve one (pixel, pass) group and trace its samples
// l, l + g, ...: the lanes of a wave trace samples of the same pixel (or of list
// neighbours), which keeps their traversals together. A group of at most 64 lanes lies
// within one wave and waits only for that wave. After each round the workgroup
// parks its 256 colours and segment counts in LDS (7 KB beside the traversal stacks)
// and the group's first lane adds them to the running sum in sample order, so nothing
// per sample goes to memory. Only r > 256 takes more than one round; a workgroup is
// then one group, and its running sum waits in LDS between rounds instead of in
// registers across the path loop.
struct PixelArgs {
    const uint32_t* pixels;  // n_pixels compact indices
    const int32_t* plane;    // nullable: per compact pixel, added to the pass
    double* out;             // n_groups x 3
    uint32_t* segments;      // nullable, n_groups
    uint32_t n_pixels;
    uint32_t n_groups;       // n_pixels x n_passes, group G = k * n_pixels + i
    uint32_t image_pixels;   // rows x width: an entry at or beyond it is not rendered
    uint32_t g;              // lanes per group: min(r, 256)
    uint32_t unit;           // lanes a group lies within: a wave (64) when g <= 64, else the workgroup (256)
    uint32_t groups_per_unit;  // unit / g
    uint32_t rounds;         // ceil(r / g)
    double inv_spp;          // RN(1 / r), the host's quotient (colorSumDiv, ray/tracer.go:123)
};

// threadIdx.x, opaque to the optimiser: what is derived from it is derived again at each use
// instead of being held in registers.
__device__ __forceinline__ uint32_t lane_index() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// The wave's LDS writes are visible to its own lanes (resolve_kernel's staging uses the same three).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane `tid` of this workgroup: sample lane l of group G = k * n_pixels + i (list entry i, pass k).
struct Place {
    uint32_t l, G, i, k;
    bool member;  // false: a lane beyond the workgroup's groups, or a group beyond the launch's
};
__device__ __forceinline__ Place place(const PixelArgs& a, uint32_t tid) {
    Place w;
    const uint32_t unit = tid / a.unit, lane = tid - unit * a.unit;  // no group straddles two units
    const uint32_t grp = lane / a.g;
    w.l = lane - grp * a.g;
    w.G = (blockIdx.x * ((uint32_t)kQueryBlock / a.unit) + unit) * a.groups_per_unit + grp;  // <= n_groups + 255
    w.member = grp < a.groups_per_unit && w.G < a.n_groups;
    w.k = w.G / a.n_pixels;
    w.i = w.G - w.k * a.n_pixels;
    return w;
}

// The kernel's one argument: KernelParams first, where kp_fresh() reads it.
struct PixelLaunch {
    KernelParams p;
    QueryArgs q;
    PixelArgs a;
};
static_assert(offsetof(PixelLaunch, p) == 0, "kp_fresh reads KernelParams at the start of the kernel arguments");

// kp_fresh for the list's arguments: read where they are used, not held across the path loop.
__device__ __forceinline__ const PixelArgs& pa_fresh() {
    typedef const __attribute__((address_space(4))) PixelLaunch* ConstLaunch;
    ConstLaunch l = (ConstLaunch)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(l));  // opaque: no load through l is hoisted above this point
    return ((const PixelLaunch*)l)->a;
}

__global__ __launch_bounds__(kQueryBlock, 5) void render_pixels_kernel(PixelLaunch L) {
    __shared__ double park[kQueryBlock * 3];
    __shared__ uint32_t park_seg[kQueryBlock];
    __shared__ double run[3];  // the running sum between rounds (r > 256: one group per workgroup)
    __shared__ uint32_t run_seg;
    const KernelParams& p = L.p;
    const QueryArgs& q = L.q;
    const SceneView sv = scene_view(p);
    const QStack S = lane_stack();
    for (uint32_t round = 0; round < pa_fresh().rounds; ++round) {  // uniform per workgroup
        D3 color = d3(0, 0, 0);
        uint32_t segs = 0;
        {
            // The lane's place in the launch is worked out here, from the thread index, and
            // again after the path loop: held across it these values spilled to scratch.
            const PixelArgs& a = pa_fresh();
            const uint32_t spp = (uint32_t)p.spp;
            const Place w = place(a, lane_index());
            const uint32_t s = round * a.g + w.l;
            bool live = w.member && s < spp;
            uint32_t pix = 0;
            if (live) {
                pix = a.pixels[w.i];
                live = pix < a.image_pixels;  // a bad entry reads nothing more and gets zeros
            }
            if (live) {
                const uint32_t width = (uint32_t)p.width;
                const uint32_t j = pix / width, x = pix - j * width;
                const int32_t y = row_of(p, (int32_t)j);
                const uint32_t pixel = (uint32_t)y * width + x;  // global index: the draw block's pixel word
                const uint32_t pass = p.pass0 + (a.plane ? (uint32_t)a.plane[pix] : 0u) + w.k;
                const uint32_t sample = pass * spp + s;  // the draw block's sample word
                // The camera, draw key, background and depth are read from the kernel arguments
                // where they are used, as the megakernel and aov_kernel read them.
                D3 org, dir;
                {
                    const KernelParams& pk = kp_fresh();
                    get_ray(pk, camera_block(pk, pixel, sample), (double)x, (double)y, org, dir);
                }
                D3 thr = d3(1, 1, 1);
                uint32_t bounce = 0;
                bool more = true;
                while (more) {
                    ++segs;
                    const QHit h = query_hit(sv, S, q, org, dir, __builtin_inf());
                    more = query_shade(kp_fresh(), sv, h, pixel, sample, bounce, org, dir, thr, color);
                }
            }
        }
        const uint32_t tid = lane_index();
        park[tid * 3] = color.x, park[tid * 3 + 1] = color.y, park[tid * 3 + 2] = color.z;
        park_seg[tid] = segs;
        // A group within a wave waits for its own wave only: a wave whose paths have ended adds up
        // and exits while the workgroup's other waves still trace.
        if (pa_fresh().unit == 64u) wave_sync();
        else __syncthreads();
        const PixelArgs& a = pa_fresh();
        const uint32_t spp = (uint32_t)kp_fresh().spp;
        const Place w = place(a, tid);
        if (w.member && w.l == 0) {
            D3 sum = d3(0, 0, 0);
            uint32_t total = 0;
            if (round > 0) sum = d3(run[0], run[1], run[2]), total = run_seg;
            const uint32_t left = spp - round * a.g, n = left < a.g ? left : a.g;
            for (uint32_t t = 0; t < n; ++t) {  // tid + t < (grp + 1) * g <= 256
                const double* c = park + (tid + t) * 3;
                sum = add(sum, d3(c[0], c[1], c[2]));
                total += park_seg[tid + t];
            }
            if (round + 1 == a.rounds) {
                double* o = a.out + (size_t)w.G * 3;
                o[0] = sum.x * a.inv_spp, o[1] = sum.y * a.inv_spp, o[2] = sum.z * a.inv_spp;
                if (a.segments) a.segments[w.G] = total;
            } else {
                run[0] = sum.x, run[1] = sum.y, run[2] = sum.z;
                run_seg = total;
            }
        }
        if (round + 1 < a.rounds) __syncthreads();  // the next round overwrites the parked colours
    }
}

namespace {

// ---- section 3: the sparse fold ------------------------------------------------------
//
// One list entry per lane: the entry's pixel state (6 doubles and a count) is gathered,
// its n_passes x 3 values are read in pass order (a wave's 64 entries are 1.5 KB of
// consecutive bytes per pass) and the state is scattered back. The divide chains of the
// three channels are independent.
constexpr int kFoldThreads = 256;

struct SparseFoldArgs {
    double* mean;
    double* m2;
    int32_t* count;
    const uint32_t* pixels;
    const double* values;
    uint32_t n_pixels, image_pixels;
    int32_t n_passes;
};

__global__ __launch_bounds__(kFoldThreads) void adaptive_fold_kernel(const SparseFoldArgs A) {
    const uint32_t i = blockIdx.x * kFoldThreads + threadIdx.x;
    if (i >= A.n_pixels) return;
    const uint32_t pix = A.pixels[i];
    if (pix >= A.image_pixels) return;  // a bad entry is skipped
    int32_t n = A.count[pix];
    double mean[3] = {0.0, 0.0, 0.0}, m2[3] = {0.0, 0.0, 0.0};
    if (n > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mean[c] = A.mean[(size_t)pix * 3 + c];
            m2[c] = A.m2[(size_t)pix * 3 + c];
        }
    }
    for (int32_t k = 0; k < A.n_passes; ++k) {
        const double* x = A.values + ((size_t)k * A.n_pixels + i) * 3;
        n = n + 1;
        const double dn = (double)n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = x[c] - mean[c];
            mean[c] = mean[c] + t / dn;
            m2[c] = m2[c] + t * (x[c] - mean[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A.mean[(size_t)pix * 3 + c] = mean[c];
        A.m2[(size_t)pix * 3 + c] = m2[c];
    }
    A.count[pix] = n;
}

// ---- section 4: the selection --------------------------------------------------------
//
// Four launches. (1) The metric pass streams the state as accum_fold_kernel does
// (tray_stream.hpp: a wave owns 384 consecutive doubles = 128 pixels, read and written as
// 16-byte pairs, then transposed through LDS to pixels), with the one difference that D
// is per pixel: each element divides by the D of pixel e / 3, from a gathered count. It
// writes the variance, the needs flag of every pixel (one byte, the workspace's flag
// plane) and the record's three sums. (2) A workgroup per 1024 pixels counts its active
// pixels (needs of the pixel and, dilated, of its 8 neighbours, and the count below
// max_passes) into the block totals. (3) One wave scans the totals in place and writes
// n_active. (4) The workgroups of (2) evaluate their pixels again and write the active
// indices at their block's offset: ballots in ascending pixel order, so the list ascends.
constexpr uint32_t kScanPixels = 1024;  // pixels per block total (the header's formula)

struct SelectArgs {
    const double* mean;
    const double* m2;
    const int32_t* count;
    double* variance;  // nullable
    uint32_t* pixels;
    tray_adaptive_record* record;
    uint8_t* flags;    // image_pixels bytes: needs(p)
    uint32_t* totals;  // n_blocks
    size_t elems, chunks;
    uint32_t image_pixels, n_blocks;
    int32_t width, rows;
    int32_t min_passes, max_passes, dilate;
    double T, floor;
};

// variance of element e (of pixel e / 3) from its m2: +inf below two passes.
__device__ __forceinline__ double variance_of(const SelectArgs& A, size_t e, double m2) {
    if (e >= A.elems) return 0.0;
    const int32_t n = A.count[e / 3];
    if (n < 2) return std::numeric_limits<double>::infinity();
    return m2 / ((double)n * (double)(n - 1));
}

__global__ __launch_bounds__(kThreads) void adaptive_metric_kernel(const SelectArgs A) {
    __shared__ double xch[2][kBlockElems];
    __shared__ unsigned long long red[3][kWaves];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    unsigned long long wave_count = 0, lane_max = 0, lane_passes = 0;

    for (size_t chunk = blockIdx.x; chunk < A.chunks; chunk += gridDim.x) {  // uniform per workgroup
        const size_t wave_base = chunk * kBlockElems + (size_t)wave * kWaveElems;
        const int mine = wave * kWaveElems + 2 * lane;
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            const size_t at = wave_base + (size_t)j * kRowElems + 2 * (size_t)lane;
            double mean0 = 0.0, mean1 = 0.0, m20 = 0.0, m21 = 0.0;
            load_pair(A.mean, at, A.elems, mean0, mean1);
            load_pair(A.m2, at, A.elems, m20, m21);
            const double var0 = variance_of(A, at, m20), var1 = variance_of(A, at + 1, m21);
            if (A.variance) store_pair(A.variance, at, A.elems, var0, var1);
            xch[0][mine + j * kRowElems] = var0;
            xch[0][mine + j * kRowElems + 1] = var1;
            xch[1][mine + j * kRowElems] = mean0;
            xch[1][mine + j * kRowElems + 1] = mean1;
        }
        __syncthreads();
        const size_t pixel0 = chunk * (kBlockElems / 3) + (size_t)wave * kWavePixels;
#pragma unroll
        for (int t = 0; t < kWavePixels / kWave; ++t) {
            const int pp = lane + t * kWave;
            const size_t pix = pixel0 + (size_t)pp;
            const bool valid = pix < (size_t)A.image_pixels;
            const double* pv = &xch[0][wave * kWaveElems + 3 * pp];
            const double* pm = &xch[1][wave * kWaveElems + 3 * pp];
            const double v = (pv[0] + pv[1]) + pv[2];
            const double e = (pm[0] * pm[0] + pm[1] * pm[1]) + pm[2] * pm[2];
            const double m = e > A.floor ? e : A.floor;
            const double q = v / m;
            const int32_t n = valid ? A.count[pix] : 0;
            const bool needs = !(n >= 2 && n >= A.min_passes && v <= A.T * m);
            wave_count += (unsigned long long)__popcll(__ballot(valid && needs));
            if (valid) {
                A.flags[pix] = needs ? 1 : 0;
                lane_passes += (unsigned long long)(n > 0 ? n : 0);
                if (q >= 0.0) {
                    const unsigned long long b = (unsigned long long)__double_as_longlong(q);
                    lane_max = b > lane_max ? b : lane_max;
                }
            }
        }
        __syncthreads();  // the next chunk overwrites xch
    }

#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(lane_max, off, kWave);
        lane_max = other > lane_max ? other : lane_max;
        lane_passes += __shfl_xor(lane_passes, off, kWave);
    }
    if (lane == 0) {
        red[0][wave] = wave_count;
        red[1][wave] = lane_max;
        red[2][wave] = lane_passes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long count = 0, most = 0, passes = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            count += red[0][w];
            most = red[1][w] > most ? red[1][w] : most;
            passes += red[2][w];
        }
        if (count) atomicAdd(reinterpret_cast<unsigned long long*>(&A.record->unconverged), count);
        if (most) atomicMax(reinterpret_cast<unsigned long long*>(&A.record->max_ratio), most);
        if (passes) atomicAdd(reinterpret_cast<unsigned long long*>(&A.record->pixel_passes), passes);
    }
}

// active(p) of the header for an in-image compact pixel.
__device__ __forceinline__ bool active_of(const SelectArgs& A, uint32_t pix) {
    if (A.count[pix] >= A.max_passes) return false;
    if (A.flags[pix]) return true;
    if (!A.dilate) return false;
    const int32_t y = (int32_t)(pix / (uint32_t)A.width), x = (int32_t)(pix - (uint32_t)y * (uint32_t)A.width);
    bool wanted = false;
    for (int32_t dy = -1; dy <= 1; ++dy) {
        for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < A.rows && xx >= 0 && xx < A.width)
                wanted = wanted || A.flags[(size_t)yy * (size_t)A.width + (size_t)xx] != 0;
        }
    }
    return wanted;
}

// kWrite false: totals[block] = the block's active pixels. kWrite true: their indices at
// pixels[totals[block] ...] (totals scanned to exclusive offsets in between), ascending.
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void adaptive_compact_kernel(const SelectArgs A) {
    __shared__ uint32_t wave_total[kWaves];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t base = kWrite ? A.totals[blockIdx.x] : 0u;  // the running offset (count)
    for (uint32_t it = 0; it < kScanPixels / kThreads; ++it) {
        const uint64_t at = (uint64_t)blockIdx.x * kScanPixels + it * kThreads + threadIdx.x;
        const bool act = at < (uint64_t)A.image_pixels && active_of(A, (uint32_t)at);
        const unsigned long long mask = __ballot(act);
        if (lane == 0) wave_total[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) {
            before += w < wave ? wave_total[w] : 0u;
            all += wave_total[w];
        }
        if constexpr (kWrite) {
            if (act) A.pixels[base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)at;
        }
        base += all;
        __syncthreads();  // wave_total is rewritten by the next iteration
    }
    if constexpr (!kWrite) {
        if (threadIdx.x == 0) A.totals[blockIdx.x] = base;
    }
}

// One wave: totals -> exclusive prefix sums in place, and the grand total to the record.
__global__ __launch_bounds__(kWave) void adaptive_scan_kernel(const SelectArgs A) {
    const uint32_t lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < A.n_blocks; b0 += kWave) {
        const uint32_t b = b0 + lane;
        const uint32_t mine = b < A.n_blocks ? A.totals[b] : 0u;
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, kWave);
            if ((int)lane >= off) incl += up;
        }
        if (b < A.n_blocks) A.totals[b] = carry + incl - mine;
        carry += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) A.record->n_active = carry;
}

// The header's workspace formula for P > 0 pixels: the flag plane, then the block totals.
size_t flag_plane_bytes(int64_t pixels) { return (size_t)((pixels + 7) / 8 * 8); }
int64_t scan_blocks(int64_t pixels) { return (pixels + kScanPixels - 1) / kScanPixels; }
size_t workspace_bytes(int64_t pixels) {
    return pixels == 0 ? 0 : flag_plane_bytes(pixels) + (size_t)((scan_blocks(pixels) + 1) / 2 * 8);
}

}  // namespace
}  // namespace tray

using namespace tray;

#pragma GCC visibility push(default)
extern "C" {

int32_t tray_adaptive_version(void) { return TRAY_ADAPTIVE_VERSION; }

int tray_adaptive_default_params(tray_adaptive_params* out) {
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params (out)");
    out->tolerance = 0.05;
    out->floor = 0.0009765625;  // 2^-10
    out->min_passes = 8;        // tools/adaptive_sweep.py, DESIGN.md 8l
    out->max_passes = 64;
    out->dilate = 1;
    out->reserved = 0;
    return TRAY_OK;
}

// Section 2: the ordered-sum pixel means of the listed compact pixels of p's row set, passes
// p->pass + pass_plane[pixel] + k for k < n_passes; pass_plane and segments nullable.
int tray_render_pixels_async(tray_scene_t sc, const tray_camera* cam, const tray_params* p,
                             const uint32_t* pixels_device, int64_t n_pixels, const int32_t* pass_plane_device,
                             int32_t n_passes, double* out_device, uint32_t* segments_device, void* stream) {
    if (!sc) return fail(TRAY_ERR_INVALID_ARGUMENT, "null scene");
    if (!cam) return fail(TRAY_ERR_INVALID_ARGUMENT, "null camera");
    int rc = validate_params(p);
    if (rc) return rc;
    if (p->output != TRAY_OUT_RGB_F64)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "a pixel list renders TRAY_OUT_RGB_F64 only");
    if (n_pixels < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative n_pixels");
    rc = validate_passes(p, n_passes);
    if (rc) return rc;
    const int64_t rows = tray_params_rows(p);
    if (rows * (int64_t)p->width > kQueryMaxRays)
        return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one row set");
    // n_pixels x n_passes x r <= 2^31 - 1, without overflow: each factor is below 2^63 / 2^31.
    if (n_pixels > kQueryMaxRays || n_pixels * (int64_t)n_passes > kQueryMaxRays ||
        n_pixels * (int64_t)n_passes > kQueryMaxRays / p->rays_per_pixel)
        return fail(TRAY_ERR_TOO_LARGE, "n_pixels x n_passes x rays_per_pixel exceeds 2^31 - 1");
    if (n_pixels == 0) return TRAY_OK;
    if (!pixels_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null pixel list");
    if (!out_device) return fail(TRAY_ERR_INVALID_ARGUMENT, "null result buffer");
    KernelParams k;
    memset(&k, 0, sizeof(k));
    scene_params(sc, k);
    frame_params(cam, p, (int32_t)rows, n_passes, k);
    k.div_tile_rows = make_fastdiv((uint32_t)std::max(k.tile_rows, 1));  // row_of
    size_t lds = 0;
    // Stacks that do not fit beside the parked colours: the scan (query_takes_tree).
    const QueryArgs q = query_args(k, wants_bvh(sc, p->flags), sc->bvh_bound, nullptr, 0, lds, kQueryPixels);
    PixelArgs a{};
    a.pixels = pixels_device;
    a.plane = pass_plane_device;
    a.out = out_device;
    a.segments = segments_device;
    a.n_pixels = (uint32_t)n_pixels;
    a.n_groups = (uint32_t)n_pixels * (uint32_t)n_passes;  // n_pixels x n_passes x r <= 2^31 - 1, above
    a.image_pixels = (uint32_t)k.rows * (uint32_t)k.width;
    const uint32_t r = (uint32_t)k.spp;
    a.g = r < (uint32_t)kQueryBlock ? r : (uint32_t)kQueryBlock;
    a.unit = a.g <= 64u ? 64u : (uint32_t)kQueryBlock;
    a.groups_per_unit = a.unit / a.g;
    const uint32_t groups_per_block = a.groups_per_unit * ((uint32_t)kQueryBlock / a.unit);
    a.rounds = (r + a.g - 1u) / a.g;
    a.inv_spp = 1.0 / (double)k.spp;
    const uint32_t blocks = (a.n_groups + groups_per_block - 1u) / groups_per_block;
    TRAY_HIP(hipSetDevice(sc->device));
    hipLaunchKernelGGL(render_pixels_kernel, dim3(blocks), dim3(kQueryBlock), lds, static_cast<hipStream_t>(stream),
                       PixelLaunch{k, q, a});
    TRAY_HIP(hipGetLastError());
    return TRAY_OK;
}

int tray_adaptive_fold_async(const tray_adaptive_state* st, const uint32_t* pixels, int64_t n_pixels,
                             const double* values, int32_t n_passes, int32_t device, void* stream) {
    if (!st) return fail(TRAY_ERR_INVALID_ARGUMENT, "null state");
    if (st->width < 0 || st->rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    if (n_pixels < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative n_pixels");
    if (n_passes < 1 || n_passes > 65535) return fail(TRAY_ERR_INVALID_ARGUMENT, "n_passes must be in 1..65535");
    const int64_t image = (int64_t)st->width * (int64_t)st->rows;
    if (image > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one state");
    if (n_pixels > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one list");
    if (image == 0 || n_pixels == 0) return TRAY_OK;
    if (!st->mean || !st->m2) return fail(TRAY_ERR_INVALID_ARGUMENT, "null mean or m2");
    if (!st->count) return fail(TRAY_ERR_INVALID_ARGUMENT, "null count");
    if (!pixels) return fail(TRAY_ERR_INVALID_ARGUMENT, "null pixels");
    if (!values) return fail(TRAY_ERR_INVALID_ARGUMENT, "null values");
    const size_t img = (size_t)image * 3 * sizeof(double);
    const Span spans[] = {{st->mean, img, 8, "mean"},
                          {st->m2, img, 8, "m2"},
                          {st->count, (size_t)image * sizeof(int32_t), 4, "count"},
                          {pixels, (size_t)n_pixels * sizeof(uint32_t), 4, "pixels"},
                          {values, (size_t)n_pixels * (size_t)n_passes * 3 * sizeof(double), 8, "values"}};
    int rc = check_alignment(spans, 5);
    if (rc) return rc;
    rc = check_overlaps(spans, 5, 5);
    if (rc) return rc;
    rc = select_device(device);
    if (rc) return rc;

    SparseFoldArgs A;
    A.mean = st->mean;
    A.m2 = st->m2;
    A.count = st->count;
    A.pixels = pixels;
    A.values = values;
    A.n_pixels = (uint32_t)n_pixels;
    A.image_pixels = (uint32_t)image;
    A.n_passes = n_passes;
    const uint32_t grid = (uint32_t)((n_pixels + kFoldThreads - 1) / kFoldThreads);
    hipLaunchKernelGGL(adaptive_fold_kernel, dim3(grid), dim3(kFoldThreads), 0, static_cast<hipStream_t>(stream), A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("sparse fold: ") + hipGetErrorString(e));
    return TRAY_OK;
}

int tray_adaptive_workspace_bytes(int32_t width, int32_t rows, size_t* bytes) {
    if (!bytes) return fail(TRAY_ERR_INVALID_ARGUMENT, "null bytes");
    if (width < 0 || rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    const int64_t image = (int64_t)width * (int64_t)rows;
    if (image > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one state");
    *bytes = workspace_bytes(image);
    return TRAY_OK;
}

int tray_adaptive_select_async(const tray_adaptive_state* st, const tray_adaptive_params* ap, double* variance,
                               uint32_t* pixels, tray_adaptive_record* record, void* workspace, size_t workspace_size,
                               int32_t device, void* stream) {
    if (!st) return fail(TRAY_ERR_INVALID_ARGUMENT, "null state");
    if (!ap) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params");
    if (st->width < 0 || st->rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    if (!(std::isfinite(ap->tolerance) && ap->tolerance >= 0.0))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "tolerance must be finite and >= 0");
    if (!(std::isfinite(ap->floor) && ap->floor > 0.0))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "floor must be finite and > 0");
    if (ap->min_passes < 1 || ap->max_passes < ap->min_passes || ap->max_passes > (1 << 30))
        return fail(TRAY_ERR_INVALID_ARGUMENT, "passes must satisfy 1 <= min_passes <= max_passes <= 2^30");
    if (ap->dilate != 0 && ap->dilate != 1) return fail(TRAY_ERR_INVALID_ARGUMENT, "dilate must be 0 or 1");
    if (ap->reserved != 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "reserved must be 0");
    if (!pixels) return fail(TRAY_ERR_INVALID_ARGUMENT, "null pixels");
    if (!record) return fail(TRAY_ERR_INVALID_ARGUMENT, "null record");
    const int64_t image = (int64_t)st->width * (int64_t)st->rows;
    if (image > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one state");
    if (image == 0) return TRAY_OK;
    if (!st->mean || !st->m2) return fail(TRAY_ERR_INVALID_ARGUMENT, "null mean or m2");
    if (!st->count) return fail(TRAY_ERR_INVALID_ARGUMENT, "null count");
    const size_t need = workspace_bytes(image);
    if (!workspace || workspace_size < need)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "workspace is null or smaller than tray_adaptive_workspace_bytes");
    const size_t img = (size_t)image * 3 * sizeof(double);
    const Span spans[] = {{st->mean, img, 8, "mean"},
                          {st->m2, img, 8, "m2"},
                          {st->count, (size_t)image * sizeof(int32_t), 4, "count"},
                          {variance, img, 8, "variance"},
                          {pixels, (size_t)image * sizeof(uint32_t), 4, "pixels"},
                          {record, sizeof(tray_adaptive_record), 8, "the record"},
                          {workspace, need, 8, "the workspace"}};
    int rc = check_alignment(spans, 7);
    if (rc) return rc;
    rc = check_overlaps(spans, 7, 7);
    if (rc) return rc;
    rc = select_device(device);
    if (rc) return rc;

    SelectArgs A;
    A.mean = st->mean;
    A.m2 = st->m2;
    A.count = st->count;
    A.variance = variance;
    A.pixels = pixels;
    A.record = record;
    A.flags = static_cast<uint8_t*>(workspace);
    A.totals = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + flag_plane_bytes(image));
    A.elems = (size_t)image * 3;
    A.chunks = (A.elems + kBlockElems - 1) / kBlockElems;
    A.image_pixels = (uint32_t)image;
    A.n_blocks = (uint32_t)scan_blocks(image);
    A.width = st->width;
    A.rows = st->rows;
    A.min_passes = ap->min_passes;
    A.max_passes = ap->max_passes;
    A.dilate = ap->dilate;
    A.T = ap->tolerance * ap->tolerance;
    A.floor = ap->floor;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(record, 0, sizeof(tray_adaptive_record), s);
    if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    const uint32_t grid = (uint32_t)((int64_t)A.chunks < kMaxGrid ? (int64_t)A.chunks : kMaxGrid);
    hipLaunchKernelGGL(adaptive_metric_kernel, dim3(grid), dim3(kThreads), 0, s, A);
    hipLaunchKernelGGL(adaptive_compact_kernel<false>, dim3(A.n_blocks), dim3(kThreads), 0, s, A);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(kWave), 0, s, A);
    hipLaunchKernelGGL(adaptive_compact_kernel<true>, dim3(A.n_blocks), dim3(kThreads), 0, s, A);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("adaptive select: ") + hipGetErrorString(e));
    return TRAY_OK;
}

}  // extern "C"
#pragma GCC visibility pop
