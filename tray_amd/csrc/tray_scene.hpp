// tray_scene.hpp — an uploaded scene (tray_scene_s) and what an entry point that is bound
// to one needs: the device-error helper, the fillers of the megakernel's KernelParams and
// the argument checks the headers share. The definitions are tray_abi.hip's; each entry
// point lives in the unit that holds its kernels. Host side only. Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/tray.h"
#include "tray_check.hpp"
#include "tray_kernel.hpp"

namespace tray {

// Records "<what>: <the HIP error's text>" and returns TRAY_ERR_DEVICE.
int hip_fail(hipError_t e, const char* what);

}  // namespace tray

#define TRAY_HIP(call)                                        \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return tray::hip_fail(e_, #call); \
    } while (0)

// What a primary-ray candidate list depends on (compared byte for byte).
struct CandKey {
    tray_camera cam;
    double ray_radius;
    int32_t width, height, y_start, rows, tile_rows, tile_count, tile_index, multi_sample;
};

// The mutable device state ONE render uses while it runs: the work-queue word
// (zero between launches: zeroed at allocation, then by each band's resolve
// pass), the per-sample buffer or chunk records of a launch band, the primary-ray
// candidate records of the last camera and row set it rendered, and the
// traversal-stack overflow area (deep BVHs). `done` is recorded on the render's
// stream after each launch that used it. A scene holds a few of these, so that
// renders of one scene on different streams (or threads) run concurrently
// without sharing any of it, as several goroutines may Render one read-only
// *Scene at once (ray/tracer.go:48, ray/objects.go:37-46).
struct LaunchCtx {
    uint32_t* queue = nullptr;
    double* samples = nullptr;
    size_t samples_bytes = 0;
    uint4* cand = nullptr;
    size_t cand_bytes = 0;
    bool cand_valid = false;
    CandKey cand_key;
    uint32_t* stack_ovf = nullptr;
    size_t ovf_bytes = 0;
    // Work order (launch_render): per 8x8 tile of the rows, the Scene.Hit calls a
    // counting launch measured and the order the next launches hand tiles out in,
    // valid for `order_key` (camera, rows, tiling, rays per pixel, depth).
    uint32_t* tile_cost = nullptr;
    size_t tile_cost_bytes = 0;
    uint32_t* tile_order = nullptr;
    size_t tile_order_bytes = 0;
    bool order_valid = false;
    CandKey order_key;
    int32_t order_spp = 0, order_depth = 0;
    hipEvent_t done = nullptr;
    bool launched = false;          // `done` has been recorded
    hipStream_t last_stream = nullptr;
    uint64_t last_use = 0;          // the scene's launch count at its last launch
};

// A scene resident on one device. Its arrays are read-only after the upload, but
// for tray_scene_update_async (include/tray_scene_update.h), which rewrites the
// centres, radii and boxes in stream order; everything a render writes lives in a
// launch context (above), taken under the scene's mutex for the time it takes to
// enqueue the render.
struct tray_scene_s {
    int32_t device = 0;
    int32_t n = 0;
    int32_t n_pad = 0;
    double4* geo = nullptr;  // n_pad entries, NaN-padded (see tray::KernelParams::geo)
    tray::MatRec* mat = nullptr;
    tray::V3 bg_a{}, bg_b{};
    double max_att = 1.0;  // max(1, |albedo| of every Lambertian/Metal sphere): bounds a path's throughput
                           // (infinite when one of them is infinite or NaN: KernelParams::wild_att)
    // exact-culling BVH (absent for tiny scenes, for scenes with a NaN or infinite
    // coordinate or radius and for scenes that reach beyond +-kBvhMaxBound, bvh.hpp:
    // those take the linear scan, and with no tree there are no candidate lists)
    bool has_bvh = false;
    double bvh_bound = 0.0;
    int32_t n_nodes = 0, n_slots = 0, n_leaves = 0, stack_cap = 0, leaf_max = 0, n_global = 0;
    tray::Bvh4Node* nodes = nullptr;
    int32_t* leaves = nullptr;
    size_t ovf_bytes = 0;  // traversal-stack overflow area a render needs (deep BVHs only; per context)
    double4* bgeo = nullptr;
    int32_t* bidx = nullptr;
    tray::MatRec* bmat = nullptr;
    // One device allocation holds geo, mat, srgb and the BVH arrays (the pointers
    // above point into it).
    void* arena = nullptr;
    double* srgb = nullptr;  // the RGBA8 encoder table (tray::srgb_thresholds), 256 doubles
    std::mutex mu;  // guards ctx and launches
    std::vector<LaunchCtx*> ctx;
    uint64_t launches = 0;
    // tray_scene_update_async: the child references of the nodes (host copy, n_nodes x
    // kBvhWidth), the level schedule built from them at the first update (a device buffer
    // of the scene's own, outside the arena) and the event recorded after the last update.
    std::vector<uint32_t> refs;
    uint32_t* schedule = nullptr;
    int32_t n_levels = 0;
    hipEvent_t updated = nullptr;
    bool update_recorded = false;
};

namespace tray {

constexpr int64_t kQueryMaxRays = kMaxPixels;  // ray indices are 32-bit on the device

// The scene's arrays and background in the kernel parameters (renders and ray queries).
void scene_params(const tray_scene_s* sc, KernelParams& k);
// The camera and the draw key of `seed` in the kernel parameters (get_ray, draw).
void camera_params(const tray_camera* cam, KernelParams& k);
void key_params(uint64_t seed, KernelParams& k);
// The image, row-set, pass, camera and draw-key fields of the kernel parameters: `n_passes`
// passes, from p->pass on, of the `rows` = tray_params_rows(p) rows of p's row set.
void frame_params(const tray_camera* cam, const tray_params* p, int32_t rows, int32_t n_passes, KernelParams& k);

int validate_params(const tray_params* p);
// n_passes passes from p->pass on (p validated): at least one, and their sample words fit 32 bits.
int validate_passes(const tray_params* p, int32_t n_passes);
// The caller's choice between the scene's BVH and the reference-order linear scan.
bool wants_bvh(const tray_scene_s* sc, int32_t flags);
// The checks the scene queries share, before any device work.
int validate_query(tray_scene_t sc, const void* rays, int64_t n, int32_t flags, const void* out);

}  // namespace tray
