/*
 * tray_debug.h — test and A/B hooks of libtray_amd.so. NOT part of the stable
 * C-ABI in tray.h: names and meanings may change with any build, and a
 * production caller (e.g. the cgo shim of INTEGRATION.md) never calls them.
 *
 * The library never reads the process environment: a stray TRAY_* variable in a
 * host process cannot change what it renders. The knobs below are process-wide
 * and apply to renders started after the call; unset knobs keep the product
 * behaviour. Each knob overrides one decision the library otherwise makes
 * itself; the frames they produce stay bit-identical to the defaults unless
 * noted (tests/test_gpu_*.py check exactly that).
 *
 *   "acc_slots"           on-chip chunk accumulators per wave (0 = off: chunk
 *                         sums through the per-sample buffer; same bits)
 *   "band_samples"        samples per launch band (< 2^30; < 2^31 with on-chip
 *                         chunk sums): splits a render into
 *                         more launches (same bits)
 *   "bvh_leaf"            BVH leaf size 1, 2 or 4 at tray_scene_upload (same bits)
 *   "bvh_lds_mode"        force LDS layout 0 / 1 / 2 when it fits (same bits)
 *   "stack_lds_slots"     cap the traversal stack's LDS slots (overflow path; same bits)
 *   "node_deep"           0 / 1: the 5- or 6-node-step kernel instance (same bits)
 *   "primary_candidates"  0: camera rays traverse the BVH instead of their
 *                         pixel's candidate list (same bits)
 *   "resolve_staged"      0: the plain per-pixel resolve instead of the LDS-staged
 *                         one for the per-sample buffer (the ordered FP64 sum, and
 *                         the fixed-point sums without on-chip slots) (same bits)
 *   "wave_chunks"         chunks a wave reserves per work-queue take (1..64), for
 *                         the whole launch (default: the build's size, single
 *                         chunks near the end of the queue) (same bits)
 *   "scene_contexts"      launch contexts per scene (default 4): renders of one
 *                         scene beyond this many in flight wait for the least
 *                         recently used one; 1 serialises them (same bits)
 *   "grid_reserve"        workgroup slots the persistent render grid leaves
 *                         free, out of the workgroups the device keeps resident
 *                         for the kernel instance (several per CU for small
 *                         instances; clamped to 0..resident-1), for kernels
 *                         that run beside it: collectives, copies (same bits)
 *   "work_order"          0: hand a launch's 8x8 tiles out in band order instead of
 *                         most expensive first by a counting launch's Scene.Hit
 *                         calls (same bits)
 *   "coop_lanes"          a wave whose work queue ran dry and that holds at most
 *                         this many paths finds their hits with the whole wave
 *                         scanning every sphere, one path at a time (0: never;
 *                         default 2) (same bits)
 *   "plain_instance"      0: every launch takes the generic megakernel instance, also
 *                         the launches that qualify for the plain-frame instance, whose
 *                         launch options are compiled in (same bits)
 */
#ifndef TRAY_DEBUG_H
#define TRAY_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets knob `name` to `value`. TRAY_ERR_INVALID_ARGUMENT for an unknown name. */
int tray_debug_set(const char *name, int64_t value);
/* Unsets knob `name`, or every knob when name is NULL. */
int tray_debug_clear(const char *name);
/* The device's progress counters as the last tray_render_progress on `device` left them:
 * finished samples per 8-row tile row of the render's rows, as the kernel counted them (the
 * host polls the same words while the launch runs). Writes min(*n_out, capacity) counters;
 * *n_out is the number of tile rows, 0 before any such render. */
int tray_debug_progress_counts(int32_t device, uint64_t *counts, int32_t capacity, int32_t *n_out);

/* What a launch is, for tray_debug_plain_instance: the buffers it has and the kernel family it runs. */
#define TRAY_PLAIN_FACT_BVH 1u          /* the BVH kernel (not the linear scan) */
#define TRAY_PLAIN_FACT_STATS 2u        /* tray_render_stats_async */
#define TRAY_PLAIN_FACT_PROGRESS 4u     /* live progress */
#define TRAY_PLAIN_FACT_STACK_SPILL 8u  /* the traversal stack overflows LDS */
#define TRAY_PLAIN_FACT_SEGMENTS 16u    /* a segment-count buffer */
#define TRAY_PLAIN_FACT_COUNTING 32u    /* a counting launch (the first of a work-order key) */
#define TRAY_PLAIN_FACT_CANDIDATES 64u  /* primary-ray candidate records */
#define TRAY_PLAIN_FACT_WORK_ORDER 128u /* a work order */
/* The library's own choice between the generic megakernel instance (*plain_out = 0) and the
 * plain-frame instance (1) for a launch with these properties: `facts` (bits above), rays per
 * pixel, tile_rows of tray_params, the scene's out-of-tree spheres, tree nodes and spheres per leaf
 * at most (tray_scene_info), on-chip sums
 * `acc` (0 none, 1 one per 64-sample chunk, 2 one per pixel-pass), LDS layout `lds_mode` (0 / 1 /
 * 2). Host only: no device is touched. The "plain_instance" knob applies. */
int tray_debug_plain_instance(uint32_t facts, int32_t rays_per_pixel, int32_t tile_rows, int32_t n_global,
                              int32_t n_nodes, int32_t leaf_max, int32_t acc, int32_t lds_mode,
                              int32_t *plain_out);
/* Launches (one per band) that took the plain-frame instance since the library was loaded. */
int tray_debug_plain_launches(uint64_t *count_out);
/* The plain-frame instance's batch trigger (phase_fires of tray_amd/csrc/tray_kernel.hpp, the very
 * function the kernel compiles): whether phase `phase` (0 leaf, 1 shade, 2 refill) runs with
 * `waiting` lanes gathered for it while `traversing` lanes are in flight, each 0..64. The generic
 * instances keep their fixed lane counts, so the "plain_instance" knob at 0 is also the switch back
 * to that schedule (same bits). Host only: no device is touched. */
int tray_debug_phase_trigger(int32_t phase, uint32_t waiting, uint32_t traversing, int32_t *fires_out);

/* The kernel families that find their hits outside the megakernel, for tray_debug_query_traversal. */
#define TRAY_QUERY_KIND_PLAIN 0    /* tray_scene_hit_async, tray_scene_occluded_async, tray_ray_color_async,
                                      tray_render_aov_async */
#define TRAY_QUERY_KIND_PIXELS 1   /* tray_render_pixels_async */
#define TRAY_QUERY_KIND_TEMPORAL 2 /* tray_temporal_step_async, tray_temporal_var_step_async */
/* The library's own choice, for a launch of `kind` on a scene with a BVH and without
 * TRAY_FLAG_LINEAR_SCAN, between traversing the tree (*bvh_out = 1) and the linear scan for every
 * ray (0): the traversal stacks, 1 KiB per slot, must fit into 64 KiB of LDS beside what the kernel
 * holds there itself (nothing / 8 KiB of parked colours / 64 bytes of the record's reduction).
 * `stack_depth` is tray_scene_info's; the stacks hold 3 slots more. Both sides give the same bits.
 * Host only: no device is touched. */
int tray_debug_query_traversal(int32_t kind, int32_t stack_depth, int32_t *bvh_out);

/* A synchronous copy of the scene's BVH nodes as they are on the device, for the tests of
 * tray_scene_update.h: n_nodes (tray_scene_info) records of 128 bytes, Bvh4Node of
 * tray_amd/csrc/bvh.hpp: float box[3][2][4] (per axis the low and the high planes of the four child
 * slots; an unused slot has +inf / -inf), uint32 ref[4] (an inner node's index, 0x8000 | a leaf's
 * index, or 0xFFFF for an unused slot), uint32 pad[4]. Waits for the renders and updates enqueued
 * on the scene. *bytes_out receives the size of the array, 0 for a scene without a tree; the copy is
 * made when capacity_bytes holds it (TRAY_ERR_INVALID_ARGUMENT when it does not; a NULL nodes_out with
 * capacity 0 asks for the size alone). */
int tray_debug_scene_nodes(tray_scene_t scene, void *nodes_out, size_t capacity_bytes, size_t *bytes_out);
/* What a leaf reference of those nodes leads to, which no update changes: leaves_out receives, per
 * leaf, (first slot << 3) | sphere count, and slots_out, per slot of the tree, the list index of the
 * sphere kept there (the out-of-tree spheres hold the last slots). *n_leaves_out and *n_slots_out
 * receive the counts, both 0 without a tree; each array is copied when its capacity (in entries)
 * holds it and its pointer is not NULL. Synchronous. */
int tray_debug_scene_leaves(tray_scene_t scene, int32_t *leaves_out, int32_t leaves_capacity, int32_t *slots_out,
                            int32_t slots_capacity, int32_t *n_leaves_out, int32_t *n_slots_out);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_DEBUG_H */
