/*
 * tray_scene_update.h — moving spheres: new centres and radii for an uploaded
 * scene, written in place on the device, with the scene's BVH refitted to them.
 * One kernel launch replaces tray_scene_release + tray_scene_upload per frame of
 * an animation, takes its geometry from DEVICE memory (a simulation's tensor),
 * and keeps the scene's launch contexts (work queue, sample and candidate
 * buffers).
 *
 * An addition beside tray.h (ABI 6, unchanged) and the other feature headers,
 * under the same rules: plain C99, tray_status / tray_last_error, arguments
 * validated before any device work.
 *
 * WHY THE FRAMES KEEP THEIR BITS. The BVH is exact-culling (tray_amd/csrc/tray_bvh.cpp): a tree whose
 * boxes contain their spheres returns the hit of the reference's linear scan,
 * whatever its topology. The update keeps the topology of the upload, recomputes
 * every leaf's box from the moved spheres with the builder's own arithmetic and
 * takes unions up the tree. So every render and query of the updated scene has
 * exactly the bits it has on a scene freshly uploaded with the new geometry. What
 * a stale topology can cost is time, never bits (DESIGN.md 8u has measurements).
 *
 * 1. WHAT MAY CHANGE. Centres and radii only. The sphere count, the materials,
 *    the background, the tree's topology, the leaf size and the out-of-tree
 *    spheres chosen at the upload all stay, and so does the scene's bound M
 *    (tray_scene_info.bound): tray_scene_get_info reports the same facts before
 *    and after.
 *
 * 2. THE CHECK, on a scene with a tree (has_bvh == 1). For every sphere and every
 *    axis, in FP64, as the builder does it:
 *        lo = c - |R|,  hi = c + |R|;   |lo| <= M  and  |hi| <= M
 *    with M the bound of the UPLOAD. A NaN or an infinity fails it. M cannot grow:
 *    the boxes' padding 4e-6 x M and the FP32 slab test's error bound are tied to
 *    it. If any sphere fails, the update is REFUSED: nothing but the record is
 *    written, the scene keeps its geometry and tree, and the caller uploads the new
 *    geometry as a new scene. A scene without a tree (has_bvh == 0) takes any
 *    values, NaN included, as tray_scene_upload does; its record has bound = 0.
 *
 * 3. WHAT IS WRITTEN on success, with the expressions of tray_scene_upload, so with
 *    its bits: per sphere {c, R x R}, the radius and the correctly rounded 1.0 / R
 *    of its material record, the same values in the tree's slot order, and the box
 *    of every used child slot of every node (include/tray_debug.h,
 *    tray_debug_scene_nodes): for a leaf, per axis,
 *        low  = min over its spheres of down((c - |R|) - pad)
 *        high = max over its spheres of   up((c + |R|) + pad),   pad = 4e-6 x M,
 *    two separately rounded FP64 operations each, then the nearest float not above
 *    (down) / not below (up) the double; for an inner child the float min / max of
 *    that node's child boxes. Unused child slots keep their empty box. An update
 *    with the uploaded geometry therefore rewrites every byte with the value it has.
 *
 * 4. ORDERING. tray_scene_update_async only enqueues on `stream` (a hipStream_t,
 *    or NULL for the device's null stream); the first update of a scene also
 *    builds the tree's level schedule on the host and copies it to the device
 *    (synchronously, once). Before the launch `stream` is made to wait, on the
 *    device, for the last render of each of the scene's launch contexts, on whatever
 *    stream it ran, so renders enqueued BEFORE the call see the old geometry. Ray
 *    queries (tray_query.h and the headers built on it) use no launch context: one
 *    enqueued before the call on another stream, and every render or query enqueued
 *    AFTER the call on another stream, is the caller's to order against the update
 *    (an event recorded on `stream` after the call). The call must not race with
 *    tray_scene_release of the same scene.
 *
 * 5. STATE DERIVED FROM THE OLD GEOMETRY. The library's own (the primary-ray
 *    candidate lists and the work order of the scene's launch contexts) is
 *    invalidated by the call, also by a refused one. The caller's is stale and the
 *    caller's: a tray_temporal_state holds index and depth planes of the old
 *    geometry, which tray_temporal_motion.h carries across the update given the
 *    geometry the scene held before it (tray_temporal_step_async itself assumes a
 *    static scene); adaptive and progressive accumulators hold means of the old
 *    scene's frames and are the caller's to reset.
 */
#ifndef TRAY_SCENE_UPDATE_H
#define TRAY_SCENE_UPDATE_H

#include <stdint.h>

#include "tray.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tray_scene_update_record { /* 32 bytes, written by the device */
    int32_t applied;       /* 1: the scene now holds the new geometry; 0: refused, the scene is untouched */
    int32_t n_refused;     /* spheres that failed the check of section 2 */
    int32_t first_refused; /* the lowest list index among them, -1 if none */
    int32_t reserved;      /* 0 */
    double extent;         /* max over the new spheres and axes of |lo| and |hi|; NaN and infinite values are left out */
    double bound;          /* the scene's M the spheres were checked against; 0 without a tree */
} tray_scene_update_record;

/* One launch on `stream` of the scene's device. geometry_device holds n_spheres x 4 doubles
 * {cx, cy, cz, radius} in list order, 8-byte aligned, and is not written; record_device receives the
 * record, in stream order. The sums of the record do not depend on an order: it is bit-repeatable.
 *
 * Errors, before anything is enqueued: TRAY_ERR_INVALID_ARGUMENT for a null scene, geometry or
 * record, and for an n_spheres other than the scene's. A refused update is TRAY_OK: read the record. */
int tray_scene_update_async(tray_scene_t scene, const double *geometry_device, int32_t n_spheres,
                            tray_scene_update_record *record_device, void *stream);

/* The same for geometry and a record in HOST memory: stages both through device memory and the call
 * above on the null stream, and returns when the update has run. */
int tray_scene_update(tray_scene_t scene, const double *geometry_host, int32_t n_spheres,
                      tray_scene_update_record *record_out);

#ifdef __cplusplus
}
#endif

#endif /* TRAY_SCENE_UPDATE_H */
