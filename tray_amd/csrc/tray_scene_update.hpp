// Internal launch interface between the C-ABI glue (tray_abi.hip) and the scene
// update kernel (tray_scene_update.hip: include/tray_scene_update.h). Host side
// only. Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/tray_scene_update.h"
#include "bvh.hpp"
#include "tray_kernel.hpp"

namespace tray {

// The scene's arrays as tray_scene_upload laid them out, and what the update reads.
struct SceneUpdateArgs {
    const double* src;  // n x {cx, cy, cz, radius}, list order
    int32_t n;
    double4* geo;       // list order
    MatRec* mat;
    int32_t has_bvh;    // 0: the fields below are unused
    int32_t n_slots;
    double4* bgeo;      // slot order
    MatRec* bmat;
    const int32_t* bidx;
    Bvh4Node* nodes;
    int32_t n_nodes;
    const int32_t* leaves;
    const uint32_t* schedule;  // refit_schedule, on the device
    int32_t n_levels;
    double bound;  // M of the upload
    double pad;    // 4e-6 * M, computed on the host as the builder does
    tray_scene_update_record* record;
};

// The order in which the inner children's boxes are recomputed, from the child references
// `refs` (n_nodes x kBvhWidth, as in Bvh4Node::ref): n_levels + 1 level starts, then the
// items node * kBvhWidth + slot of every slot that refers to an inner node, sorted by the
// level of that node (0: all its children are leaves; else 1 + the highest level among its
// inner children). Level l's items read only boxes that the leaves and the levels below l
// wrote. Nodes are emitted pre-order (a child's index exceeds its parent's).
std::vector<uint32_t> refit_schedule(const uint32_t* refs, int32_t n_nodes, int32_t* n_levels);

// One workgroup: check, then (unless refused) geometry, leaf boxes, inner boxes level by level.
hipError_t launch_scene_update(const SceneUpdateArgs& a, hipStream_t stream);

}  // namespace tray
