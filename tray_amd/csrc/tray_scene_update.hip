// tray_scene_update.hip — include/tray_scene_update.h: new centres and radii for an
// uploaded scene and the refit of its BVH, in one launch of one workgroup.
//
// The trees are small (C2: about 170 nodes, C5: a few hundred, at most 32,768), so the
// job is bound by latency, not by bandwidth. One workgroup makes a refusal all-or-nothing
// without a second launch (nothing is stored before the check has finished) and needs
// no fence or atomic between workgroups: the phases are separated by __syncthreads(), which
// orders one workgroup's global stores before its later loads. The node boxes are worked on
// in global memory (the workgroup's CU holds them in its L1 and the L2) for every tree size:
// one path instead of an LDS path for the trees of at most 512 nodes and this one for the
// rest; DESIGN.md 8u has what a launch takes.
//
// The box arithmetic is tray_bvh.cpp's: (c - |R|) - pad and (c + |R|) + pad, two roundings
// each (this unit is compiled without FMA contraction, and nothing here multiplies), then
// outward to float. A node's box is the float min / max of its children's boxes: the builder
// takes the double union first and rounds then, and rounding is monotone, so both agree.
//
// The header's two entry points are at the end of the file; they reach the scene through
// tray_scene.hpp.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tray_scene_update.h"
#include "bvh.hpp"
#include "tray_scene.hpp"

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

namespace {

constexpr int kUpdateThreads = 1024;

// The nearest float not above / not below v, as Builder::down / up (tray_bvh.cpp): convert,
// compare back in double, step one float. |v| is at most M (1 + 4e-6) <= 2^28 (1 + 4e-6) here,
// so the step never leaves the finite floats; the float next to +-0 is the smallest subnormal.
__device__ __forceinline__ float step_float(float f, bool up) {
    const uint32_t b = __float_as_uint(f);
    if ((b & 0x7FFFFFFFu) == 0) return __uint_as_float(up ? 0x00000001u : 0x80000001u);
    const bool away = (f > 0.0f) == up;  // away from zero: the bit pattern grows
    return __uint_as_float(away ? b + 1u : b - 1u);
}
__device__ __forceinline__ float round_down(double v) {
    const float f = (float)v;
    return (double)f > v ? step_float(f, false) : f;
}
__device__ __forceinline__ float round_up(double v) {
    const float f = (float)v;
    return (double)f < v ? step_float(f, true) : f;
}

__global__ __launch_bounds__(kUpdateThreads) void scene_update_kernel(const SceneUpdateArgs a) {
    __shared__ int s_refused, s_first;
    __shared__ unsigned long long s_extent;  // the bits of a non-negative double: ordered as integers
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        s_refused = 0;
        s_first = 0x7FFFFFFF;
        s_extent = 0ull;
    }
    __syncthreads();

    // 1. The check (include/tray_scene_update.h section 2). Count, minimum and maximum: no order in them.
    {
        int refused = 0, first = 0x7FFFFFFF;
        double extent = 0.0;
        for (int i = tid; i < a.n; i += kUpdateThreads) {
            const double* s = a.src + 4 * (size_t)i;
            const double r = fabs(s[3]);
            bool bad = false;
            for (int k = 0; k < 3; ++k) {
                const double lo = fabs(s[k] - r), hi = fabs(s[k] + r);
                bad = bad || !(lo <= a.bound) || !(hi <= a.bound);  // also a NaN
                if (lo < HUGE_VAL && lo > extent) extent = lo;
                if (hi < HUGE_VAL && hi > extent) extent = hi;
            }
            if (bad && a.has_bvh) {
                ++refused;
                first = i < first ? i : first;
            }
        }
        if (refused) {
            atomicAdd(&s_refused, refused);
            atomicMin(&s_first, first);
        }
        if (extent > 0.0) atomicMax(&s_extent, (unsigned long long)__double_as_longlong(extent));
    }
    __syncthreads();
    const int n_refused = s_refused;
    if (tid == 0) {
        tray_scene_update_record rec;
        rec.applied = n_refused == 0 ? 1 : 0;
        rec.n_refused = n_refused;
        rec.first_refused = n_refused ? s_first : -1;
        rec.reserved = 0;
        rec.extent = __longlong_as_double((long long)s_extent);
        rec.bound = a.has_bvh ? a.bound : 0.0;
        *a.record = rec;
    }
    if (n_refused) return;  // the whole workgroup: nothing of the scene has been written

    // 2. Geometry, in list order and in slot order, with tray_scene_upload's expressions.
    for (int i = tid; i < a.n; i += kUpdateThreads) {
        const double* s = a.src + 4 * (size_t)i;
        a.geo[i] = make_double4(s[0], s[1], s[2], s[3] * s[3]);
        a.mat[i].radius = s[3];
        a.mat[i].rinv = 1.0 / s[3];
    }
    if (!a.has_bvh) return;
    for (int j = tid; j < a.n_slots; j += kUpdateThreads) {
        const int i = a.bidx[j];
        if (i < 0 || i >= a.n) continue;
        const double* s = a.src + 4 * (size_t)i;
        a.bgeo[j] = make_double4(s[0], s[1], s[2], s[3] * s[3]);
        a.bmat[j].radius = s[3];
        a.bmat[j].rinv = 1.0 / s[3];
    }

    // 3. Leaf boxes: one (node, child slot) pair per lane. Reads the caller's geometry only.
    for (int q = tid; q < a.n_nodes * kBvhWidth; q += kUpdateThreads) {
        Bvh4Node& node = a.nodes[q / kBvhWidth];
        const int slot = q % kBvhWidth;
        const uint32_t ref = node.ref[slot];
        if (ref == kBvhNone || !(ref & kBvhLeafBit)) continue;
        const int32_t leaf = a.leaves[ref & (kBvhLeafBit - 1u)];
        const int first = leaf >> 3, count = leaf & 7;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int j = first; j < first + count; ++j) {
            const double* s = a.src + 4 * (size_t)a.bidx[j];
            const double r = fabs(s[3]);
            for (int k = 0; k < 3; ++k) {
                const float l = round_down((s[k] - r) - a.pad), h = round_up((s[k] + r) + a.pad);
                lo[k] = l < lo[k] ? l : lo[k];
                hi[k] = h > hi[k] ? h : hi[k];
            }
        }
        for (int k = 0; k < 3; ++k) {
            node.box[k][0][slot] = lo[k];
            node.box[k][1][slot] = hi[k];
        }
    }

    // 4. Inner boxes, a level at a time from the deepest nodes up: the box of a slot that refers
    // to node c is the union of c's child boxes (an unused slot's +inf / -inf is neutral).
    for (int level = 0; level < a.n_levels; ++level) {
        __syncthreads();  // the leaf boxes and the levels below are written
        const int begin = (int)a.schedule[level], end = (int)a.schedule[level + 1];
        for (int it = begin + tid; it < end; it += kUpdateThreads) {
            const uint32_t q = a.schedule[a.n_levels + 1 + it];
            Bvh4Node& node = a.nodes[q / kBvhWidth];
            const int slot = (int)(q % kBvhWidth);
            const Bvh4Node& child = a.nodes[node.ref[slot]];
            for (int k = 0; k < 3; ++k) {
                float lo = child.box[k][0][0], hi = child.box[k][1][0];
                for (int c = 1; c < kBvhWidth; ++c) {
                    lo = child.box[k][0][c] < lo ? child.box[k][0][c] : lo;
                    hi = child.box[k][1][c] > hi ? child.box[k][1][c] : hi;
                }
                node.box[k][0][slot] = lo;
                node.box[k][1][slot] = hi;
            }
        }
    }
}

}  // namespace

// The order in which the inner children's boxes are recomputed, from the child references
// `refs` (n_nodes x kBvhWidth, as in Bvh4Node::ref): n_levels + 1 level starts, then the
// items node * kBvhWidth + slot of every slot that refers to an inner node, sorted by the
// level of that node (0: all its children are leaves; else 1 + the highest level among its
// inner children). Level l's items read only boxes that the leaves and the levels below l
// wrote. Nodes are emitted pre-order (a child's index exceeds its parent's).
static std::vector<uint32_t> refit_schedule(const uint32_t* refs, int32_t n_nodes, int32_t* n_levels) {
    const auto inner = [](uint32_t ref) { return ref != kBvhNone && !(ref & kBvhLeafBit); };
    std::vector<int32_t> level((size_t)std::max(n_nodes, 0), 0);
    std::vector<uint32_t> items;  // node * kBvhWidth + slot of the slots that refer to an inner node
    int32_t top = -1;             // the highest level that has an item
    for (int32_t node = n_nodes - 1; node >= 0; --node)  // children first: their indices are higher
        for (int k = 0; k < kBvhWidth; ++k) {
            const uint32_t ref = refs[(size_t)node * kBvhWidth + k];
            if (!inner(ref) || (int32_t)ref <= node || (int32_t)ref >= n_nodes) continue;
            level[node] = std::max(level[node], level[ref] + 1);
            top = std::max(top, level[ref]);
            items.push_back((uint32_t)node * kBvhWidth + (uint32_t)k);
        }
    *n_levels = top + 1;
    // A counting sort by level: the starts, then each item at its level's next free place.
    const size_t head = (size_t)*n_levels + 1;
    std::vector<uint32_t> out(head + items.size(), 0u);
    for (uint32_t q : items) ++out[(size_t)level[refs[q]] + 1];
    for (size_t l = 1; l < head; ++l) out[l] += out[l - 1];
    std::vector<uint32_t> next(out.begin(), out.begin() + (std::ptrdiff_t)head);
    for (uint32_t q : items) out[head + next[(size_t)level[refs[q]]]++] = q;
    return out;
}

// What both forms check before any device work; `geometry` and `record` are the device's
// for the asynchronous form and the host's for the synchronous one.
static int validate_update(tray_scene_t sc, const double* geometry, int32_t n_spheres,
                           const tray_scene_update_record* record) {
    if (!sc) return fail(TRAY_ERR_INVALID_ARGUMENT, "null scene");
    if (!geometry) return fail(TRAY_ERR_INVALID_ARGUMENT, "null geometry");
    if (!record) return fail(TRAY_ERR_INVALID_ARGUMENT, "null record");
    if (n_spheres != sc->n)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "n_spheres is " + std::to_string(n_spheres) + ", the scene has " +
                                                   std::to_string(sc->n) + ": an update keeps the sphere count");
    return TRAY_OK;
}

}  // namespace tray

using namespace tray;

#pragma GCC visibility push(default)
extern "C" {

int tray_scene_update_async(tray_scene_t sc, const double* geometry_device, int32_t n_spheres,
                            tray_scene_update_record* record_device, void* stream_arg) {
    const int rc = validate_update(sc, geometry_device, n_spheres, record_device);
    if (rc) return rc;
    const hipStream_t stream = static_cast<hipStream_t>(stream_arg);
    TRAY_HIP(hipSetDevice(sc->device));
    std::lock_guard<std::mutex> lk(sc->mu);
    if (sc->has_bvh && !sc->schedule) {  // the first update: topology only, so built once
        int32_t n_levels = 0;
        const std::vector<uint32_t> sched = refit_schedule(sc->refs.data(), sc->n_nodes, &n_levels);
        uint32_t* dev = nullptr;
        TRAY_HIP(hipMalloc(reinterpret_cast<void**>(&dev), sched.size() * sizeof(uint32_t)));
        const hipError_t e = hipMemcpy(dev, sched.data(), sched.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return hip_fail(e, "level schedule");
        }
        sc->schedule = dev;
        sc->n_levels = n_levels;
    }
    if (!sc->updated) TRAY_HIP(hipEventCreateWithFlags(&sc->updated, hipEventDisableTiming));
    // Renders enqueued so far read the old geometry: the update waits for each context's last
    // one (on the device). Their candidate lists and work orders were the old geometry's.
    for (LaunchCtx* c : sc->ctx) {
        if (c->launched && c->last_stream != stream) TRAY_HIP(hipStreamWaitEvent(stream, c->done, 0));
        c->cand_valid = c->order_valid = false;
    }
    SceneUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.src = geometry_device;
    a.n = sc->n;
    a.geo = sc->geo;
    a.mat = sc->mat;
    a.has_bvh = sc->has_bvh ? 1 : 0;
    if (sc->has_bvh) {
        a.n_slots = sc->n_slots;
        a.bgeo = sc->bgeo;
        a.bmat = sc->bmat;
        a.bidx = sc->bidx;
        a.nodes = sc->nodes;
        a.n_nodes = sc->n_nodes;
        a.leaves = sc->leaves;
        a.schedule = sc->schedule;
        a.n_levels = sc->n_levels;
        a.bound = sc->bvh_bound;
        a.pad = 4e-6 * sc->bvh_bound;  // Builder::pad (tray_bvh.cpp)
    }
    a.record = record_device;
    // One workgroup: check, then (unless refused) geometry, leaf boxes, inner boxes level by level.
    hipLaunchKernelGGL(scene_update_kernel, dim3(1), dim3(kUpdateThreads), 0, stream, a);
    TRAY_HIP(hipGetLastError());
    const hipError_t e = hipEventRecord(sc->updated, stream);
    if (e != hipSuccess) {  // nothing marks the update's end: wait for it here
        (void)hipStreamSynchronize(stream);
        return hip_fail(e, "hipEventRecord");
    }
    sc->update_recorded = true;
    return TRAY_OK;
}

int tray_scene_update(tray_scene_t sc, const double* geometry_host, int32_t n_spheres,
                      tray_scene_update_record* record_out) {
    int rc = validate_update(sc, geometry_host, n_spheres, record_out);
    if (rc) return rc;
    TRAY_HIP(hipSetDevice(sc->device));
    const size_t geo_bytes = sizeof(double) * 4 * (size_t)n_spheres;
    uint8_t* staging = nullptr;  // the record, then the geometry
    TRAY_HIP(hipMalloc(reinterpret_cast<void**>(&staging), sizeof(tray_scene_update_record) + geo_bytes + 32));
    tray_scene_update_record* record_device = reinterpret_cast<tray_scene_update_record*>(staging);
    double* geometry_device = reinterpret_cast<double*>(staging + sizeof(tray_scene_update_record));
    hipError_t e = geo_bytes ? hipMemcpy(geometry_device, geometry_host, geo_bytes, hipMemcpyHostToDevice) : hipSuccess;
    rc = e == hipSuccess ? tray_scene_update_async(sc, geometry_device, n_spheres, record_device, nullptr)
                         : hip_fail(e, "geometry staging");
    if (rc == TRAY_OK) {
        e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess) e = hipMemcpy(record_out, record_device, sizeof(*record_out), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "scene update");
    }
    (void)hipFree(staging);
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop
