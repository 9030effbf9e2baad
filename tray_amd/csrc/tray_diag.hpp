// tray_diag.hpp — everything that exists only for a diagnostic build of the megakernel
// (render_kernel, tray_kernel.hip; device only): the phase profile and its sub-modes, the
// timeline, the primary-ray and ground censuses, the cost probes and the ISA census marks.
//
// render_kernel holds one Diag and calls a hook at each place a diagnostic build looks at: a
// hook is named for that place, not for the build that uses it, and its body holds the
// conditionals. A hook is handed what it reads (the lane, masks, a lane's state); none reaches
// into the kernel's locals. In the product build Diag has no members, every hook is empty, and
// the kernel calls none: each call stands under `if constexpr` of the hook's own constant
// (Diag::kNodeStep for node_step), true only in the builds, and where the body is all under kStats
// only in the instance, in which the hook has a body. Even an empty forced-inline call (or an
// empty local) in the loop changes the device code: the compiler inlines behind its first
// simplification passes, which shape the loop differently around a call. So the
// product, and every instance of a diagnostic build that a build's hooks leave alone, compile
// as if the hooks were not there. Never part of a timed build: the stamps' waits serialise the phases.
//
//   flags                                        tool                       what it adds
//   -DTRAY_PROFILE                               tools/phase_profile.py     ProfSlot counters in stats[3..29]
//     with -DTRAY_PROFILE_BEGIN                    --begin                  slots 10-12: the scatter step's sources
//     with -DTRAY_PROFILE_REFILL                   --refill-split           slots 10, 13-15: the refill's parts
//     with -DTRAY_PROFILE_CANDWAIT                                          slot 15: the candidate record's wait
//     with -DTRAY_PROFILE_MATERIAL                 --material               prof_material, behind the stamps
//     with -DTRAY_TRIGGERS_ALL                                              the stats instance (a generic one) runs the
//                                                                           plain-frame instance's cost-rule triggers
//   -DTRAY_PROFILE_TIMELINE                      tools/timeline.py          a record per wave from stats[32]
//   -DTRAY_STATS_PRIMARY                         tools/primary_share.py     Stats fields, stats[3..7]
//   -DTRAY_STATS_GROUND                          tools/ground_share.py      Stats fields, stats[3..10]
//   -DTRAY_PROBE_{REFILL,NODE,LEAF,SHADE,SHADE64}=N  tools/ab_bench.py      N extra instructions in a phase
//   -DTRAY_CENSUS                                tools/isa_census.py        TRAY_MARK comments in the assembly
// `make diag-asm` (tray_amd/Makefile) compiles every one of them.
#pragma once

#if defined(TRAY_PROFILE_BEGIN) && (defined(TRAY_PROFILE_REFILL) || defined(TRAY_PROFILE_CANDWAIT))
#error "TRAY_PROFILE_BEGIN shares profile slots with TRAY_PROFILE_REFILL / TRAY_PROFILE_CANDWAIT"
#endif
#if defined(TRAY_STATS_PRIMARY) && defined(TRAY_STATS_GROUND)
#error "TRAY_STATS_PRIMARY and TRAY_STATS_GROUND both count in Stats::nodes / leaves and in stats[3..7]"
#endif

#if !defined(TRAY_PROFILE) && (defined(TRAY_PROFILE_BEGIN) || defined(TRAY_PROFILE_REFILL) || \
                               defined(TRAY_PROFILE_CANDWAIT) || defined(TRAY_PROFILE_MATERIAL))
#error "TRAY_PROFILE_BEGIN / _REFILL / _CANDWAIT / _MATERIAL are sub-modes of TRAY_PROFILE: define it too"
#endif

#include "tray_device.hpp"

namespace tray {

// ISA census build only (-DTRAY_CENSUS, tools/isa_census.py): a comment in the
// assembly where each phase of the BVH loop starts, so the census can attribute
// instructions to phases. Never in a timed build.
#ifdef TRAY_CENSUS
#define TRAY_MARK(name) asm volatile(";@phase " name);
#else
#define TRAY_MARK(name)
#endif

// The phase profile's slots (-DTRAY_PROFILE): per-wave counters in LDS (lane 0 adds: registers
// would change the kernel being measured), added at the wave's end into the stats buffer, which
// must then hold 30 counters: slots 0-15 land in stats[3..18], slots 16-23 in stats[22..29]
// (stats[19..21] hold the wave lifetimes, kernel_end). tools/phase_profile.py names them by
// position. A sub-mode re-uses slots, under the names below the table:
//   -DTRAY_PROFILE_BEGIN     10-12  (passes << 40) + lanes of the scatter step's sources
//   -DTRAY_PROFILE_REFILL    10, 13-15  cycles of the refill's parts (all inside slot 0's)
//   -DTRAY_PROFILE_CANDWAIT  15
enum ProfSlot : int {
    kProfRefill = 0,           // cycles: the refill, its end half included (timeline: lone-path phase 0)
    kProfNode = 1,             // cycles: the node steps and the drain (timeline: phase 1)
    kProfLeaf = 2,             // cycles: the leaf phase (timeline: phase 2)
    kProfShade = 3,            // cycles: the shade phase (timeline: phase 3)
    kProfNodeSteps = 4,        // node steps
    kProfNodeLanes = 5,        //   their traversing lanes
    kProfLeafPhases = 6,       // leaf phases
    kProfLeafLanes = 7,        //   their lanes
    kProfShadePhases = 8,      // shade phases
    kProfShadeLanes = 9,       //   their lanes
    kProfLoopIters = 10,       // loop iterations
    kProfLeafWaitLanes = 11,   // per node step: lanes waiting for the leaf phase
    kProfShadeWaitLanes = 12,  // per node step: lanes waiting for the shade phase
    kProfRefillPhases = 13,    // refills that assigned an item
    kProfRefillLanes = 14,     //   their lanes
    kProfBeginSteps = 15,      // scatter steps whose begin part sets a segment up
    kProfRefillEnd = 16,       // cycles: the refill's end half (also inside slot 0's)
    kProfRefillEndPhases = 17,
    kProfRefillEndLanes = 18,
    kProfScatter = 19,         // cycles: the scatter step's scatter part (timeline: with the shading)
    kProfScatterSteps = 20,
    kProfScatterLanes = 21,
    kProfAbsorbedLanes = 22,   // lanes absorbed in the scatter part
    kProfBegin = 23,           // cycles: the scatter step's begin part (timeline: with the refill)
    kProfSlots = 24,
    // -DTRAY_PROFILE_BEGIN (tools/phase_profile.py --begin)
    kProfMarkedByShade = 10,   // hits marked by the shade phase, (passes << 40) + lanes
    kProfMarkedByRefill = 11,  // hits marked by the refill's camera-hit shading, likewise
    kProfScatterSources = 12,  // (refills that found lanes marked by the shade phase just before << 40)
                               // + lanes of the scatter steps
    // -DTRAY_PROFILE_REFILL (--refill-split)
    kProfRefillAssign = 10,    // cycles: item assignment (pool, queue)
    kProfRefillCamera = 13,    // cycles: decoding + camera ray (draw block, discs)
    kProfRefillHit = 14,       // cycles: out-of-tree spheres + candidates (or the FP32 setup)
    kProfRefillShade = 15,     // cycles: shading of the candidate-answered camera rays
    // -DTRAY_PROFILE_CANDWAIT
    kProfCandWait = 15,        // cycles: the candidate record's exposed latency after the camera ray
};
// The timeline build times the phases of a wave's lone last path into tl_ph[0..3] (refill, node
// steps, leaves, shading): the phase a slot's stamp pair counts with there.
__device__ constexpr int tl_phase(ProfSlot slot) {
    return slot == kProfScatter ? (int)kProfShade : slot == kProfBegin ? (int)kProfRefill : (int)slot;
}

// Which diagnostic build this is, for the hooks' constants in Diag (a profile build counts in LDS
// and switches the censuses' per-lane counters off: Stats, tray_device.hpp).
#if defined(TRAY_PROFILE)
constexpr bool kBuildProf = true;
#else
constexpr bool kBuildProf = false;
#endif
#if defined(TRAY_PROFILE_BEGIN)
constexpr bool kBuildBegin = true;
#else
constexpr bool kBuildBegin = false;
#endif
#if defined(TRAY_PROFILE_REFILL)
constexpr bool kBuildRefill = true;
#else
constexpr bool kBuildRefill = false;
#endif
#if defined(TRAY_PROFILE_CANDWAIT)
constexpr bool kBuildCandwait = true;
#else
constexpr bool kBuildCandwait = false;
#endif
#if defined(TRAY_PROFILE_TIMELINE)
constexpr bool kBuildTl = true;
#else
constexpr bool kBuildTl = false;
#endif
#if defined(TRAY_STATS_PRIMARY) && !defined(TRAY_PROFILE)
constexpr bool kBuildPrim = true;
#else
constexpr bool kBuildPrim = false;
#endif
#if defined(TRAY_STATS_GROUND) && !defined(TRAY_PROFILE)
constexpr bool kBuildGround = true;
#else
constexpr bool kBuildGround = false;
#endif

// Diagnostic build only (-DTRAY_PROFILE -DTRAY_PROFILE_MATERIAL): the divergence
// census of the scatter step's passes. Per site (the marked lanes that come 0: from
// the refill's camera-hit shading, 1: from the shade phase) and per class of lane (0
// miss/sky and 1 hit at the last level: none since the end half serves them, 2
// Lambertian, 3 Metal without fuzz, 4 Metal with fuzz, 5 Dielectric): [c] passes with such a lane, [6 + c] such lanes; [12 + b] passes
// executing b of the three material bodies (b = 0..3); [16] passes, [17] lanes;
// [18 + h] / [22 + h] passes with 1, 2-3, 4-7, >= 8 Dielectric / Metal lanes.
// Added with global atomics after the per-wave stamps (stats[32 + 2 x waves + k]).
#ifdef TRAY_PROFILE_MATERIAL
constexpr int kMatCounters = 26;
__device__ __forceinline__ void prof_material(int site, bool active, int32_t slot, uint32_t bounce, int32_t max_depth,
                                              const MatRec* bmat, uint32_t lane, unsigned long long* pm) {
    int cls = -1;
    if (active) {
        if (slot < 0) cls = 0;
        else if (bounce + 1u >= (uint32_t)max_depth) cls = 1;
        else {
            const MatRec& m = bmat[slot];
            cls = m.type == kLambertian ? 2 : m.type == kDielectric ? 5 : m.param > 0.0 ? 4 : 3;
        }
    }
    unsigned long long* c = pm + site * kMatCounters;
    int bodies = 0;
    for (int k = 0; k < 6; ++k) {
        const uint64_t m = __ballot(cls == k);
        if (lane == 0 && m) {
            atomicAdd(c + k, 1ull);
            atomicAdd(c + 6 + k, (unsigned long long)__popcll(m));
        }
    }
    bodies = (__ballot(cls == 2) ? 1 : 0) + (__ballot(cls == 3 || cls == 4) ? 1 : 0) + (__ballot(cls == 5) ? 1 : 0);
    const int n_di = __popcll(__ballot(cls == 5)), n_me = __popcll(__ballot(cls == 3 || cls == 4));
    const int n_active = __popcll(__ballot(active));  // ahead of the branch: inside it only lane 0 votes
    if (lane == 0) {
        if (n_di) atomicAdd(c + 18 + (n_di >= 8 ? 3 : n_di >= 4 ? 2 : n_di >= 2 ? 1 : 0), 1ull);
        if (n_me) atomicAdd(c + 22 + (n_me >= 8 ? 3 : n_me >= 4 ? 2 : n_me >= 2 ? 1 : 0), 1ull);
        atomicAdd(c + 12 + bodies, 1ull);
        atomicAdd(c + 16, 1ull);
        atomicAdd(c + 17, (unsigned long long)n_active);
    }
}
#endif

// Diagnostic build only (-DTRAY_PROFILE_TIMELINE, stats instance; tools/timeline.py):
// per wave, busy lanes integrated over time in kTlTicks buckets of the shader clock
// (s_memtime, read once per loop iteration; the 100 MHz constant clock, s_memrealtime,
// only at the wave's start, dry point and end: read per iteration it stalled waves),
// constant clock, relative to the wave's start, plus its start, end, the time its
// queue ran dry and the chunks it took. Record of wave w at stats[32 + w x kTlStride]:
// [0] start, [1] end, [2] exhausted (ticks after start), [3] chunks, [4..] buckets.
#ifdef TRAY_PROFILE_TIMELINE
// [0] start, [1] end, [2] dry (constant clock), [3] chunks, [4] / [5] shader clock at start / end,
// [6 ..] buckets; the last nine: the shader ticks the wave's lone last path spent in the
// refill, node-step, leaf and shading phases, when it became the wave's only path
// (shader ticks after the start) and its segments then, and that path's segments,
// pixel and sample at the end (its latency per segment with no other path in the wave).
constexpr uint32_t kTlBuckets = 1024, kTlTicks = 25000, kTlHdr = 6, kTlStride = kTlBuckets + kTlHdr;
#endif

// Cost probes (diagnostic builds only, never timed as the product): N extra
// independent VALU instructions in one phase, to measure what an instruction
// there costs (tools/ab_bench.py A/B against the plain build).
#define TRAY_PROBE_F32(n)                                                     \
    {                                                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) {                  \
            float t_;                                                         \
            asm volatile("v_add_f32_e64 %0, 1.0, 1.0" : "=v"(t_));            \
        }                                                                     \
    }
#define TRAY_PROBE_F64(n)                                                     \
    {                                                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) {                  \
            double t_;                                                        \
            asm volatile("v_add_f64 %0, 1.0, 1.0" : "=v"(t_));                \
        }                                                                     \
    }
// The probe sites: -DTRAY_PROBE_<SITE>=N puts N instructions where the kernel calls probe<site>()
// (FP32 adds; FP64 adds at kProbeShade64, which stands next to kProbeShade).
enum ProbeSite { kProbeRefill, kProbeNode, kProbeLeaf, kProbeShade, kProbeShade64 };
template <ProbeSite kSite>
constexpr bool kProbed = false  // whether this build probes the site: the kernel calls probe<site>() under it
#ifdef TRAY_PROBE_REFILL
                         || kSite == kProbeRefill
#endif
#ifdef TRAY_PROBE_NODE
                         || kSite == kProbeNode
#endif
#ifdef TRAY_PROBE_LEAF
                         || kSite == kProbeLeaf
#endif
#ifdef TRAY_PROBE_SHADE
                         || kSite == kProbeShade
#endif
#ifdef TRAY_PROBE_SHADE64
                         || kSite == kProbeShade64
#endif
    ;
template <ProbeSite kSite>
__device__ __forceinline__ void probe() {
#ifdef TRAY_PROBE_REFILL
    if constexpr (kSite == kProbeRefill) TRAY_PROBE_F32(TRAY_PROBE_REFILL)
#endif
#ifdef TRAY_PROBE_NODE
    if constexpr (kSite == kProbeNode) TRAY_PROBE_F32(TRAY_PROBE_NODE)
#endif
#ifdef TRAY_PROBE_LEAF
    if constexpr (kSite == kProbeLeaf) TRAY_PROBE_F32(TRAY_PROBE_LEAF)
#endif
#ifdef TRAY_PROBE_SHADE
    if constexpr (kSite == kProbeShade) TRAY_PROBE_F32(TRAY_PROBE_SHADE)
#endif
#ifdef TRAY_PROBE_SHADE64
    if constexpr (kSite == kProbeShade64) TRAY_PROBE_F64(TRAY_PROBE_SHADE64)
#endif
}

// The state of a diagnostic build and its hooks, in the order render_kernel calls them.
// kStats: the kernel's instrumented instance (the only one with a stats buffer).
struct Diag {
#if defined(TRAY_PROFILE) || defined(TRAY_PROFILE_TIMELINE)
    uint64_t t0;  // shader clock at the start of the running phase (phase_begin): one pair at a time;
                  // refill_done reads the refill's start from it (kProfRefillAssign)
#endif
#ifdef TRAY_PROFILE
    uint64_t t0_nested;        // and of the refill's end half, inside the refill (end_half_begin)
    unsigned long long* prof;  // this wave's kProfSlots counters in LDS
    uint64_t prof_start;       // constant clock at the wave's start
#endif
#ifdef TRAY_PROFILE_MATERIAL  // counts only (global atomics: its timings are not used)
    unsigned long long* prof_mat;
#endif
#ifdef TRAY_PROFILE_REFILL  // of the current refill: stamps after the item assignment, after the camera
    uint64_t prof_assigned, prof_cam, prof_hit, prof_shade0;  // ray / its Scene.Hit (per lane), before the end half
#endif
#ifdef TRAY_PROFILE_CANDWAIT
    uint64_t prof_wait;  // of the current refill, per lane: the wait + 1, or 0 for none
#endif
#ifdef TRAY_PROFILE_TIMELINE
    unsigned long long* tl;  // only the stats instance has a buffer; every use is under kStats
    uint64_t tl_start, tl_mt0, tl_prev, tl_acc;
    uint32_t tl_busy, tl_bucket, tl_chunks, tl_dry;
    bool tl_lone;
    uint64_t tl_ph[4];
#endif
#ifdef TRAY_STATS_GROUND
    uint32_t gcls;  // class of the lane's current segment (1/2: from an out-of-tree sphere, up / other)
#endif

#ifdef TRAY_PROFILE
    __device__ __forceinline__ void cnt(ProfSlot slot, unsigned long long v, uint32_t lane) {
        if (lane == 0) atomicAdd(prof + slot, v);
    }
#endif

    // Phase timing: phase_begin() ahead of a phase, phase_end<slot>() behind it; the pairs do not
    // nest (the start is one member, not a local of the kernel: see the top of the file). The
    // timeline build times only the wave's lone last path, into tl_ph[tl_phase(slot)].
    template <bool kStats>
    static constexpr bool kPhase = kBuildProf || (kBuildTl && kStats);
    template <bool kStats>
    __device__ __forceinline__ void phase_begin() {
#ifdef TRAY_PROFILE
        t0 = __builtin_amdgcn_s_memtime();
#elif defined(TRAY_PROFILE_TIMELINE)
        t0 = (kStats && tl_lone) ? __builtin_amdgcn_s_memtime() : 0;
#endif
    }
    template <ProfSlot kSlot, bool kStats>
    __device__ __forceinline__ void phase_end(uint32_t lane) {
#ifdef TRAY_PROFILE
        cnt(kSlot, __builtin_amdgcn_s_memtime() - t0, lane);
#elif defined(TRAY_PROFILE_TIMELINE)
        if (kStats && tl_lone) tl_ph[tl_phase(kSlot)] += __builtin_amdgcn_s_memtime() - t0;
#endif
    }
    template <bool kStats>
    static constexpr bool kKernelBegin = kBuildProf || ((kBuildTl || kBuildGround) && kStats);
    template <bool kStats>
    __device__ __forceinline__ void kernel_begin(const KernelParams& p, uint32_t lane) {
#ifdef TRAY_STATS_GROUND
        gcls = 0;
#endif
#ifdef TRAY_PROFILE
        __shared__ unsigned long long prof_lds[16 * kProfSlots];
        prof = prof_lds + kProfSlots * (threadIdx.x / 64u);
        if (lane == 0)
            for (int i = 0; i < kProfSlots; ++i) prof[i] = 0;
        prof_start = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef TRAY_PROFILE_MATERIAL
        prof_mat = p.stats + 32 + 2 * gridDim.x * (blockDim.x / 64u);
#endif
#ifdef TRAY_PROFILE_TIMELINE
        tl = kStats ? p.stats + 32 + (size_t)(blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u) * kTlStride : nullptr;
        tl_start = __builtin_amdgcn_s_memrealtime(), tl_mt0 = __builtin_amdgcn_s_memtime();
        tl_prev = tl_mt0, tl_acc = 0;
        tl_busy = 0, tl_bucket = 0, tl_chunks = 0, tl_dry = 0;
        tl_lone = false;
        for (int k = 0; k < 4; ++k) tl_ph[k] = 0;
#endif
    }

    // The top of a loop iteration. busy, segments, pixel, sample: the lane's path.
    template <bool kStats>
    static constexpr bool kIteration = (kBuildProf && !kBuildBegin) || (kBuildTl && kStats);
    template <bool kStats>
    __device__ __forceinline__ void iteration(uint32_t lane, bool exhausted, bool busy, uint32_t segments,
                                              uint32_t pixel, uint32_t sample) {
#ifdef TRAY_PROFILE_TIMELINE
        if constexpr (kStats) {  // p.stats is null in every other instance
            const uint64_t now = __builtin_amdgcn_s_memtime();
            const uint32_t b = min((uint32_t)((tl_prev - tl_mt0) / kTlTicks), kTlBuckets - 10u);
            if (b != tl_bucket) {
                if (lane == 0) tl[kTlHdr + tl_bucket] = tl_acc;
                tl_bucket = b;
                tl_acc = 0;
            }
            tl_acc += (now - tl_prev) * tl_busy;
            tl_prev = now;
            // The wave's last path after its queue ran dry: its segments so far, pixel, sample.
            const uint64_t m = __ballot(busy);
            if (exhausted && __popcll(m) == 1) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m);
                const uint32_t seg = __builtin_amdgcn_readlane(segments, l);
                const uint32_t pix = __builtin_amdgcn_readlane(pixel, l);
                const uint32_t smp = __builtin_amdgcn_readlane(sample, l);
                if (lane == 0) {
                    if (!tl_lone) {
                        tl[kTlHdr + kTlBuckets - 5] = now - tl_mt0;
                        tl[kTlHdr + kTlBuckets - 4] = seg;
                    }
                    tl[kTlHdr + kTlBuckets - 3] = seg;
                    tl[kTlHdr + kTlBuckets - 2] = pix;
                    tl[kTlHdr + kTlBuckets - 1] = smp;
                }
                tl_lone = true;
            }
        }
#endif
#if defined(TRAY_PROFILE) && !defined(TRAY_PROFILE_REFILL) && !defined(TRAY_PROFILE_BEGIN)
        cnt(kProfLoopIters, 1, lane);
#endif
#ifdef TRAY_PROFILE_CANDWAIT
        prof_wait = 0;
#endif
#ifdef TRAY_PROFILE_REFILL
        prof_cam = 0, prof_hit = 0;
#endif
    }

    // The refill. The global queue ran dry; the wave took n chunks from it.
    template <bool kStats>
    static constexpr bool kQueueDry = kBuildTl && kStats;
    template <bool kStats>
    __device__ __forceinline__ void queue_dry() {
#ifdef TRAY_PROFILE_TIMELINE
        if constexpr (kStats) tl_dry = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl_start);
#endif
    }
    template <bool kStats>
    static constexpr bool kChunksTaken = kBuildTl && kStats;
    __device__ __forceinline__ void chunks_taken(uint32_t n) {
#ifdef TRAY_PROFILE_TIMELINE
        tl_chunks += n;
#endif
    }
    // Items are assigned. fresh: this lane got one; cur: its Trav::cur.
    static constexpr bool kRefillAssigned = kBuildProf;
    template <bool kBVH>
    __device__ __forceinline__ void refill_assigned(uint32_t lane, bool fresh, uint32_t cur) {
#if defined(TRAY_PROFILE) && !defined(TRAY_PROFILE_REFILL)
        {
            const uint64_t m = __ballot(fresh);
            cnt(kProfRefillPhases, m != 0ull ? 1 : 0, lane);
            cnt(kProfRefillLanes, __popcll(m), lane);
#ifdef TRAY_PROFILE_BEGIN  // refills that find segments readied by the shade phase just before
            if constexpr (kBVH)
                cnt(kProfScatterSources, (uint64_t)(m != 0ull && __ballot(cur == kTravHit) != 0ull) << 40, lane);
#endif
        }
#endif
#ifdef TRAY_PROFILE_REFILL
        prof_assigned = __builtin_amdgcn_s_memtime();
#endif
    }
    // The lane's camera ray is built, its candidate record still in flight.
    template <bool kStats>
    static constexpr bool kCameraRayBuilt = kBuildRefill || kBuildCandwait || (kBuildGround && kStats);
    __device__ __forceinline__ void camera_ray_built() {
#ifdef TRAY_PROFILE_REFILL
        prof_cam = __builtin_amdgcn_s_memtime();
#endif
#ifdef TRAY_STATS_GROUND
        gcls = 0;
#endif
#ifdef TRAY_PROFILE_CANDWAIT
        {  // the candidate record's exposed latency after the camera ray
            const uint64_t w0 = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            prof_wait = __builtin_amdgcn_s_memtime() - w0 + 1u;
        }
#endif
    }
    // The lane's camera ray has its Scene.Hit (or its traversal set up).
    static constexpr bool kCameraHitDone = kBuildRefill;
    __device__ __forceinline__ void camera_hit_done() {
#ifdef TRAY_PROFILE_REFILL
        prof_hit = __builtin_amdgcn_s_memtime();
#endif
    }
    // Every fresh lane has its camera ray: the refill's end half follows.
    static constexpr bool kCameraRaysDone = kBuildRefill;
    __device__ __forceinline__ void camera_rays_done() {
#ifdef TRAY_PROFILE_REFILL
        prof_shade0 = __builtin_amdgcn_s_memtime();
#endif
    }
    // Ahead of the end half and behind it: a stamp pair inside the refill's, which the timeline
    // build has no phase for. cam_hit: this lane was in it.
    static constexpr bool kEndHalf = kBuildProf;
    __device__ __forceinline__ void end_half_begin() {
#ifdef TRAY_PROFILE
        t0_nested = __builtin_amdgcn_s_memtime();
#endif
    }
    __device__ __forceinline__ void end_half_end(uint32_t lane, uint32_t cur, bool cam_hit) {
#ifdef TRAY_PROFILE
#ifdef TRAY_PROFILE_BEGIN
        {
            const uint64_t m = __ballot(cur == kTravHitCam);
            cnt(kProfMarkedByRefill, ((uint64_t)(m != 0ull) << 40) + (uint64_t)__popcll(m), lane);
        }
#endif
        cnt(kProfRefillEnd, __builtin_amdgcn_s_memtime() - t0_nested, lane);
        cnt(kProfRefillEndPhases, 1, lane);
        cnt(kProfRefillEndLanes, __popcll(__ballot(cam_hit)), lane);
#endif
    }
    // The end of the refill (phase_begin() stands at its start).
    template <bool kStats>
    static constexpr bool kRefillDone = kBuildProf || (kBuildTl && kStats);
    template <bool kStats>
    __device__ __forceinline__ void refill_done(uint32_t lane, bool busy) {
#ifdef TRAY_PROFILE_REFILL
        {
            const uint64_t prof_shade1 = __builtin_amdgcn_s_memtime();
            cnt(kProfRefillAssign, prof_assigned - t0, lane);
            cnt(kProfRefillShade, prof_shade1 - prof_shade0, lane);
            const uint64_t mw = __ballot(prof_cam != 0u);
            if (mw != 0ull) {
                const uint32_t lw = (uint32_t)__builtin_ctzll(mw);
                const uint64_t c = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(prof_cam >> 32), lw) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((uint32_t)prof_cam, lw);
                const uint64_t h = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(prof_hit >> 32), lw) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((uint32_t)prof_hit, lw);
                cnt(kProfRefillCamera, c - prof_assigned, lane);
                cnt(kProfRefillHit, h - c, lane);
            }
        }
#endif
#ifdef TRAY_PROFILE_CANDWAIT
        {
            const uint64_t mw = __ballot(prof_wait != 0u);
            if (mw != 0ull) {
                const uint32_t lw = (uint32_t)__builtin_ctzll(mw);
                const uint64_t w = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(prof_wait >> 32), lw) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((uint32_t)prof_wait, lw);
                cnt(kProfCandWait, w - 1u, lane);
            }
        }
#endif
        phase_end<kProfRefill, kStats>(lane);
#ifdef TRAY_PROFILE_TIMELINE
        tl_busy = (uint32_t)__popcll(__ballot(busy));
#endif
    }

    // The scatter step has marked lanes. cur, slot, bounce: the lane's Trav::cur, Trav::slot, Lane::bounce.
    static constexpr bool kScatterBegin = kBuildProf;
    __device__ __forceinline__ void scatter_begin(const KernelParams& p, uint32_t lane, uint32_t cur, int32_t slot,
                                                  uint32_t bounce) {
#ifdef TRAY_PROFILE
        cnt(kProfScatterSteps, 1, lane);
        cnt(kProfScatterLanes, __popcll(__ballot(is_marked(cur))), lane);
#ifdef TRAY_PROFILE_BEGIN
        cnt(kProfScatterSources, __popcll(__ballot(is_marked(cur))), lane);
#endif
#endif
#ifdef TRAY_PROFILE_MATERIAL
        prof_material(0, cur == kTravHitCam, slot, bounce, p.max_depth, p.bmat, lane, prof_mat);
        prof_material(1, cur == kTravHit, slot, bounce, p.max_depth, p.bmat, lane, prof_mat);
#endif
    }
    // The lane scattered into a new segment. from_global: off an out-of-tree sphere; dir: the new direction.
    template <bool kStats>
    static constexpr bool kScatterSegment = kBuildGround && kStats;
    template <bool kStats>
    __device__ __forceinline__ void scatter_segment(bool from_global, const D3& dir, Stats& st) {
#if defined(TRAY_STATS_GROUND) && !defined(TRAY_PROFILE)
        const bool up = dir.y >= __builtin_fmax(__builtin_fabs(dir.x), __builtin_fabs(dir.z));
        gcls = from_global ? (up ? 1u : 2u) : 0u;
        if constexpr (kStats) {
            if (gcls == 1) ++st.g_seg[0];
            if (gcls != 0) ++st.g_seg[1];
        }
#endif
    }
    // Behind the scatter part. ended: this lane was absorbed in it.
    static constexpr bool kScatterEnd = kBuildProf;
    __device__ __forceinline__ void scatter_end(uint32_t lane, bool ended) {
#ifdef TRAY_PROFILE
        cnt(kProfAbsorbedLanes, __popcll(__ballot(ended)), lane);
#endif
    }
    // Ahead of the begin part.
    static constexpr bool kBeginPart = kBuildProf && !kBuildRefill && !kBuildCandwait;
    __device__ __forceinline__ void begin_part(uint32_t lane, uint32_t cur) {
#if defined(TRAY_PROFILE) && !defined(TRAY_PROFILE_REFILL) && !defined(TRAY_PROFILE_CANDWAIT)  // (they time into slot 15)
        cnt(kProfBeginSteps, __ballot(cur == kTravReady) != 0ull ? 1 : 0, lane);
#endif
    }

    // A node step runs. m: the traversing lanes.
    static constexpr bool kNodeStep = kBuildProf;
    __device__ __forceinline__ void node_step(uint32_t lane, uint64_t m, uint32_t cur, bool busy) {
#ifdef TRAY_PROFILE
        cnt(kProfNodeSteps, 1, lane);
        cnt(kProfNodeLanes, __popcll(m), lane);
#ifndef TRAY_PROFILE_BEGIN
        cnt(kProfLeafWaitLanes, __popcll(__ballot(is_leaf(cur))), lane);
        cnt(kProfShadeWaitLanes, __popcll(__ballot(busy && cur == kBvhNone)), lane);
#endif
#endif
    }
    // The lane visited a node and tested `tested` boxes there.
    template <bool kStats>
    static constexpr bool kNodeVisit = (kBuildPrim || kBuildGround) && kStats;
    template <bool kStats>
    __device__ __forceinline__ void node_visit(Stats& st, uint32_t tested, uint32_t bounce) {
#if defined(TRAY_STATS_PRIMARY) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            ++st.nodes;
            if (bounce == 0) ++st.nodes0, st.boxes0 += tested;
        }
#endif
#if defined(TRAY_STATS_GROUND) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            ++st.nodes;
            if (gcls == 1) ++st.g_nodes[0];
            if (gcls != 0) ++st.g_nodes[1];
        }
#endif
    }
    // The leaf phase runs on the lanes m_leaf.
    static constexpr bool kLeafPhase = kBuildProf;
    __device__ __forceinline__ void leaf_phase(uint32_t lane, uint64_t m_leaf) {
#ifdef TRAY_PROFILE
        cnt(kProfLeafPhases, 1, lane);
        cnt(kProfLeafLanes, __popcll(m_leaf), lane);
#endif
    }
    // The lane visited a leaf.
    template <bool kStats>
    static constexpr bool kLeafVisit = (kBuildPrim || kBuildGround) && kStats;
    template <bool kStats>
    __device__ __forceinline__ void leaf_visit(Stats& st, uint32_t bounce) {
#if defined(TRAY_STATS_PRIMARY) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            ++st.leaves;
            if (bounce == 0) ++st.leaves0;
        }
#endif
#if defined(TRAY_STATS_GROUND) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            ++st.leaves;
            if (gcls == 1) ++st.g_leaves[0];
            if (gcls != 0) ++st.g_leaves[1];
        }
#endif
    }
    // The shade phase runs on the lanes m_shade.
    static constexpr bool kShadePhase = kBuildProf;
    __device__ __forceinline__ void shade_phase(uint32_t lane, uint64_t m_shade) {
#ifdef TRAY_PROFILE
        cnt(kProfShadePhases, 1, lane);
        cnt(kProfShadeLanes, __popcll(m_shade), lane);
#endif
    }
    // Behind the shade phase's end half, which marked its hits (cur == kTravHit).
    static constexpr bool kShadeMarked = kBuildProf && kBuildBegin;
    __device__ __forceinline__ void shade_marked(uint32_t lane, uint32_t cur) {
#ifdef TRAY_PROFILE_BEGIN
        const uint64_t m = __ballot(cur == kTravHit);
        cnt(kProfMarkedByShade, ((uint64_t)(m != 0ull) << 40) + (uint64_t)__popcll(m), lane);
#endif
    }

    // The wave leaves the kernel: what the build counted goes to the stats buffer.
    template <bool kStats>
    static constexpr bool kKernelEnd = (kBuildProf || kBuildTl || kBuildPrim || kBuildGround) && kStats;
    template <bool kStats>
    __device__ __forceinline__ void kernel_end(const KernelParams& p, const Stats& st, uint32_t lane) {
#if defined(TRAY_STATS_PRIMARY) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            atomicAdd(p.stats + 3, (unsigned long long)st.nodes0);
            atomicAdd(p.stats + 4, (unsigned long long)st.leaves0);
            atomicAdd(p.stats + 5, (unsigned long long)st.boxes0);
            atomicAdd(p.stats + 6, (unsigned long long)st.nodes);
            atomicAdd(p.stats + 7, (unsigned long long)st.leaves);
        }
#endif
#if defined(TRAY_STATS_GROUND) && !defined(TRAY_PROFILE)
        if constexpr (kStats) {
            for (int k = 0; k < 2; ++k) {
                atomicAdd(p.stats + 3 + k, (unsigned long long)st.g_seg[k]);
                atomicAdd(p.stats + 5 + k, (unsigned long long)st.g_nodes[k]);
                atomicAdd(p.stats + 7 + k, (unsigned long long)st.g_leaves[k]);
            }
            atomicAdd(p.stats + 9, (unsigned long long)st.nodes);
            atomicAdd(p.stats + 10, (unsigned long long)st.leaves);
        }
#endif
#ifdef TRAY_PROFILE_TIMELINE
        if (kStats && lane == 0) {
            const uint64_t end = __builtin_amdgcn_s_memrealtime();
            const uint64_t mt_end = __builtin_amdgcn_s_memtime();
            tl_acc += (mt_end - tl_prev) * tl_busy;
            tl[kTlHdr + tl_bucket] = tl_acc;
            for (int k = 0; k < 4; ++k) tl[kTlHdr + kTlBuckets - 9 + k] = tl_ph[k];
            tl[0] = tl_start;
            tl[1] = end;
            tl[2] = tl_dry;
            tl[3] = tl_chunks;
            tl[4] = tl_mt0;
            tl[5] = mt_end;
        }
#endif
#ifdef TRAY_PROFILE
        if (kStats && lane == 0) {
            for (int i = 0; i < 16; ++i) atomicAdd(p.stats + 3 + i, (unsigned long long)prof[i]);
            for (int i = 16; i < kProfSlots; ++i) atomicAdd(p.stats + 6 + i, (unsigned long long)prof[i]);
            // Wave lifetimes on the constant-rate clock: latest exit, sum of lifetimes, earliest start.
            const uint64_t end = __builtin_amdgcn_s_memrealtime();
            atomicMax(p.stats + 19, (unsigned long long)end);
            atomicAdd(p.stats + 20, (unsigned long long)(end - prof_start));
            atomicMax(p.stats + 21, (unsigned long long)~prof_start);
            // Per-wave (start, end) from stats[32] on (the buffer must hold 32 + 2 x waves).
            const uint32_t wave = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
            p.stats[32 + 2 * wave] = prof_start;
            p.stats[33 + 2 * wave] = end;
        }
#endif
    }
};

}  // namespace tray
