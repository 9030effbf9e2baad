// tray_progressive.hip — include/tray_progressive.h sections 1 and 2: the running mean
// and M2 over pass frames (Welford), with the variance of the mean and the
// convergence metric fused into the same launch. (Section 3, the variance-guided
// filter, is a sibling of the a-trous kernel and lives in tray_denoise.hip.)
//
// The header is the contract: every value is a fixed sequence of correctly
// rounded FP64 operations in the header's order (built with -ffp-contract=off).
//
// A streaming kernel: 24 * n_frames + 96 bytes per pixel (the state read and
// written once, every frame element read once; + 24 for `variance`). The fold is
// per element, so lanes do not own pixels: a wave owns 384 consecutive doubles
// (128 pixels) and reads them as three rows of 128, lane l taking doubles 2l and
// 2l + 1 of each row. Every load and store instruction of a wave then covers 1 KiB
// of consecutive bytes, whole cache lines, at any image size (a frame of an odd
// number of pixels starts 8 bytes off a 16-byte boundary: the 16-byte accesses are
// declared 8-byte aligned). Frames are fetched four at a time ahead of the
// dependent divide chains, 12 independent 16-byte loads per lane.
//
// The metric is per pixel. The wave transposes through LDS: each lane writes the
// variance and the mean of its six elements, and reads back the three channels of
// pixels l and l + 64 of the wave's 128 (stride 3 doubles over the lanes: 3 is odd,
// so the 32 lanes of a half-wave fall on 32 different 8-byte bank pairs). Counts
// come from a ballot per wave, the maximum from a wave reduction over bit patterns;
// a workgroup adds its four waves' and issues one integer atomic add and one
// integer atomic max, and the grid is capped, so a frame costs a few thousand
// atomics whatever its size. Both are order independent: the bits repeat.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <string>

#include "../../include/tray_progressive.h"
#include "tray_check.hpp"
#include "tray_stream.hpp"

namespace tray {
namespace {

constexpr int kFramesAhead = 4;  // frames fetched ahead of the divide chains

struct FoldArgs {
    double* mean;
    double* m2;
    const double* frames;  // n_frames x elems
    double* variance;      // nullable
    tray_accum_metric* metric;  // nullable
    size_t elems;          // 3 x pixels
    size_t pixels;
    size_t chunks;         // ceil(elems / kBlockElems)
    int32_t count;         // frames in the state before this call
    int32_t n_frames;
    double D;              // (double)n * (double)(n - 1) for the state after the call
    double T;              // tolerance * tolerance
    double floor;
};

template <bool kMetric>
__global__ __launch_bounds__(kThreads) void accum_fold_kernel(const FoldArgs A) {
    __shared__ double xch[kMetric ? 2 : 1][kMetric ? kBlockElems : 1];
    __shared__ unsigned long long red[2][kWaves];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const int n_after = A.count + A.n_frames;
    unsigned long long wave_count = 0, lane_max = 0;

    for (size_t chunk = blockIdx.x; chunk < A.chunks; chunk += gridDim.x) {  // uniform per workgroup
        const size_t wave_base = chunk * kBlockElems + (size_t)wave * kWaveElems;
        size_t at[kSlots];
        double mean[2 * kSlots], m2[2 * kSlots];
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            at[j] = wave_base + (size_t)j * kRowElems + 2 * (size_t)lane;
            mean[2 * j] = mean[2 * j + 1] = m2[2 * j] = m2[2 * j + 1] = 0.0;
            if (A.count > 0) {
                load_pair(A.mean, at[j], A.elems, mean[2 * j], mean[2 * j + 1]);
                load_pair(A.m2, at[j], A.elems, m2[2 * j], m2[2 * j + 1]);
            }
        }
        for (int k0 = 0; k0 < A.n_frames; k0 += kFramesAhead) {
            double x[kFramesAhead][2 * kSlots];
#pragma unroll
            for (int u = 0; u < kFramesAhead; ++u) {
#pragma unroll
                for (int j = 0; j < kSlots; ++j) {
                    x[u][2 * j] = x[u][2 * j + 1] = 0.0;
                    if (k0 + u < A.n_frames)
                        load_pair(A.frames + (size_t)(k0 + u) * A.elems, at[j], A.elems, x[u][2 * j], x[u][2 * j + 1]);
                }
            }
#pragma unroll
            for (int u = 0; u < kFramesAhead; ++u) {
                if (k0 + u < A.n_frames) {
                    const double n = (double)(A.count + k0 + u + 1);
#pragma unroll
                    for (int c = 0; c < 2 * kSlots; ++c) {
                        const double t = x[u][c] - mean[c];
                        mean[c] = mean[c] + t / n;
                        m2[c] = m2[c] + t * (x[u][c] - mean[c]);
                    }
                }
            }
        }
        if (A.n_frames > 0) {
#pragma unroll
            for (int j = 0; j < kSlots; ++j) {
                store_pair(A.mean, at[j], A.elems, mean[2 * j], mean[2 * j + 1]);
                store_pair(A.m2, at[j], A.elems, m2[2 * j], m2[2 * j + 1]);
            }
        }
        if constexpr (kMetric) {
            double var[2 * kSlots];
#pragma unroll
            for (int c = 0; c < 2 * kSlots; ++c)
                var[c] = n_after >= 2 ? m2[c] / A.D : std::numeric_limits<double>::infinity();
            if (A.variance) {
#pragma unroll
                for (int j = 0; j < kSlots; ++j) store_pair(A.variance, at[j], A.elems, var[2 * j], var[2 * j + 1]);
            }
            if (A.metric) {  // uniform
                const int mine = wave * kWaveElems + 2 * lane;
#pragma unroll
                for (int j = 0; j < kSlots; ++j) {
                    xch[0][mine + j * kRowElems] = var[2 * j];
                    xch[0][mine + j * kRowElems + 1] = var[2 * j + 1];
                    xch[1][mine + j * kRowElems] = mean[2 * j];
                    xch[1][mine + j * kRowElems + 1] = mean[2 * j + 1];
                }
                __syncthreads();
                const size_t pixel0 = chunk * (kBlockElems / 3) + (size_t)wave * kWavePixels;
#pragma unroll
                for (int t = 0; t < kWavePixels / kWave; ++t) {
                    const int pp = lane + t * kWave;
                    const bool valid = pixel0 + (size_t)pp < A.pixels;
                    const double* pv = &xch[0][wave * kWaveElems + 3 * pp];
                    const double* pm = &xch[1][wave * kWaveElems + 3 * pp];
                    const double v = (pv[0] + pv[1]) + pv[2];
                    const double e = (pm[0] * pm[0] + pm[1] * pm[1]) + pm[2] * pm[2];
                    const double m = e > A.floor ? e : A.floor;
                    const double q = v / m;
                    const bool converged = n_after >= 2 && v <= A.T * m;
                    wave_count += (unsigned long long)__popcll(__ballot(valid && !converged));
                    if (valid && q >= 0.0) {
                        const unsigned long long b = (unsigned long long)__double_as_longlong(q);
                        lane_max = b > lane_max ? b : lane_max;
                    }
                }
                __syncthreads();  // the next chunk overwrites xch
            }
        }
    }

    if constexpr (kMetric) {
        if (A.metric) {
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const unsigned long long other = __shfl_xor(lane_max, off, kWave);
                lane_max = other > lane_max ? other : lane_max;
            }
            if (lane == 0) {
                red[0][wave] = wave_count;
                red[1][wave] = lane_max;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long count = 0, most = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    count += red[0][w];
                    most = red[1][w] > most ? red[1][w] : most;
                }
                if (count) atomicAdd(reinterpret_cast<unsigned long long*>(&A.metric->unconverged), count);
                if (most) atomicMax(reinterpret_cast<unsigned long long*>(&A.metric->max_ratio), most);
            }
        }
    }
}

int fold(tray_accum* acc, const double* frames, int32_t n_frames, bool with_metric,
         const tray_accum_metric_params* mp, double* variance, tray_accum_metric* metric, int32_t device,
         void* stream) {
    if (!acc) return fail(TRAY_ERR_INVALID_ARGUMENT, "null acc");
    if (acc->width < 0 || acc->rows < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative width or rows");
    if (acc->count < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative count");
    if (acc->reserved != 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "reserved must be 0");
    if (n_frames < 0) return fail(TRAY_ERR_INVALID_ARGUMENT, "negative n_frames");
    if ((int64_t)acc->count + n_frames > INT32_MAX)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "count + n_frames overflows int32");
    if (with_metric) {
        if (!mp) return fail(TRAY_ERR_INVALID_ARGUMENT, "null metric params");
        if (!(std::isfinite(mp->tolerance) && mp->tolerance >= 0.0))
            return fail(TRAY_ERR_INVALID_ARGUMENT, "tolerance must be finite and >= 0");
        if (!(std::isfinite(mp->floor) && mp->floor > 0.0))
            return fail(TRAY_ERR_INVALID_ARGUMENT, "floor must be finite and > 0");
    }
    const int64_t pixels = (int64_t)acc->width * (int64_t)acc->rows;
    if (pixels > kMaxPixels) return fail(TRAY_ERR_TOO_LARGE, "more than 2^31 - 1 pixels in one accumulator");
    if (pixels == 0) return TRAY_OK;
    if (!with_metric && n_frames == 0) return TRAY_OK;
    if (!acc->mean || !acc->m2) return fail(TRAY_ERR_INVALID_ARGUMENT, "null mean or m2");
    if (n_frames > 0 && !frames) return fail(TRAY_ERR_INVALID_ARGUMENT, "null frames");
    const size_t image = (size_t)pixels * 3 * sizeof(double);
    const Span spans[] = {{metric, sizeof(tray_accum_metric), 8, "the metric record"},
                          {variance, image, 8, "variance"},
                          {acc->mean, image, 8, "mean"},
                          {acc->m2, image, 8, "m2"},
                          {frames, image * (size_t)n_frames, 8, "the frames"}};
    int rc = check_alignment(spans, 5);
    if (rc) return rc;
    if (with_metric && acc->count + n_frames == 0)
        return fail(TRAY_ERR_INVALID_ARGUMENT, "no frames folded: nothing to evaluate");
    rc = check_overlaps(spans, 5, 4);
    if (rc) return rc;
    const bool evaluate = with_metric && (variance || metric);
    if (!evaluate && n_frames == 0) return TRAY_OK;
    rc = select_device(device);
    if (rc) return rc;

    FoldArgs A;
    A.mean = acc->mean;
    A.m2 = acc->m2;
    A.frames = frames;
    A.variance = evaluate ? variance : nullptr;
    A.metric = evaluate ? metric : nullptr;
    A.pixels = (size_t)pixels;
    A.elems = A.pixels * 3;
    A.chunks = (A.elems + kBlockElems - 1) / kBlockElems;
    A.count = acc->count;
    A.n_frames = n_frames;
    const int32_t n = acc->count + n_frames;
    A.D = (double)n * (double)(n - 1);
    A.T = with_metric ? mp->tolerance * mp->tolerance : 0.0;
    A.floor = with_metric ? mp->floor : 1.0;
    const uint32_t grid = (uint32_t)((int64_t)A.chunks < kMaxGrid ? (int64_t)A.chunks : kMaxGrid);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    if (A.metric) {
        e = hipMemsetAsync(metric, 0, sizeof(tray_accum_metric), s);
        if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }
    if (evaluate)
        hipLaunchKernelGGL(accum_fold_kernel<true>, dim3(grid), dim3(kThreads), 0, s, A);
    else
        hipLaunchKernelGGL(accum_fold_kernel<false>, dim3(grid), dim3(kThreads), 0, s, A);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("accumulator fold: ") + hipGetErrorString(e));
    acc->count = n;
    return TRAY_OK;
}

}  // namespace
}  // namespace tray

using namespace tray;

#pragma GCC visibility push(default)
extern "C" {

int32_t tray_progressive_version(void) { return TRAY_PROGRESSIVE_VERSION; }

int tray_accum_metric_default_params(tray_accum_metric_params* out) {
    if (!out) return fail(TRAY_ERR_INVALID_ARGUMENT, "null params (out)");
    out->tolerance = 0.05;
    out->floor = 0.0009765625;  // 2^-10
    return TRAY_OK;
}

int tray_accum_fold_async(tray_accum* acc, const double* frames, int32_t n_frames, int32_t device, void* stream) {
    return fold(acc, frames, n_frames, false, nullptr, nullptr, nullptr, device, stream);
}

int tray_accum_fold_metric_async(tray_accum* acc, const double* frames, int32_t n_frames,
                                 const tray_accum_metric_params* mp, double* variance, tray_accum_metric* metric,
                                 int32_t device, void* stream) {
    return fold(acc, frames, n_frames, true, mp, variance, metric, device, stream);
}

}  // extern "C"
#pragma GCC visibility pop
