// tray_stream.hpp — the access pattern of the kernels that stream an image's doubles
// (accum_fold_kernel in tray_progressive.hip, the metric pass of the selection in
// tray_adaptive.hip): a wave owns 384 consecutive doubles (128 pixels) and reads them as
// three rows of 128, lane l taking doubles 2l and 2l + 1 of each row, as 16-byte pairs
// declared 8-byte aligned (a frame of an odd number of pixels starts 8 bytes off a 16-byte
// boundary). Every load and store instruction of a wave covers 1 KiB of consecutive bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tray {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kSlots = 3;                            // 16-byte accesses per lane and image
constexpr int kRowElems = 2 * kWave;                 // doubles one wave access covers
constexpr int kWaveElems = kSlots * kRowElems;       // 384 doubles = 128 pixels
constexpr int kWavePixels = kWaveElems / 3;
constexpr int kBlockElems = kWaves * kWaveElems;     // 1536 doubles = 512 pixels
constexpr int64_t kMaxGrid = 2048;                   // 8 workgroups for each of 256 CUs

struct __attribute__((packed, aligned(8))) Pair {  // 16 bytes at 8-byte alignment
    double a, b;
};

__device__ __forceinline__ void load_pair(const double* base, size_t i, size_t elems, double& a, double& b) {
    if (i + 1 < elems) {
        const Pair v = *reinterpret_cast<const Pair*>(base + i);
        a = v.a;
        b = v.b;
    } else if (i < elems) {
        a = base[i];
    }
}

__device__ __forceinline__ void store_pair(double* base, size_t i, size_t elems, double a, double b) {
    if (i + 1 < elems) {
        Pair v;
        v.a = a;
        v.b = b;
        *reinterpret_cast<Pair*>(base + i) = v;
    } else if (i < elems) {
        base[i] = a;
    }
}

}  // namespace tray
