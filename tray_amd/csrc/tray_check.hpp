// Argument checks shared by the post-processing entry points (the denoiser, the accumulator,
// adaptive sampling and the temporal steps): a table of named buffers and three passes over it,
// device selection and the pixel limit. Host side only. A new entry point describes its
// buffers as a Span table and calls these; a check whose wording the ABI tests pin stays in
// its unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/tray.h"
#include "tray_internal.hpp"

namespace tray {

constexpr int64_t kMaxPixels = 0x7FFFFFFF;  // pixel and ray indices are 32-bit on the device

struct Span {
    const void* p;
    size_t bytes;
    uintptr_t align;  // 0 or 1: not checked
    const char* name;
};

// Null or empty spans never overlap.
inline bool spans_overlap(const Span& a, const Span& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// Each: the first offender among s[0..n) as an error, else TRAY_OK.
// Bit i of `nullable` lets s[i] be null.
inline int check_nulls(const Span* s, int n, uint32_t nullable) {
    for (int i = 0; i < n; ++i)
        if (!s[i].p && !(nullable >> i & 1u))
            return fail(TRAY_ERR_INVALID_ARGUMENT, std::string("null buffer: ") + s[i].name);
    return TRAY_OK;
}

inline int check_alignment(const Span* s, int n) {
    for (int i = 0; i < n; ++i)
        if (s[i].align > 1 && ((uintptr_t)s[i].p & (s[i].align - 1)))
            return fail(TRAY_ERR_INVALID_ARGUMENT,
                        std::string(s[i].name) + " is not " + std::to_string(s[i].align) + "-byte aligned");
    return TRAY_OK;
}

// The first n_out spans (what a call writes) against everything after each of them.
inline int check_overlaps(const Span* s, int n, int n_out) {
    for (int i = 0; i < n_out; ++i)
        for (int j = i + 1; j < n; ++j)
            if (spans_overlap(s[i], s[j]))
                return fail(TRAY_ERR_INVALID_ARGUMENT, std::string(s[i].name) + " overlaps " + s[j].name);
    return TRAY_OK;
}

// Makes `device` current; no gfx950 setup (that is device_usable()).
inline int select_device(int32_t device) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) return fail(TRAY_ERR_NO_DEVICE, "no device");
    if (device < 0 || device >= n_devices) return fail(TRAY_ERR_INVALID_ARGUMENT, "no such device");
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(TRAY_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return TRAY_OK;
}

}  // namespace tray
