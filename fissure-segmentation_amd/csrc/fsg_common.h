// Shared host-side helpers for libfsg_hip.so (gfx950 only); the device-side ones are in fsg_device.h, included at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/fsg_hip.h"

#define FSG_WAVE 64

void fsg_set_error(const char *fmt, ...);

#define FSG_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            fsg_set_error(__VA_ARGS__);   \
            return FSG_ERR_ARG;           \
        }                                 \
    } while (0)

#define FSG_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            fsg_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return FSG_ERR_HIP;                                                       \
        }                                                                             \
    } while (0)

// Raise the dynamic-LDS limit of `kernel` to `bytes` on the current device or fail the entry point `entry` with FSG_ERR_HIP.
// Each expansion owns one FsgLdsGrant (below): one per call site / template instantiation, as that struct requires.
// FSG_LDS_GRANTED is the bare test for a caller that reports the refusal itself.
#define FSG_LDS_GRANTED(kernel, bytes)                               \
    ([&]() -> bool {                                                 \
        static FsgLdsGrant grant_;                                   \
        return grant_.raise((const void *)(kernel), (size_t)(bytes)); \
    }())
#define FSG_GRANT_LDS(entry, kernel, bytes)                                                        \
    do {                                                                                           \
        if (!FSG_LDS_GRANTED(kernel, bytes)) {                                                     \
            fsg_set_error("%s: cannot raise dynamic LDS to %zu", entry, (size_t)(bytes));          \
            return FSG_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)
// what the kernels that take "all" of a CU's 160 KiB of LDS ask for
constexpr size_t FSG_LDS_WHOLE_CU = 160 * 1024 - 512;

static inline int fsg_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Dynamic LDS above the 64 KiB every kernel may use is granted per kernel AND per device (hipFuncSetAttribute acts on the
// current device's copy of the function).  One instance per call site -- a function-local static of the launching function /
// template instantiation --, remembering what each device has been granted; safe when several host threads launch.
struct FsgLdsGrant {
    static constexpr int kMaxDevices = 64;
    std::atomic<size_t> bytes[kMaxDevices];
    FsgLdsGrant() {
        for (auto &b : bytes) b.store(64 * 1024, std::memory_order_relaxed);
    }
    // make sure the kernel may be launched with `need` bytes of dynamic LDS on the current device; false if the runtime refuses
    bool raise(const void *kernel, size_t need) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        const bool tracked = dev >= 0 && dev < kMaxDevices;
        if (tracked && need <= bytes[dev].load(std::memory_order_acquire)) return true;
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need) != hipSuccess) return false;
        if (tracked) {     // monotone maximum (another thread may have raised it further in the meantime)
            size_t cur = bytes[dev].load(std::memory_order_relaxed);
            while (cur < need && !bytes[dev].compare_exchange_weak(cur, need, std::memory_order_release)) {
            }
        }
        return true;
    }
};

#ifdef __HIPCC__
#include "fsg_device.h"   // the device-side helpers every kernel file shares
#endif
