// libwaymotrack internal helpers (host side).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/waymotrack.h"

namespace wt {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
int ensure_device();               // WT_OK when a gfx950 device is current and usable

// Launcher state that belongs to a DEVICE, not to the process (a process may drive more than one GPU): the CU count the grids are sized from
// and "has this launcher raised its kernels' dynamic-LDS limit on this device yet" (hipFuncSetAttribute is per device).
constexpr int MAX_DEVICES = 32;
int device_index();                // hipGetDevice; -1 when it fails
int device_cus();                  // CU count of the current device (cached per device, safe inside a stream capture after the first call); 0 = unknown
struct OncePerDevice {
    bool done[MAX_DEVICES] = {};   // written with the same value by every thread that races here: the guarded calls are idempotent
    bool needed(int dev) const { return dev < 0 || dev >= MAX_DEVICES || !done[dev]; }
    void mark(int dev) { if (dev >= 0 && dev < MAX_DEVICES) done[dev] = true; }
};

#define WT_HIP(call)                                                   \
    do {                                                               \
        hipError_t e__ = (call);                                       \
        if (e__ != hipSuccess) return ::wt::hip_fail(e__, #call);      \
    } while (0)

#define WT_TRY(call)                 \
    do {                             \
        int rc__ = (call);           \
        if (rc__ != WT_OK) return rc__; \
    } while (0)

// RAII device allocation for the *_host entry points
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {
        if (p) { (void)hipFree(p); p = nullptr; }
        bytes = n;
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc"); }
        return WT_OK;
    }
    int upload(const void* src, size_t n) {      // alloc, then host -> device when there is anything to copy
        const int rc = alloc(n);
        if (rc != WT_OK) return rc;
        if (n) WT_HIP(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
        return WT_OK;
    }
    int download(void* dst) const {              // device -> host, all of it, when there is anything to copy
        if (bytes) WT_HIP(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
        return WT_OK;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
// the first 256-byte boundary at or behind p: where every launcher starts to carve the workspace it was handed (NULL stays NULL)
inline char* align_ptr(void* p) { return reinterpret_cast<char*>(p) + (align_up((uintptr_t)p) - (uintptr_t)p); }

// Allocated VGPRs per wave (blocks of 8) of the two kernels that return wrong results while a wave of theirs shares a SIMD with repeated-operand bf16 MFMA
// waves (profiles/r06_costream_victim_side.txt): read from the COMPILED kernels; 0 = could not be determined.  det_gconv.hip / det_deform.hip.
int victim_regs_grouped_conv();
int victim_regs_deform64();

// carve typed arrays out of one workspace block
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(reinterpret_cast<char*>(b)) {}
    template <class T> T* take(size_t count) {
        T* r = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += align_up(count * sizeof(T));
        return r;
    }
};

}  // namespace wt
