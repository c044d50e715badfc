// mrp_host.h -- the host code that the units behind the C ABI share (mrp_kernels.hip, mrp_norm.hip,
// mrp_policy.hip, mrp_ppo.hip): the error macro, the device check, the alias rule of the training
// entry points, a call's temporary buffers and the driver of the element-wise self-tests.  Host only:
// nothing here is device code, and the env units (mrp_unit.hip) do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/mrp.h"

// a failed HIP call becomes the object's message and MRP_E_HIP
#define MRP_HIPCHK(obj, expr)                                               \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) {                                             \
            (obj)->err = std::string(#expr) + ": " + hipGetErrorString(_e); \
            return MRP_E_HIP;                                               \
        }                                                                   \
    } while (0)

namespace mrp_host {

inline int pad32(int n) { return (n + 31) & ~31; }

// MRP_OK when `device` names a visible HIP device; else the code, with the reason in `err`
inline int select_device(int device, std::string& err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        err = "no HIP device available (no CPU fallback)";
        return MRP_E_HIP;
    }
    if (device < 0 || device >= ndev) {
        err = "device index out of range";
        return MRP_E_ARG;
    }
    return MRP_OK;
}

// ---- the alias rule: an output may share no byte with an input or with another output.  The extents
// are the arrays' sizes in bytes, so a view into the same allocation at an offset (a row of a rollout
// buffer) is refused when it overlaps, and accepted when it starts where the other array ends.
struct Span { const void* p; size_t bytes; };

inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// null entries (optional arrays) are skipped; returns nullptr when the outputs are fine, else what is wrong
inline const char* check_outputs(std::initializer_list<Span> ins, std::initializer_list<Span> outs) {
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (o.p && i.p && overlaps(o.p, o.bytes, i.p, i.bytes)) return "an output aliases an input";
    for (const Span* o = outs.begin(); o != outs.end(); ++o)
        for (const Span* q = outs.begin(); q != o; ++q)
            if (o->p && q->p && overlaps(o->p, o->bytes, q->p, q->bytes)) return "two outputs overlap";
    return nullptr;
}

// A temporary buffer of one call, freed when the call returns: device memory, or with PINNED
// device-mapped host memory.
template <class T, bool PINNED = false>
class Scoped {
    T* p_ = nullptr;

public:
    Scoped() = default;
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
    ~Scoped() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    }
    hipError_t alloc(size_t bytes) {
        if (p_) return hipErrorInvalidValue;   // one buffer per owner: a second one would leak the first
        return PINNED ? hipHostMalloc((void**)&p_, bytes, hipHostMallocMapped) : hipMalloc((void**)&p_, bytes);
    }
    T* get() const { return p_; }
    T* release() { T* p = p_; p_ = nullptr; return p; }   // mrp_debug_progress hands its buffer to the caller
};

// The element-wise self-tests (mrp_selftest_*): n host inputs to the device, the caller's kernel
// through launch(grid, block, d_x, d_out0, d_out1, n) on the null stream, one or two outputs back
// (out1, and then d_out1, may be null).
template <class Launch>
int selftest_elementwise(int device, const float* x, float* out0, float* out1, int n, Launch launch) {
    if (!x || !out0 || n <= 0) return MRP_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return MRP_E_HIP;
    Scoped<float> dx, d0, d1;
    const size_t bytes = (size_t)n * sizeof(float);
    if (dx.alloc(bytes) != hipSuccess || d0.alloc(bytes) != hipSuccess || (out1 && d1.alloc(bytes) != hipSuccess) ||
        hipMemcpy(dx.get(), x, bytes, hipMemcpyHostToDevice) != hipSuccess)
        return MRP_E_HIP;
    launch(dim3((n + 255) / 256), dim3(256), dx.get(), d0.get(), d1.get(), n);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out0, d0.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        (out1 && hipMemcpy(out1, d1.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess))
        return MRP_E_HIP;
    return MRP_OK;
}

}  // namespace mrp_host
