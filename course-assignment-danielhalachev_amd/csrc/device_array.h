// device_array.h -- the scratch arrays of crt_query.hip and crt_giframe.hip: a device array that only grows and is kept for the next call.
#pragma once

#include "crt_internal.h"

namespace {
// Freed with its owner.  Every array that grows bumps crt_query_scratch_generation: a graph captured from an enqueue call holds the old
// pointers.
template <typename T>
struct DeviceArray {
    T *p = nullptr;
    uint64_t cap = 0;
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { release(); }
    int reserve(crt_ctx *ctx, const uint64_t n) {
        if (n <= cap) return CRT_OK;
        if (p) CRT_HIP_CHECK(ctx, hipDeviceSynchronize());   // nothing may still be using the old array
        release();
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        ctx->scratch_generation++;
        return CRT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
// reserve_all(ctx, a, n, b, m, ...): room for n elements in a, m in b, ...; the first failure ends it
inline int reserve_all(crt_ctx *) { return CRT_OK; }
template <typename T, typename... More>
int reserve_all(crt_ctx *ctx, DeviceArray<T> &a, const uint64_t n, More &&...more) {
    if (int rc = a.reserve(ctx, n)) return rc;
    return reserve_all(ctx, more...);
}
// elements of a float4 array that hold `bytes` bytes: the work areas of the denoiser and the chain guides are aligned to 16
inline uint64_t float4s(const uint64_t bytes) { return (bytes + sizeof(float4) - 1) / sizeof(float4); }
}  // namespace
