// What export.hip and render.hip share: the 16-byte loads of four consecutive pixels of a view's planes and the colour byte rule.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace m3r {

// four consecutive floats at p + i (i % 4 == 0): one 16-byte load when all four exist and the address is aligned
__device__ __forceinline__ void load4(const float* __restrict__ p, const unsigned i, const unsigned n, float (&o)[4]) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(p + i) & 15) == 0)) {
        const float4 v = *reinterpret_cast<const float4*>(p + i);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = i + j < n ? p[i + j] : 0.f;
    }
}

// twelve consecutive floats (four xyz triples) at p + 3 i
__device__ __forceinline__ void load12(const float* __restrict__ p, const unsigned i, const unsigned n, float (&o)[12]) {
    const float* q = p + 3ull * i;
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 v = reinterpret_cast<const float4*>(q)[j];
            o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) o[j] = i + j / 3 < n ? q[j] : 0.f;
    }
}

// rint(clip(c, 0, 1) * 255) in fp32: the colour byte of the export and of the renderer
__device__ __forceinline__ unsigned quant8(const float c) {
    return (unsigned)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.f);
}

}  // namespace m3r
