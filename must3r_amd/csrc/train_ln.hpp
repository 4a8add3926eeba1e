// The LayerNorm row routine of the training kernels, once: one wave holds a row of D fp32 (D % 64 == 0, D <= 1024) in four float4 per lane, lane `lane`
// the columns (j 64 + lane) 4 .. + 3 of j = 0..3, zeros beyond D.  ln_fwd_f32 (train_block.hip) and the feedback kernels (train_decoder.hip) are built from
// these three pieces, so that the same row gives the same statistics and the same output bits in both.  The arithmetic is pinned (no contraction of a product
// and a sum into an fma: which ones the compiler fuses depends on the code around the routine), so that the bits do not depend on the kernel it is inlined into.
#pragma once
#include "common.hpp"

namespace m3r {

__device__ __forceinline__ void ln_row_load(const float* __restrict__ xr, int lane, int D, f32x4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (j * 64 + lane) * 4;
        v[j] = c < D ? *reinterpret_cast<const f32x4*>(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// two-pass statistics of the row in registers
__device__ __forceinline__ void ln_row_stats(const f32x4 (&v)[4], int lane, int D, float eps, float& mu, float& rstd) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    mu = wave_sum_dpp(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((j * 64 + lane) * 4 < D) {
            const f32x4 d = v[j] - mu;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    rstd = 1.0f / sqrtf(wave_sum_dpp(q) / (float)D + eps);
}

__device__ __forceinline__ void ln_row_store(const f32x4 (&v)[4], float mu, float rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             float* __restrict__ yr, int lane, int D) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (j * 64 + lane) * 4;
        if (c < D) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), b = *reinterpret_cast<const f32x4*>(beta + c);
            *reinterpret_cast<f32x4*>(yr + c) = (v[j] - mu) * rstd * g + b;
        }
    }
}

}  // namespace m3r
