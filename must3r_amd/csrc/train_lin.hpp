// What the two forms of the training Linear's forward share (linear_fwd_f32 of train_block.hip on the fp32 MFMA, linear_fwd_bf16 of train_lin16.hip on the
// 16-bit MFMA): the launch arguments, the epilogue names, the erfc GELU and the epilogue itself, so that both kernels write their outputs with the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "train_tile.hpp"

namespace m3r {

enum { LIN_BIAS = 0, LIN_BIAS_RES = 1, LIN_BIAS_GELU = 2 };

struct LinArgs {
    const float* A; const float* W; const float* bias;
    const float* res;   // LIN_BIAS_RES; may alias out
    float* out;
    float* zout;        // LIN_BIAS_GELU, optional: the pre-activation
    int M, N, K, lda, ldc, ldres, ldz, n_tiles;
};

__device__ __forceinline__ float gelu_cdf(float z) { return 0.5f * erfcf(-0.70710678118654752440f * z); }
__device__ __forceinline__ float gelu_f32(float z) { return z * gelu_cdf(z); }

// The epilogue of a wave's 64 x 64 with origin (m0, n0): z = acc + bias, then out = z | res + z | gelu(z) (and z itself where zout is given).
// Tail rows and columns are not stored.  p travels by value (train_tile.hpp for_each_acc64).  fr and fk are derived here from the lane: handed down from
// the kernel they moved linear_fwd_f32's loop by 8 bytes, and its median was 1.3 to 2.1 % above the parent's at K >= 3072 in two runs (inside the spread;
// profiles/train_shared_ab.txt).
template <int EPI>
__device__ __forceinline__ void lin_epilogue(const LinArgs p, const f32x4 (&acc)[4][4], int m0, int n0, int lane) {
    const int fr = lane & 15, fk = lane >> 4;
    float bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + fr;
        bj[j] = p.bias && n < p.N ? p.bias[n] : 0.f;
    }
    for_each_acc64(acc, m0, n0, p.M, p.N, fr, fk, [=](int m, int n, int j, float x) {
        const float z = x + bj[j];
        if constexpr (EPI == LIN_BIAS) p.out[(size_t)m * p.ldc + n] = z;
        if constexpr (EPI == LIN_BIAS_RES) p.out[(size_t)m * p.ldc + n] = p.res[(size_t)m * p.ldres + n] + z;
        if constexpr (EPI == LIN_BIAS_GELU) {
            if (p.zout) p.zout[(size_t)m * p.ldz + n] = z;
            p.out[(size_t)m * p.ldc + n] = gelu_f32(z);
        }
    });
}

}  // namespace m3r
