// What the two forms of the training Linear's forward share (linear_fwd_f32 of train_block.hip on the fp32 MFMA, linear_fwd_bf16 of train_lin16.hip on the
// 16-bit MFMA): the launch arguments, the epilogue names and the erfc GELU of the epilogue, so that both kernels write their epilogues with the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace m3r
