// Ground truth of a training batch from its depth maps (what the reference's datasets compute per view in numpy, must3r_base_dataset.py:185-198, from
// dust3r's depthmap_to_absolute_camera_coordinates): depth [V][Hs][Ws], stored landscape, fp32 or raw uint16 with a per-view (div, mul) pair, the intrinsics
// K [V][3][3] of the true image and the camera-to-world pose c2w [V][4][4] become pts3d fp32 [V][Hs][Ws][3], valid and sky u8 [V][Hs][Ws] and the per-view
// count n_valid of depth > 0.  transposed[v] != 0 (a DEVICE array, NULL: no view) marks a portrait view that was stored with its axes swapped: its stored
// pixel (r, c) is true pixel (row = c, col = r), so u = r and v = c; no data is moved.  Per pixel, with z the depth (include/must3r_hip.h has the contract):
//   x = fp32((double(u) - double(cu)) * double(z) / double(fu))      y likewise with v, cv, fv      X_w[i] = ((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i]
//   valid = z > 0 && isfinite(X_w[0..2])      sky = z < 0      pts3d is written for every pixel
// every operation rounded: this file is built with -ffp-contract=off, so that a CPU expression reproduces the bits.
//
//   gt_from_depth_kernel<U16>   grid (blocks per view, V): lane t of a block owns the pixels 4 g .. 4 g + 3 of a stored row (Ws is a multiple of 4), g walking
//                               the view's groups in steps of the view's threads: one 16-byte depth load (8-byte: uint16), three 16-byte pts3d stores, one
//                               4-byte store per mask.  The view's 18 constants sit at wave-uniform addresses and are read once per block, before the walk.
//                               fp64 for the two back-projections alone (two divisions per pixel); the pose in fp32.  With n_valid: the lanes' counts are
//                               added over the wave (xor butterfly) and the block (LDS, wave order) -> partial[view][block]; no LDS otherwise.
//   gt_count_final_kernel       one thread per view adds the view's partials in block order -> n_valid[view].  Launched with n_valid alone.
// No atomics, one writer per element, 64-bit offsets.  The block count of a view depends on Hs Ws alone, so a view's outputs do not depend on the batch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abi.hpp"
#include "common.hpp"

namespace m3r {
namespace {

constexpr int GT_T = 256;                              // threads per block
constexpr int GT_VIEW_BLOCKS = MUST3R_GT_VIEW_BLOCKS;  // at most, per view

typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;

struct GtDev {
    const void* depth;
    const float* scale;
    const float* K;
    const float* c2w;
    const int32_t* transposed;
    float* pts;
    unsigned char* valid;
    unsigned char* sky;
    int32_t* partial;
    int Ws;
    unsigned groups;   // Hs Ws / 4
};

template <bool U16>
__global__ void __launch_bounds__(GT_T) gt_from_depth_kernel(const GtDev p) {
    __shared__ int s_cnt[GT_T / 64];
    const unsigned view = blockIdx.y;
    // the view's constants: uniform addresses, read once
    const float* __restrict__ Kv = p.K + (size_t)view * 9;
    const float* __restrict__ T = p.c2w + (size_t)view * 16;
    const double fu = Kv[0], cu = Kv[2], fv = Kv[4], cv = Kv[5];
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = T[4 * i + k];
        t[i] = T[4 * i + 3];
    }
    const bool tr = p.transposed && p.transposed[view] != 0;
    float div = 1.f, mul = 1.f;
    if constexpr (U16) {
        div = p.scale[2 * (size_t)view];
        mul = p.scale[2 * (size_t)view + 1];
    }
    const size_t base = (size_t)view * p.groups;   // in groups of 4 pixels
    int cnt = 0;
    for (unsigned g = blockIdx.x * GT_T + threadIdx.x; g < p.groups; g += gridDim.x * GT_T) {
        const unsigned pix = 4 * g, r = pix / (unsigned)p.Ws, c = pix - r * (unsigned)p.Ws;
        float z[4];
        if constexpr (U16) {
            const u16x4 raw = reinterpret_cast<const u16x4*>(p.depth)[base + g];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = ((float)raw[j] / div) * mul;
        } else {
            const f32x4 d = reinterpret_cast<const f32x4*>(p.depth)[base + g];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = d[j];
        }
        float X[12];
        unsigned ok = 0, sk = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = tr ? r : c + j, v = tr ? c + j : r;
            const double zd = (double)z[j];
            const float x = (float)((((double)u - cu) * zd) / fu);
            const float y = (float)((((double)v - cv) * zd) / fv);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float w = ((R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z[j]) + t[i];
                X[3 * j + i] = w;
                fin = fin && isfinite(w);
            }
            const bool pos = z[j] > 0.f;
            cnt += pos ? 1 : 0;
            ok |= (pos && fin ? 1u : 0u) << (8 * j);
            sk |= (z[j] < 0.f ? 1u : 0u) << (8 * j);
        }
        if (p.pts) {
            f32x4* q = reinterpret_cast<f32x4*>(p.pts) + 3 * (base + g);
#pragma unroll
            for (int j = 0; j < 3; ++j) q[j] = f32x4{X[4 * j], X[4 * j + 1], X[4 * j + 2], X[4 * j + 3]};
        }
        if (p.valid) reinterpret_cast<unsigned*>(p.valid)[base + g] = ok;
        if (p.sky) reinterpret_cast<unsigned*>(p.sky)[base + g] = sk;
    }
    if (!p.partial) return;   // uniform over the launch
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = s_cnt[0];
#pragma unroll
        for (int w = 1; w < GT_T / 64; ++w) total += s_cnt[w];
        p.partial[(size_t)view * gridDim.x + blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(GT_T) gt_count_final_kernel(const int32_t* __restrict__ partial, int32_t* __restrict__ n_valid, const int V, const int blocks) {
    const int view = blockIdx.x * GT_T + threadIdx.x;
    if (view >= V) return;
    int total = 0;
    for (int b = 0; b < blocks; ++b) total += partial[(size_t)view * blocks + b];
    n_valid[view] = total;
}

inline bool off16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; }
inline bool off4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) != 0; }

// nullptr, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed
const char* gt_args_error(const must3r_hip_gt_args* a) {
    if (!a->depth || !a->K || !a->c2w) return "null argument (depth, K, c2w)";
    if (a->depth_u16 != 0 && a->depth_u16 != 1) return "depth_u16 must be 0 or 1";
    if (a->depth_u16 && !a->depth_scale) return "null argument (depth_scale: the uint16 form needs its (div, mul) pairs)";
    if (!a->pts3d && !a->valid && !a->sky && !a->n_valid) return "null argument (pts3d, valid, sky and n_valid: one output is needed)";
    if (a->V <= 0 || a->V > 65535) return "V must be in 1 .. 65535";
    if (a->Hs <= 0 || a->Ws <= 0 || a->Ws % 4) return "Hs and Ws must be positive, Ws a multiple of 4";
    if ((long long)a->Hs * a->Ws > 0x7fffffffLL) return "a view of more than 2^31 - 1 pixels";
    if (a->depth_u16 ? (reinterpret_cast<uintptr_t>(a->depth) & 7) != 0 : off16(a->depth)) return "depth must be 16-byte aligned (8-byte: uint16)";
    if (off16(a->pts3d)) return "pts3d must be 16-byte aligned";
    if (off4(a->valid) || off4(a->sky) || off4(a->n_valid) || off4(a->transposed) || off4(a->K) || off4(a->c2w) || off4(a->depth_scale) || off4(a->scratch))
        return "valid, sky, n_valid, transposed, K, c2w, depth_scale and scratch must be 4-byte aligned";
    if (a->n_valid && (!a->scratch || a->scratch_bytes < sizeof(int32_t) * (size_t)a->V * GT_VIEW_BLOCKS))
        return "n_valid needs a scratch of 4 V MUST3R_GT_VIEW_BLOCKS bytes";
    return nullptr;
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_gt_from_depth(const must3r_hip_gt_args* a) {
    const char* who = "gt_from_depth";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = gt_args_error(a)) return fail("%s: %s", who, e);
    GtDev p{};
    p.depth = a->depth; p.scale = a->depth_scale; p.K = a->K; p.c2w = a->c2w; p.transposed = a->transposed;
    p.pts = a->pts3d; p.valid = a->valid; p.sky = a->sky;
    p.partial = a->n_valid ? static_cast<int32_t*>(a->scratch) : nullptr;
    p.Ws = a->Ws;
    p.groups = (unsigned)((long long)a->Hs * a->Ws / 4);
    const unsigned chunks = (p.groups + GT_T - 1) / GT_T;
    const unsigned blocks = chunks < (unsigned)GT_VIEW_BLOCKS ? chunks : (unsigned)GT_VIEW_BLOCKS;
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->depth_u16) hipLaunchKernelGGL(gt_from_depth_kernel<true>, dim3(blocks, (unsigned)a->V), dim3(GT_T), 0, stream, p);
    else hipLaunchKernelGGL(gt_from_depth_kernel<false>, dim3(blocks, (unsigned)a->V), dim3(GT_T), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    if (a->n_valid) {
        hipLaunchKernelGGL(gt_count_final_kernel, dim3((unsigned)((a->V + GT_T - 1) / GT_T)), dim3(GT_T), 0, stream, p.partial, a->n_valid, a->V, (int)blocks);
        if (hipGetLastError() != hipSuccess) return fail("%s: launch failed (count)", who);
    }
    return 0;
}
