// The gather in front of the trainable encoder's patch embedding (dust3r's PatchEmbedDust3R and ManyAR_PatchEmbed as a Linear over rows): the fp32 image
// batch [V][3][H][W] becomes fp32 rows [V N][768], N = (H / 16)(W / 16), in the column order of the flattened conv weight, k = c 256 + dy 16 + dx (the order
// of im2col_kernel), and the int64 positions [V N][2] of the tokens.  The orientation is per view, from a DEVICE array `transposed` (NULL: no view is):
//   landscape   grid H/16 x W/16, token t = (py, px) = (t / (W/16), t % (W/16)),  rows[t][k] = img[v][c][16 py + dy][16 px + dx],  pos = (py, px)
//   portrait    grid W/16 x H/16, token t = (py, px) = (t / (H/16), t % (H/16)),  rows[t][k] = img[v][c][16 px + dx][16 py + dy],  pos = (py, px)
// the portrait form being proj(img.swapaxes(-1, -2)) with the positions of the swapped grid.  The Linear that follows is train_block's; nothing is fused.
//
//   patch_rows_f32   a wave owns one 16 x 16 tile, a (token, channel) pair: 1 KB of one row, contiguous.  Lane l = (r, q) = (l >> 2, l & 3) loads the four
//                    floats img[..][y0 + r][x0 + 4 q ..] (16 bytes; four lanes cover a 64-byte segment of an image row) and stores the four floats
//                    rows[t][c 256 + 16 r + 4 q ..] (16 bytes; the wave writes its KB in lane order).  In a landscape view these are the same four floats.
//                    In a portrait view the tile is turned in the wave's own part of the LDS in between: element (row, col) of the loaded tile lives at
//                        A(row, col) = 16 row + 16 (row >> 2) + (col ^ f(row)),   f(row) = ((row >> 1) & 3) | (row & 8)
//                    (320 floats per wave), written with four ds_write_b32 (element (r, 4 q + j)) and read with four ds_read_b32 (element (4 q + j, r)).
//                    Both are free of bank conflicts by the rule for 4-byte accesses (bank = dword address mod 32, lanes 0-31 and 32-63 apart):
//                      write j   a half holds rows r = 8 h .. 8 h + 7; bit 4 of A is (r + (r >> 2)) & 1, so the rows 8 h + {0, 2, 5, 7} share one half of the
//                                banks and 8 h + {1, 3, 4, 6} the other; within either, (r >> 1) & 3 takes the four values once, so the low bits
//                                4 q + (j ^ f) of the 16 lanes are distinct (the bit 3 of f is the same for the whole half and permutes q).
//                      read j    a half holds rows 4 q + j and columns r = 8 h .. 8 h + 7; bit 4 of A is (q + j) & 1, so q = {0, 2} and {1, 3} use different
//                                halves of the banks; rows 4 q + j and 4 (q + 2) + j differ in bit 3 of f, so their eight columns r ^ f fall in
//                                different aligned groups of eight.
//                    The first lane of a token's channel-0 tile writes the token's position, two int64 in one 16-byte store.  With rows == NULL the kernel
//                    is launched over the tokens and writes positions alone.
// One writer per element, no atomics, 64-bit offsets; the block's barrier is reached by every wave (a block's four tiles may lie in views of both kinds).
#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "common.hpp"
#include "train_common.hpp"

namespace m3r {

typedef __attribute__((ext_vector_type(2))) long long i64x2;

constexpr int PR_TILE_LDS = 320;   // floats of one wave's turned tile: A(15, 15) = 303

struct PatchRows {
    const float* img;
    const int32_t* transposed;
    float* rows;
    int64_t* pos;
    int H, W;
    long long tokens, tiles;   // V N, 3 V N
};

__device__ __forceinline__ int pr_lds_at(int row, int col) { return 16 * row + 16 * (row >> 2) + (col ^ (((row >> 1) & 3) | (row & 8))); }

// token t of view v: its position and the image coordinates of its patch's corner
__device__ __forceinline__ void pr_token(const PatchRows& p, bool tr, int t, int& py, int& px, int& y0, int& x0) {
    const int cols = (tr ? p.H : p.W) / 16;
    py = t / cols;
    px = t - py * cols;
    y0 = 16 * (tr ? px : py);
    x0 = 16 * (tr ? py : px);
}

__global__ void __launch_bounds__(256) patch_rows_f32(PatchRows p) {
    const int N = (p.H / 16) * (p.W / 16);
    if (!p.rows) {   // positions alone: a lane per token (uniform over the launch: no barrier is skipped by a part of a block)
        const long long token = (long long)blockIdx.x * 256 + threadIdx.x;
        if (token >= p.tokens) return;
        const int v = (int)(token / N), t = (int)(token - (long long)v * N);
        int py, px, y0, x0;
        pr_token(p, p.transposed && p.transposed[v] != 0, t, py, px, y0, x0);
        *reinterpret_cast<i64x2*>(p.pos + 2 * token) = i64x2{py, px};
        return;
    }
    __shared__ float lds[4 * PR_TILE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane >> 2, q = lane & 3;
    float* tile_lds = lds + wave * PR_TILE_LDS;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    const bool live = tile < p.tiles;
    bool tr = false;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    float* dst = nullptr;
    if (live) {
        const long long token = tile / 3;
        const int c = (int)(tile - token * 3), v = (int)(token / N), t = (int)(token - (long long)v * N);
        tr = p.transposed && p.transposed[v] != 0;
        int py, px, y0, x0;
        pr_token(p, tr, t, py, px, y0, x0);
        val = *reinterpret_cast<const f32x4*>(p.img + (((size_t)v * 3 + c) * p.H + y0 + r) * p.W + x0 + 4 * q);
        dst = p.rows + (size_t)token * 768 + c * 256 + 16 * r + 4 * q;
        if (p.pos && c == 0 && lane == 0) *reinterpret_cast<i64x2*>(p.pos + 2 * token) = i64x2{py, px};
        if (tr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tile_lds[pr_lds_at(r, 4 * q + j)] = val[j];
        }
    }
    __syncthreads();
    if (!live) return;
    if (tr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) val[j] = tile_lds[pr_lds_at(4 * q + j, r)];
    }
    *reinterpret_cast<f32x4*>(dst) = val;
}

// nullptr, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed
static const char* pr_args_error(const must3r_hip_patch_rows_args* a) {
    if (!a->img) return "null argument (img)";
    if (!a->rows && !a->pos) return "null argument (rows and pos: one of the two outputs is needed)";
    if (a->V <= 0) return "V must be positive";
    if (a->H <= 0 || a->H % 16 || a->W <= 0 || a->W % 16) return "H and W must be positive multiples of 16";
    if (misaligned(a->img) || misaligned(a->rows) || misaligned(a->pos)) return "tensors must be 16-byte aligned";
    if ((size_t)a->transposed & 3) return "transposed must be 4-byte aligned";
    if ((long long)a->V * (a->H / 16) * (a->W / 16) > 0x7fffffff / 4) return "too many rows";
    return nullptr;
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_patch_rows(const must3r_hip_patch_rows_args* a) {
    const char* who = "patch_rows";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = pr_args_error(a)) return fail("%s: %s", who, e);
    PatchRows p{};
    p.img = a->img; p.transposed = a->transposed; p.rows = a->rows; p.pos = a->pos;
    p.H = a->H; p.W = a->W;
    p.tokens = (long long)a->V * (a->H / 16) * (a->W / 16);
    p.tiles = 3 * p.tokens;
    const long long blocks = a->rows ? (p.tiles + 3) / 4 : (p.tokens + 255) / 256;
    hipLaunchKernelGGL(patch_rows_f32, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(a->stream), p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}
