// Training forward and backward of the prediction head (decoder.py:149-156, blocks/head.py:63-72, tools/image.py:9-14):
//   y = LN(x) gamma + beta,  z = y W^T + b,  pointmaps[v, 16 gy + i, 16 gx + j, c] = z[v N + gy gw + gx, c 256 + i 16 + j].
// The forward is the decoder's own head (kernels.hpp head_layernorm / head_linear) on operands packed from the fp32 parameters of
// the call.  The backward keeps fp32 operands on v_mfma_f32_16x16x4_f32 (exact products, k-ordered fmaf chain: a result does not
// depend on how the rows were tiled), recomputes the row statistics from x and saves nothing:
//
//   row_stats_kernel      (mu, rstd) per row of x, one wave per row, two passes over the row.
//   perm_w_kernel         W rows in the order o' = (i 16 + j) 7 + c, in which one token's 1792 upstream values are 16 runs of 112
//                         consecutive floats of G (448-byte reads); dZ is never materialised.
//   dgrad_kernel<GATHER>  dY[M, K] = dZ[M, O] W[O, K]: 128 x 128 tiles, 16-deep steps over O through LDS, 4 waves of 64 x 64.  dZ rows are
//                         read along their fast dimension (LDS rows padded to 20 floats: conflict-free), W rows as they lie.
//                         <., SEG> (ABI 21, additive): the rows of W live in two parameters (launch_dgrad_seg_f32, kernels.hpp: dmem = dK Wk + dV Wv
//                         of train_cross.hip); the same steps and the same k-ordered chain, so the bits of the plain kernel on a packed copy.
//   wgrad_kernel<GATHER>  P_s[O, K] = sum_{r in split s} dZ[r, o] x^[r, k]: both operands have the contraction as their slow dimension, the
//                         LDS tiles [r][.] feed the MFMA lanes with consecutive addresses.  x^ = (x - mu) rstd is formed on load.  The
//                         blocks of the first column tile also leave the column sums of their dZ rows (db partials).
//   wgrad_reduce_kernel   sums the S partials in split order and writes dW[o, k] = gamma[k] sum_s P_s[o', k] + beta[k] db[o] at the
//                         un-permuted row, db[o] = sum_s of the column-sum partials.
//   ln_grad_kernel        per row: g^ = dY gamma, dx = rstd (g^ - mean(g^) - x^ mean(g^ x^)), in place over dY; row-walking waves keep
//                         per-lane column sums of dY x^ and dY, one partial per block.
//                         <ADD> (ABI 21): dx = add + that, the residual of a pre-norm sublayer (train_block.hip); <false> is the kernel as it was.
//   ln_grad_reduce_kernel sums the block partials in a fixed two-level order (16 interleaved slices, then the slices): dgamma, dbeta.
//   head_turn_kernel, head_copy_flagged_kernel (ABI 21, additive: must3r_hip_head_forward_many_ar / _grad_many_ar) portrait views of a batch stored
//                         landscape, flagged per view by a DEVICE array: the forward's tiles of those views are turned into their stored places after
//                         the head's two launches, the backward's are laid out in the slot order of the tokens first, and dgrad_kernel<2> /
//                         wgrad_kernel<2> pick each row's source by its view's flag (the comment above head_turn_kernel; DzSrc).  Without flags the
//                         entry points launch what they launched.
// In MUST3R_TRAIN_LINEAR_BF16 mode (must3r_hip_train_linear_mode) the plain forms -- run_dgrad and run_wgrad without GATHER and without statistics, and
// launch_dgrad_seg_f32 -- launch dgrad_bf16 / wgrad_bf16 of train_lin16.hip after the same checks; the gather forms (the head's own) stay fp32.
// The split count of the weight gradient and the block count of the LayerNorm backward are functions of the row count alone.  No atomics:
// every output element has one writer and a fixed order of operations.
#include "abi.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "train_common.hpp"
#include "train_tile.hpp"

namespace m3r {

constexpr int HM = 128, HN = 128, HK = 16, HAP = 20, HBP = 144;   // HAP / HBP: LDS row strides (floats) of [128][16] / [16][128] tiles
constexpr int HEAD_P2 = 256, HEAD_C = 7, HEAD_RUN = 16 * HEAD_C;  // 16 x 16 patch, 7 channels, one pixel row of a patch = 112 floats
constexpr int WGRAD_MAX_SPLITS = 16, WGRAD_ROWS_PER_SPLIT = 128;
constexpr int LNG_MAX_BLOCKS = 1024, LNG_MIN_ROWS = 16, LNG_MAX_T = 16;   // LayerNorm backward: D <= 64 * LNG_MAX_T

// where the rows of dZ come from: a plain [M][ld] matrix (DZ_PLAIN), the pixel-unshuffle of G [n_views][H][W][7] (DZ_GATHER), or that with a source
// per view (DZ_GATHER_AR): the rows of a view with flags[v] != 0 are read at the same offsets from a second tensor, `alt` floats after p (head_turn_kernel
// has laid the view's tiles out there in the slot order of its tokens).  A row's 16 runs of 448 bytes are the same in all three gather cases.
constexpr int DZ_PLAIN = 0, DZ_GATHER = 1, DZ_GATHER_AR = 2;
struct DzSrc {
    const float* p;
    long long ld;          // plain: row stride
    int ntok, gw, H, Wimg; // gather: tokens per view, patches per image row, image size
    const int32_t* flags;  // DZ_GATHER_AR: [n_views] on the device
    long long alt;         // DZ_GATHER_AR: the second tensor's distance from p, in floats
};
template <int GATHER> __device__ __forceinline__ size_t dz_row(const DzSrc& z, int r) {
    if constexpr (!GATHER) return (size_t)r * (size_t)z.ld;
    const int v = r / z.ntok, t = r - v * z.ntok, gy = t / z.gw, gx = t - gy * z.gw;
    const size_t at = (((size_t)v * z.H + 16 * gy) * z.Wimg + 16 * gx) * HEAD_C;
    if constexpr (GATHER == DZ_GATHER_AR) return z.flags[v] != 0 ? at + (size_t)z.alt : at;
    return at;
}
// column o' (a multiple of 4) of a row -> offset from the row's start
template <int GATHER> __device__ __forceinline__ size_t dz_col(const DzSrc& z, int o) {
    if constexpr (!GATHER) return (size_t)o;
    const int i = o / HEAD_RUN;
    return (size_t)i * z.Wimg * HEAD_C + (o - i * HEAD_RUN);
}

__global__ void __launch_bounds__(256) row_stats_kernel(const float* __restrict__ x, int M, int D, float eps, float2* __restrict__ stats) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += xr[c];
    const float mu = wave_sum_dpp(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = xr[c] - mu; q += d * d; }
    const float var = wave_sum_dpp(q) / (float)D;
    if (lane == 0) stats[row] = make_float2(mu, 1.0f / sqrtf(var + eps));
}

// Wp[(i 16 + j) 7 + c][:] = W[c 256 + i 16 + j][:]
__global__ void __launch_bounds__(256) perm_w_kernel(const float* __restrict__ W, int D, float* __restrict__ Wp) {
    const int o = blockIdx.x, src = (o % HEAD_C) * HEAD_P2 + o / HEAD_C;
    for (int k = threadIdx.x * 4; k < D; k += 1024)
        *reinterpret_cast<f32x4*>(Wp + (size_t)o * D + k) = *reinterpret_cast<const f32x4*>(W + (size_t)src * D + k);
}

// Portrait views of a batch stored landscape (the reference's transpose_to_landscape(head, activate=True), blocks/head.py:24-60).  A view is [H][Wimg][7]
// with H <= Wimg, gh = H / 16, gw = Wimg / 16.  Token t of a portrait view is (py, px) = (t / gh, t % gh) of its own gw x gh grid, and its 16 x 16 x 7 tile
// belongs, with i and j exchanged, at the stored slot (px, py); one launch over all rows with the landscape geometry puts (or expects) it unturned at the
// token's slot (t / gw, t % gw).  head_turn_kernel moves the tiles of the flagged views between the two arrangements:
//   to_slots = 0 (forward)   src [view][slot of t][i][j][c]  ->  dst [view][px][py][j][i][c]        the head's output -> the stored layout
//   to_slots = 1 (backward)  src [view][px][py][j][i][c]     ->  dst [view][slot of t][i][j][c]     the upstream gradient -> what dz_row reads
// A wave owns one tile: 7168 bytes, 16 pixel rows of 448 bytes (112 floats, 28 float4) at a stride of Wimg 28 bytes.  In each of 7 rounds lane l takes
// float4 q = 64 n + l of the tile, (row, part) = (q / 28, q % 28): a 16-byte global load, and after the turn a 16-byte global store of float4 q of the
// destination tile, so both sides move whole 448-byte runs.  A pixel is 28 bytes and does not fit the 16-byte grid, so the turn goes through the wave's own
// part of the LDS, element (row i, float e = 7 j + c) of the source tile at dword
//     A(i, e) = 116 i + e                                                            (HT_PITCH = 116, 1856 floats = 7424 bytes per wave)
// written with one ds_write_b128 per round (A(i, 4 f .. 4 f + 3), 16-byte aligned as 116 % 4 == 0) and read with four ds_read_b32 per round: float k of the
// destination's float4 (row j', part f) is element e' = 4 f + k of that row, pixel i = e' / 7, channel c = e' % 7, at A(e' / 7, 7 j' + e' % 7).
// Bank conflicts by the rules for these widths (bank = dword address mod 32 for both; a ds_write_b128 is served in 8 groups of 8 consecutive lanes, a
// ds_read_b32 in the two halves of the wave; each further distinct address on a bank of a group costs one cycle): over the 7 writes of a tile 8 extra cycles
// (a group that crosses from row i to i + 1 skips 4 dwords), over its 28 reads 96 extra cycles on 56 conflict-free ones; 104 per tile.  Other pitches were
// counted the same way: 112 gives 0 + 144, 124 gives 8 + 120, 128 gives 8 + 144, and an odd pitch loses the 16-byte write.
// The blocks of an unflagged view return at once (a block's four tiles lie in one view, so the barrier is reached by all or none of its waves): those views
// cost one flag read per block and no pass over their pixels.  One writer per element, no arithmetic on the values, 64-bit offsets.
constexpr int HT_PITCH = 116, HT_TILE_LDS = 16 * HT_PITCH, HT_Q = 16 * HEAD_RUN / 4, HT_ROUNDS = HT_Q / 64, HT_RUN4 = HEAD_RUN / 4;

struct HeadTurn {
    const float* src;
    float* dst;
    const int32_t* transposed;   // [n_views] on the device
    int H, Wimg, ntok, to_slots;
};

__global__ void __launch_bounds__(256) head_turn_kernel(HeadTurn p) {
    __shared__ __attribute__((aligned(16))) float lds[4 * HT_TILE_LDS];
    const int bpv = (p.ntok + 3) / 4, v = blockIdx.x / bpv;
    if (p.transposed[v] == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = (blockIdx.x - v * bpv) * 4 + wave;
    const bool live = t < p.ntok;
    const int gh = p.H / 16, gw = p.Wimg / 16;
    float* tile = lds + wave * HT_TILE_LDS;
    const size_t row = (size_t)p.Wimg * HEAD_C;
    // the token's slot in the launch's landscape order and its slot in the stored layout
    const int ly = t / gw, lx = t - ly * gw, sx = t / gh, sy = t - sx * gh;
    const size_t at_l = (((size_t)v * p.H + 16 * ly) * p.Wimg + 16 * lx) * HEAD_C, at_s = (((size_t)v * p.H + 16 * sy) * p.Wimg + 16 * sx) * HEAD_C;
    const float* src = p.src + (p.to_slots ? at_s : at_l);
    float* dst = p.dst + (p.to_slots ? at_l : at_s);
    if (live) {
#pragma unroll
        for (int n = 0; n < HT_ROUNDS; ++n) {
            const int q = 64 * n + lane, i = q / HT_RUN4, f = q - i * HT_RUN4;
            *reinterpret_cast<f32x4*>(tile + i * HT_PITCH + 4 * f) = *reinterpret_cast<const f32x4*>(src + i * row + 4 * f);
        }
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int n = 0; n < HT_ROUNDS; ++n) {
        const int q = 64 * n + lane, j = q / HT_RUN4, f = q - j * HT_RUN4;
        f32x4 val;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 4 * f + k, i = e / HEAD_C;
            val[k] = tile[i * HT_PITCH + HEAD_C * j + (e - i * HEAD_C)];
        }
        *reinterpret_cast<f32x4*>(dst + j * row + 4 * f) = val;
    }
}

// the flagged views of src [n_views][n4 float4] over dst; HC_PER_BLOCK float4 (64 KB) per block, the blocks of an unflagged view return at once
constexpr int HC_PER_BLOCK = 4096;
__global__ void __launch_bounds__(256) head_copy_flagged_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, const int32_t* __restrict__ transposed,
                                                                int n4, int bpv) {
    const int v = blockIdx.x / bpv, c0 = (blockIdx.x - v * bpv) * HC_PER_BLOCK;
    if (transposed[v] == 0) return;
    const size_t base = (size_t)v * n4;
#pragma unroll 4
    for (int u = 0; u < HC_PER_BLOCK / 256; ++u) {
        const int c = c0 + u * 256 + threadIdx.x;
        if (c < n4) dst[base + c] = src[base + c];
    }
}

// forward operands from the fp32 parameters: rows in pixel-shuffle order, [W_hi | W_hi | W_lo] (model.hip w3) and the permuted bias
template <class T>
__global__ void __launch_bounds__(256) pack_w3_kernel(const float* __restrict__ W, const float* __restrict__ b, int D, T* __restrict__ wcat,
                                                      float* __restrict__ bias_ps) {
    typedef typename Vec<T>::v4 v4;
    const int o = blockIdx.x, src = (o % HEAD_C) * HEAD_P2 + o / HEAD_C;
    T* row = wcat + (size_t)o * 3 * D;
    for (int k = threadIdx.x * 4; k < D; k += 1024) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)src * D + k);
        const v4 h = cvt4<T>(w);
        const f32x4 hf = __builtin_convertvector(h, f32x4);
        *reinterpret_cast<v4*>(row + k) = h;
        *reinterpret_cast<v4*>(row + D + k) = h;
        *reinterpret_cast<v4*>(row + 2 * D + k) = cvt4<T>(w - hf);
    }
    if (threadIdx.x == 0) bias_ps[o] = b[src];
}

// y fp32 [M][D] -> [y_hi | y_lo | y_hi] rows of 3 D, as the head LayerNorm leaves them
template <class T>
__global__ void __launch_bounds__(256) split3_kernel(const float* __restrict__ y, int D, T* __restrict__ hcat) {
    typedef typename Vec<T>::v4 v4;
    const size_t r = blockIdx.x;
    T* row = hcat + r * 3 * D;
    for (int k = threadIdx.x * 4; k < D; k += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * D + k);
        const v4 h = cvt4<T>(v);
        const f32x4 hf = __builtin_convertvector(h, f32x4);
        *reinterpret_cast<v4*>(row + k) = h;
        *reinterpret_cast<v4*>(row + D + k) = cvt4<T>(v - hf);
        *reinterpret_cast<v4*>(row + 2 * D + k) = h;
    }
}

// the second row block of a two-segment W and the row stride of out (dgrad_kernel<., true>)
struct DgSeg {
    const float* W1;
    int O0, ldo;
};

// out[M, K] = dZ[M, O] W[O, K];  O % 16 == 0, K % 4 == 0; tail rows and columns are zero-filled on load and not stored
// SEG: the rows of W live in two parameters, W [O0][K] and seg.W1 [O - O0][K] with O0 % 16 == 0 (a 16-deep step never straddles the seam), and out has
// the row stride seg.ldo.  The steps and the k-ordered chain are the same: the bits of the plain kernel on a packed copy of W over W1.  The instantiations
// without it are the kernel as it was.
template <int GATHER, bool SEG = false>
__global__ void __launch_bounds__(256) dgrad_kernel(DzSrc z, const float* __restrict__ W, float* __restrict__ out, int M, int O, int K, int n_tiles,
                                                    DgSeg seg = DgSeg{nullptr, 0, 0}) {
    __shared__ __attribute__((aligned(16))) float As[HM * HAP];
    __shared__ __attribute__((aligned(16))) float Bs[HK * HBP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int m0 = (blockIdx.x / n_tiles) * HM, n0 = (blockIdx.x % n_tiles) * HN;
    // staging: A 128 rows x 16 floats and B 16 rows x 128 floats, 512 float4 each, two per thread
    int ar[2], ac[2], br[2], bc[2];
    size_t abase[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = e * 256 + tid;
        ar[e] = idx >> 2; ac[e] = (idx & 3) * 4;
        br[e] = idx >> 5; bc[e] = (idx & 31) * 4;
        aok[e] = m0 + ar[e] < M;
        abase[e] = aok[e] ? dz_row<GATHER>(z, m0 + ar[e]) : 0;
        bok[e] = n0 + bc[e] < K;
    }
    f32x4 acc[4][4];
    // spelled out, not zero_acc (train_tile.hpp): with the call the compiler put one more scalar instruction into the prologue, the loop moved by 4 bytes and
    // the plain form was 4 to 5 % slower at K = 768 (profiles/train_shared_ab.txt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ra[e] = aok[e] ? *reinterpret_cast<const f32x4*>(z.p + abase[e] + dz_col<GATHER>(z, k0 + ac[e])) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float* wrow = W + (size_t)(k0 + br[e]) * K;
            if constexpr (SEG) {
                if (k0 >= seg.O0) wrow = seg.W1 + (size_t)(k0 - seg.O0 + br[e]) * K;
            }
            rb[e] = bok[e] ? *reinterpret_cast<const f32x4*>(wrow + n0 + bc[e]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < O; k0 += HK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            *reinterpret_cast<f32x4*>(As + ar[e] * HAP + ac[e]) = ra[e];
            *reinterpret_cast<f32x4*>(Bs + br[e] * HBP + bc[e]) = rb[e];
        }
        __syncthreads();
        if (k0 + HK < O) fetch(k0 + HK);
#pragma unroll
        for (int ks = 0; ks < HK / 4; ++ks) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[(wm * 64 + i * 16 + fr) * HAP + ks * 4 + fk];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[(ks * 4 + fk) * HBP + wn * 64 + j * 16 + fr];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    const int ldo = SEG ? seg.ldo : K;
    for_each_acc64(acc, m0 + wm * 64, n0 + wn * 64, M, K, fr, fk, [=](int m, int n, int, float x) { out[(size_t)m * ldo + n] = x; });
}

// part[split][O][K] = sum over the split's rows of dZ[r, o] a[r, k], a = (A - mu) rstd with `stats`, A itself without; pdb[split][O] = the
// column sums of the split's dZ rows (blocks of column tile 0).  want_dw = 0: only the column sums (grid of one column tile).
template <int GATHER>
__global__ void __launch_bounds__(256) wgrad_kernel(DzSrc z, const float* __restrict__ A, int lda, const float2* __restrict__ stats, int M, int O, int K,
                                                    int rows_per_split, int o_tiles, int n_tiles, int want_dw, float* __restrict__ part,
                                                    float* __restrict__ pdb) {
    __shared__ __attribute__((aligned(16))) float As[HK * HBP];
    __shared__ __attribute__((aligned(16))) float Bs[HK * HBP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int tile = blockIdx.x % (o_tiles * n_tiles), split = blockIdx.x / (o_tiles * n_tiles);
    const int o0 = (tile / n_tiles) * HM, n0 = (tile % n_tiles) * HN;
    const int r_lo = split * rows_per_split, r_hi = min(M, r_lo + rows_per_split);
    int sr[2], sc[2];
    size_t zcol[2];
    bool zok[2], bok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = e * 256 + tid;
        sr[e] = idx >> 5; sc[e] = (idx & 31) * 4;
        zok[e] = o0 + sc[e] < O;
        zcol[e] = zok[e] ? dz_col<GATHER>(z, o0 + sc[e]) : 0;
        bok[e] = want_dw && n0 + sc[e] < K;
    }
    f32x4 acc[4][4];
    zero_acc(acc);
    f32x4 ra[2], rb[2];
    // DZ_GATHER_AR: a staged row's (view, slot row, slot column) and its view's flag are carried from fetch to fetch -- the row advances by HK, so the slot is
    // stepped, not divided out again, and the flag is read again only where the view changes.  Read in every fetch, the flag put a dependent load and a
    // third division in front of each row's address: 1.0 ms of this kernel's 18 ms at 430080 rows with no view flagged (kernel trace).
    int cv[2] = {0, 0}, cgy[2] = {0, 0}, cgx[2] = {0, 0}, cfl[2] = {0, 0};
    if constexpr (GATHER == DZ_GATHER_AR) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r = r_lo + sr[e];
            if (r < r_hi) {
                cv[e] = r / z.ntok;
                const int t = r - cv[e] * z.ntok;
                cgy[e] = t / z.gw;
                cgx[e] = t - cgy[e] * z.gw;
                cfl[e] = z.flags[cv[e]];
            }
        }
    }
    auto fetch = [&](int r0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r = r0 + sr[e];
            const bool in = r < r_hi;
            size_t at = 0;
            if constexpr (GATHER == DZ_GATHER_AR) {
                at = (((size_t)cv[e] * z.H + 16 * cgy[e]) * z.Wimg + 16 * cgx[e]) * HEAD_C + (cfl[e] != 0 ? (size_t)z.alt : 0);
                // the row of the next fetch
                const int gh = z.H / 16, view = cv[e];
                cgx[e] += HK;
                while (cgx[e] >= z.gw) { cgx[e] -= z.gw; ++cgy[e]; }
                while (cgy[e] >= gh) { cgy[e] -= gh; ++cv[e]; }
                if (cv[e] != view) cfl[e] = r + HK < r_hi ? z.flags[cv[e]] : 0;
            } else {
                at = in ? dz_row<GATHER>(z, r) : 0;
            }
            ra[e] = in && zok[e] ? *reinterpret_cast<const f32x4*>(z.p + at + zcol[e]) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (in && bok[e]) {
                v = *reinterpret_cast<const f32x4*>(A + (size_t)r * lda + n0 + sc[e]);
                if (stats) { const float2 st = stats[r]; v = (v - st.x) * st.y; }
            }
            rb[e] = v;
        }
    };
    const bool sum_cols = n0 == 0 && tid < HM;
    float colsum = 0.f;
    fetch(r_lo);
    for (int r0 = r_lo; r0 < r_hi; r0 += HK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            *reinterpret_cast<f32x4*>(As + sr[e] * HBP + sc[e]) = ra[e];
            *reinterpret_cast<f32x4*>(Bs + sr[e] * HBP + sc[e]) = rb[e];
        }
        __syncthreads();
        if (r0 + HK < r_hi) fetch(r0 + HK);
        if (sum_cols) {
#pragma unroll
            for (int rr = 0; rr < HK; ++rr) colsum += As[rr * HBP + tid];
        }
        if (want_dw) {
#pragma unroll
            for (int ks = 0; ks < HK / 4; ++ks) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = As[(ks * 4 + fk) * HBP + wm * 64 + i * 16 + fr];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = Bs[(ks * 4 + fk) * HBP + wn * 64 + j * 16 + fr];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    if (sum_cols && o0 + tid < O) pdb[(size_t)split * O + o0 + tid] = colsum;
    if (!want_dw) return;
    float* P = part + (size_t)split * O * K;
    for_each_acc64(acc, o0 + wm * 64, n0 + wn * 64, O, K, fr, fk, [=](int o, int n, int, float x) { P[(size_t)o * K + n] = x; });
}

// one block per row o' of the partials; unperm: the row is written at (o' % 7) 256 + o' / 7.  gamma / beta NULL: dW = sum_s P_s.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ pdb, int S, int O, int K,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int unperm,
                                                           float* __restrict__ dW, float* __restrict__ db) {
    const int o = blockIdx.x, dst = unperm ? (o % HEAD_C) * HEAD_P2 + o / HEAD_C : o;
    float bsum = 0.f;
    for (int s = 0; s < S; ++s) bsum += pdb[(size_t)s * O + o];
    if (db && threadIdx.x == 0) db[dst] = bsum;
    if (!dW) return;
    for (int k = threadIdx.x; k < K; k += 256) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += part[((size_t)s * O + o) * K + k];
        dW[(size_t)dst * K + k] = gamma ? gamma[k] * v + beta[k] * bsum : v;
    }
}

// dx may alias dy (each element is read before it is written, by the lane that writes it).  part [blocks][2][D]: column sums of dy x^ and dy.
// ADD: dx = add + (the LayerNorm backward), the residual branch of a pre-norm sublayer; add may alias dx for the same reason.  The instantiation
// without it is the kernel as it was.
template <bool ADD>
__global__ void __launch_bounds__(256) ln_grad_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float2* __restrict__ stats,
                                                      const float* dy, const float* add, float* dx, int M, int D, int rows_per_block,
                                                      float* __restrict__ part) {
    __shared__ float red[3 * 2 * 64 * LNG_MAX_T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, T = D / 64;
    const int r_lo = blockIdx.x * rows_per_block, r_hi = min(M, r_lo + rows_per_block);
    float g[LNG_MAX_T], ag[LNG_MAX_T], ab[LNG_MAX_T];
#pragma unroll
    for (int t = 0; t < LNG_MAX_T; ++t) {
        g[t] = t < T ? gamma[t * 64 + lane] : 0.f;
        ag[t] = 0.f; ab[t] = 0.f;
    }
    for (int r = r_lo + wave; r < r_hi; r += 4) {
        const float2 st = stats[r];
        const size_t o = (size_t)r * D;
        float xh[LNG_MAX_T], gh[LNG_MAX_T];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int t = 0; t < LNG_MAX_T; ++t)
            if (t < T) {
                const float d = dy[o + t * 64 + lane];
                xh[t] = (x[o + t * 64 + lane] - st.x) * st.y;
                gh[t] = d * g[t];
                s1 += gh[t];
                s2 += gh[t] * xh[t];
                ag[t] += d * xh[t];
                ab[t] += d;
            }
        const float m1 = wave_sum_dpp(s1) / (float)D, m2 = wave_sum_dpp(s2) / (float)D;
        if (dx) {
#pragma unroll
            for (int t = 0; t < LNG_MAX_T; ++t)
                if (t < T) {
                    const float v = st.y * (gh[t] - m1 - xh[t] * m2);
                    if constexpr (ADD) dx[o + t * 64 + lane] = add[o + t * 64 + lane] + v;
                    else dx[o + t * 64 + lane] = v;
                }
        }
    }
    if (!part) return;
    // waves 1..3 -> LDS, wave 0 adds them in wave order
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < LNG_MAX_T; ++t)
            if (t < T) {
                red[((wave - 1) * 2 + 0) * 64 * LNG_MAX_T + t * 64 + lane] = ag[t];
                red[((wave - 1) * 2 + 1) * 64 * LNG_MAX_T + t * 64 + lane] = ab[t];
            }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < LNG_MAX_T; ++t)
            if (t < T) {
                float a = ag[t], b = ab[t];
                for (int w = 0; w < 3; ++w) {
                    a += red[(w * 2 + 0) * 64 * LNG_MAX_T + t * 64 + lane];
                    b += red[(w * 2 + 1) * 64 * LNG_MAX_T + t * 64 + lane];
                }
                part[((size_t)blockIdx.x * 2 + 0) * D + t * 64 + lane] = a;
                part[((size_t)blockIdx.x * 2 + 1) * D + t * 64 + lane] = b;
            }
    }
}

// 16 columns per block; slice q of 16 adds the partials of blocks q, q + 16, ... in that order, then one thread per column adds the 16 slices in slice order
__global__ void __launch_bounds__(256) ln_grad_reduce_kernel(const float* __restrict__ part, int NB, int D, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
    __shared__ float ra[16][17], rb[16][17];
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4, k = blockIdx.x * 16 + c;
    float a = 0.f, b = 0.f;
    for (int i = q; i < NB; i += 16) {
        a += part[((size_t)i * 2 + 0) * D + k];
        b += part[((size_t)i * 2 + 1) * D + k];
    }
    ra[q][c] = a; rb[q][c] = b;
    __syncthreads();
    if (q != 0) return;
    a = ra[0][c]; b = rb[0][c];
    for (int j = 1; j < 16; ++j) { a += ra[j][c]; b += rb[j][c]; }
    if (dgamma) dgamma[k] = a;
    if (dbeta) dbeta[k] = b;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------
static int wgrad_splits(long long R) {
    const long long s = (R + WGRAD_ROWS_PER_SPLIT - 1) / WGRAD_ROWS_PER_SPLIT;
    return (int)(s < 1 ? 1 : (s > WGRAD_MAX_SPLITS ? WGRAD_MAX_SPLITS : s));
}
static int wgrad_rows_per_split(int R) {   // a multiple of the 16-row step, so that no step straddles two splits
    const int S = wgrad_splits(R), rows = (R + S - 1) / S;
    return (rows + HK - 1) / HK * HK;
}
static int lng_rows_per_block(int R) {
    const int rows = (R + LNG_MAX_BLOCKS - 1) / LNG_MAX_BLOCKS;
    return rows < LNG_MIN_ROWS ? LNG_MIN_ROWS : rows;
}
static int lng_blocks(int R) { const int rpb = lng_rows_per_block(R); return (R + rpb - 1) / rpb; }

static size_t wgrad_scratch(int M, int O, int K) { return up256((size_t)wgrad_splits(M) * O * K * 4) + up256((size_t)wgrad_splits(M) * O * 4); }
static size_t lng_scratch(int M, int D) { return up256((size_t)M * 8) + up256((size_t)lng_blocks(M) * 2 * D * 4); }

// gather: DZ_PLAIN, DZ_GATHER or DZ_GATHER_AR
static int run_dgrad(int gather, const DzSrc& z, const float* W, float* out, int M, int O, int K, hipStream_t s) {
    const int n_tiles = (K + HN - 1) / HN;
    const long long blocks = (long long)((M + HM - 1) / HM) * n_tiles;
    if (blocks > 0x7fffffffLL) return fail("linear_dgrad: too many rows");
    if (!gather && train_linear_bf16()) return launch_dgrad_bf16("linear_dgrad", z.p, (int)z.ld, W, nullptr, O, out, K, M, O, K, s);
    if (gather == DZ_GATHER_AR)
        hipLaunchKernelGGL((dgrad_kernel<DZ_GATHER_AR, false>), dim3((unsigned)blocks), dim3(256), 0, s, z, W, out, M, O, K, n_tiles, DgSeg{nullptr, 0, 0});
    else if (gather) hipLaunchKernelGGL((dgrad_kernel<DZ_GATHER, false>), dim3((unsigned)blocks), dim3(256), 0, s, z, W, out, M, O, K, n_tiles, DgSeg{nullptr, 0, 0});
    else hipLaunchKernelGGL((dgrad_kernel<DZ_PLAIN, false>), dim3((unsigned)blocks), dim3(256), 0, s, z, W, out, M, O, K, n_tiles, DgSeg{nullptr, 0, 0});
    if (hipGetLastError() != hipSuccess) return fail("linear_dgrad: launch failed");
    return 0;
}

// scratch: [partials S O K | column-sum partials S O]
static int run_wgrad(int gather, const DzSrc& z, const float* A, int lda, const float2* stats, int M, int O, int K, const float* gamma,
                     const float* beta, float* dW, float* db, char* scratch, hipStream_t s) {
    const int S = wgrad_splits(M), rps = wgrad_rows_per_split(M), want_dw = dW ? 1 : 0;
    const int o_tiles = (O + HM - 1) / HM, n_tiles = want_dw ? (K + HN - 1) / HN : 1;
    float* part = reinterpret_cast<float*>(scratch);
    float* pdb = reinterpret_cast<float*>(scratch + up256((size_t)S * O * K * 4));
    const dim3 grid((unsigned)(o_tiles * n_tiles * S));
    if (!gather && !stats && train_linear_bf16()) M3R_RUN(launch_wgrad_parts_bf16(z.p, (int)z.ld, A, lda, M, O, K, rps, S, want_dw, part, pdb, s));
    else if (gather == DZ_GATHER_AR)
        hipLaunchKernelGGL(wgrad_kernel<DZ_GATHER_AR>, grid, dim3(256), 0, s, z, A, lda, stats, M, O, K, rps, o_tiles, n_tiles, want_dw, part, pdb);
    else if (gather) hipLaunchKernelGGL(wgrad_kernel<DZ_GATHER>, grid, dim3(256), 0, s, z, A, lda, stats, M, O, K, rps, o_tiles, n_tiles, want_dw, part, pdb);
    else hipLaunchKernelGGL(wgrad_kernel<DZ_PLAIN>, grid, dim3(256), 0, s, z, A, lda, stats, M, O, K, rps, o_tiles, n_tiles, want_dw, part, pdb);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(O), dim3(256), 0, s, part, pdb, S, O, K, gamma, beta, gather ? 1 : 0, dW, db);
    if (hipGetLastError() != hipSuccess) return fail("linear_wgrad: launch failed");
    return 0;
}

static int run_stats(const float* x, int M, int D, float eps, float2* stats, hipStream_t s) {
    hipLaunchKernelGGL(row_stats_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, M, D, eps, stats);
    if (hipGetLastError() != hipSuccess) return fail("head_grad: the statistics launch failed");
    return 0;
}

// part: lng_blocks(M) x 2 x D floats, or NULL when neither dgamma nor dbeta is asked for
static int run_ln_grad(const float* x, const float* gamma, const float2* stats, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta,
                       int M, int D, float* part, hipStream_t s) {
    const int NB = lng_blocks(M), rpb = lng_rows_per_block(M);
    const bool cols = dgamma || dbeta;
    if (add && dx) hipLaunchKernelGGL(ln_grad_kernel<true>, dim3(NB), dim3(256), 0, s, x, gamma, stats, dy, add, dx, M, D, rpb, cols ? part : nullptr);
    else hipLaunchKernelGGL(ln_grad_kernel<false>, dim3(NB), dim3(256), 0, s, x, gamma, stats, dy, nullptr, dx, M, D, rpb, cols ? part : nullptr);
    if (cols) hipLaunchKernelGGL(ln_grad_reduce_kernel, dim3(D / 16), dim3(256), 0, s, part, NB, D, dgamma, dbeta);
    if (hipGetLastError() != hipSuccess) return fail("layernorm_grad: launch failed");
    return 0;
}

static const char* head_shape_error(int n_views, int H, int Wimg, int D) {
    if (n_views <= 0 || H <= 0 || Wimg <= 0) return "n_views, H and W must be positive";
    if (H % 16 || Wimg % 16) return "H and W must be multiples of 16";
    if (D <= 0 || D % 64) return "D must be a positive multiple of 64";
    if (D > 64 * LNG_MAX_T) return "D must not exceed 1024";
    if ((long long)n_views * (H / 16) * (Wimg / 16) > 0x7fffffffLL / 4) return "too many tokens";
    return nullptr;
}

static size_t head_forward_scratch(int R, int D) {
    const size_t O = HEAD_C * HEAD_P2;
    return up256((size_t)R * 3 * D * 2) + up256(O * 3 * D * 2) + up256(O * 4);
}

// y fp32 [R][D] given: the Linear stage alone; x given: LayerNorm first
static int head_forward(int dtype, const float* x, const float* y, const float* gamma, const float* beta, const float* W, const float* b, int n_views,
                        int H, int Wimg, int D, float eps, float* pointmaps, void* scratch, size_t scratch_bytes, void* stream, const char* who) {
    if (const char* e = head_shape_error(n_views, H, Wimg, D)) return fail("%s: %s", who, e);
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("%s: dtype must be MUST3R_BF16 or MUST3R_F16", who);
    if (!(x || y) || !W || !b || !pointmaps || (x && (!gamma || !beta))) return fail("%s: null argument", who);
    if (misaligned(x) || misaligned(y) || misaligned(W) || misaligned(pointmaps)) return fail("%s: tensors must be 16-byte aligned", who);
    const int ntok = (H / 16) * (Wimg / 16), R = n_views * ntok, O = HEAD_C * HEAD_P2;
    if (!scratch || scratch_bytes < head_forward_scratch(R, D) || misaligned(scratch)) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DType dt = dtype == MUST3R_BF16 ? DT_BF16 : DT_F16;
    char* p = reinterpret_cast<char*>(scratch);
    void* hcat = p;
    void* wcat = p + up256((size_t)R * 3 * D * 2);
    float* bias_ps = reinterpret_cast<float*>(p + up256((size_t)R * 3 * D * 2) + up256((size_t)O * 3 * D * 2));
    if (dt == DT_BF16) hipLaunchKernelGGL(pack_w3_kernel<bf16_t>, dim3(O), dim3(256), 0, s, W, b, D, (bf16_t*)wcat, bias_ps);
    else hipLaunchKernelGGL(pack_w3_kernel<f16_t>, dim3(O), dim3(256), 0, s, W, b, D, (f16_t*)wcat, bias_ps);
    if (x) {
        if (head_layernorm(nullptr, dt, x, gamma, beta, hcat, nullptr, R, D, eps, s)) return 1;
    } else {
        if (dt == DT_BF16) hipLaunchKernelGGL(split3_kernel<bf16_t>, dim3(R), dim3(256), 0, s, y, D, (bf16_t*)hcat);
        else hipLaunchKernelGGL(split3_kernel<f16_t>, dim3(R), dim3(256), 0, s, y, D, (f16_t*)hcat);
    }
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return head_linear(nullptr, dt, hcat, wcat, bias_ps, pointmaps, R, D, O, ntok, Wimg / 16, H, Wimg, 0, 0, s);
}

int launch_dgrad_seg_f32(const float* dZ, int ldz, const float* W0, const float* W1, int O0, float* out, int ldo, int M, int O, int K, hipStream_t s) {
    if (M <= 0 || O <= 0 || K <= 0) return fail("linear_dgrad (two segments): bad shape");
    if (!dZ || !W0 || !W1 || !out) return fail("linear_dgrad (two segments): null argument");
    if (O % 16 || O0 % 16 || O0 <= 0 || O0 >= O) return fail("linear_dgrad (two segments): O and the seam must be multiples of 16, the seam inside (0, O)");
    if (K % 4 || ldz < O || ldz % 4 || ldo < K) return fail("linear_dgrad (two segments): K and ldz must be multiples of 4, ldz >= O, ldo >= K");
    if (misaligned(dZ) || misaligned(W0) || misaligned(W1)) return fail("linear_dgrad (two segments): dZ and the weights must be 16-byte aligned");
    const int n_tiles = (K + HN - 1) / HN;
    const long long blocks = (long long)((M + HM - 1) / HM) * n_tiles;
    if (blocks > 0x7fffffffLL) return fail("linear_dgrad (two segments): too many rows");
    if (train_linear_bf16()) return launch_dgrad_bf16("linear_dgrad (two segments)", dZ, ldz, W0, W1, O0, out, ldo, M, O, K, s);
    const DzSrc z{dZ, ldz, 0, 0, 0, 0};
    hipLaunchKernelGGL((dgrad_kernel<DZ_PLAIN, true>), dim3((unsigned)blocks), dim3(256), 0, s, z, W0, out, M, O, K, n_tiles, DgSeg{W1, O0, ldo});
    if (hipGetLastError() != hipSuccess) return fail("linear_dgrad (two segments): launch failed");
    return 0;
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_head_grad_splits(int rows) { return rows > 0 ? wgrad_splits(rows) : 0; }

extern "C" size_t must3r_hip_head_forward_scratch_bytes(int n_views, int H, int Wimg, int D) {
    if (const char* e = head_shape_error(n_views, H, Wimg, D)) { fail("head_forward_scratch_bytes: %s", e); return 0; }
    return head_forward_scratch(n_views * (H / 16) * (Wimg / 16), D);
}

extern "C" int must3r_hip_head_forward(int dtype, const float* x, const float* gamma, const float* beta, const float* W, const float* b, int n_views,
                                       int H, int Wimg, int D, float eps, float* pointmaps, void* scratch, size_t scratch_bytes, void* stream) {
    if (!x) return fail("head_forward: null argument");
    return head_forward(dtype, x, nullptr, gamma, beta, W, b, n_views, H, Wimg, D, eps, pointmaps, scratch, scratch_bytes, stream, "head_forward");
}

extern "C" int must3r_hip_op_head_linear(int dtype, const float* y, const float* W, const float* b, int n_views, int H, int Wimg, int D,
                                         float* pointmaps, void* scratch, size_t scratch_bytes, void* stream) {
    if (!y) return fail("op_head_linear: null argument");
    return head_forward(dtype, nullptr, y, nullptr, nullptr, W, b, n_views, H, Wimg, D, 0.f, pointmaps, scratch, scratch_bytes, stream, "op_head_linear");
}

// scratch of must3r_hip_head_grad: [statistics R x 2 | permuted W | weight-gradient partials and column sums | LayerNorm column partials]
static size_t head_grad_scratch(int R, int D) {
    const int O = HEAD_C * HEAD_P2;
    return up256((size_t)R * 8) + up256((size_t)O * D * 4) + wgrad_scratch(R, O, D) + up256((size_t)lng_blocks(R) * 2 * D * 4);
}
extern "C" size_t must3r_hip_head_grad_scratch_bytes(int n_views, int H, int Wimg, int D) {
    if (const char* e = head_shape_error(n_views, H, Wimg, D)) { fail("head_grad_scratch_bytes: %s", e); return 0; }
    return head_grad_scratch(n_views * (H / 16) * (Wimg / 16), D);
}

// what the per-view orientation adds to a head call: one copy of the pointmaps / of the upstream gradient, for the turned tiles of the flagged views
static size_t head_ar_scratch(int n_views, int H, int Wimg) { return up256((size_t)n_views * H * Wimg * HEAD_C * 4); }
static const char* head_ar_error(int H, int Wimg, const int32_t* transposed) {
    if (H > Wimg) return "a batch with portrait flags is stored landscape (H <= W)";
    if ((size_t)transposed & 3) return "transposed must be 4-byte aligned";
    if ((long long)H * Wimg * HEAD_C / 4 > 0x7fffffffLL) return "a view is too large";
    return nullptr;
}
static int run_head_turn(const float* src, float* dst, const int32_t* transposed, int n_views, int H, int Wimg, int to_slots, hipStream_t s) {
    const int ntok = (H / 16) * (Wimg / 16), bpv = (ntok + 3) / 4;
    hipLaunchKernelGGL(head_turn_kernel, dim3((unsigned)(n_views * bpv)), dim3(256), 0, s, HeadTurn{src, dst, transposed, H, Wimg, ntok, to_slots});
    if (hipGetLastError() != hipSuccess) return fail("head (portrait views): the turn launch failed");
    return 0;
}

// transposed == NULL: must3r_hip_head_grad as it was, launch for launch.  Otherwise `turned`, head_ar_scratch bytes, takes the flagged views' gradient tiles
// in the slot order of their tokens and the gather forms pick their source per view.
static int head_grad(const must3r_hip_head_grad_args* a, const int32_t* transposed, float* turned, char* p, hipStream_t s, const char* who) {
    const bool want_w = a->dW || a->db, want_x = a->dx || a->dgamma || a->dbeta;
    const int D = a->D, ntok = (a->H / 16) * (a->Wimg / 16), R = a->n_views * ntok, O = HEAD_C * HEAD_P2;
    float2* stats = reinterpret_cast<float2*>(p); p += up256((size_t)R * 8);
    float* Wp = reinterpret_cast<float*>(p); p += up256((size_t)O * D * 4);
    char* wscr = p; p += wgrad_scratch(R, O, D);
    float* lpart = reinterpret_cast<float*>(p);
    DzSrc z{a->G, 0, ntok, a->Wimg / 16, a->H, a->Wimg};
    const int gather = transposed ? DZ_GATHER_AR : DZ_GATHER;
    if (transposed && (want_w || want_x)) {
        z.flags = transposed;
        z.alt = (long long)((reinterpret_cast<intptr_t>(turned) - reinterpret_cast<intptr_t>(a->G)) / 4);
        M3R_RUN(run_head_turn(a->G, turned, transposed, a->n_views, a->H, a->Wimg, 1, s));
    }
    if (a->dW || want_x) M3R_RUN(run_stats(a->x, R, D, a->eps, stats, s));
    if (want_w) M3R_RUN(run_wgrad(gather, z, a->x, D, stats, R, O, D, a->gamma, a->beta, a->dW, a->db, wscr, s));
    if (want_x) {
        // dY goes where dx will be; without dx it needs a home of its own, which the caller did not give: the partials' space is free again
        // only after the reduce above has read it (stream order), and R D floats may not fit there -- so dgamma / dbeta alone still need dx
        if (!a->dx) return fail("%s: dgamma / dbeta without dx is not provided for (dY lives in the dx buffer)", who);
        hipLaunchKernelGGL(perm_w_kernel, dim3(O), dim3(256), 0, s, a->W, D, Wp);
        M3R_RUN(run_dgrad(gather, z, Wp, a->dx, R, O, D, s));
        M3R_RUN(run_ln_grad(a->x, a->gamma, stats, a->dx, nullptr, a->dx, a->dgamma, a->dbeta, R, D, lpart, s));
    }
    return 0;
}
// 0, or the descriptor is refused with the reason as the last error; nothing is read through a device pointer
static int head_grad_check(const must3r_hip_head_grad_args* a, const char* who) {
    if (const char* e = head_shape_error(a->n_views, a->H, a->Wimg, a->D)) return fail("%s: %s", who, e);
    const bool want_x = a->dx || a->dgamma || a->dbeta;
    if (!a->G) return fail("%s: null argument (G)", who);
    if (a->dW && (!a->x || !a->gamma || !a->beta)) return fail("%s: null argument (dW needs x, gamma and beta)", who);
    if (want_x && (!a->x || !a->gamma || !a->W)) return fail("%s: null argument (dx, dgamma and dbeta need x, gamma and W)", who);
    if (misaligned(a->x) || misaligned(a->W) || misaligned(a->G) || misaligned(a->dx) || misaligned(a->dW))
        return fail("%s: tensors must be 16-byte aligned", who);
    return 0;
}

extern "C" int must3r_hip_head_grad(const must3r_hip_head_grad_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    if (!a) return fail("head_grad: null argument");
    M3R_RUN(head_grad_check(a, "head_grad"));
    if (!scratch || misaligned(scratch) || scratch_bytes < must3r_hip_head_grad_scratch_bytes(a->n_views, a->H, a->Wimg, a->D))
        return fail("head_grad: scratch too small");
    return head_grad(a, nullptr, nullptr, reinterpret_cast<char*>(scratch), reinterpret_cast<hipStream_t>(stream), "head_grad");
}

// The head over a batch stored landscape whose views carry portrait flags (ABI 21, additive; the kernels' comment is above head_turn_kernel).
// scratch: [the scratch of the plain entry point | one copy of the pointmaps / of the upstream gradient]; the second part is asked for with or without flags.
extern "C" size_t must3r_hip_head_forward_many_ar_scratch_bytes(int n_views, int H, int Wimg, int D) {
    if (const char* e = head_shape_error(n_views, H, Wimg, D)) { fail("head_forward_many_ar_scratch_bytes: %s", e); return 0; }
    return head_forward_scratch(n_views * (H / 16) * (Wimg / 16), D) + head_ar_scratch(n_views, H, Wimg);
}

extern "C" int must3r_hip_head_forward_many_ar(const must3r_hip_head_forward_ar_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "head_forward_many_ar";
    if (!a) return fail("%s: null argument", who);
    if (!a->x) return fail("%s: null argument", who);
    if (const char* e = head_shape_error(a->n_views, a->H, a->Wimg, a->D)) return fail("%s: %s", who, e);
    if (a->transposed) {
        if (const char* e = head_ar_error(a->H, a->Wimg, a->transposed)) return fail("%s: %s", who, e);
    }
    const size_t plain = head_forward_scratch(a->n_views * (a->H / 16) * (a->Wimg / 16), a->D);
    if (!scratch || misaligned(scratch) || scratch_bytes < plain + head_ar_scratch(a->n_views, a->H, a->Wimg)) return fail("%s: scratch too small", who);
    // the head writes every view in place with the landscape geometry: an unflagged view is finished by that
    M3R_RUN(head_forward(a->dtype, a->x, nullptr, a->gamma, a->beta, a->W, a->b, a->n_views, a->H, a->Wimg, a->D, a->eps, a->pointmaps, scratch, plain, a->stream, who));
    if (!a->transposed) return 0;
    // a flagged view's tiles change places among themselves, so they are turned into the scratch and copied back: two passes over those views alone
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    float* turned = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + plain);
    M3R_RUN(run_head_turn(a->pointmaps, turned, a->transposed, a->n_views, a->H, a->Wimg, 0, s));
    const int n4 = a->H * a->Wimg * HEAD_C / 4, bpv = (n4 + HC_PER_BLOCK - 1) / HC_PER_BLOCK;
    if ((long long)a->n_views * bpv > 0x7fffffffLL) return fail("%s: too many pixels", who);
    hipLaunchKernelGGL(head_copy_flagged_kernel, dim3((unsigned)(a->n_views * bpv)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(turned),
                       reinterpret_cast<f32x4*>(a->pointmaps), a->transposed, n4, bpv);
    if (hipGetLastError() != hipSuccess) return fail("%s: the copy launch failed", who);
    return 0;
}

extern "C" size_t must3r_hip_head_grad_many_ar_scratch_bytes(int n_views, int H, int Wimg, int D) {
    if (const char* e = head_shape_error(n_views, H, Wimg, D)) { fail("head_grad_many_ar_scratch_bytes: %s", e); return 0; }
    return head_grad_scratch(n_views * (H / 16) * (Wimg / 16), D) + head_ar_scratch(n_views, H, Wimg);
}

extern "C" int must3r_hip_head_grad_many_ar(const must3r_hip_head_grad_ar_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "head_grad_many_ar";
    if (!a) return fail("%s: null argument", who);
    const must3r_hip_head_grad_args* g = &a->g;
    M3R_RUN(head_grad_check(g, who));
    if (a->transposed) {
        if (const char* e = head_ar_error(g->H, g->Wimg, a->transposed)) return fail("%s: %s", who, e);
    }
    const size_t plain = head_grad_scratch(g->n_views * (g->H / 16) * (g->Wimg / 16), g->D);
    if (!scratch || misaligned(scratch) || scratch_bytes < plain + head_ar_scratch(g->n_views, g->H, g->Wimg)) return fail("%s: scratch too small", who);
    char* p = reinterpret_cast<char*>(scratch);
    return head_grad(g, a->transposed, reinterpret_cast<float*>(p + plain), p, reinterpret_cast<hipStream_t>(a->stream), who);
}

extern "C" int must3r_hip_op_linear_dgrad_f32(const float* dZ, int ldz, const float* W, float* out, int M, int O, int K, void* stream) {
    if (M < 0 || O <= 0 || K <= 0) return fail("op_linear_dgrad_f32: bad shape");
    if (M == 0) return 0;
    if (!dZ || !W || !out) return fail("op_linear_dgrad_f32: null argument");
    if (O % 16 || K % 4 || ldz < O || ldz % 4) return fail("op_linear_dgrad_f32: O must be a multiple of 16, K and ldz of 4, ldz >= O");
    if (misaligned(dZ) || misaligned(W)) return fail("op_linear_dgrad_f32: dZ and W must be 16-byte aligned");
    const DzSrc z{dZ, ldz, 0, 0, 0, 0};
    return run_dgrad(false, z, W, out, M, O, K, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t must3r_hip_op_linear_wgrad_scratch_bytes(int M, int O, int K) {
    if (M <= 0 || O <= 0 || K <= 0) return 0;
    return wgrad_scratch(M, O, K);
}

extern "C" int must3r_hip_op_linear_wgrad_f32(const float* dZ, int ldz, const float* A, int lda, float* dW, float* db, int M, int O, int K,
                                              void* scratch, size_t scratch_bytes, void* stream) {
    if (M <= 0 || O <= 0 || K <= 0) return fail("op_linear_wgrad_f32: bad shape");
    if (!dZ || (dW && !A)) return fail("op_linear_wgrad_f32: null argument");
    if (!dW && !db) return 0;
    if (O % 4 || K % 4 || ldz < O || ldz % 4 || (dW && (lda < K || lda % 4))) return fail("op_linear_wgrad_f32: O, K, ldz and lda must be multiples of 4, ldz >= O, lda >= K");
    if (misaligned(dZ) || misaligned(A)) return fail("op_linear_wgrad_f32: dZ and A must be 16-byte aligned");
    if (!scratch || misaligned(scratch) || scratch_bytes < wgrad_scratch(M, O, K)) return fail("op_linear_wgrad_f32: scratch too small");
    const DzSrc z{dZ, ldz, 0, 0, 0, 0};
    return run_wgrad(false, z, A, lda, nullptr, M, O, K, nullptr, nullptr, dW, db, reinterpret_cast<char*>(scratch), reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t must3r_hip_op_layernorm_grad_scratch_bytes(int M, int D) {
    if (M <= 0 || D <= 0) return 0;
    return lng_scratch(M, D);
}

static int op_layernorm_grad(const char* who, const float* x, const float* gamma, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta,
                             int M, int D, float eps, void* scratch, size_t scratch_bytes, void* stream) {
    if (M <= 0 || D <= 0 || D % 64 || D > 64 * LNG_MAX_T) return fail("%s: M must be positive, D a multiple of 64 and at most 1024", who);
    if (!x || !gamma || !dy) return fail("%s: null argument", who);
    if (!dx && !dgamma && !dbeta) return 0;
    if (!scratch || misaligned(scratch) || scratch_bytes < lng_scratch(M, D)) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float2* stats = reinterpret_cast<float2*>(scratch);
    float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + up256((size_t)M * 8));
    M3R_RUN(run_stats(x, M, D, eps, stats, s));
    return run_ln_grad(x, gamma, stats, dy, add, dx, dgamma, dbeta, M, D, part, s);
}

extern "C" int must3r_hip_op_layernorm_grad(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int M, int D,
                                            float eps, void* scratch, size_t scratch_bytes, void* stream) {
    return op_layernorm_grad("op_layernorm_grad", x, gamma, dy, nullptr, dx, dgamma, dbeta, M, D, eps, scratch, scratch_bytes, stream);
}

extern "C" int must3r_hip_op_layernorm_grad_add(const float* x, const float* gamma, const float* dy, const float* add, float* dx, float* dgamma,
                                                float* dbeta, int M, int D, float eps, void* scratch, size_t scratch_bytes, void* stream) {
    return op_layernorm_grad("op_layernorm_grad_add", x, gamma, dy, add, dx, dgamma, dbeta, M, D, eps, scratch, scratch_bytes, stream);
}
