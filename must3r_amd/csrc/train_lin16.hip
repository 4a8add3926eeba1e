// The three forms of a training Linear on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, and the per-thread mode that selects them
// (must3r_hip_train_linear_mode, ABI 21 additive).  Everything in memory stays fp32 -- activations, master weights, outputs, gradients, scratch: the operands are
// rounded to bf16 (nearest even, NaN and inf kept: the result of Tensor.to(torch.bfloat16)) in registers on their way into LDS.  There is no cast pass and no
// 16-bit copy of a weight.  Products of two bf16 values are exact in fp32, so the only error beside the operand rounding is the fp32 summation.
//
//   linear_fwd_bf16<EPI>  NT: out[M, N] = bf16(A)[M, K] bf16(W)[N, K]^T + bias, then the epilogue it shares with linear_fwd_f32 (train_lin.hpp lin_epilogue).
//   dgrad_bf16            NN: out[M, K] = bf16(dZ)[M, O] bf16(W)[O, K]; the rows of W may live in two parameters (launch_dgrad_seg_f32): one kernel, the seam a
//                         kernel argument, so that the segmented form has the bits of the plain one on a packed copy.
//   wgrad_bf16            TN: P_s[O, K] = sum_{r in split s} bf16(dZ)[r, o] bf16(A)[r, k]; split rule, partial layout and reduce are wgrad_kernel's
//                         (train_head.hip).  The column sums of dZ (db partials) are added in fp32 from the unrounded values.
//
// One tile shape for all three, that of the fp32 kernels: 128 x 128 outputs per block, 4 waves of 64 x 64 (4 x 4 accumulators), 32-deep steps through LDS, the next
// step's operands fetched into registers (fp32) under the products of the current one.  An operand whose contraction index is its fast dimension in memory (A and
// W of the forward, dZ of dgrad) is staged as 8 floats -> one 16-byte write into a [128 free][32 contraction] bf16 tile with rows padded to 40 elements (80 bytes):
// a lane's fragment, 8 consecutive contraction indices of one row, is one 16-byte read, and the 16 rows of a fragment start in 16 different groups of 4 banks.
// An operand whose contraction index is its slow dimension (W of dgrad, both operands of wgrad) goes to LDS as it lies, [32 contraction][128 free] with rows
// padded to 144 elements, one 8-byte write per thread and row, and is transposed by the read: a fragment is two ds_read_b64_tr_b16 (train_tile.hpp frag_tr4).
// With 144-element rows the 8 rows a 32-lane half reads start 8 banks apart.  Transposing at the LDS write instead was built and timed for both kernels and was
// 2 to 16 % slower (profiles/linear16_transpose_ab.txt).
// Tails: a step that reaches past the contraction (K = 16, 48: half a step; the last rows of a split) and rows and columns past M, N, O are filled by a select
// on the load, never by a product with zero, and no load touches the padding of a strided row.  No atomics: every output element has one writer and a fixed
// order of additions; a row of out / dX depends on no other row (a padded row is zero in registers and is not stored).
#include "abi.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "train_common.hpp"
#include "train_lin.hpp"
#include "train_tile.hpp"

namespace m3r {

constexpr int TM = 128, TN = 128, TK = 32, TP = 40;   // TP: LDS row stride (bf16 elements) of a [128][32] tile
constexpr int TRP = 144;                               // and of a [32][128] tile that is read transposed

static thread_local int g_train_linear_mode = MUST3R_TRAIN_LINEAR_F32;
bool train_linear_bf16() { return g_train_linear_mode == MUST3R_TRAIN_LINEAR_BF16; }

// 8 consecutive contraction indices of one row: one 16-byte LDS write
__device__ __forceinline__ void put_row8(bf16_t* dst, f32x4 lo, f32x4 hi) {
    *reinterpret_cast<bf16x8*>(dst) = cat8(cvt4<bf16_t>(lo), cvt4<bf16_t>(hi));
}
// one 32-deep step of a wave's 64 x 64: A[row lane & 15][k = 8 (lane >> 4) + e], B[k][column lane & 15]; both tiles are [free][contraction] (the forward)
__device__ __forceinline__ void mma_step(const bf16_t* As, const bf16_t* Bs, int wm, int wn, int fr, int fk, f32x4 (&acc)[4][4]) {
    bf16x8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(As + (wm * 64 + i * 16 + fr) * TP + fk * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 64 + j * 16 + fr) * TP + fk * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
}

// K % 16 == 0: a thread's 8 floats (columns 8 (tid & 3) ... + 7 of a step) lie inside the contraction or past it as a whole
template <int EPI>
__global__ void __launch_bounds__(256) linear_fwd_bf16(LinArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t As[TM * TP];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[TN * TP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int m0 = (blockIdx.x / p.n_tiles) * TM, n0 = (blockIdx.x % p.n_tiles) * TN;
    // staging: 128 rows x 32 floats of each operand, 512 runs of 8 floats each, two per thread (rows tid / 4 and 64 + tid / 4, the same columns)
    const int sc = (tid & 3) * 8;
    int sr[2];
    const float* ap[2];
    const float* wp[2];
    bool aok[2], wok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        sr[e] = e * 64 + (tid >> 2);
        aok[e] = m0 + sr[e] < p.M;
        wok[e] = n0 + sr[e] < p.N;
        ap[e] = p.A + (aok[e] ? (size_t)(m0 + sr[e]) * p.lda + sc : 0);
        wp[e] = p.W + (wok[e] ? (size_t)(n0 + sr[e]) * p.K + sc : 0);
    }
    f32x4 acc[4][4];
    zero_acc(acc);
    f32x4 ra[4], rb[4];
    auto fetch = [&](int k0) {
        const bool in = k0 + sc < p.K;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ra[2 * e] = ld4_or_zero(ap[e] + k0, in && aok[e]);
            ra[2 * e + 1] = ld4_or_zero(ap[e] + k0 + 4, in && aok[e]);
            rb[2 * e] = ld4_or_zero(wp[e] + k0, in && wok[e]);
            rb[2 * e + 1] = ld4_or_zero(wp[e] + k0 + 4, in && wok[e]);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < p.K; k0 += TK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            put_row8(As + sr[e] * TP + sc, ra[2 * e], ra[2 * e + 1]);
            put_row8(Bs + sr[e] * TP + sc, rb[2 * e], rb[2 * e + 1]);
        }
        __syncthreads();
        if (k0 + TK < p.K) fetch(k0 + TK);
        mma_step(As, Bs, wm, wn, fr, fk, acc);
    }
    lin_epilogue<EPI>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// O % 16 == 0, O0 % 16 == 0, K % 4 == 0.  Rows [0, O0) of W come from W0, rows [O0, O) from W1 (O0 = O: W0 alone), chosen row by row.
// dZ is staged like the forward's A; W, whose contraction index is its slow dimension, goes to LDS as it lies, [32 rows][128 columns] with rows of TRP elements,
// and is transposed by the read (train_tile.hpp frag_tr4, which states the row permutation): a lane group reads the same 8 contraction indices of dZ's step
// with two 8-byte reads, at 4 fk and 16 + 4 fk.  (Transposing W at the LDS write instead was built and timed: 9 to 16 % slower.)
__global__ void __launch_bounds__(256) dgrad_bf16(const float* __restrict__ dZ, int ldz, const float* __restrict__ W0, const float* __restrict__ W1, int O0,
                                                  float* __restrict__ out, int ldo, int M, int O, int K, int n_tiles) {
    __shared__ __attribute__((aligned(16))) bf16_t As[TM * TP];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[TK * TRP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int m0 = (blockIdx.x / n_tiles) * TM, n0 = (blockIdx.x % n_tiles) * TN;
    // A (dZ): as the forward's.  B (W): 32 rows x 128 columns as they lie; thread = 4 columns (4 cg) of the rows rg, rg + 8, rg + 16, rg + 24 of a step
    const int sc = (tid & 3) * 8, cg = tid & 31, rg = tid >> 5;
    int sr[2];
    const float* ap[2];
    bool aok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        sr[e] = e * 64 + (tid >> 2);
        aok[e] = m0 + sr[e] < M;
        ap[e] = dZ + (aok[e] ? (size_t)(m0 + sr[e]) * ldz + sc : 0);
    }
    const bool bok = n0 + cg * 4 < K;
    f32x4 acc[4][4];
    zero_acc(acc);
    f32x4 ra[4], rb[4];
    auto fetch = [&](int k0) {
        const bool in = k0 + sc < O;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ra[2 * e] = ld4_or_zero(ap[e] + k0, in && aok[e]);
            ra[2 * e + 1] = ld4_or_zero(ap[e] + k0 + 4, in && aok[e]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = k0 + rg + 8 * i;
            const bool bin = bok && o < O;
            const float* wrow = o < O0 ? W0 + (size_t)o * K : W1 + (size_t)(o - O0) * K;
            rb[i] = ld4_or_zero(bin ? wrow + n0 + cg * 4 : W0, bin);
        }
    };
    const int trow = fk * 4 + (fr >> 2), tcol = (fr & 3) * 4;
    fetch(0);
    for (int k0 = 0; k0 < O; k0 += TK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) put_row8(As + sr[e] * TP + sc, ra[2 * e], ra[2 * e + 1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<bf16x4*>(Bs + (rg + 8 * i) * TRP + cg * 4) = cvt4<bf16_t>(rb[i]);
        __syncthreads();
        if (k0 + TK < O) fetch(k0 + TK);
        // lane group g multiplies the contraction indices 4 g ... 4 g + 3 and 16 + 4 g ... 16 + 4 g + 3 of the step: A by two 8-byte reads, W by two transposing ones
        bf16x8 a[4], b[4];
        frag_tr4<TRP>(Bs + trow * TRP + wn * 64 + tcol, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bf16_t* pa = As + (wm * 64 + i * 16 + fr) * TP + fk * 4;
            a[i] = cat8(*reinterpret_cast<const bf16x4*>(pa), *reinterpret_cast<const bf16x4*>(pa + 16));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
    }
    for_each_acc64(acc, m0 + wm * 64, n0 + wn * 64, M, K, fr, fk, [=](int m, int n, int, float x) { out[(size_t)m * ldo + n] = x; });
}

// part[split][O][K] and pdb[split][O] as wgrad_kernel leaves them (train_head.hip); O % 4 == 0, K % 4 == 0.  want_dw = 0: only the column sums (one column tile).
// Both operands have the contraction (the rows) as their slow dimension, and the transpose is left to the LDS read: the tiles are [32 rows][128 columns] bf16 as
// the operands lie in memory (rows padded to TRP elements), written with one 8-byte store per thread and row, and both are read with train_tile.hpp frag_tr4 -- the same permutation
// of the 32 rows of a step for both operands, so the products that meet are those of equal rows; with TRP = 144 the 8 rows a 32-lane half reads start 8 banks
// apart.  (Transposing at the LDS write instead was built and timed: 2 to 14 % slower.)
// The column sums: a thread adds the fp32 dZ values it fetched, step after step in row order; the 8 threads of a column group are added in a fixed order.
__global__ void __launch_bounds__(256) wgrad_bf16(const float* __restrict__ dZ, int ldz, const float* __restrict__ A, int lda, int M, int O, int K,
                                                     int rows_per_split, int o_tiles, int n_tiles, int want_dw, float* __restrict__ part,
                                                     float* __restrict__ pdb) {
    __shared__ __attribute__((aligned(16))) bf16_t As[TK * TRP];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[TK * TRP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int tile = blockIdx.x % (o_tiles * n_tiles), split = blockIdx.x / (o_tiles * n_tiles);
    const int o0 = (tile / n_tiles) * TM, n0 = (tile % n_tiles) * TN;
    const int r_lo = split * rows_per_split, r_hi = min(M, r_lo + rows_per_split);
    // staging: thread = 4 columns (4 cg) of the rows rg, rg + 8, rg + 16, rg + 24 of a step
    const int cg = tid & 31, rg = tid >> 5;
    const bool zok = o0 + cg * 4 < O, bok = want_dw && n0 + cg * 4 < K;
    const bool sum_cols = n0 == 0;
    f32x4 acc[4][4];
    zero_acc(acc);
    f32x4 ra[4], rb[4];
    f32x4 colsum = f32x4{0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + rg + 8 * i;
            const bool in = r < r_hi;
            ra[i] = ld4_or_zero(in && zok ? dZ + (size_t)r * ldz + o0 + cg * 4 : dZ, in && zok);
            rb[i] = ld4_or_zero(in && bok ? A + (size_t)r * lda + n0 + cg * 4 : dZ, in && bok);
        }
    };
    // a lane's chunk of a transposing read: row (lane & 15) >> 2 of its group's four, columns 4 (lane & 3) ... + 3 of the fragment's sixteen
    const int trow = fk * 4 + (fr >> 2), tcol = (fr & 3) * 4;
    fetch(r_lo);
    for (int r0 = r_lo; r0 < r_hi; r0 += TK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sum_cols) colsum += ra[i];
            *reinterpret_cast<bf16x4*>(As + (rg + 8 * i) * TRP + cg * 4) = cvt4<bf16_t>(ra[i]);
            if (want_dw) *reinterpret_cast<bf16x4*>(Bs + (rg + 8 * i) * TRP + cg * 4) = cvt4<bf16_t>(rb[i]);
        }
        __syncthreads();
        if (r0 + TK < r_hi) fetch(r0 + TK);
        if (want_dw) {
            bf16x8 a[4], b[4];
            frag_tr4<TRP>(As + trow * TRP + wm * 64 + tcol, a);
            frag_tr4<TRP>(Bs + trow * TRP + wn * 64 + tcol, b);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    }
    if (sum_cols) {
        // the 8 threads of a column group: lanes l and l + 32 of each wave, then the waves in wave order through LDS
        float* red = reinterpret_cast<float*>(As);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) colsum[j] += __shfl_xor(colsum[j], 32, 64);
        if (lane < 32) *reinterpret_cast<f32x4*>(red + wave * TM + cg * 4) = colsum;
        __syncthreads();
        if (tid < TM && o0 + tid < O) pdb[(size_t)split * O + o0 + tid] = ((red[tid] + red[TM + tid]) + red[2 * TM + tid]) + red[3 * TM + tid];
    }
    if (!want_dw) return;
    float* P = part + (size_t)split * O * K;
    for_each_acc64(acc, o0 + wm * 64, n0 + wn * 64, O, K, fr, fk, [=](int o, int n, int, float x) { P[(size_t)o * K + n] = x; });
}

int launch_linear_bf16(const char* who, int epi, const LinArgs& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.M + TM - 1) / TM * p.n_tiles));
    if (epi == LIN_BIAS) hipLaunchKernelGGL(linear_fwd_bf16<LIN_BIAS>, grid, dim3(256), 0, s, p);
    else if (epi == LIN_BIAS_RES) hipLaunchKernelGGL(linear_fwd_bf16<LIN_BIAS_RES>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(linear_fwd_bf16<LIN_BIAS_GELU>, grid, dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

int launch_dgrad_bf16(const char* who, const float* dZ, int ldz, const float* W0, const float* W1, int O0, float* out, int ldo, int M, int O, int K, hipStream_t s) {
    const int n_tiles = (K + TN - 1) / TN;
    hipLaunchKernelGGL(dgrad_bf16, dim3((unsigned)((M + TM - 1) / TM * n_tiles)), dim3(256), 0, s, dZ, ldz, W0, W1 ? W1 : W0, W1 ? O0 : O, out, ldo, M, O, K, n_tiles);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

int launch_wgrad_parts_bf16(const float* dZ, int ldz, const float* A, int lda, int M, int O, int K, int rows_per_split, int S, int want_dw, float* part,
                            float* pdb, hipStream_t s) {
    const int o_tiles = (O + TM - 1) / TM, n_tiles = want_dw ? (K + TN - 1) / TN : 1;
    hipLaunchKernelGGL(wgrad_bf16, dim3((unsigned)(o_tiles * n_tiles * S)), dim3(256), 0, s, dZ, ldz, A, lda, M, O, K, rows_per_split, o_tiles, n_tiles, want_dw,
                       part, pdb);
    if (hipGetLastError() != hipSuccess) return fail("linear_wgrad: launch failed");
    return 0;
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_train_linear_mode(int mode) {
    return swap_thread_mode(g_train_linear_mode, mode, MUST3R_TRAIN_LINEAR_BF16,
                            "train_linear_mode: unknown mode %d (MUST3R_TRAIN_LINEAR_F32 = 0, MUST3R_TRAIN_LINEAR_BF16 = 1, -1 to query)");
}
