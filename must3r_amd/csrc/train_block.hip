// Training forward and backward of the two residual sublayers of the reference's Block (blocks/layers.py:36-54) in fp32, stateless:
//   attention sublayer   y = x + proj(attn(rope(qkv(LN(x)))))      (blocks/attention.py:92-99, RoPE2D on q and k :42-44)
//   MLP sublayer         y = x + fc2(gelu(fc1(LN(x))))             (croco Mlp, erf GELU)
// The forward saves nothing but its inputs; the backward recomputes the sublayer's forward into scratch and differentiates it with the plain operator
// forms of train_head.hip (linear_dgrad_f32, linear_wgrad_f32, layernorm_grad with the residual added) and the attention core of train_attention.hip.
// What the two backward passes share with each other and with the cross sublayer's (the shortcut for the last bias alone, the gradients at proj, the closing
// tail) is train_common.hpp's, as are the host helpers and the view-table check; what is written out here is a sublayer's own: RoPE and its transpose, GELU
// and its derivative.
//
//   linear_fwd_f32<EPI>   out[M, N] = A[M, K] W[N, K]^T + bias on v_mfma_f32_16x16x4_f32: the NT sibling of dgrad_kernel -- 128 x 128 tiles, 16-deep steps
//                         over K through LDS, 4 waves of 64 x 64, the next K-tile fetched into registers under the products of the current one.  Both
//                         operands are K-contiguous: both LDS tiles are [128][20] (rows padded to 20 floats: conflict-free).  Epilogues: bias; bias +
//                         residual; bias + GELU (gelu(z), and z itself where a second pointer is given).  In MUST3R_TRAIN_LINEAR_BF16 mode run_linear
//                         launches linear_fwd_bf16 of train_lin16.hip instead (same arguments and tiles; the epilogue itself is train_lin.hpp's, one copy for both).
//   ln_fwd_f32            y = (x - mu) rstd gamma + beta, one wave per row, 16-byte accesses, the row in registers; its own two-pass statistics (the
//                         formulas of row_stats_kernel in another summation order: the backward's statistics differ from these by rounding only).
//   gelu_grad_f32         dz = dh gelu'(z), 16-byte accesses, in place over dh.
//   rope_rows_f32         croco RoPE2D in place over the first rope_cols columns of [R][ld] rows; direction -1 is the transposed rotation (the backward).
// The GELU here is z Phi(z) with Phi(z) = erfc(-z / sqrt 2) / 2: the negative tail is a product, not the cancellation 1 + erf; its derivative is
// Phi(z) + z phi(z).  (gelu_erf of common.hpp is a fitted quartic for 16-bit outputs and has no matching derivative.)
// No atomics: every output element has one writer and a fixed order of operations; a row of any row-wise output does not depend on the other rows.
#include <algorithm>

#include "abi.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "train_common.hpp"
#include "train_lin.hpp"
#include "train_ln.hpp"
#include "train_tile.hpp"

namespace m3r {

constexpr int BM = 128, BN = 128, BK = 16, BP = 20;   // BP: LDS row stride (floats) of a [128][16] tile

// LinArgs, the epilogue (lin_epilogue) and gelu_cdf / gelu_f32: train_lin.hpp, shared with the bf16 form
// exp(-z^2 / 2) is 0 from |z| = 14.6 on (fp32 underflow), so that the derivative is exactly Phi there: 1 or 0 beyond |z| = 40
__device__ __forceinline__ float gelu_deriv_f32(float z) {
    const float pdf = 0.39894228040143267794f * expf(-0.5f * z * z);
    return pdf > 0.f ? fmaf(z, pdf, gelu_cdf(z)) : gelu_cdf(z);
}

// K % 16 == 0; tail rows of A and W are zero-filled on load, tail rows and columns of the tile are not stored
template <int EPI>
__global__ void __launch_bounds__(256) linear_fwd_f32(LinArgs p) {
    __shared__ __attribute__((aligned(16))) float As[BM * BP];
    __shared__ __attribute__((aligned(16))) float Bs[BN * BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int m0 = (blockIdx.x / p.n_tiles) * BM, n0 = (blockIdx.x % p.n_tiles) * BN;
    // staging: 128 rows x 16 floats of each operand, 512 float4 each, two per thread
    int sr[2], sc[2];
    const float* ap[2];
    const float* wp[2];
    bool aok[2], wok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = e * 256 + tid;
        sr[e] = idx >> 2; sc[e] = (idx & 3) * 4;
        aok[e] = m0 + sr[e] < p.M;
        wok[e] = n0 + sr[e] < p.N;
        ap[e] = p.A + (aok[e] ? (size_t)(m0 + sr[e]) * p.lda + sc[e] : 0);
        wp[e] = p.W + (wok[e] ? (size_t)(n0 + sr[e]) * p.K + sc[e] : 0);
    }
    f32x4 acc[4][4];
    zero_acc(acc);
    f32x4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ra[e] = aok[e] ? *reinterpret_cast<const f32x4*>(ap[e] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[e] = wok[e] ? *reinterpret_cast<const f32x4*>(wp[e] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < p.K; k0 += BK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            *reinterpret_cast<f32x4*>(As + sr[e] * BP + sc[e]) = ra[e];
            *reinterpret_cast<f32x4*>(Bs + sr[e] * BP + sc[e]) = rb[e];
        }
        __syncthreads();
        if (k0 + BK < p.K) fetch(k0 + BK);
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[(wm * 64 + i * 16 + fr) * BP + ks * 4 + fk];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[(wn * 64 + j * 16 + fr) * BP + ks * 4 + fk];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    lin_epilogue<EPI>(p, acc, m0 + wm * 64, n0 + wn * 64, lane);
}

// one wave per row, the row read once with 16-byte loads and kept in registers (D % 64 == 0, D <= 1024: four float4 per lane); two-pass statistics.
// The row routine is train_ln.hpp's, shared with the feedback kernels of train_decoder.hip.
__global__ void __launch_bounds__(256) ln_fwd_f32(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ y, int M, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    f32x4 v[4];
    float mu, rstd;
    ln_row_load(x + (size_t)row * D, lane, D, v);
    ln_row_stats(v, lane, D, eps, mu, rstd);
    ln_row_store(v, mu, rstd, gamma, beta, y + (size_t)row * D, lane, D);
}

// dz = dh gelu'(z) over [M][N], N % 4 == 0; dz may alias dh (each float4 is read before it is written, by the thread that writes it)
__global__ void __launch_bounds__(256) gelu_grad_f32(const float* dh, long long ldh, const float* __restrict__ z, long long ldz, float* dz, long long lddz,
                                                     int M, int N4) {
    const long long total = (long long)M * N4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / N4;
        const int c = (int)(i - r * N4) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dh + r * ldh + c);
        const f32x4 zz = *reinterpret_cast<const f32x4*>(z + r * ldz + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g[e] * gelu_deriv_f32(zz[e]);
        *reinterpret_cast<f32x4*>(dz + r * lddz + c) = o;
    }
}

// gelu(z) and gelu'(z) of a flat array (the activation alone, for its own test)
__global__ void __launch_bounds__(256) gelu_eval_f32(const float* __restrict__ z, float* __restrict__ g, float* __restrict__ dg, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (g) g[i] = gelu_f32(z[i]);
        if (dg) dg[i] = gelu_deriv_f32(z[i]);
    }
}

// One thread rotates the four pairs (c + e, c + 16 + e), e < 4, of one row: per head of 64 there are 8 such items, items 0..3 in the half that rotates with
// pos[r][0], items 4..7 in the half that rotates with pos[r][1].  tab [npos][16][2] (cos, sin); a position outside [0, npos) is clamped (the host refuses it).
__global__ void __launch_bounds__(256) rope_rows_f32(float* __restrict__ t, long long ld, const long long* __restrict__ pos, const float* __restrict__ tab,
                                                     int npos, long long R, int items_per_row, float dir) {
    const long long total = R * items_per_row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / items_per_row;
        const int w = (int)(i - r * items_per_row), head = w >> 3, half = (w >> 2) & 1, q4 = w & 3;
        long long pp = pos[r * 2 + half];
        pp = pp < 0 ? 0 : (pp >= npos ? npos - 1 : pp);
        const float* tb = tab + ((size_t)pp * 16 + q4 * 4) * 2;
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(tb), t1 = *reinterpret_cast<const f32x4*>(tb + 4);
        const float cs[4] = {t0[0], t0[2], t1[0], t1[2]};
        const float sn[4] = {t0[1] * dir, t0[3] * dir, t1[1] * dir, t1[3] * dir};
        float* pa = t + r * ld + head * 64 + half * 32 + q4 * 4;
        const f32x4 a = *reinterpret_cast<const f32x4*>(pa), b = *reinterpret_cast<const f32x4*>(pa + 16);
        f32x4 oa, ob;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            oa[e] = a[e] * cs[e] - b[e] * sn[e];
            ob[e] = b[e] * cs[e] + a[e] * sn[e];
        }
        *reinterpret_cast<f32x4*>(pa) = oa;
        *reinterpret_cast<f32x4*>(pa + 16) = ob;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------
static unsigned tb_grid(long long items) {
    const long long b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

static int run_linear(const char* who, int epi, const float* A, int lda, const float* W, const float* bias, const float* res, int ldres, float* out, int ldc,
                      float* zout, int ldz, int M, int N, int K, hipStream_t s) {
    if (M < 0 || N <= 0 || K <= 0) return fail("%s: bad shape", who);
    if (epi != LIN_BIAS && epi != LIN_BIAS_RES && epi != LIN_BIAS_GELU) return fail("%s: unknown epilogue", who);
    if (M == 0) return 0;
    if (!A || !W || !out || (epi == LIN_BIAS_RES && !res)) return fail("%s: null argument", who);
    if (K % 16 || N % 4) return fail("%s: K must be a multiple of 16 and N of 4", who);
    if (lda < K || lda % 4 || ldc < N || ldc % 4 || (epi == LIN_BIAS_RES && (ldres < N || ldres % 4)) || (epi == LIN_BIAS_GELU && zout && (ldz < N || ldz % 4)))
        return fail("%s: a leading dimension must cover its row and be a multiple of 4", who);
    if (misaligned(A) || misaligned(W) || misaligned(bias) || misaligned(out) || (epi == LIN_BIAS_RES && misaligned(res)) ||
        (epi == LIN_BIAS_GELU && misaligned(zout)))
        return fail("%s: tensors must be 16-byte aligned", who);
    const int n_tiles = (N + BN - 1) / BN;
    const long long blocks = (long long)((M + BM - 1) / BM) * n_tiles;
    if (blocks > 0x7fffffffLL) return fail("%s: too many rows", who);
    const LinArgs p{A, W, bias, res, out, epi == LIN_BIAS_GELU ? zout : nullptr, M, N, K, lda, ldc, ldres, ldz, n_tiles};
    if (train_linear_bf16()) return launch_linear_bf16(who, epi, p, s);   // must3r_hip_train_linear_mode: the same tiles on the 16-bit MFMA
    const dim3 grid((unsigned)blocks);
    if (epi == LIN_BIAS) hipLaunchKernelGGL(linear_fwd_f32<LIN_BIAS>, grid, dim3(256), 0, s, p);
    else if (epi == LIN_BIAS_RES) hipLaunchKernelGGL(linear_fwd_f32<LIN_BIAS_RES>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(linear_fwd_f32<LIN_BIAS_GELU>, grid, dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

static int run_ln(const char* who, const float* x, const float* gamma, const float* beta, float* y, int M, int D, float eps, hipStream_t s) {
    hipLaunchKernelGGL(ln_fwd_f32, dim3((M + 3) / 4), dim3(256), 0, s, x, gamma, beta, y, M, D, eps);
    if (hipGetLastError() != hipSuccess) return fail("%s: the LayerNorm launch failed", who);
    return 0;
}

static int run_rope(const char* who, float* t, int ld, const int64_t* pos, const float* tab, int npos, int R, int rope_cols, int direction, hipStream_t s) {
    if (R < 0 || rope_cols < 0 || rope_cols % 64) return fail("%s: rope_cols must be a non-negative multiple of 64", who);
    if (direction != 1 && direction != -1) return fail("%s: direction must be +1 or -1", who);
    if (R == 0 || rope_cols == 0) return 0;
    if (!t || !pos || !tab) return fail("%s: null argument", who);
    if (npos <= 0) return fail("%s: the table needs at least one position", who);
    if (ld < rope_cols || ld % 4) return fail("%s: the leading dimension must cover rope_cols and be a multiple of 4", who);
    if (misaligned(t) || misaligned(pos) || misaligned(tab)) return fail("%s: tensors must be 16-byte aligned", who);
    const int items = rope_cols / 8;
    hipLaunchKernelGGL(rope_rows_f32, dim3(tb_grid((long long)R * items)), dim3(256), 0, s, t, (long long)ld, reinterpret_cast<const long long*>(pos), tab, npos,
                       (long long)R, items, (float)direction);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

static int run_gelu_grad(const char* who, const float* dh, int ldh, const float* z, int ldz, float* dz, int lddz, int M, int N, hipStream_t s) {
    if (M < 0 || N <= 0 || N % 4) return fail("%s: N must be a positive multiple of 4", who);
    if (M == 0) return 0;
    if (!dh || !z || !dz) return fail("%s: null argument", who);
    if (ldh < N || ldh % 4 || ldz < N || ldz % 4 || lddz < N || lddz % 4) return fail("%s: a leading dimension must cover its row and be a multiple of 4", who);
    if (misaligned(dh) || misaligned(z) || misaligned(dz)) return fail("%s: tensors must be 16-byte aligned", who);
    hipLaunchKernelGGL(gelu_grad_f32, dim3(tb_grid((long long)M * (N / 4))), dim3(256), 0, s, dh, (long long)ldh, z, (long long)ldz, dz, (long long)lddz, M, N / 4);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

// MLP scratch: [y M D | S1 M hidden | S2 M hidden | weight-gradient partials | LayerNorm backward]
struct MlpLayout { size_t y, s1, s2, wg, wg_bytes, ln, ln_bytes, total; };
static MlpLayout mlp_layout(int M, int D, int hidden) {
    MlpLayout L{};
    ScratchCursor c;
    L.y = c.take((size_t)M * D * 4);
    L.s1 = c.take((size_t)M * hidden * 4);
    L.s2 = c.take((size_t)M * hidden * 4);
    L.wg_bytes = std::max(must3r_hip_op_linear_wgrad_scratch_bytes(M, D, hidden), must3r_hip_op_linear_wgrad_scratch_bytes(M, hidden, D));
    L.wg = c.take(L.wg_bytes);
    L.ln_bytes = must3r_hip_op_layernorm_grad_scratch_bytes(M, D);
    L.ln = c.take(L.ln_bytes);
    L.total = c.off;
    return L;
}

// attention scratch: [y M D | qkv M 3D | o M D | dO M D | dqkv M 3D | weight-gradient partials | LayerNorm backward | attention core]
struct AttnLayout { size_t y, qkv, o, dO, dqkv, wg, wg_bytes, ln, ln_bytes, core, core_bytes, total; };
static AttnLayout attn_layout(int M, int D, int n_views) {
    AttnLayout L{};
    ScratchCursor c;
    L.y = c.take((size_t)M * D * 4);
    L.qkv = c.take((size_t)M * 3 * D * 4);
    L.o = c.take((size_t)M * D * 4);
    L.dO = c.take((size_t)M * D * 4);
    L.dqkv = c.take((size_t)M * 3 * D * 4);
    L.wg_bytes = std::max(must3r_hip_op_linear_wgrad_scratch_bytes(M, 3 * D, D), must3r_hip_op_linear_wgrad_scratch_bytes(M, D, D));
    L.wg = c.take(L.wg_bytes);
    L.ln_bytes = must3r_hip_op_layernorm_grad_scratch_bytes(M, D);
    L.ln = c.take(L.ln_bytes);
    L.core_bytes = must3r_hip_attn_train_scratch_bytes(n_views, M, M, D / 64);
    L.core = c.take(L.core_bytes);
    L.total = c.off;
    return L;
}

static const char* mlp_args_error(const must3r_hip_mlp_sublayer_args* a, bool grad) {
    if (const char* e = rows_width_error(a->M, a->D)) return e;
    if (a->hidden <= 0 || a->hidden % 16) return "hidden must be a positive multiple of 16";
    if (!a->x || !a->gamma || !a->beta || !a->W1 || !a->W2) return "null argument (x, gamma, beta, W1, W2)";
    if (grad ? !a->dy : !a->out) return grad ? "null argument (dy)" : "null argument (out)";
    if (misaligned(a->x) || misaligned(a->gamma) || misaligned(a->beta) || misaligned(a->W1) || misaligned(a->W2) || misaligned(a->b1) || misaligned(a->b2) || misaligned(a->dy) ||
        misaligned(a->out) || misaligned(a->dx) || misaligned(a->dW1) || misaligned(a->dW2))
        return "tensors must be 16-byte aligned";
    return nullptr;
}

// *covered: every row is a query row of a view and a key row of a group (nothing to zero)
static const char* attn_args_error(const must3r_hip_attn_sublayer_args* a, bool grad, bool* covered) {
    if (const char* e = rows_width_error(a->M, a->D)) return e;
    if (!a->x || !a->gamma || !a->beta || !a->Wqkv || !a->Wproj) return "null argument (x, gamma, beta, Wqkv, Wproj)";
    if (!a->pos || !a->rope_tab) return "null argument (pos, rope_tab)";
    if (a->rope_npos <= 0) return "the RoPE table needs at least one position";
    if (grad ? !a->dy : !a->out) return grad ? "null argument (dy)" : "null argument (out)";
    if (misaligned(a->x) || misaligned(a->gamma) || misaligned(a->beta) || misaligned(a->Wqkv) || misaligned(a->Wproj) || misaligned(a->bqkv) || misaligned(a->bproj) || misaligned(a->dy) ||
        misaligned(a->out) || misaligned(a->dx) || misaligned(a->dWqkv) || misaligned(a->dWproj) || misaligned(a->pos) || misaligned(a->rope_tab))
        return "tensors must be 16-byte aligned";
    bool q_covered = false, kv_covered = false;
    const char* e = view_table_error(a->views, a->n_views, a->M, a->M, &q_covered, &kv_covered);
    *covered = q_covered && kv_covered;
    return e;
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_op_linear_f32(int epi, const float* A, int lda, const float* W, const float* bias, const float* res, int ldres, float* out, int ldc,
                                        float* zout, int ldz, int M, int N, int K, void* stream) {
    return run_linear("op_linear_f32", epi, A, lda, W, bias, res, ldres, out, ldc, zout, ldz, M, N, K, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int must3r_hip_op_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int M, int D, float eps, void* stream) {
    if (M <= 0 || D <= 0 || D % 64 || D > 1024) return fail("op_layernorm_f32: M must be positive, D a multiple of 64 and at most 1024");
    if (!x || !gamma || !beta || !y) return fail("op_layernorm_f32: null argument");
    if (misaligned(x) || misaligned(gamma) || misaligned(beta) || misaligned(y)) return fail("op_layernorm_f32: tensors must be 16-byte aligned");
    return run_ln("op_layernorm_f32", x, gamma, beta, y, M, D, eps, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int must3r_hip_op_gelu_f32(const float* z, float* g, float* dg, long long n, void* stream) {
    if (n < 0) return fail("op_gelu_f32: bad size");
    if (n == 0 || (!g && !dg)) return 0;
    if (!z) return fail("op_gelu_f32: null argument");
    hipLaunchKernelGGL(gelu_eval_f32, dim3(tb_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, g, dg, n);
    if (hipGetLastError() != hipSuccess) return fail("op_gelu_f32: launch failed");
    return 0;
}

extern "C" int must3r_hip_op_gelu_grad_f32(const float* dh, int ldh, const float* z, int ldz, float* dz, int lddz, int M, int N, void* stream) {
    return run_gelu_grad("op_gelu_grad_f32", dh, ldh, z, ldz, dz, lddz, M, N, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int must3r_hip_op_rope_f32(float* t, int ld, const int64_t* pos, const float* rope_tab, int rope_npos, int R, int rope_cols, int direction,
                                      void* stream) {
    return run_rope("op_rope_f32", t, ld, pos, rope_tab, rope_npos, R, rope_cols, direction, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t must3r_hip_mlp_sublayer_scratch_bytes(int M, int D, int hidden) {
    if (rows_width_error(M, D) || hidden <= 0 || hidden % 16) return 0;
    return mlp_layout(M, D, hidden).total;
}

extern "C" size_t must3r_hip_attn_sublayer_scratch_bytes(int M, int D, int n_views) {
    if (rows_width_error(M, D) || n_views <= 0 || n_views > 65535) return 0;
    return attn_layout(M, D, n_views).total;
}

// Inside the sublayer entry points the stream is `s`, a hipStream_t: the run_* launchers take it as it is, the must3r_hip_op_* calls as their void*.

extern "C" int must3r_hip_mlp_sublayer_forward(const must3r_hip_mlp_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "mlp_sublayer_forward";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = mlp_args_error(a, false)) return fail("%s: %s", who, e);
    const int M = a->M, D = a->D, Hd = a->hidden;
    const MlpLayout L = mlp_layout(M, D, Hd);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* p = reinterpret_cast<char*>(scratch);
    float* y = reinterpret_cast<float*>(p + L.y);
    float* h = reinterpret_cast<float*>(p + L.s2);
    M3R_RUN(run_ln(who, a->x, a->gamma, a->beta, y, M, D, a->eps, s));
    M3R_RUN(run_linear(who, LIN_BIAS_GELU, y, D, a->W1, a->b1, nullptr, 0, h, Hd, nullptr, 0, M, Hd, D, s));
    return run_linear(who, LIN_BIAS_RES, h, Hd, a->W2, a->b2, a->x, D, a->out, D, nullptr, 0, M, D, Hd, s);
}

extern "C" int must3r_hip_mlp_sublayer_grad(const must3r_hip_mlp_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "mlp_sublayer_grad";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = mlp_args_error(a, true)) return fail("%s: %s", who, e);
    const int M = a->M, D = a->D, Hd = a->hidden;
    const MlpLayout L = mlp_layout(M, D, Hd);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    const bool want_dz = a->dW1 || a->db1 || a->dx || a->dgamma || a->dbeta;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* p = reinterpret_cast<char*>(scratch);
    float* y = reinterpret_cast<float*>(p + L.y);
    float* s1 = reinterpret_cast<float*>(p + L.s1);
    float* s2 = reinterpret_cast<float*>(p + L.s2);
    M3R_RUN(last_bias_alone(a, L, p, a->dW2, a->db2, Hd, s));
    if (!a->dW2 && !want_dz) return 0;
    // the forward once more: y = LN(x), z = fc1(y) -> S1 (only the activation's derivative reads it), h = gelu(z) -> S2 (only dW2 reads it)
    M3R_RUN(run_ln(who, a->x, a->gamma, a->beta, y, M, D, a->eps, s));
    M3R_RUN(run_linear(who, LIN_BIAS_GELU, y, D, a->W1, a->b1, nullptr, 0, s2, Hd, want_dz ? s1 : nullptr, Hd, M, Hd, D, s));
    if (a->dW2) M3R_RUN(must3r_hip_op_linear_wgrad_f32(a->dy, D, s2, Hd, a->dW2, a->db2, M, D, Hd, p + L.wg, L.wg_bytes, s));
    if (!want_dz) return 0;
    M3R_RUN(must3r_hip_op_linear_dgrad_f32(a->dy, D, a->W2, s2, M, D, Hd, s));                      // dh over h
    M3R_RUN(run_gelu_grad(who, s2, Hd, s1, Hd, s2, Hd, M, Hd, s));                                  // dz over dh
    return sublayer_grad_tail(a, L, p, s2, Hd, a->W1, Hd, a->dW1, a->db1, y, s);
}

// y = LN(x) -> qkv = y Wqkv^T + b, rotated on its first 2 D columns -> o = attention(q, k, v)
static int attn_recompute(const char* who, const must3r_hip_attn_sublayer_args* a, const AttnLayout& L, char* p, bool covered, hipStream_t s) {
    const int M = a->M, D = a->D;
    float* y = reinterpret_cast<float*>(p + L.y);
    float* qkv = reinterpret_cast<float*>(p + L.qkv);
    M3R_RUN(run_ln(who, a->x, a->gamma, a->beta, y, M, D, a->eps, s));
    M3R_RUN(run_linear(who, LIN_BIAS, y, D, a->Wqkv, a->bqkv, nullptr, 0, qkv, 3 * D, nullptr, 0, M, 3 * D, D, s));
    M3R_RUN(run_rope(who, qkv, 3 * D, a->pos, a->rope_tab, a->rope_npos, M, 2 * D, 1, s));
    return sublayer_attend(who, a, L, p, core_args(a, qkv, 3 * D, qkv + D, qkv + 2 * D, 3 * D), reinterpret_cast<float*>(p + L.o), covered, s);
}

extern "C" int must3r_hip_attn_sublayer_forward(const must3r_hip_attn_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "attn_sublayer_forward";
    if (!a) return fail("%s: null argument", who);
    bool covered = false;
    if (const char* e = attn_args_error(a, false, &covered)) return fail("%s: %s", who, e);
    const AttnLayout L = attn_layout(a->M, a->D, a->n_views);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* p = reinterpret_cast<char*>(scratch);
    M3R_RUN(attn_recompute(who, a, L, p, covered, s));
    const int M = a->M, D = a->D;
    return run_linear(who, LIN_BIAS_RES, reinterpret_cast<float*>(p + L.o), D, a->Wproj, a->bproj, a->x, D, a->out, D, nullptr, 0, M, D, D, s);
}

extern "C" int must3r_hip_attn_sublayer_grad(const must3r_hip_attn_sublayer_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "attn_sublayer_grad";
    if (!a) return fail("%s: null argument", who);
    bool covered = false;
    if (const char* e = attn_args_error(a, true, &covered)) return fail("%s: %s", who, e);
    const int M = a->M, D = a->D;
    if (must3r_hip_attn_train_groups(a->views, a->n_views) < 0) return 1;   // overlapping key groups: the error text is the core's
    const AttnLayout L = attn_layout(M, D, a->n_views);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    const bool want_dqkv = a->dWqkv || a->dbqkv || a->dx || a->dgamma || a->dbeta;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* p = reinterpret_cast<char*>(scratch);
    float* y = reinterpret_cast<float*>(p + L.y);
    float* qkv = reinterpret_cast<float*>(p + L.qkv);
    float* dO = reinterpret_cast<float*>(p + L.dO);
    float* dqkv = reinterpret_cast<float*>(p + L.dqkv);
    M3R_RUN(last_bias_alone(a, L, p, a->dWproj, a->dbproj, D, s));
    if (!a->dWproj && !want_dqkv) return 0;
    M3R_RUN(attn_recompute(who, a, L, p, covered, s));
    M3R_RUN(proj_grad(a, L, p, reinterpret_cast<float*>(p + L.o), want_dqkv ? dO : nullptr, s));
    if (!want_dqkv) return 0;
    if (!covered && hipMemsetAsync(dqkv, 0, (size_t)M * 3 * D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
    must3r_hip_attn_train_args t = core_args(a, qkv, 3 * D, qkv + D, qkv + 2 * D, 3 * D);
    t.dO = dO; t.lddo = D;
    t.dQ = dqkv; t.dK = dqkv + D; t.dV = dqkv + 2 * D;
    t.lddq = t.lddk = t.lddv = 3 * D;
    M3R_RUN(must3r_hip_attn_grad(&t, p + L.core, L.core_bytes, s));
    M3R_RUN(run_rope(who, dqkv, 3 * D, a->pos, a->rope_tab, a->rope_npos, M, 2 * D, -1, s));
    return sublayer_grad_tail(a, L, p, dqkv, 3 * D, a->Wqkv, 3 * D, a->dWqkv, a->dbqkv, y, s);
}
