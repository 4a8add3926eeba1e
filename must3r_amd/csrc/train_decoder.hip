// Training forward and backward of what the reference's decoder does to the new tokens of ALL layers after a memory update (feedback_mechanism.py:39-53,
// decoder.py:325-330): the feedback offset is added to the tokens of every layer but the last, and each layer's norm_y is applied -- one launch each way
// instead of L - 1 adds and L LayerNorms (and as many backward launches plus L - 1 gradient adds):
//   Y_l = LN_l(X_l + (l < add_layers ? offset : 0))          l = 0 .. L - 1, X_l [R][D] fp32 contiguous, offset [R][D] or NULL
// with every gamma / beta NULL the `raw` memory mode: the add alone.  The backward gives dX_l, doffset = sum over l < add_layers of dX_l (ascending l),
// dgamma_l and dbeta_l.
//
//   feedback_fwd_f32      one wave owns a row and walks the layers with the offset's row in registers (four float4 per lane, the layout of ln_fwd_f32); the
//                         row routine is train_ln.hpp's, ln_fwd_f32's own: a layer without the add has the bits of must3r_hip_op_layernorm_f32.
//   feedback_grad_f32     a block owns 16 rows, four per wave; it walks the layers, and inside a layer its rows.  Across the layers a wave keeps the running
//                         doffset of its four rows in registers; across its rows it keeps the layer's column sums of dY x^ and dY, which the block adds in
//                         wave order and writes as one partial per (layer, block).  The statistics are the forward's (ln_row_stats on X_l + offset).
//   feedback_reduce_f32   dgamma_l, dbeta_l from the partials in a fixed two-level order (16 interleaved slices, then the slices), as ln_grad_reduce_kernel.
// The block count is a function of R alone.  No atomics, one writer per element; a row's Y, dX and doffset do not depend on the other rows.  Every output
// is optional: a NULL Y_l / dX_l is not written, without doffset nothing is accumulated, and with no dgamma_l and dbeta_l at all there are no column sums.
#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "common.hpp"
#include "train_common.hpp"
#include "train_ln.hpp"

namespace m3r {

constexpr int FB_MAX_L = MUST3R_FEEDBACK_MAX_LAYERS, FB_ROWS = 16, FB_RPW = FB_ROWS / 4;

struct FbFwd {
    const float* x[FB_MAX_L]; const float* gamma[FB_MAX_L]; const float* beta[FB_MAX_L]; float* y[FB_MAX_L];
    const float* offset;
    int L, R, D, add_layers;
    float eps;
};

struct FbGrad {
    const float* x[FB_MAX_L]; const float* gamma[FB_MAX_L]; const float* dy[FB_MAX_L]; float* dx[FB_MAX_L];
    const float* offset;
    float* doffset;
    float* part;   // [L][blocks][2][D], or NULL: no column sums
    int L, R, D, add_layers;
    float eps;
};

struct FbReduce {
    float* dgamma[FB_MAX_L]; float* dbeta[FB_MAX_L];
    const float* part;
    int NB, D;
};

__global__ void __launch_bounds__(256) feedback_fwd_f32(FbFwd p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, D = p.D;
    if (row >= p.R) return;
    const size_t o = (size_t)row * D;
    f32x4 off[4];
    if (p.add_layers > 0) ln_row_load(p.offset + o, lane, D, off);
    for (int l = 0; l < p.L; ++l) {
        if (!p.y[l]) continue;
        f32x4 v[4];
        ln_row_load(p.x[l] + o, lane, D, v);
        if (l < p.add_layers) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += off[j];
        }
        if (p.gamma[l]) {
            float mu, rstd;
            ln_row_stats(v, lane, D, p.eps, mu, rstd);
            ln_row_store(v, mu, rstd, p.gamma[l], p.beta[l], p.y[l] + o, lane, D);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((j * 64 + lane) * 4 < D) *reinterpret_cast<f32x4*>(p.y[l] + o + (j * 64 + lane) * 4) = v[j];
        }
    }
}

__global__ void __launch_bounds__(256) feedback_grad_f32(FbGrad p) {
    __shared__ __attribute__((aligned(16))) float red[3 * 2 * 1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.D;
    const int r0 = blockIdx.x * FB_ROWS + wave;   // this wave's rows: r0 + 4 i
    const bool want_off = p.doffset != nullptr;
    f32x4 doff[FB_RPW][4];
#pragma unroll
    for (int i = 0; i < FB_RPW; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) doff[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < p.L; ++l) {
        const bool add = l < p.add_layers, norm = p.gamma[l] != nullptr, cols = norm && p.part != nullptr;
        const float* dyl = p.dy[l];
        float* dxl = p.dx[l];
        if (!cols && !dxl && !(add && want_off)) continue;   // uniform over the block: no barrier is skipped by a part of it
        f32x4 g[4], ag[4], ab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (j * 64 + lane) * 4;
            g[j] = norm && c < D ? *reinterpret_cast<const f32x4*>(p.gamma[l] + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            ag[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            ab[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < FB_RPW; ++i) {
            const int row = r0 + 4 * i;
            if (row >= p.R) continue;
            const size_t o = (size_t)row * D;
            f32x4 d[4];
            ln_row_load(dyl + o, lane, D, d);
            if (norm) {
                f32x4 v[4];
                ln_row_load(p.x[l] + o, lane, D, v);
                if (add) {
                    f32x4 off[4];
                    ln_row_load(p.offset + o, lane, D, off);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += off[j];
                }
                float mu, rstd;
                ln_row_stats(v, lane, D, p.eps, mu, rstd);
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = (v[j] - mu) * rstd;           // x^ (zero columns beyond D stay out of the sums: d and g are zero there)
                    const f32x4 gh = d[j] * g[j];
                    s1 += (gh[0] + gh[1]) + (gh[2] + gh[3]);
                    const f32x4 gx = gh * v[j];
                    s2 += (gx[0] + gx[1]) + (gx[2] + gx[3]);
                    ag[j] += d[j] * v[j];
                    ab[j] += d[j];
                }
                const float m1 = wave_sum_dpp(s1) / (float)D, m2 = wave_sum_dpp(s2) / (float)D;
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = rstd * (d[j] * g[j] - m1 - v[j] * m2);   // dX_l over dY_l
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (j * 64 + lane) * 4;
                if (c >= D) continue;
                if (dxl) *reinterpret_cast<f32x4*>(dxl + o + c) = d[j];
                if (add) doff[i][j] += d[j];
            }
        }
        if (!cols) continue;
        // waves 1..3 -> LDS, wave 0 adds them in wave order: one partial per (layer, block)
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                *reinterpret_cast<f32x4*>(red + ((wave - 1) * 2 + 0) * 1024 + (j * 64 + lane) * 4) = ag[j];
                *reinterpret_cast<f32x4*>(red + ((wave - 1) * 2 + 1) * 1024 + (j * 64 + lane) * 4) = ab[j];
            }
        }
        __syncthreads();
        if (wave == 0) {
            float* pa = p.part + ((size_t)l * gridDim.x + blockIdx.x) * 2 * D;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (j * 64 + lane) * 4;
                if (c >= D) continue;
                f32x4 a = ag[j], b = ab[j];
                for (int w = 0; w < 3; ++w) {
                    a += *reinterpret_cast<const f32x4*>(red + (w * 2 + 0) * 1024 + c);
                    b += *reinterpret_cast<const f32x4*>(red + (w * 2 + 1) * 1024 + c);
                }
                *reinterpret_cast<f32x4*>(pa + c) = a;
                *reinterpret_cast<f32x4*>(pa + D + c) = b;
            }
        }
        __syncthreads();
    }
    if (!want_off) return;
#pragma unroll
    for (int i = 0; i < FB_RPW; ++i) {
        const int row = r0 + 4 * i;
        if (row >= p.R) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (j * 64 + lane) * 4;
            if (c < D) *reinterpret_cast<f32x4*>(p.doffset + (size_t)row * D + c) = doff[i][j];
        }
    }
}

// blockIdx.y: the layer; 16 columns per block; slice q of 16 adds the partials of blocks q, q + 16, ... in that order, then one thread per column the slices
__global__ void __launch_bounds__(256) feedback_reduce_f32(FbReduce p) {
    __shared__ float ra[16][17], rb[16][17];
    const int l = blockIdx.y;
    if (!p.dgamma[l] && !p.dbeta[l]) return;
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4, k = blockIdx.x * 16 + c, D = p.D;
    const float* part = p.part + (size_t)l * p.NB * 2 * D;
    float a = 0.f, b = 0.f;
    for (int i = q; i < p.NB; i += 16) {
        a += part[((size_t)i * 2 + 0) * D + k];
        b += part[((size_t)i * 2 + 1) * D + k];
    }
    ra[q][c] = a; rb[q][c] = b;
    __syncthreads();
    if (q != 0) return;
    a = ra[0][c]; b = rb[0][c];
    for (int j = 1; j < 16; ++j) { a += ra[j][c]; b += rb[j][c]; }
    if (p.dgamma[l]) p.dgamma[l][k] = a;
    if (p.dbeta[l]) p.dbeta[l][k] = b;
}

static int fb_blocks(int R) { return (R + FB_ROWS - 1) / FB_ROWS; }

static const char* fb_shape_error(int L, int R, int D) {
    if (L < 1 || L > FB_MAX_L) return "L must be in [1, 32]";
    if (R <= 0) return "R must be positive";
    if (D <= 0 || D % 64) return "D must be a positive multiple of 64";
    if (D > 1024) return "D must not exceed 1024";
    if (R > 0x7fffffff / 4) return "too many rows";
    return nullptr;
}

static size_t fb_scratch(int L, int R, int D) { return up256((size_t)L * fb_blocks(R) * 2 * D * 4); }

// nullptr, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed
static const char* fb_args_error(const must3r_hip_feedback_prepare_args* a, bool grad) {
    if (const char* e = fb_shape_error(a->L, a->R, a->D)) return e;
    if (a->add_layers < 0 || a->add_layers > a->L) return "add_layers must be in [0, L]";
    if (a->add_layers > 0 && !a->offset) return "null argument (offset, with add_layers > 0)";
    if (misaligned(a->offset) || misaligned(a->doffset)) return "tensors must be 16-byte aligned";
    int norms = 0;
    for (int l = 0; l < a->L; ++l) {
        if (!a->gamma[l] != !a->beta[l]) return "gamma and beta of a layer come together";
        norms += a->gamma[l] ? 1 : 0;
        if (!a->x[l]) return "null argument (x)";
        if (grad && !a->dy[l]) return "null argument (dy)";
        if (!a->gamma[l] && (a->dgamma[l] || a->dbeta[l])) return "dgamma and dbeta need gamma and beta";
        const void* ptrs[] = {a->x[l], a->gamma[l], a->beta[l], a->dy[l], a->y[l], a->dx[l], a->dgamma[l], a->dbeta[l]};
        for (const void* q : ptrs)
            if (misaligned(q)) return "tensors must be 16-byte aligned";
    }
    if (norms != 0 && norms != a->L) return "gamma and beta are given for every layer or for none (the raw mode)";
    return nullptr;
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_feedback_prepare_scratch_bytes(int L, int R, int D) {
    if (const char* e = fb_shape_error(L, R, D)) {
        fail("feedback_prepare_scratch_bytes: %s", e);
        return 0;
    }
    return fb_scratch(L, R, D);
}

extern "C" int must3r_hip_feedback_prepare_forward(const must3r_hip_feedback_prepare_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "feedback_prepare_forward";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = fb_args_error(a, false)) return fail("%s: %s", who, e);
    (void)scratch; (void)scratch_bytes;   // the forward needs none: the parameters are there so that both entry points are called alike
    FbFwd p{};
    bool any = false;
    for (int l = 0; l < a->L; ++l) {
        p.x[l] = a->x[l]; p.gamma[l] = a->gamma[l]; p.beta[l] = a->beta[l]; p.y[l] = a->y[l];
        any = any || a->y[l];
    }
    if (!any) return 0;
    p.offset = a->offset; p.L = a->L; p.R = a->R; p.D = a->D; p.add_layers = a->add_layers; p.eps = a->eps;
    hipLaunchKernelGGL(feedback_fwd_f32, dim3((a->R + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(a->stream), p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

extern "C" int must3r_hip_feedback_prepare_grad(const must3r_hip_feedback_prepare_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "feedback_prepare_grad";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = fb_args_error(a, true)) return fail("%s: %s", who, e);
    bool cols = false;
    for (int l = 0; l < a->L; ++l) cols = cols || a->dgamma[l] || a->dbeta[l];
    // the scratch holds the column-sum partials: without a dgamma or dbeta none is needed, and neither argument is read
    if (cols && (!scratch || misaligned(scratch) || scratch_bytes < fb_scratch(a->L, a->R, a->D))) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    FbGrad p{};
    FbReduce r{};
    bool any = a->doffset && a->add_layers > 0;
    for (int l = 0; l < a->L; ++l) {
        p.x[l] = a->x[l]; p.gamma[l] = a->gamma[l]; p.dy[l] = a->dy[l]; p.dx[l] = a->dx[l];
        r.dgamma[l] = a->dgamma[l]; r.dbeta[l] = a->dbeta[l];
        any = any || a->dx[l];
    }
    if (a->doffset && a->add_layers == 0 && hipMemsetAsync(a->doffset, 0, (size_t)a->R * a->D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
    if (!any && !cols) return 0;
    const int NB = fb_blocks(a->R);
    p.offset = a->offset; p.doffset = a->add_layers > 0 ? a->doffset : nullptr;
    p.part = cols ? reinterpret_cast<float*>(scratch) : nullptr;
    p.L = a->L; p.R = a->R; p.D = a->D; p.add_layers = a->add_layers; p.eps = a->eps;
    hipLaunchKernelGGL(feedback_grad_f32, dim3(NB), dim3(256), 0, s, p);
    if (cols) {
        r.part = p.part; r.NB = NB; r.D = a->D;
        hipLaunchKernelGGL(feedback_reduce_f32, dim3(a->D / 16, a->L), dim3(256), 0, s, r);
    }
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}
