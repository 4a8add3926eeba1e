// Training forward and backward of the third residual sublayer of the reference's CachedDecoderBlock (blocks/layers.py:90-99, CachedCrossAttention
// blocks/attention.py:129-149): the cross attention of the tokens x over the token memory, fp32, stateless:
//   out = x + proj(attn(projq(LN(x)), projk(mem), projv(mem)))         no RoPE (the reference builds cross_attn with pos_embed=None)
// or, in the reference's `kv` memory mode, over a memory that already holds k | v.  Queries and keys are rows of different tensors, several views of a scene
// read the same key rows (the key groups of train_attention.hip), and the gradient also arrives at the memory.  This file has no kernel of its own: it
// composes the operator forms of train_block.hip (LayerNorm, the NT Linear) and train_head.hip (the data and weight gradients of a Linear, the LayerNorm
// backward with the residual added), the attention core of train_attention.hip, and the two-segment data gradient of train_head.hip
// (launch_dgrad_seg_f32: dmem = dK Wk + dV Wv in one launch and one accumulator chain per element).  The forward saves nothing; the backward recomputes the
// forward into scratch and differentiates it.  All work goes to the stream of the descriptor.  No atomics.
#include <algorithm>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "kernels.hpp"

namespace m3r {

#define M3R_RUN(expr)                 \
    do {                              \
        int rc__ = (expr);            \
        if (rc__) return rc__;        \
    } while (0)

static size_t tc_up256(size_t v) { return (v + 255) / 256 * 256; }
static bool tc_misaligned(const void* p) { return ((size_t)p & 15) != 0; }

static const char* tc_shape_error(int M, int Rm, int D) {
    if (M <= 0) return "M must be positive";
    if (Rm <= 0) return "Rm must be positive";
    if (D <= 0 || D % 64) return "D must be a positive multiple of 64";
    if (D > 1024) return "D must not exceed 1024";
    if (M > 0x7fffffff / 4 || Rm > 0x7fffffff / 4) return "too many rows";
    return nullptr;
}

// [y^ M D | q M D | k|v Rm 2D | o M D | do M D | dq M D | dk|dv Rm 2D | weight-gradient partials | LayerNorm backward | attention core]; kv_ready: no Rm x 2 D parts
struct CrossLayout { size_t y, q, kv, o, dO, dq, dkv, wg, wg_bytes, ln, ln_bytes, core, core_bytes, total; };
static CrossLayout cross_layout(int M, int Rm, int D, int n_views, bool kv_ready) {
    CrossLayout L{};
    size_t o = 0;
    const size_t md = tc_up256((size_t)M * D * 4), rd = kv_ready ? 0 : tc_up256((size_t)Rm * 2 * D * 4);
    L.y = o; o += md;
    L.q = o; o += md;
    L.kv = o; o += rd;
    L.o = o; o += md;
    L.dO = o; o += md;
    L.dq = o; o += md;
    L.dkv = o; o += rd;
    L.wg_bytes = must3r_hip_op_linear_wgrad_scratch_bytes(M, D, D);
    if (!kv_ready) L.wg_bytes = std::max(L.wg_bytes, must3r_hip_op_linear_wgrad_scratch_bytes(Rm, D, D));
    L.wg = o; o += tc_up256(L.wg_bytes);
    L.ln_bytes = must3r_hip_op_layernorm_grad_scratch_bytes(M, D);
    L.ln = o; o += tc_up256(L.ln_bytes);
    L.core_bytes = must3r_hip_attn_train_scratch_bytes(n_views, M, Rm, D / 64);
    L.core = o; o += tc_up256(L.core_bytes);
    L.total = o;
    return L;
}

static bool tc_spans_cover(std::vector<std::pair<long long, long long>> spans, long long rows) {
    std::sort(spans.begin(), spans.end());
    long long end = 0;
    for (const auto& sp : spans) {
        if (sp.second <= sp.first) continue;
        if (sp.first > end) return false;
        end = std::max(end, sp.second);
    }
    return end >= rows;
}

// nullptr, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed.
// *q_covered: every row of x is a query row of a view; *kv_covered: every row of mem lies inside a key group's span (nothing to zero).
static const char* cross_args_error(const must3r_hip_cross_sublayer_args* a, bool grad, bool* q_covered, bool* kv_covered) {
    if (const char* e = tc_shape_error(a->M, a->Rm, a->D)) return e;
    if (!a->x || !a->mem || !a->gamma || !a->beta || !a->Wq || !a->Wproj) return "null argument (x, mem, gamma, beta, Wq, Wproj)";
    if (grad ? !a->dy : !a->out) return grad ? "null argument (dy)" : "null argument (out)";
    if (!a->Wk != !a->Wv) return "Wk and Wv come together: both for a memory of tokens, neither for a memory that holds k | v";
    const bool kv_ready = !a->Wk;
    if (kv_ready && (a->bk || a->bv || a->dWk || a->dbk || a->dWv || a->dbv)) return "bk, bv and the gradients of Wk, bk, Wv, bv need Wk and Wv";
    const int D = a->D, need = kv_ready ? 2 * D : D;
    if (a->ldmem < need || a->ldmem % 4) return "the leading dimension of mem must cover its row (D, or 2 D for k | v) and be a multiple of 4";
    if (a->dmem && (a->lddmem < need || a->lddmem % 4)) return "the leading dimension of dmem must cover its row (D, or 2 D for k | v) and be a multiple of 4";
    const void* ptrs[] = {a->x, a->mem, a->gamma, a->beta, a->Wq, a->bq, a->Wk, a->bk, a->Wv, a->bv, a->Wproj, a->bproj, a->dy, a->out, a->dx, a->dmem,
                          a->dgamma, a->dbeta, a->dWq, a->dbq, a->dWk, a->dbk, a->dWv, a->dbv, a->dWproj, a->dbproj};
    for (const void* p : ptrs)
        if (tc_misaligned(p)) return "tensors must be 16-byte aligned";
    if (!a->views) return "null argument (views)";
    if (a->n_views <= 0 || a->n_views > 65535) return "n_views must be in [1, 65535]";
    std::vector<std::pair<long long, long long>> q, kv;
    for (int i = 0; i < a->n_views; ++i) {
        const int32_t* v = a->views + 6 * (size_t)i;
        for (int e = 0; e < 6; ++e)
            if (v[e] < 0) return "negative table entry";
        if ((long long)v[0] + v[1] > a->M) return "the table reaches past the M query rows";
        if ((long long)v[2] + v[3] > a->Rm) return "the table reaches past the Rm key rows";
        if (v[4] > v[5] || v[5] > v[3]) return "a skip range needs skip_lo <= skip_hi <= nk";
        q.emplace_back(v[0], (long long)v[0] + v[1]);
        kv.emplace_back(v[2], (long long)v[2] + v[3]);
    }
    *q_covered = tc_spans_cover(q, a->M);
    *kv_covered = tc_spans_cover(kv, a->Rm);
    return nullptr;
}

struct CrossBufs { float *y, *q, *kv, *o, *dO, *dq, *dkv; const float *k, *v; int ldkv; };
static CrossBufs cross_bufs(const must3r_hip_cross_sublayer_args* a, const CrossLayout& L, char* p) {
    auto f = [&](size_t off) { return reinterpret_cast<float*>(p + off); };
    CrossBufs b{f(L.y), f(L.q), f(L.kv), f(L.o), f(L.dO), f(L.dq), f(L.dkv), nullptr, nullptr, 0};
    if (a->Wk) { b.k = b.kv; b.v = b.kv + a->D; b.ldkv = 2 * a->D; }
    else { b.k = a->mem; b.v = a->mem + a->D; b.ldkv = a->ldmem; }
    return b;
}

// y^ = LN(x), q = y^ Wq^T + bq, k | v = mem Wk^T + bk | mem Wv^T + bv (one projection per memory row, the two column blocks of one packed tensor)
static int cross_project(const must3r_hip_cross_sublayer_args* a, const CrossBufs& b) {
    const int M = a->M, Rm = a->Rm, D = a->D;
    M3R_RUN(must3r_hip_op_layernorm_f32(a->x, a->gamma, a->beta, b.y, M, D, a->eps, a->stream));
    M3R_RUN(must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, b.y, D, a->Wq, a->bq, nullptr, 0, b.q, D, nullptr, 0, M, D, D, a->stream));
    if (!a->Wk) return 0;
    M3R_RUN(must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, a->mem, a->ldmem, a->Wk, a->bk, nullptr, 0, b.kv, 2 * D, nullptr, 0, Rm, D, D, a->stream));
    return must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, a->mem, a->ldmem, a->Wv, a->bv, nullptr, 0, b.kv + D, 2 * D, nullptr, 0, Rm, D, D, a->stream);
}

static must3r_hip_attn_train_args cross_core_args(const must3r_hip_cross_sublayer_args* a, const CrossBufs& b) {
    must3r_hip_attn_train_args t{};
    t.q = b.q; t.k = b.k; t.v = b.v;
    t.ldq = a->D; t.ldk = t.ldv = b.ldkv;
    t.heads = a->D / 64; t.n_views = a->n_views; t.views = a->views;
    return t;
}

// o = attention(q, k, v); a row of x that belongs to no view attends nothing
static int cross_attend(const char* who, const must3r_hip_cross_sublayer_args* a, const CrossLayout& L, char* p, const CrossBufs& b, bool q_covered) {
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    if (!q_covered && hipMemsetAsync(b.o, 0, (size_t)a->M * a->D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
    must3r_hip_attn_train_args t = cross_core_args(a, b);
    t.O = b.o; t.ldo = a->D;
    return must3r_hip_attn_forward_f32(&t, p + L.core, L.core_bytes, a->stream);
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_cross_sublayer_scratch_bytes(int M, int Rm, int D, int n_views, int kv_ready) {
    if (tc_shape_error(M, Rm, D) || n_views <= 0 || n_views > 65535) return 0;
    return cross_layout(M, Rm, D, n_views, kv_ready != 0).total;
}

extern "C" int must3r_hip_cross_sublayer_forward(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "cross_sublayer_forward";
    if (!a) return fail("%s: null argument", who);
    bool q_covered = false, kv_covered = false;
    if (const char* e = cross_args_error(a, false, &q_covered, &kv_covered)) return fail("%s: %s", who, e);
    const CrossLayout L = cross_layout(a->M, a->Rm, a->D, a->n_views, !a->Wk);
    if (!scratch || tc_misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    char* p = reinterpret_cast<char*>(scratch);
    const CrossBufs b = cross_bufs(a, L, p);
    M3R_RUN(cross_project(a, b));
    M3R_RUN(cross_attend(who, a, L, p, b, q_covered));
    const int M = a->M, D = a->D;
    return must3r_hip_op_linear_f32(MUST3R_LIN_BIAS_RES, b.o, D, a->Wproj, a->bproj, a->x, D, a->out, D, nullptr, 0, M, D, D, a->stream);
}

extern "C" int must3r_hip_cross_sublayer_grad(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "cross_sublayer_grad";
    if (!a) return fail("%s: null argument", who);
    bool q_covered = false, kv_covered = false;
    if (const char* e = cross_args_error(a, true, &q_covered, &kv_covered)) return fail("%s: %s", who, e);
    if (must3r_hip_attn_train_groups(a->views, a->n_views) < 0) return 1;   // overlapping key groups: the error text is the core's
    const int M = a->M, Rm = a->Rm, D = a->D;
    const bool kv_ready = !a->Wk;
    const CrossLayout L = cross_layout(M, Rm, D, a->n_views, kv_ready);
    if (!scratch || tc_misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    const bool want_wp = a->dWproj || a->dbproj, want_wq = a->dWq || a->dbq, want_ln = a->dx || a->dgamma || a->dbeta;
    const bool want_wk = a->dWk || a->dbk, want_wv = a->dWv || a->dbv;
    const bool want_q = want_wq || want_ln, want_kv = a->dmem || want_wk || want_wv;
    if (!want_wp && !want_q && !want_kv) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    char* p = reinterpret_cast<char*>(scratch);
    const CrossBufs b = cross_bufs(a, L, p);
    if (want_wp && !a->dWproj) {
        // db of proj alone needs neither o nor the forward
        M3R_RUN(must3r_hip_op_linear_wgrad_f32(a->dy, D, nullptr, 0, nullptr, a->dbproj, M, D, D, p + L.wg, L.wg_bytes, a->stream));
        if (!want_q && !want_kv) return 0;
    }
    M3R_RUN(cross_project(a, b));
    if (a->dWproj) {
        M3R_RUN(cross_attend(who, a, L, p, b, q_covered));
        M3R_RUN(must3r_hip_op_linear_wgrad_f32(a->dy, D, b.o, D, a->dWproj, a->dbproj, M, D, D, p + L.wg, L.wg_bytes, a->stream));
    }
    if (!want_q && !want_kv) return 0;
    M3R_RUN(must3r_hip_op_linear_dgrad_f32(a->dy, D, a->Wproj, b.dO, M, D, D, a->stream));
    must3r_hip_attn_train_args t = cross_core_args(a, b);
    t.dO = b.dO; t.lddo = D;
    if (want_q) {
        if (!q_covered && hipMemsetAsync(b.dq, 0, (size_t)M * D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
        t.dQ = b.dq; t.lddq = D;
    }
    if (want_kv) {
        // the attention backward leaves rows outside every key group's span unwritten: they take exact zeros here, on the caller's stream
        if (kv_ready) {
            if (!kv_covered && hipMemset2DAsync(a->dmem, (size_t)a->lddmem * 4, 0, (size_t)2 * D * 4, (size_t)Rm, s) != hipSuccess) return fail("%s: memset failed", who);
            t.dK = a->dmem; t.dV = a->dmem + D;
            t.lddk = t.lddv = a->lddmem;
        } else {
            if (!kv_covered && hipMemsetAsync(b.dkv, 0, (size_t)Rm * 2 * D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
            if (a->dmem || want_wk) t.dK = b.dkv;
            if (a->dmem || want_wv) t.dV = b.dkv + D;
            t.lddk = t.lddv = 2 * D;
        }
    }
    M3R_RUN(must3r_hip_attn_grad(&t, p + L.core, L.core_bytes, a->stream));
    if (want_kv && !kv_ready) {
        if (want_wk) M3R_RUN(must3r_hip_op_linear_wgrad_f32(b.dkv, 2 * D, a->mem, a->ldmem, a->dWk, a->dbk, Rm, D, D, p + L.wg, L.wg_bytes, a->stream));
        if (want_wv) M3R_RUN(must3r_hip_op_linear_wgrad_f32(b.dkv + D, 2 * D, a->mem, a->ldmem, a->dWv, a->dbv, Rm, D, D, p + L.wg, L.wg_bytes, a->stream));
        if (a->dmem) M3R_RUN(launch_dgrad_seg_f32(b.dkv, 2 * D, a->Wk, a->Wv, D, a->dmem, a->lddmem, Rm, 2 * D, D, s));   // dmem = dK Wk + dV Wv
    }
    if (!want_q) return 0;
    if (want_wq) M3R_RUN(must3r_hip_op_linear_wgrad_f32(b.dq, D, b.y, D, a->dWq, a->dbq, M, D, D, p + L.wg, L.wg_bytes, a->stream));
    if (!want_ln) return 0;
    M3R_RUN(must3r_hip_op_linear_dgrad_f32(b.dq, D, a->Wq, b.y, M, D, D, a->stream));               // dL/dy^ over y^
    return must3r_hip_op_layernorm_grad_add(a->x, a->gamma, b.y, a->dy, a->dx, a->dgamma, a->dbeta, M, D, a->eps, p + L.ln, L.ln_bytes, a->stream);
}
