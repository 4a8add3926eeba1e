// Training forward and backward of the third residual sublayer of the reference's CachedDecoderBlock (blocks/layers.py:90-99, CachedCrossAttention
// blocks/attention.py:129-149): the cross attention of the tokens x over the token memory, fp32, stateless:
//   out = x + proj(attn(projq(LN(x)), projk(mem), projv(mem)))         no RoPE (the reference builds cross_attn with pos_embed=None)
// or, in the reference's `kv` memory mode, over a memory that already holds k | v.  Queries and keys are rows of different tensors, several views of a scene
// read the same key rows (the key groups of train_attention.hip), and the gradient also arrives at the memory.  This file has no kernel of its own: it
// composes the operator forms of train_block.hip (LayerNorm, the NT Linear) and train_head.hip (the data and weight gradients of a Linear, the LayerNorm
// backward with the residual added), the attention core of train_attention.hip, and the two-segment data gradient of train_head.hip
// (launch_dgrad_seg_f32: dmem = dK Wk + dV Wv in one launch and one accumulator chain per element).  The forward saves nothing; the backward recomputes the
// forward into scratch and differentiates it along the skeleton of train_common.hpp (shared with train_block.hip's two sublayers); what is written out here is
// this sublayer's own: the k | v projections, their weight gradients and dmem.  All work goes to the stream of the descriptor.  No atomics.
// The *_masked_* entry points are the same two functions with the key masks of memory dropout handed to the attention core (must3r_hip_attn_masked_*).
#include <algorithm>

#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "kernels.hpp"
#include "train_common.hpp"

namespace m3r {

// [y^ M D | q M D | k|v Rm 2D | o M D | do M D | dq M D | dk|dv Rm 2D | weight-gradient partials | LayerNorm backward | attention core]; kv_ready: no Rm x 2 D parts
struct CrossLayout { size_t y, q, kv, o, dO, dq, dkv, wg, wg_bytes, ln, ln_bytes, core, core_bytes, total; };
static CrossLayout cross_layout(int M, int Rm, int D, int n_views, bool kv_ready, bool masked = false) {
    CrossLayout L{};
    ScratchCursor c;
    const size_t md = (size_t)M * D * 4, rd = kv_ready ? 0 : (size_t)Rm * 2 * D * 4;
    L.y = c.take(md);
    L.q = c.take(md);
    L.kv = c.take(rd);
    L.o = c.take(md);
    L.dO = c.take(md);
    L.dq = c.take(md);
    L.dkv = c.take(rd);
    L.wg_bytes = must3r_hip_op_linear_wgrad_scratch_bytes(M, D, D);
    if (!kv_ready) L.wg_bytes = std::max(L.wg_bytes, must3r_hip_op_linear_wgrad_scratch_bytes(Rm, D, D));
    L.wg = c.take(L.wg_bytes);
    L.ln_bytes = must3r_hip_op_layernorm_grad_scratch_bytes(M, D);
    L.ln = c.take(L.ln_bytes);
    L.core_bytes = (masked ? must3r_hip_attn_masked_scratch_bytes : must3r_hip_attn_train_scratch_bytes)(n_views, M, Rm, D / 64);
    L.core = c.take(L.core_bytes);
    L.total = c.off;
    return L;
}

// nullptr, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed.
// *q_covered: every row of x is a query row of a view; *kv_covered: every row of mem lies inside a key group's span (nothing to zero).
static const char* cross_args_error(const must3r_hip_cross_sublayer_args* a, bool grad, bool* q_covered, bool* kv_covered) {
    if (const char* e = rows_width_error(a->M, a->D, a->Rm)) return e;
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
        if (misaligned(p)) return "tensors must be 16-byte aligned";
    return view_table_error(a->views, a->n_views, a->M, a->Rm, q_covered, kv_covered);
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
static int cross_project(const must3r_hip_cross_sublayer_args* a, const CrossBufs& b, hipStream_t s) {
    const int M = a->M, Rm = a->Rm, D = a->D;
    M3R_RUN(must3r_hip_op_layernorm_f32(a->x, a->gamma, a->beta, b.y, M, D, a->eps, s));
    M3R_RUN(must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, b.y, D, a->Wq, a->bq, nullptr, 0, b.q, D, nullptr, 0, M, D, D, s));
    if (!a->Wk) return 0;
    M3R_RUN(must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, a->mem, a->ldmem, a->Wk, a->bk, nullptr, 0, b.kv, 2 * D, nullptr, 0, Rm, D, D, s));
    return must3r_hip_op_linear_f32(MUST3R_LIN_BIAS, a->mem, a->ldmem, a->Wv, a->bv, nullptr, 0, b.kv + D, 2 * D, nullptr, 0, Rm, D, D, s);
}

// the key masks of a call (bits == nullptr: none) and the attention core with them: the unmasked entry points without masks, so that their bits are theirs
struct CrossMask { const uint32_t* bits; const int32_t* view_mask; int rows, ld; };
static must3r_hip_attn_masked_args masked_core(const must3r_hip_attn_train_args& t, const CrossMask& m, hipStream_t s) {
    must3r_hip_attn_masked_args k{};
    k.core = t;
    k.mask_bits = m.bits; k.view_mask = m.view_mask; k.mask_rows = m.rows; k.mask_ld = m.ld;
    k.stream = s;
    return k;
}
// what must3r_hip_attn_masked_* would refuse of the masks, found before anything is launched (the core repeats it); the table has passed view_table_error
static const char* cross_mask_error(const must3r_hip_cross_sublayer_args* a, const CrossMask& m) {
    if (!m.bits != !m.view_mask) return "mask_bits and view_mask come together (both NULL: no masks)";
    if (!m.bits) return nullptr;
    if (m.ld <= 0 || m.ld % 2) return "mask_ld must be positive and even";
    if (m.rows < 0) return "mask_rows must not be negative";
    if ((size_t)m.bits & 7) return "mask_bits must be 8-byte aligned";
    for (int i = 0; i < a->n_views; ++i) {
        const int r = m.view_mask[i];
        if (r < -1 || r >= m.rows) return "a view_mask entry outside [-1, mask_rows)";
        if (r >= 0 && 32LL * m.ld < a->views[6 * (size_t)i + 3]) return "a mask row is shorter than the nk of a view that names it (32 mask_ld < nk)";
    }
    return nullptr;
}

// Inside the two functions the descriptor's stream is `s`, a hipStream_t; the must3r_hip_op_* calls take it as their void*.

static int cross_forward(const char* who, const must3r_hip_cross_sublayer_args* a, const CrossMask& m, void* scratch, size_t scratch_bytes) {
    bool q_covered = false, kv_covered = false;
    if (const char* e = cross_args_error(a, false, &q_covered, &kv_covered)) return fail("%s: %s", who, e);
    if (const char* e = cross_mask_error(a, m)) return fail("%s: %s", who, e);
    const CrossLayout L = cross_layout(a->M, a->Rm, a->D, a->n_views, !a->Wk, m.bits != nullptr);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    char* p = reinterpret_cast<char*>(scratch);
    const CrossBufs b = cross_bufs(a, L, p);
    const int M = a->M, D = a->D;
    M3R_RUN(cross_project(a, b, s));
    const must3r_hip_attn_train_args t = core_args(a, b.q, D, b.k, b.v, b.ldkv);
    if (!m.bits) {
        M3R_RUN(sublayer_attend(who, a, L, p, t, b.o, q_covered, s));
    } else {
        if (!q_covered && hipMemsetAsync(b.o, 0, (size_t)M * D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
        must3r_hip_attn_masked_args k = masked_core(t, m, s);
        k.core.O = b.o; k.core.ldo = D;
        M3R_RUN(must3r_hip_attn_masked_forward(&k, p + L.core, L.core_bytes));
    }
    return must3r_hip_op_linear_f32(MUST3R_LIN_BIAS_RES, b.o, D, a->Wproj, a->bproj, a->x, D, a->out, D, nullptr, 0, M, D, D, s);
}

static int cross_grad(const char* who, const must3r_hip_cross_sublayer_args* a, const CrossMask& m, void* scratch, size_t scratch_bytes) {
    bool q_covered = false, kv_covered = false;
    if (const char* e = cross_args_error(a, true, &q_covered, &kv_covered)) return fail("%s: %s", who, e);
    if (const char* e = cross_mask_error(a, m)) return fail("%s: %s", who, e);
    if (must3r_hip_attn_train_groups(a->views, a->n_views) < 0) return 1;   // overlapping key groups: the error text is the core's
    const int M = a->M, Rm = a->Rm, D = a->D;
    const bool kv_ready = !a->Wk;
    const CrossLayout L = cross_layout(M, Rm, D, a->n_views, kv_ready, m.bits != nullptr);
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    const bool want_wk = a->dWk || a->dbk, want_wv = a->dWv || a->dbv;
    const bool want_q = a->dWq || a->dbq || a->dx || a->dgamma || a->dbeta, want_kv = a->dmem || want_wk || want_wv;
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    char* p = reinterpret_cast<char*>(scratch);
    const CrossBufs b = cross_bufs(a, L, p);
    M3R_RUN(last_bias_alone(a, L, p, a->dWproj, a->dbproj, D, s));
    if (!a->dWproj && !want_q && !want_kv) return 0;
    M3R_RUN(cross_project(a, b, s));
    must3r_hip_attn_train_args t = core_args(a, b.q, D, b.k, b.v, b.ldkv);
    if (a->dWproj) {   // only dWproj reads o
        if (!m.bits) {
            M3R_RUN(sublayer_attend(who, a, L, p, t, b.o, q_covered, s));
        } else {
            if (!q_covered && hipMemsetAsync(b.o, 0, (size_t)M * D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
            must3r_hip_attn_masked_args k = masked_core(t, m, s);
            k.core.O = b.o; k.core.ldo = D;
            M3R_RUN(must3r_hip_attn_masked_forward(&k, p + L.core, L.core_bytes));
        }
    }
    M3R_RUN(proj_grad(a, L, p, b.o, want_q || want_kv ? b.dO : nullptr, s));
    if (!want_q && !want_kv) return 0;
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
    if (!m.bits) {
        M3R_RUN(must3r_hip_attn_grad(&t, p + L.core, L.core_bytes, s));
    } else {
        const must3r_hip_attn_masked_args k = masked_core(t, m, s);
        M3R_RUN(must3r_hip_attn_masked_grad(&k, p + L.core, L.core_bytes));
    }
    if (want_kv && !kv_ready) {
        if (want_wk) M3R_RUN(must3r_hip_op_linear_wgrad_f32(b.dkv, 2 * D, a->mem, a->ldmem, a->dWk, a->dbk, Rm, D, D, p + L.wg, L.wg_bytes, s));
        if (want_wv) M3R_RUN(must3r_hip_op_linear_wgrad_f32(b.dkv + D, 2 * D, a->mem, a->ldmem, a->dWv, a->dbv, Rm, D, D, p + L.wg, L.wg_bytes, s));
        if (a->dmem) M3R_RUN(launch_dgrad_seg_f32(b.dkv, 2 * D, a->Wk, a->Wv, D, a->dmem, a->lddmem, Rm, 2 * D, D, s));   // dmem = dK Wk + dV Wv
    }
    return sublayer_grad_tail(a, L, p, b.dq, D, a->Wq, D, a->dWq, a->dbq, b.y, s);
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_cross_sublayer_scratch_bytes(int M, int Rm, int D, int n_views, int kv_ready) {
    if (rows_width_error(M, D, Rm) || n_views <= 0 || n_views > 65535) return 0;
    return cross_layout(M, Rm, D, n_views, kv_ready != 0).total;
}

extern "C" size_t must3r_hip_cross_sublayer_masked_scratch_bytes(int M, int Rm, int D, int n_views, int kv_ready) {
    if (rows_width_error(M, D, Rm) || n_views <= 0 || n_views > 65535) return 0;
    return cross_layout(M, Rm, D, n_views, kv_ready != 0, true).total;
}

extern "C" int must3r_hip_cross_sublayer_forward(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("%s: null argument", "cross_sublayer_forward");
    return cross_forward("cross_sublayer_forward", a, CrossMask{}, scratch, scratch_bytes);
}

extern "C" int must3r_hip_cross_sublayer_grad(const must3r_hip_cross_sublayer_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("%s: null argument", "cross_sublayer_grad");
    return cross_grad("cross_sublayer_grad", a, CrossMask{}, scratch, scratch_bytes);
}

extern "C" int must3r_hip_cross_sublayer_masked_forward(const must3r_hip_cross_sublayer_masked_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("%s: null argument", "cross_sublayer_masked_forward");
    return cross_forward("cross_sublayer_masked_forward", &a->core, CrossMask{a->mask_bits, a->view_mask, a->mask_rows, a->mask_ld}, scratch, scratch_bytes);
}

extern "C" int must3r_hip_cross_sublayer_masked_grad(const must3r_hip_cross_sublayer_masked_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("%s: null argument", "cross_sublayer_masked_grad");
    return cross_grad("cross_sublayer_masked_grad", &a->core, CrossMask{a->mask_bits, a->view_mask, a->mask_rows, a->mask_ld}, scratch, scratch_bytes);
}
