// Host-side helpers of the four training sources (train_head.hip, train_attention.hip, train_block.hip, train_cross.hip), once each: the early-return macro,
// the 256-byte scratch parts, the alignment test, the per-thread mode switch, the argument checks that more than one file makes, and the pieces every residual sublayer's backward shares:
//   x -> y = LN(x) -> first Linear -> ... -> last Linear -> + x
// The backward of all three sublayers opens with the same shortcut (last_bias_alone) and closes with the same tail (sublayer_grad_tail); the two attention
// sublayers also share the forward of the core (sublayer_attend) and the gradients at proj (proj_grad).  The sublayer templates read the operands that the three
// descriptors name alike (x, gamma, dy, dx, dgamma, dbeta, M, D, eps; Wproj, dWproj, dbproj) and the scratch parts that their layouts name alike (wg, ln, core).
// No device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "abi.hpp"

namespace m3r {

#define M3R_RUN(expr)                 \
    do {                              \
        int rc__ = (expr);            \
        if (rc__) return rc__;        \
    } while (0)

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
inline bool misaligned(const void* p) { return ((size_t)p & 15) != 0; }

// the parts of a scratch buffer, each a multiple of 256 bytes: take() answers where the part begins, off where the next one will
struct ScratchCursor {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    }
};

// The one entry point of a per-thread mode (must3r_hip_train_linear_mode, must3r_hip_train_attention_mode) over the caller's own thread-local `cur`, whose
// modes are 0 .. last: -1 answers the mode and changes nothing; a mode sets it and answers the one it replaces; anything else leaves `refusal` (a format
// taking the refused mode) as the last error and answers -1.
__attribute__((format(printf, 4, 0))) inline int swap_thread_mode(int& cur, int mode, int last, const char* refusal) {
    if (mode == -1) return cur;
    if (mode < 0 || mode > last) {
        fail(refusal, mode);
        return -1;
    }
    return std::exchange(cur, mode);
}

// M token rows of width D (and Rm rows of a second tensor, where there is one)
inline const char* rows_width_error(int M, int D, int Rm = 1) {
    if (M <= 0) return "M must be positive";
    if (Rm <= 0) return "Rm must be positive";
    if (D <= 0 || D % 64) return "D must be a positive multiple of 64";
    if (D > 1024) return "D must not exceed 1024";
    if (M > 0x7fffffff / 4 || Rm > 0x7fffffff / 4) return "too many rows";
    return nullptr;
}

// do the half-open spans cover [0, rows)?
inline bool spans_cover(std::vector<std::pair<long long, long long>> spans, long long rows) {
    std::sort(spans.begin(), spans.end());
    long long end = 0;
    for (const auto& sp : spans) {
        if (sp.second <= sp.first) continue;
        if (sp.first > end) return false;
        end = std::max(end, sp.second);
    }
    return end >= rows;
}

// nullptr, or why the 6-int view table (on the host) is refused by a sublayer whose queries are q_rows (M) rows and whose keys are kv_rows (Rm; M in the self
// attention) rows.  *q_covered: every query row belongs to a view; *kv_covered: every key row lies inside a key group's span (nothing for the caller to zero).
inline const char* view_table_error(const int32_t* views, int n, int q_rows, int kv_rows, bool* q_covered, bool* kv_covered) {
    if (!views) return "null argument (views)";
    if (n <= 0 || n > 65535) return "n_views must be in [1, 65535]";
    std::vector<std::pair<long long, long long>> q, kv;
    for (int i = 0; i < n; ++i) {
        const int32_t* v = views + 6 * (size_t)i;
        for (int e = 0; e < 6; ++e)
            if (v[e] < 0) return "negative table entry";
        if ((long long)v[0] + v[1] > q_rows) return "the table reaches past the M query rows";
        if ((long long)v[2] + v[3] > kv_rows) return "the table reaches past the Rm key rows (the M rows, in a self attention)";
        if (v[4] > v[5] || v[5] > v[3]) return "a skip range needs skip_lo <= skip_hi <= nk";
        q.emplace_back(v[0], (long long)v[0] + v[1]);
        kv.emplace_back(v[2], (long long)v[2] + v[3]);
    }
    *q_covered = spans_cover(q, q_rows);
    *kv_covered = spans_cover(kv, kv_rows);
    return nullptr;
}

// the attention core's descriptor of a sublayer: heads of 64 over the sublayer's width, its table, q [.][ldq] and k, v [.][ldkv]
template <class Args>
must3r_hip_attn_train_args core_args(const Args* a, const float* q, int ldq, const float* k, const float* v, int ldkv) {
    must3r_hip_attn_train_args t{};
    t.q = q; t.k = k; t.v = v;
    t.ldq = ldq; t.ldk = t.ldv = ldkv;
    t.heads = a->D / 64; t.n_views = a->n_views; t.views = a->views;
    return t;
}

// o [M][D] = attention(q, k, v) of t; a query row of no view attends nothing: it takes zeros
template <class Args, class Layout>
int sublayer_attend(const char* who, const Args* a, const Layout& L, char* p, must3r_hip_attn_train_args t, float* o, bool q_covered, hipStream_t s) {
    if (!q_covered && hipMemsetAsync(o, 0, (size_t)a->M * a->D * 4, s) != hipSuccess) return fail("%s: memset failed", who);
    t.O = o; t.ldo = a->D;
    return must3r_hip_attn_forward_f32(&t, p + L.core, L.core_bytes, s);
}

// The bias gradient of the last Linear ([D][K]) without its weight gradient is the column sums of dy: it needs no forward.  Nothing is launched otherwise.
template <class Args, class Layout>
int last_bias_alone(const Args* a, const Layout& L, char* p, const float* dW, float* db, int K, hipStream_t s) {
    if (dW || !db) return 0;
    return must3r_hip_op_linear_wgrad_f32(a->dy, a->D, nullptr, 0, nullptr, db, a->M, a->D, K, p + L.wg, L.wg_bytes, s);
}

// The gradients at proj, the last Linear of an attention sublayer: dWproj | dbproj from o (where dWproj is asked for), then dO = dy Wproj (where dO is given)
template <class Args, class Layout>
int proj_grad(const Args* a, const Layout& L, char* p, const float* o, float* dO, hipStream_t s) {
    const int M = a->M, D = a->D;
    if (a->dWproj) M3R_RUN(must3r_hip_op_linear_wgrad_f32(a->dy, D, o, D, a->dWproj, a->dbproj, M, D, D, p + L.wg, L.wg_bytes, s));
    return dO ? must3r_hip_op_linear_dgrad_f32(a->dy, D, a->Wproj, dO, M, D, D, s) : 0;
}

// The close of a sublayer's backward, from dz [M][N] = dL/d(first Linear's output) and y = LN(x): dW1 | db1 of the first Linear W1 [N][D], its data gradient
// written over y, and the LayerNorm backward with the residual's dy added.  Each step runs only where its outputs are asked for.
template <class Args, class Layout>
int sublayer_grad_tail(const Args* a, const Layout& L, char* p, const float* dz, int ldz, const float* W1, int N, float* dW1, float* db1, float* y, hipStream_t s) {
    const int M = a->M, D = a->D;
    if (dW1 || db1) M3R_RUN(must3r_hip_op_linear_wgrad_f32(dz, ldz, y, D, dW1, db1, M, N, D, p + L.wg, L.wg_bytes, s));
    if (!a->dx && !a->dgamma && !a->dbeta) return 0;
    M3R_RUN(must3r_hip_op_linear_dgrad_f32(dz, ldz, W1, y, M, N, D, s));
    return must3r_hip_op_layernorm_grad_add(a->x, a->gamma, y, a->dy, a->dx, a->dgamma, a->dbeta, M, D, a->eps, p + L.ln, L.ln_bytes, s);
}

}  // namespace m3r
