// Training forward and backward of the attention core (blocks/attention.py CoreAttention.attention): softmax(Q K^T / 8) V per head of 64, driven by the
// 6-int view table of the inference kernels (kernels.hpp AttnView).  Per head, s = 1/8, query row i of a view, key row j of its key range; j is valid when
// j < nk and j is not in [skip_lo, skip_hi):
//
//   S_ij = s q_i.k_j      lse_i = log sum_valid exp(S_ij)      P_ij = exp(S_ij - lse_i)  (0 where invalid)
//   O_i  = sum_j P_ij v_j                 delta_i = dO_i . O_i
//   dV_j = sum_i P_ij dO_i                dP_ij = dO_i . v_j            dS_ij = P_ij (dP_ij - delta_i)
//   dQ_i = s sum_j dS_ij k_j              dK_j  = s sum_i dS_ij q_i
//
// A query row without a valid key has O = 0, contributes nothing to dK / dV and gets dQ = 0 (as the inference kernels define it).
// Key masks (the must3r_hip_attn_masked_* entry points; memory dropout): a view may also name a row of a packed bit matrix uint32 [mask_rows][mask_ld]; key j
// is then valid only if bit j % 32 of word j / 32 of that row is set.  The three kernels are templates on MASK: the unmasked instantiations are the code they
// were, the masked ones read a view's 64 bits of a key tile as one 8-byte load (mask_ld is even), test them on the key index a lane already holds, and skip
// a (view, key tile) pair whose bits are all zero exactly like a tile wholly inside the skip range.
// fp32 operands on v_mfma_f32_16x16x4_f32 (upstream gradients of a mean-reduced loss are of order 1e-8, below fp16's range); exp2f with log2(e) folded into the
// scale.  The forward saves nothing but its inputs, the backward recomputes S:
//
//   attn_fwd_f32   one block per (view, head, 64-row query tile): online softmax over the view's 64-row key tiles.  Optional outputs O, lse (natural
//                  log, -inf for a row without keys), lse2 (log2 domain, +inf for such a row: the backward's P is then 0) and delta (needs dO).  The training
//                  forward (O) and the backward's first launch (lse2 and delta into scratch, O never stored) are this one kernel.
//   attn_dkv_f32   one block per (key group, head, 64-row key tile): dK and dV of the tile stay in registers while the block walks the group's views in table
//                  order and each view's query tiles in row order; a (view, key tile) pair at or past the view's nk or wholly inside its skip range is
//                  skipped.  It computes S^T = K Q^T and dP^T = V dO^T, so that P^T and dS^T come out with the key on the accumulator row.
//   attn_dq_f32    one block per (view, head, 64-row query tile): walks the view's key tiles in order, recomputes S and dP, writes dQ once.
//
// A block is 4 waves, each owning 16 rows of the tile's 64 and all 64 columns (4 accumulators of 16 x 16).  The operand that belongs to the block's own rows (Q and
// dO, or K and V in attn_dkv_f32) lives in registers as 16-step A fragments read once from global memory; the walked tiles go through LDS ([64][68] floats: rows
// 16-byte aligned, at most 2-way bank conflicts in either read orientation), each fetched into registers one step ahead, under the products of the tile before it.  P and dS leave the MFMA in the accumulator layout (row 4 (lane / 16) + r, column
// lane % 16) and are the A operand of the next product: they pass through one LDS tile, each wave its own 16 rows.
// No atomics: every output element has one writer and a fixed order of additions (views in table order, tiles in row order, k ascending inside a product).
#include <algorithm>
#include <string.h>
#include <vector>

#include "abi.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "train_attn.hpp"
#include "train_common.hpp"
#include "train_tile.hpp"

namespace m3r {

constexpr int TA_LD = 68;   // LDS row stride in floats (TA_T, the constants, TaArgs, the tile fetches, the key rules and the walk: train_attn.hpp, shared with train_attn16.hip)

// registers (ta_fetch_tile) -> dst [64][TA_LD]
__device__ __forceinline__ void ta_put_tile(float* dst, const f32x4 (&x)[4], int tid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = e * 256 + tid, r = idx >> 4, c = (idx & 15) * 4;
        *reinterpret_cast<f32x4*>(dst + r * TA_LD + c) = x[e];
    }
}
// the A fragments of one row: a[ks] = row[4 ks + fk]
__device__ __forceinline__ void ta_load_frag(float (&a)[16], const float* __restrict__ row, bool ok, int fk) {
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) a[ks] = ok ? row[4 * ks + fk] : 0.f;
}
// acc (16 x 64 of the wave) += A B, A in registers.  TB: B[k][col] = Bs[col][k], else Bs[k][col]
template <bool TB>
__device__ __forceinline__ void ta_mm_reg(f32x4 (&acc)[4], const float (&a)[16], const float* Bs, int fr, int fk) {
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const int k = ks * 4 + fk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b = TB ? Bs[(j * 16 + fr) * TA_LD + k] : Bs[k * TA_LD + j * 16 + fr];
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], b, acc[j], 0, 0, 0);
        }
    }
}
// the same with A = the wave's 16 rows of an LDS tile, B[k][col] = Bs[k][col]
__device__ __forceinline__ void ta_mm_lds(f32x4 (&acc)[4], const float* As, const float* Bs, int fr, int fk) {
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const int k = ks * 4 + fk;
        const float a = As[fr * TA_LD + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[k * TA_LD + j * 16 + fr], acc[j], 0, 0, 0);
    }
}
// accumulator layout -> the wave's 16 rows of an LDS tile
__device__ __forceinline__ void ta_stage(float* Ws, const f32x4 (&x)[4], int fr, int fk) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ws[(fk * 4 + r) * TA_LD + j * 16 + fr] = x[j][r];
}
__device__ __forceinline__ float ta_max16(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float ta_sum16(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_fwd_f32(TaArgs a) {
    __shared__ __attribute__((aligned(16))) float Ks[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Vs[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Ps[TA_T * TA_LD];
    const AttnView v = a.views[blockIdx.z];
    const int q0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (q0 >= v.nq) return;
    const uint32_t* mrow = ta_mask_row<MASK>(a, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const float inf = __builtin_inff();
    float qa[16];
    {
        const int qr = q0 + w * 16 + fr;
        ta_load_frag(qa, a.Q + (size_t)(v.q_row0 + qr) * a.ldq + h * TA_T, qr < v.nq, fk);
    }
    float m[4], l[4];
    f32x4 o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -inf; l[r] = 0.f; }
    zero_acc(o);
    f32x4 rk[4], rv[4];
    auto fetch = [&](int k) { ta_fetch_kv(rk, rv, a, v, k, h, tid); };   // bound once: see ta_fetch_kv
    int k0 = ta_next_tile_m<MASK>(v, 0, mrow);
    if (k0 < v.nk) fetch(k0);
    while (k0 < v.nk) {
        __syncthreads();
        ta_put_tile(Ks, rk, tid);
        ta_put_tile(Vs, rv, tid);
        __syncthreads();
        const int k_next = ta_next_tile_m<MASK>(v, k0 + TA_T, mrow);
        const uint64_t mb = MASK ? ta_tile_bits(mrow, k0, v.nk) : ~0ull;
        if (k_next < v.nk) fetch(k_next);
        f32x4 s[4];
        zero_acc(s);
        ta_mm_reg<true>(s, qa, Ks, fr, fk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = ta_valid(v, k0 + j * 16 + fr) && (!MASK || (mb >> (j * 16 + fr) & 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) s[j][r] = ok ? s[j][r] * TA_C : -inf;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mx = ta_max16(fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])));
            const float mn = fmaxf(m[r], mx), ms = mn == -inf ? 0.f : mn;
            const float alpha = exp2f(m[r] - ms);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p = exp2f(s[j][r] - ms);
                s[j][r] = p;
                sum += p;
                o[j][r] *= alpha;
            }
            l[r] = l[r] * alpha + ta_sum16(sum);
            m[r] = mn;
        }
        ta_stage(Ps + w * 16 * TA_LD, s, fr, fk);
        __syncthreads();
        ta_mm_lds(o, Ps + w * 16 * TA_LD, Vs, fr, fk);
        k0 = k_next;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qr = q0 + w * 16 + fk * 4 + r;
        const bool ok = qr < v.nq;
        const size_t row = (size_t)(v.q_row0 + qr);
        const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = o[j][r] * inv;
            if (ok && a.O) a.O[row * a.ldo + h * TA_T + j * 16 + fr] = x;
            if (a.delta) d += x * (ok ? a.dO[row * a.lddo + h * TA_T + j * 16 + fr] : 0.f);
        }
        if (a.delta) {
            d = ta_sum16(d);
            if (ok && fr == 0) a.delta[row * a.heads + h] = d;
        }
        if (ok && fr == 0) {
            const float l2 = l[r] > 0.f ? m[r] + log2f(l[r]) : inf;
            if (a.lse2) a.lse2[row * a.heads + h] = l2;
            if (a.lse) a.lse[row * a.heads + h] = l[r] > 0.f ? l2 * TA_LN2 : -inf;
        }
    }
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_dq_f32(TaArgs a) {
    __shared__ __attribute__((aligned(16))) float Ks[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Vs[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Ps[TA_T * TA_LD];
    const AttnView v = a.views[blockIdx.z];
    const int q0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (q0 >= v.nq) return;
    const uint32_t* mrow = ta_mask_row<MASK>(a, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const float inf = __builtin_inff();
    float qa[16], da[16];
    {
        const int qr = q0 + w * 16 + fr;
        ta_load_frag(qa, a.Q + (size_t)(v.q_row0 + qr) * a.ldq + h * TA_T, qr < v.nq, fk);
        ta_load_frag(da, a.dO + (size_t)(v.q_row0 + qr) * a.lddo + h * TA_T, qr < v.nq, fk);
    }
    float lr[4], dl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qr = q0 + w * 16 + fk * 4 + r;
        const size_t i = (size_t)(v.q_row0 + qr) * a.heads + h;
        lr[r] = qr < v.nq ? a.lse2[i] : inf;
        dl[r] = qr < v.nq ? a.delta[i] : 0.f;
    }
    f32x4 dq[4];
    zero_acc(dq);
    f32x4 rk[4], rv[4];
    auto fetch = [&](int k) { ta_fetch_kv(rk, rv, a, v, k, h, tid); };   // bound once: see ta_fetch_kv
    int k0 = ta_next_tile_m<MASK>(v, 0, mrow);
    if (k0 < v.nk) fetch(k0);
    while (k0 < v.nk) {
        __syncthreads();
        ta_put_tile(Ks, rk, tid);
        ta_put_tile(Vs, rv, tid);
        __syncthreads();
        const int k_next = ta_next_tile_m<MASK>(v, k0 + TA_T, mrow);
        const uint64_t mb = MASK ? ta_tile_bits(mrow, k0, v.nk) : ~0ull;
        if (k_next < v.nk) fetch(k_next);
        f32x4 s[4], dp[4];
        zero_acc(s);
        zero_acc(dp);
        ta_mm_reg<true>(s, qa, Ks, fr, fk);
        ta_mm_reg<true>(dp, da, Vs, fr, fk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = ta_valid(v, k0 + j * 16 + fr) && (!MASK || (mb >> (j * 16 + fr) & 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = ok ? exp2f(s[j][r] * TA_C - lr[r]) : 0.f;
                s[j][r] = p * (dp[j][r] - dl[r]);
            }
        }
        ta_stage(Ps + w * 16 * TA_LD, s, fr, fk);
        __syncthreads();
        ta_mm_lds(dq, Ps + w * 16 * TA_LD, Ks, fr, fk);
        k0 = k_next;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qr = q0 + w * 16 + fk * 4 + r;
        if (qr >= v.nq) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) a.dQ[(size_t)(v.q_row0 + qr) * a.lddq + h * TA_T + j * 16 + fr] = dq[j][r] * TA_SCALE;
    }
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_dkv_f32(TaArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Ds[TA_T * TA_LD];
    __shared__ __attribute__((aligned(16))) float Ps[TA_T * TA_LD];
    const TaGroup g = a.groups[blockIdx.z];
    const int k0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (k0 >= g.extent) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const float inf = __builtin_inff();
    float ka[16], va[16];
    {
        const int kr = k0 + w * 16 + fr;
        ta_load_frag(ka, a.K + (size_t)(g.kv_row0 + kr) * a.ldk + h * TA_T, kr < g.extent, fk);
        ta_load_frag(va, a.V + (size_t)(g.kv_row0 + kr) * a.ldv + h * TA_T, kr < g.extent, fk);
    }
    f32x4 dk[4], dv[4];
    zero_acc(dk);
    zero_acc(dv);
    f32x4 rq[4], rd[4];
    int vi = -1, q0 = 0;
    AttnView v{};
    uint64_t mb = ~0ull;
    // the walk (train_attn.hpp ta_walk_next) runs one step ahead of the products
    ta_walk_next<MASK>(a, g, k0, vi, q0, v, mb);
    if (vi < g.count) ta_fetch_qdo(rq, rd, a, v, q0, h, tid);
    while (vi < g.count) {
        __syncthreads();
        ta_put_tile(Qs, rq, tid);
        ta_put_tile(Ds, rd, tid);
        __syncthreads();
        int vi_next = vi, q_next = q0;
        AttnView v_next = v;
        uint64_t mb_next = mb;
        ta_walk_next<MASK>(a, g, k0, vi_next, q_next, v_next, mb_next);
        if (vi_next < g.count) ta_fetch_qdo(rq, rd, a, v_next, q_next, h, tid);
        bool kok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) kok[r] = ta_valid(v, k0 + w * 16 + fk * 4 + r) && (!MASK || (mb >> (w * 16 + fk * 4 + r) & 1));
        float lc[4], dc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int qi = q0 + j * 16 + fr;
            const size_t i = (size_t)(v.q_row0 + qi) * a.heads + h;
            lc[j] = qi < v.nq ? a.lse2[i] : inf;
            dc[j] = qi < v.nq ? a.delta[i] : 0.f;
        }
        f32x4 st[4], dpt[4];
        zero_acc(st);
        zero_acc(dpt);
        ta_mm_reg<true>(st, ka, Qs, fr, fk);
        ta_mm_reg<true>(dpt, va, Ds, fr, fk);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = kok[r] ? exp2f(st[j][r] * TA_C - lc[j]) : 0.f;
                st[j][r] = p;
                dpt[j][r] = p * (dpt[j][r] - dc[j]);
            }
        ta_stage(Ps + w * 16 * TA_LD, st, fr, fk);
        __syncthreads();
        ta_mm_lds(dv, Ps + w * 16 * TA_LD, Ds, fr, fk);
        __syncthreads();
        ta_stage(Ps + w * 16 * TA_LD, dpt, fr, fk);
        __syncthreads();
        ta_mm_lds(dk, Ps + w * 16 * TA_LD, Qs, fr, fk);
        vi = vi_next; q0 = q_next; v = v_next; mb = mb_next;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kr = k0 + w * 16 + fk * 4 + r;
        if (kr >= g.extent) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (a.dK) a.dK[(size_t)(g.kv_row0 + kr) * a.lddk + h * TA_T + j * 16 + fr] = dk[j][r] * TA_SCALE;
            if (a.dV) a.dV[(size_t)(g.kv_row0 + kr) * a.lddv + h * TA_T + j * 16 + fr] = dv[j][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------
// what the table says, found on the host: the key groups (views partitioned by kv_row0, in order of first appearance; inside a group the
// views keep the order of the table), the row counts and the grid extents
struct TaPlan {
    std::vector<TaGroup> groups;
    std::vector<int> list;
    int total_q_rows = 0, max_nq = 0, max_extent = 0;
    long long total_kv_rows = 0;
};

// nullptr, or why the table is refused.  want_groups: also build the key groups and refuse overlapping ones.
static const char* ta_plan(const int32_t* views, int n, bool want_groups, TaPlan& P) {
    if (!views) return "null argument (views)";
    if (n <= 0) return "n_views must be positive";
    if (n > 65535) return "more than 65535 views in one call";
    for (int i = 0; i < n; ++i) {
        const int32_t* v = views + 6 * (size_t)i;
        for (int e = 0; e < 6; ++e)
            if (v[e] < 0) return "negative table entry";
        if (v[4] > v[5] || v[5] > v[3]) return "a skip range needs skip_lo <= skip_hi <= nk";
        if ((long long)v[0] + v[1] > 0x7fffffffLL / 2 || (long long)v[2] + v[3] > 0x7fffffffLL / 2) return "row index too large";
        P.total_q_rows = std::max(P.total_q_rows, v[0] + v[1]);
        P.max_nq = std::max(P.max_nq, v[1]);
        P.total_kv_rows = std::max<long long>(P.total_kv_rows, (long long)v[2] + v[3]);
    }
    if (!want_groups) return nullptr;
    // views ordered by (kv_row0, table index): one run per group
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return views[6 * (size_t)x + 2] < views[6 * (size_t)y + 2]; });
    std::vector<TaGroup> sorted;   // in kv_row0 order; `first` holds the smallest table index of the group for now
    std::vector<int> group_of(n);
    for (int i = 0; i < n; ++i) {
        const int32_t* v = views + 6 * (size_t)order[i];
        if (sorted.empty() || sorted.back().kv_row0 != v[2]) sorted.push_back(TaGroup{v[2], 0, order[i], 0});
        sorted.back().extent = std::max(sorted.back().extent, (int)v[3]);
        sorted.back().count += 1;
        group_of[order[i]] = (int)sorted.size() - 1;
    }
    long long end = -1;
    for (const TaGroup& g : sorted) {
        if (g.extent == 0) continue;
        if (g.kv_row0 < end) return "overlapping key groups: views that share key rows must share kv_row0";
        end = (long long)g.kv_row0 + g.extent;
    }
    // groups in order of first appearance, lists in table order
    std::vector<int> by_first(sorted.size());
    for (size_t i = 0; i < sorted.size(); ++i) by_first[i] = (int)i;
    std::sort(by_first.begin(), by_first.end(), [&](int x, int y) { return sorted[x].first < sorted[y].first; });
    std::vector<int> new_id(sorted.size());
    int first = 0;
    for (size_t i = 0; i < by_first.size(); ++i) {
        TaGroup g = sorted[by_first[i]];
        new_id[by_first[i]] = (int)i;
        g.first = first;
        first += g.count;
        g.count = 0;   // refilled below
        P.max_extent = std::max(P.max_extent, g.extent);
        P.groups.push_back(g);
    }
    P.list.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        TaGroup& g = P.groups[new_id[group_of[i]]];
        P.list[g.first + g.count++] = i;
    }
    return nullptr;
}

// scratch: [views n x 6 int32 | groups n x 4 int32 | list n int32 | (masked: mask rows n int32) | lse2 rows x heads fp32 | delta rows x heads fp32], each part a
// multiple of 256 bytes
struct TaLayout { size_t views, groups, list, vmask, tables_bytes, lse2, delta, total; };   // tables_bytes: the tables, one upload
static TaLayout ta_layout(int n, long long q_rows, int heads, bool masked = false) {
    TaLayout L{};
    ScratchCursor c;
    L.views = c.take((size_t)n * 24);
    L.groups = c.take((size_t)n * 16);
    L.list = c.take((size_t)n * 4);
    L.vmask = c.take(masked ? (size_t)n * 4 : 0);
    L.tables_bytes = c.off;
    L.lse2 = c.take((size_t)q_rows * heads * 4);
    L.delta = c.take((size_t)q_rows * heads * 4);
    L.total = c.off;
    return L;
}

// the key masks of a call: nullptr bits, the unmasked call
struct TaMask { const uint32_t* bits; const int32_t* view_mask; int rows, ld; };

// The tables travel through a ring of pinned buffers per calling thread (as resample's, image.hip); a slot's event says when the copy out of it has left it, and
// the slot is reused only then.  With ONE buffer the second upload of a call waited for the first, which is queued behind everything the stream still has to do:
// attn_sublayer_grad uploads twice (forward recompute, backward), so every such call drained the caller's stream on the host (tests/test_stream_order_gpu.py).
struct TaPin {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
};
constexpr int kTaPinSlots = 4;
static thread_local TaPin ta_pins[kTaPinSlots];
static thread_local int ta_pin_next = 0;

static int ta_upload(const TaPlan& P, const int32_t* views, int n, bool want_groups, const int32_t* view_mask, char* scratch, hipStream_t s, const char* who) {
    const TaLayout L = ta_layout(n, 0, 0, view_mask != nullptr);
    const size_t bytes = L.tables_bytes;
    TaPin& pin = ta_pins[ta_pin_next];
    ta_pin_next = (ta_pin_next + 1) % kTaPinSlots;
    if (pin.ev) {
        if (hipEventSynchronize(pin.ev) != hipSuccess) return fail("%s: waiting for the previous table upload failed", who);
        hipEventDestroy(pin.ev);
        pin.ev = nullptr;
    }
    if (pin.cap < bytes) {
        if (pin.host) hipHostFree(pin.host);
        pin.host = nullptr; pin.cap = 0;
        if (hipHostMalloc(&pin.host, bytes, hipHostMallocDefault) != hipSuccess) { pin.host = nullptr; return fail("%s: no pinned memory for the tables", who); }
        pin.cap = bytes;
    }
    char* h = reinterpret_cast<char*>(pin.host);
    memset(h, 0, bytes);
    memcpy(h, views, (size_t)n * 24);
    if (want_groups) {
        memcpy(h + L.groups, P.groups.data(), P.groups.size() * sizeof(TaGroup));
        memcpy(h + L.list, P.list.data(), (size_t)n * 4);
    }
    if (view_mask) memcpy(h + L.vmask, view_mask, (size_t)n * 4);
    if (hipMemcpyAsync(scratch, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("%s: the table upload failed", who);
    if (hipEventCreateWithFlags(&pin.ev, hipEventDisableTiming) != hipSuccess) { pin.ev = nullptr; return fail("%s: no event", who); }
    if (hipEventRecord(pin.ev, s) != hipSuccess) return fail("%s: no event", who);
    return 0;
}

static const char* ta_args_error(const must3r_hip_attn_train_args* a, bool grad) {
    if (!a->q || !a->k || !a->v) return "null argument (q, k, v)";
    if (grad && !a->dO) return "null argument (dO)";
    if (!grad && !a->O) return "null argument (O)";
    if (a->heads <= 0) return "heads must be positive";
    const int D = a->heads * TA_T;
    auto bad_ld = [&](int ld) { return ld < D || ld % 4 != 0; };
    if (bad_ld(a->ldq) || bad_ld(a->ldk) || bad_ld(a->ldv)) return "a leading dimension must be at least heads * 64 and a multiple of 4";
    if (grad ? bad_ld(a->lddo) || (a->dQ && bad_ld(a->lddq)) || (a->dK && bad_ld(a->lddk)) || (a->dV && bad_ld(a->lddv)) : bad_ld(a->ldo))
        return "a leading dimension must be at least heads * 64 and a multiple of 4";
    if (misaligned(a->q) || misaligned(a->k) || misaligned(a->v) || misaligned(a->dO) || misaligned(a->O) || misaligned(a->lse) ||
        misaligned(a->dQ) || misaligned(a->dK) || misaligned(a->dV))
        return "tensors must be 16-byte aligned";
    return nullptr;
}

// nullptr, or why the key masks of a call are refused; the table has passed ta_plan.  Nothing is read through mask_bits.
static const char* ta_mask_error(const TaMask& m, const int32_t* views, int n) {
    if (!m.bits != !m.view_mask) return "mask_bits and view_mask come together (both NULL: no masks)";
    if (!m.bits) return nullptr;
    if (m.ld <= 0 || m.ld % 2) return "mask_ld must be positive and even";
    if (m.rows < 0) return "mask_rows must not be negative";
    if ((size_t)m.bits & 7) return "mask_bits must be 8-byte aligned";
    for (int i = 0; i < n; ++i) {
        const int r = m.view_mask[i];
        if (r < -1 || r >= m.rows) return "a view_mask entry outside [-1, mask_rows)";
        if (r >= 0 && 32LL * m.ld < views[6 * (size_t)i + 3]) return "a mask row is shorter than the nk of a view that names it (32 mask_ld < nk)";
    }
    return nullptr;
}

static TaArgs ta_kernel_args(const must3r_hip_attn_train_args* a, const TaPlan& P, const TaMask& m, char* scratch) {
    TaArgs k{};
    k.Q = a->q; k.K = a->k; k.V = a->v; k.dO = a->dO;
    k.ldq = a->ldq; k.ldk = a->ldk; k.ldv = a->ldv; k.lddo = a->lddo; k.heads = a->heads;
    const TaLayout L = ta_layout(a->n_views, P.total_q_rows, a->heads, m.bits != nullptr);
    k.views = reinterpret_cast<const AttnView*>(scratch + L.views);
    k.groups = reinterpret_cast<const TaGroup*>(scratch + L.groups);
    k.list = reinterpret_cast<const int*>(scratch + L.list);
    k.lse2 = reinterpret_cast<float*>(scratch + L.lse2);
    k.delta = reinterpret_cast<float*>(scratch + L.delta);
    if (m.bits) { k.mask = m.bits; k.vmask = reinterpret_cast<const int*>(scratch + L.vmask); k.mask_ld = m.ld; }
    return k;
}

// the kernels of a call, chosen once: the calling thread's mode (must3r_hip_train_attention_mode) picks the family, `masked` the instantiation
static TaKernels ta_kernels(bool masked) {
    if (train_attention_bf16()) return ta_kernels_bf16(masked);
    if (masked) return TaKernels{attn_fwd_f32<true>, attn_dkv_f32<true>, attn_dq_f32<true>};
    return TaKernels{attn_fwd_f32<false>, attn_dkv_f32<false>, attn_dq_f32<false>};
}

// the two entry points of each kind, behind their argument checks: m.bits == nullptr launches the unmasked instantiations over the unmasked scratch layout
static int ta_forward(const char* who, const must3r_hip_attn_train_args* a, const TaMask& m, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (const char* e = ta_args_error(a, false)) return fail("%s: %s", who, e);
    if (a->heads > 65535) return fail("%s: more than 65535 heads", who);
    TaPlan P;
    if (const char* e = ta_plan(a->views, a->n_views, false, P)) return fail("%s: %s", who, e);
    if (const char* e = ta_mask_error(m, a->views, a->n_views)) return fail("%s: %s", who, e);
    const bool masked = m.bits != nullptr;
    if (!scratch || misaligned(scratch) || scratch_bytes < ta_layout(a->n_views, P.total_q_rows, a->heads, masked).total) return fail("%s: scratch too small", who);
    if (P.max_nq == 0) return 0;
    if (ta_upload(P, a->views, a->n_views, false, m.view_mask, reinterpret_cast<char*>(scratch), s, who)) return 1;
    TaArgs k = ta_kernel_args(a, P, m, reinterpret_cast<char*>(scratch));
    k.dO = nullptr; k.lse2 = nullptr; k.delta = nullptr;
    k.O = a->O; k.ldo = a->ldo; k.lse = a->lse;
    const dim3 qgrid((P.max_nq + TA_T - 1) / TA_T, a->heads, a->n_views);
    hipLaunchKernelGGL(ta_kernels(masked).fwd, qgrid, dim3(256), 0, s, k);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

static int ta_grad(const char* who, const must3r_hip_attn_train_args* a, const TaMask& m, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (const char* e = ta_args_error(a, true)) return fail("%s: %s", who, e);
    if (a->heads > 65535) return fail("%s: more than 65535 heads", who);
    TaPlan P;
    if (const char* e = ta_plan(a->views, a->n_views, true, P)) return fail("%s: %s", who, e);
    if (const char* e = ta_mask_error(m, a->views, a->n_views)) return fail("%s: %s", who, e);
    const bool masked = m.bits != nullptr;
    if (!scratch || misaligned(scratch) || scratch_bytes < ta_layout(a->n_views, P.total_q_rows, a->heads, masked).total) return fail("%s: scratch too small", who);
    const bool want_kv = a->dK || a->dV;
    if (!a->dQ && !want_kv) return 0;
    if (ta_upload(P, a->views, a->n_views, true, m.view_mask, reinterpret_cast<char*>(scratch), s, who)) return 1;
    TaArgs k = ta_kernel_args(a, P, m, reinterpret_cast<char*>(scratch));
    k.dQ = a->dQ; k.dK = a->dK; k.dV = a->dV; k.lddq = a->lddq; k.lddk = a->lddk; k.lddv = a->lddv;
    const dim3 qgrid((P.max_nq + TA_T - 1) / TA_T, a->heads, a->n_views), kgrid((P.max_extent + TA_T - 1) / TA_T, a->heads, (unsigned)P.groups.size());
    const bool run_q = P.max_nq > 0, run_kv = want_kv && P.max_extent > 0;
    // lse2 and delta into scratch, then dK | dV, then dQ
    const TaKernels K = ta_kernels(masked);
    if (run_q) hipLaunchKernelGGL(K.fwd, qgrid, dim3(256), 0, s, k);
    if (run_kv) hipLaunchKernelGGL(K.dkv, kgrid, dim3(256), 0, s, k);
    if (a->dQ && run_q) hipLaunchKernelGGL(K.dq, qgrid, dim3(256), 0, s, k);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

}  // namespace m3r
using namespace m3r;

static bool ta_scratch_shape_ok(int n_views, int total_q_rows, int total_kv_rows, int heads) {
    return !(n_views <= 0 || n_views > 65535 || total_q_rows < 0 || total_kv_rows < 0 || heads <= 0 || heads > 65535);
}

extern "C" size_t must3r_hip_attn_train_scratch_bytes(int n_views, int total_q_rows, int total_kv_rows, int heads) {
    if (!ta_scratch_shape_ok(n_views, total_q_rows, total_kv_rows, heads)) {
        fail("attn_train_scratch_bytes: n_views in [1, 65535], non-negative row counts and heads in [1, 65535] are required");
        return 0;
    }
    return ta_layout(n_views, total_q_rows, heads).total;
}

extern "C" size_t must3r_hip_attn_masked_scratch_bytes(int n_views, int total_q_rows, int total_kv_rows, int heads) {
    if (!ta_scratch_shape_ok(n_views, total_q_rows, total_kv_rows, heads)) {
        fail("attn_masked_scratch_bytes: n_views in [1, 65535], non-negative row counts and heads in [1, 65535] are required");
        return 0;
    }
    return ta_layout(n_views, total_q_rows, heads, true).total;
}

extern "C" int must3r_hip_attn_train_groups(const int32_t* views_host, int n_views) {
    TaPlan P;
    if (const char* e = ta_plan(views_host, n_views, true, P)) { fail("attn_train_groups: %s", e); return -1; }
    return (int)P.groups.size();
}

extern "C" int must3r_hip_attn_forward_f32(const must3r_hip_attn_train_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    if (!a) return fail("attn_forward_f32: null argument");
    return ta_forward("attn_forward_f32", a, TaMask{}, scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int must3r_hip_attn_grad(const must3r_hip_attn_train_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    if (!a) return fail("attn_grad: null argument");
    return ta_grad("attn_grad", a, TaMask{}, scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int must3r_hip_attn_masked_forward(const must3r_hip_attn_masked_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("attn_masked_forward: null argument");
    return ta_forward("attn_masked_forward", &a->core, TaMask{a->mask_bits, a->view_mask, a->mask_rows, a->mask_ld}, scratch, scratch_bytes,
                      reinterpret_cast<hipStream_t>(a->stream));
}

extern "C" int must3r_hip_attn_masked_grad(const must3r_hip_attn_masked_args* a, void* scratch, size_t scratch_bytes) {
    if (!a) return fail("attn_masked_grad: null argument");
    return ta_grad("attn_masked_grad", &a->core, TaMask{a->mask_bits, a->view_mask, a->mask_rows, a->mask_ld}, scratch, scratch_bytes,
                   reinterpret_cast<hipStream_t>(a->stream));
}
