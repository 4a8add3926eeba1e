// The bf16 siblings of the three kernels of the training attention core (train_attention.hip) on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, and the
// per-thread mode that selects them (must3r_hip_train_attention_mode, ABI 21 additive).  Nothing outside the kernels changes: the same TaArgs and view table,
// key groups, skip ranges and mask bits, the same scratch (lse2 and delta fp32 [rows][heads]), the same grids and launch order.  Everything in memory stays
// fp32: an operand is rounded to bf16 (nearest even, NaN and inf kept, cvt4<bf16_t>) in registers on its way into LDS or into a fragment, as train_lin16.hip
// does it.  Products of two bf16 values are exact in fp32, so beside the operand roundings the only error is the fp32 summation.  With s = 1/8 and ^ = bf16:
//
//   S = s (Q^ K^T^) (fp32 accumulation; s and log2 e applied in fp32 after the product)      online softmax in fp32, l sums the unrounded p
//   O = (sum_tiles P^ V^) / l        delta = dO . O  (unrounded dO, the O just computed)      P = exp2(S c - lse2), 0 for an invalid key
//   dV = P^T^ dO^        dP = dO^ V^T^        dS = P (dP - delta) in fp32        dQ = s dS^ K^        dK = s dS^T^ Q^
//
// Every product is computed TRANSPOSED, so that P and dS never leave the registers.  A block is 4 waves; a wave owns 16 rows of the block's own tile (queries in
// attn_fwd_bf16 and attn_dq_bf16, keys in attn_dkv_bf16) and holds them as B fragments (lane: own row lane & 15, 8 consecutive head dimensions per 32-deep step),
// read once from global memory.  The walked tile (K and V, or Q and dO) lies in LDS as [64 rows][64 + 16] bf16:
//   * the score of a step, (walked rows) x (own rows), takes the walked tile as A by rows: one 16-byte read per fragment (contraction along the fast dimension);
//     the accumulator then holds, in lane l, own row l & 15 and walked rows 16 t + 4 (l >> 4) + r (t, r = 0..3);
//   * rounded to bf16 these 16 values ARE the B fragments of the second product, (head dimension) x (own rows) = (walked tile)^T x P: for the 32-deep step ks,
//     lane group g = l >> 4 holds the walked rows 32 ks + 4 g ... + 3 and 32 ks + 16 + 4 g ... + 3, and the A operand, the walked tile contracted along its slow
//     dimension, is read transposed with two ds_read_b64_tr_b16 per fragment that name exactly those rows (train_tile.hpp frag_tr4, the code and the
//     row-permutation contract that dgrad_bf16 and wgrad_bf16 use): the same permutation of a step's 32 rows on both operands.
// The outputs come out transposed as well: lane l holds own row l & 15 and head dimensions 16 t + 4 (l >> 4) ... + 3, one 16-byte store per t.  The softmax
// statistics of a query are per lane in the query-owning kernels (the four lanes l, l ^ 16, l ^ 32, l ^ 48 share a query and combine with two VALU swaps), and
// per accumulator row in attn_dkv_bf16, which reads lse2 and delta of the walked 64 queries through LDS.
// With 160-byte rows the 16 rows of a 16-byte fragment read fall on 16 different 4-bank slots in each ds_read_b128 lane group, and the 8 rows a 32-lane half
// names in a transposing read start 8 banks apart (40 r mod 64 = 0, 40, 16, 56, 32, 8, 48, 24): both reads are free of bank conflicts.
// LDS: two tiles, 20480 B (20992 B with the statistics in attn_dkv_bf16), against 52224 B of the fp32 kernels.
// Tails are filled by a select on the load (rows past nq, nk, extent), and no load touches the padding of a strided row.  No atomics: every output element has
// one writer and a fixed order of additions (views in table order, tiles in row order, the MFMA's own order inside a step); a view's O and dQ and a scene's
// dK and dV are the same bits alone and in a batch.
#include "abi.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "train_attn.hpp"
#include "train_common.hpp"
#include "train_tile.hpp"

namespace m3r {

constexpr int TB_LD = 80;   // LDS row stride of a [64][64] bf16 tile, in elements

static thread_local int g_train_attention_mode = MUST3R_TRAIN_ATTENTION_F32;
bool train_attention_bf16() { return g_train_attention_mode == MUST3R_TRAIN_ATTENTION_BF16; }

// registers (ta_fetch_tile) -> dst [64][TB_LD], rounded: one 8-byte write per float4
__device__ __forceinline__ void tb_put_tile(bf16_t* dst, const f32x4 (&x)[4], int tid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = e * 256 + tid, r = idx >> 4, c = (idx & 15) * 4;
        *reinterpret_cast<bf16x4*>(dst + r * TB_LD + c) = cvt4<bf16_t>(x[e]);
    }
}
// the B fragments of one of the wave's own rows: b[ks] = row[32 ks + 8 fk ... + 7], rounded
__device__ __forceinline__ void tb_load_own(bf16x8 (&b)[2], const float* __restrict__ row, bool ok, int fk) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b[ks] = cat8(cvt4<bf16_t>(ld4_or_zero(row + 32 * ks + 8 * fk, ok)), cvt4<bf16_t>(ld4_or_zero(row + 32 * ks + 8 * fk + 4, ok)));
}
// acc[t] (rows 16 t ... + 15 of the LDS tile x the wave's 16 own rows) += Ts[row][d] own[d]: the tile by rows
__device__ __forceinline__ void tb_mm_rows(f32x4 (&acc)[4], const bf16_t* Ts, const bf16x8 (&b)[2], int fr, int fk) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            acc[t] = mfma16(*reinterpret_cast<const bf16x8*>(Ts + (t * 16 + fr) * TB_LD + ks * 32 + fk * 8), b[ks], acc[t]);
}
// acc[t] (head dimensions 16 t ... + 15 x the wave's 16 own rows) += Ts[row][d] p[row]: the tile transposed by the read; p[ks] as tb_pack leaves it
__device__ __forceinline__ void tb_mm_cols(f32x4 (&acc)[4], const bf16_t* Ts, const bf16x8 (&p)[2], int fr, int fk) {
    const bf16_t* base = Ts + (fk * 4 + (fr >> 2)) * TB_LD + (fr & 3) * 4;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 f[4];
        frag_tr4<TB_LD>(base + ks * 32 * TB_LD, f);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mfma16(f[t], p[ks], acc[t]);
    }
}
// the accumulators of a score (lane: walked rows 16 t + 4 fk + r) -> the B fragments of the second product, rounded
__device__ __forceinline__ void tb_pack(bf16x8 (&p)[2], const f32x4 (&x)[4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) p[ks] = cat8(cvt4<bf16_t>(x[2 * ks]), cvt4<bf16_t>(x[2 * ks + 1]));
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_fwd_bf16(TaArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[TA_T * TB_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[TA_T * TB_LD];
    const AttnView v = a.views[blockIdx.z];
    const int q0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (q0 >= v.nq) return;
    const uint32_t* mrow = ta_mask_row<MASK>(a, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const float inf = __builtin_inff();
    // the lane's query; the four lanes fr, fr + 16, fr + 32, fr + 48 share it and keep the same m and l
    const int qr = q0 + w * 16 + fr;
    const bool qok = qr < v.nq;
    const size_t row = (size_t)(v.q_row0 + qr);
    bf16x8 qb[2];
    tb_load_own(qb, a.Q + row * a.ldq + h * TA_T, qok, fk);
    float m = -inf, l = 0.f;
    f32x4 o[4];
    zero_acc(o);
    f32x4 rk[4], rv[4];
    auto fetch = [&](int k) { ta_fetch_kv(rk, rv, a, v, k, h, tid); };   // bound once: see ta_fetch_kv
    int k0 = ta_next_tile_m<MASK>(v, 0, mrow);
    if (k0 < v.nk) fetch(k0);
    while (k0 < v.nk) {
        __syncthreads();
        tb_put_tile(Ks, rk, tid);
        tb_put_tile(Vs, rv, tid);
        __syncthreads();
        const int k_next = ta_next_tile_m<MASK>(v, k0 + TA_T, mrow);
        const uint64_t mb = (MASK ? ta_tile_bits(mrow, k0, v.nk) : ~0ull) >> (fk * 4);
        if (k_next < v.nk) fetch(k_next);
        f32x4 s[4];
        zero_acc(s);
        tb_mm_rows(s, Ks, qb, fr, fk);   // S^T: s[t][r] is key k0 + 16 t + 4 fk + r against the lane's query
        float mx = -inf;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = ta_valid(v, k0 + t * 16 + fk * 4 + r) && (!MASK || (mb >> (t * 16 + r) & 1));
                s[t][r] = ok ? s[t][r] * TA_C : -inf;
                mx = fmaxf(mx, s[t][r]);
            }
        mx = quad_row_max(mx);
        const float mn = fmaxf(m, mx), ms = mn == -inf ? 0.f : mn;
        const float alpha = exp2f(m - ms);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp2f(s[t][r] - ms);
                s[t][r] = p;
                sum += p;   // the unrounded p
            }
            o[t] *= alpha;
        }
        l = l * alpha + quad_row_sum(sum);
        m = mn;
        bf16x8 pb[2];
        tb_pack(pb, s);
        tb_mm_cols(o, Vs, pb, fr, fk);   // O^T += V^T P^T
        k0 = k_next;
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    float d = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = h * TA_T + t * 16 + fk * 4;
        const f32x4 x = o[t] * inv;
        if (qok && a.O) *reinterpret_cast<f32x4*>(a.O + row * a.ldo + col) = x;
        if (a.delta) {
            const f32x4 g = ld4_or_zero(a.dO + row * a.lddo + col, qok);
#pragma unroll
            for (int r = 0; r < 4; ++r) d += x[r] * g[r];
        }
    }
    if (a.delta) {
        d = quad_row_sum(d);
        if (qok && fk == 0) a.delta[row * a.heads + h] = d;
    }
    if (qok && fk == 0) {
        const float l2 = l > 0.f ? m + log2f(l) : inf;
        if (a.lse2) a.lse2[row * a.heads + h] = l2;
        if (a.lse) a.lse[row * a.heads + h] = l > 0.f ? l2 * TA_LN2 : -inf;
    }
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_dq_bf16(TaArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[TA_T * TB_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[TA_T * TB_LD];
    const AttnView v = a.views[blockIdx.z];
    const int q0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (q0 >= v.nq) return;
    const uint32_t* mrow = ta_mask_row<MASK>(a, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int qr = q0 + w * 16 + fr;
    const bool qok = qr < v.nq;
    const size_t row = (size_t)(v.q_row0 + qr);
    bf16x8 qb[2], db[2];
    tb_load_own(qb, a.Q + row * a.ldq + h * TA_T, qok, fk);
    tb_load_own(db, a.dO + row * a.lddo + h * TA_T, qok, fk);
    const float lr = qok ? a.lse2[row * a.heads + h] : __builtin_inff();
    const float dl = qok ? a.delta[row * a.heads + h] : 0.f;
    f32x4 dq[4];
    zero_acc(dq);
    f32x4 rk[4], rv[4];
    auto fetch = [&](int k) { ta_fetch_kv(rk, rv, a, v, k, h, tid); };   // bound once: see ta_fetch_kv
    int k0 = ta_next_tile_m<MASK>(v, 0, mrow);
    if (k0 < v.nk) fetch(k0);
    while (k0 < v.nk) {
        __syncthreads();
        tb_put_tile(Ks, rk, tid);
        tb_put_tile(Vs, rv, tid);
        __syncthreads();
        const int k_next = ta_next_tile_m<MASK>(v, k0 + TA_T, mrow);
        const uint64_t mb = (MASK ? ta_tile_bits(mrow, k0, v.nk) : ~0ull) >> (fk * 4);
        if (k_next < v.nk) fetch(k_next);
        f32x4 s[4], dp[4];
        zero_acc(s);
        zero_acc(dp);
        tb_mm_rows(s, Ks, qb, fr, fk);    // S^T = K Q^T
        tb_mm_rows(dp, Vs, db, fr, fk);   // dP^T = V dO^T
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = ta_valid(v, k0 + t * 16 + fk * 4 + r) && (!MASK || (mb >> (t * 16 + r) & 1));
                const float p = ok ? exp2f(s[t][r] * TA_C - lr) : 0.f;
                s[t][r] = p * (dp[t][r] - dl);
            }
        bf16x8 ds[2];
        tb_pack(ds, s);
        tb_mm_cols(dq, Ks, ds, fr, fk);   // dQ^T += K^T dS^T
        k0 = k_next;
    }
    if (!qok) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(a.dQ + row * a.lddq + h * TA_T + t * 16 + fk * 4) = dq[t] * TA_SCALE;
}

template <bool MASK>
__global__ void __launch_bounds__(256) attn_dkv_bf16(TaArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[TA_T * TB_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Ds[TA_T * TB_LD];
    __shared__ __attribute__((aligned(16))) float Ls[2 * TA_T];   // lse2 | delta of the walked 64 queries
    const TaGroup g = a.groups[blockIdx.z];
    const int k0 = blockIdx.x * TA_T, h = blockIdx.y;
    if (k0 >= g.extent) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const float inf = __builtin_inff();
    // the lane's key
    const int kr = k0 + w * 16 + fr;
    const bool kin = kr < g.extent;
    const size_t krow = (size_t)(g.kv_row0 + kr);
    bf16x8 kb[2], vb[2];
    tb_load_own(kb, a.K + krow * a.ldk + h * TA_T, kin, fk);
    tb_load_own(vb, a.V + krow * a.ldv + h * TA_T, kin, fk);
    f32x4 dk[4], dv[4];
    zero_acc(dk);
    zero_acc(dv);
    f32x4 rq[4], rd[4];
    float rs = 0.f;   // threads 0..63: lse2 of query q0 + tid (+inf past nq); threads 64..127: delta of query q0 + tid - 64 (0 past nq)
    auto fetch = [&](const AttnView& v, int q0) {
        ta_fetch_qdo(rq, rd, a, v, q0, h, tid);
        if (tid < 2 * TA_T) {
            const int qi = q0 + (tid & 63);
            const bool second = tid >= TA_T;
            rs = second ? 0.f : inf;
            if (qi < v.nq) rs = (second ? a.delta : a.lse2)[(size_t)(v.q_row0 + qi) * a.heads + h];
        }
    };
    int vi = -1, q0 = 0;
    AttnView v{};
    uint64_t mb = ~0ull;
    // the walk (train_attn.hpp ta_walk_next) runs one step ahead of the products
    ta_walk_next<MASK>(a, g, k0, vi, q0, v, mb);
    if (vi < g.count) fetch(v, q0);
    while (vi < g.count) {
        __syncthreads();
        tb_put_tile(Qs, rq, tid);
        tb_put_tile(Ds, rd, tid);
        if (tid < 2 * TA_T) Ls[tid] = rs;
        __syncthreads();
        int vi_next = vi, q_next = q0;
        AttnView v_next = v;
        uint64_t mb_next = mb;
        ta_walk_next<MASK>(a, g, k0, vi_next, q_next, v_next, mb_next);
        if (vi_next < g.count) fetch(v_next, q_next);
        const bool kok = ta_valid(v, kr) && (!MASK || (mb >> (w * 16 + fr) & 1));
        f32x4 s[4], dp[4];
        zero_acc(s);
        zero_acc(dp);
        tb_mm_rows(s, Qs, kb, fr, fk);    // S = Q K^T: s[t][r] is query q0 + 16 t + 4 fk + r against the lane's key
        tb_mm_rows(dp, Ds, vb, fr, fk);   // dP = dO V^T
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 lc = *reinterpret_cast<const f32x4*>(Ls + t * 16 + fk * 4);
            const f32x4 dc = *reinterpret_cast<const f32x4*>(Ls + TA_T + t * 16 + fk * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = kok ? exp2f(s[t][r] * TA_C - lc[r]) : 0.f;
                s[t][r] = p;
                dp[t][r] = p * (dp[t][r] - dc[r]);
            }
        }
        bf16x8 pb[2], ds[2];
        tb_pack(pb, s);
        tb_pack(ds, dp);
        tb_mm_cols(dv, Ds, pb, fr, fk);   // dV^T += dO^T P
        tb_mm_cols(dk, Qs, ds, fr, fk);   // dK^T += Q^T dS
        vi = vi_next; q0 = q_next; v = v_next; mb = mb_next;
    }
    if (!kin) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = h * TA_T + t * 16 + fk * 4;
        if (a.dK) *reinterpret_cast<f32x4*>(a.dK + krow * a.lddk + col) = dk[t] * TA_SCALE;
        if (a.dV) *reinterpret_cast<f32x4*>(a.dV + krow * a.lddv + col) = dv[t];
    }
}

TaKernels ta_kernels_bf16(bool masked) {
    if (masked) return TaKernels{attn_fwd_bf16<true>, attn_dkv_bf16<true>, attn_dq_bf16<true>};
    return TaKernels{attn_fwd_bf16<false>, attn_dkv_bf16<false>, attn_dq_bf16<false>};
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_train_attention_mode(int mode) {
    return swap_thread_mode(g_train_attention_mode, mode, MUST3R_TRAIN_ATTENTION_BF16,
                            "train_attention_mode: unknown mode %d (MUST3R_TRAIN_ATTENTION_F32 = 0, MUST3R_TRAIN_ATTENTION_BF16 = 1, -1 to query)");
}
