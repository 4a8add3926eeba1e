// What the fp32 kernels of the training attention core (train_attention.hip) and their bf16 siblings (train_attn16.hip) share: the kernel arguments, the
// key-group record, the tile fetches, the rules that say which keys and which key tiles a view reads, the walk of the backward over a key group, and the
// record of kernel pointers by which the host launches either family.  The host side (plan, scratch layout, upload, argument
// checks) lives in train_attention.hip alone: both kernel families are launched from ta_forward and ta_grad there, over the same tables, scratch and grids.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace m3r {

constexpr int TA_T = 64;                          // tile rows / head size
constexpr float TA_SCALE = 0.125f;
constexpr float TA_C = 0.125f * 1.4426950408889634f;   // scale * log2(e)
constexpr float TA_LN2 = 0.6931471805599453f;

struct TaGroup { int kv_row0, extent, first, count; };   // views list[first .. first + count) read key rows [kv_row0, kv_row0 + extent)

struct TaArgs {
    const float* Q; const float* K; const float* V; const float* dO;
    int ldq, ldk, ldv, lddo, heads;
    const AttnView* views;
    const TaGroup* groups; const int* list;
    float* O; int ldo;
    float* lse;                  // [rows][heads], natural log (public)
    float* lse2; float* delta;   // [rows][heads], scratch of the backward
    float* dQ; float* dK; float* dV;
    int lddq, lddk, lddv;
    // MASK instantiations only: the packed key masks [mask_rows][mask_ld], and per view of the table its row (-1: none)
    const uint32_t* mask; const int* vmask; int mask_ld;
};

// rows [0, rows_valid) of a [.][64] slab at src (row stride ld) -> registers (4 float4 per thread), the rest zero.
// The next tile is fetched while the current one is multiplied, so that its global-memory latency hides under the MFMAs.
__device__ __forceinline__ void ta_fetch_tile(f32x4 (&x)[4], const float* __restrict__ src, int ld, int rows_valid, int tid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = e * 256 + tid, r = idx >> 4, c = (idx & 15) * 4;
        x[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < rows_valid) x[e] = *reinterpret_cast<const f32x4*>(src + (size_t)r * ld + c);
    }
}
__device__ __forceinline__ bool ta_valid(const AttnView& v, int j) { return j < v.nk && !(j >= v.skip_lo && j < v.skip_hi); }
__device__ __forceinline__ bool ta_tile_skipped(const AttnView& v, int k0) { return k0 >= v.nk || (k0 >= v.skip_lo && k0 + TA_T <= v.skip_hi); }
// the first key tile at or after k0 that the view reads (>= nk: none)
__device__ __forceinline__ int ta_next_tile(const AttnView& v, int k0) {
    while (k0 < v.nk && ta_tile_skipped(v, k0)) k0 += TA_T;
    return k0;
}

// MASK: the mask row of a view of the table, nullptr where it names none
template <bool MASK>
__device__ __forceinline__ const uint32_t* ta_mask_row(const TaArgs& a, int view) {
    if (!MASK) return nullptr;
    const int r = a.vmask[view];
    return r >= 0 ? a.mask + (size_t)r * a.mask_ld : nullptr;
}
// bit t: key k0 + t of the tile at k0 < nk passes the mask row (all ones without a row); the bits of keys at or past nk are cleared.  k0 is a multiple of 64 and
// 32 mask_ld >= nk with mask_ld even, so that the two words are inside the row and 8-byte aligned.
__device__ __forceinline__ uint64_t ta_tile_bits(const uint32_t* mrow, int k0, int nk) {
    if (!mrow) return ~0ull;
    const uint2 w = *reinterpret_cast<const uint2*>(mrow + (k0 >> 5));
    const uint64_t b = (uint64_t)w.y << 32 | w.x;
    const int left = nk - k0;
    return left >= 64 ? b : b & ((1ull << left) - 1);
}
template <bool MASK>
__device__ __forceinline__ bool ta_tile_skipped_m(const AttnView& v, int k0, const uint32_t* mrow) {
    if (ta_tile_skipped(v, k0)) return true;
    return MASK && ta_tile_bits(mrow, k0, v.nk) == 0;
}
template <bool MASK>
__device__ __forceinline__ int ta_next_tile_m(const AttnView& v, int k0, const uint32_t* mrow) {
    while (k0 < v.nk && ta_tile_skipped_m<MASK>(v, k0, mrow)) k0 += TA_T;
    return k0;
}

// the K | V tiles at key row k of view v, head h, into registers (attn_fwd_*, attn_dq_*), and the Q | dO tiles at query row q0 (attn_dkv_*).
// attn_fwd_* and attn_dq_* bind ta_fetch_kv to their registers in one local lambda and call that before and inside the loop: with the two sites calling
// it directly the compiler zeroed the 32 registers at each of them, 56 to 86 instructions more per kernel (profiles/train_shared_ab.txt).
__device__ __forceinline__ void ta_fetch_kv(f32x4 (&rk)[4], f32x4 (&rv)[4], const TaArgs& a, const AttnView& v, int k, int h, int tid) {
    ta_fetch_tile(rk, a.K + (size_t)(v.kv_row0 + k) * a.ldk + h * TA_T, a.ldk, v.nk - k, tid);
    ta_fetch_tile(rv, a.V + (size_t)(v.kv_row0 + k) * a.ldv + h * TA_T, a.ldv, v.nk - k, tid);
}
__device__ __forceinline__ void ta_fetch_qdo(f32x4 (&rq)[4], f32x4 (&rd)[4], const TaArgs& a, const AttnView& v, int q0, int h, int tid) {
    ta_fetch_tile(rq, a.Q + (size_t)(v.q_row0 + q0) * a.ldq + h * TA_T, a.ldq, v.nq - q0, tid);
    ta_fetch_tile(rd, a.dO + (size_t)(v.q_row0 + q0) * a.lddo + h * TA_T, a.lddo, v.nq - q0, tid);
}

// The walk of attn_dkv_* over its key group g for the key tile at k0: views in table order, each view's query tiles in row order.  One call moves
// (vi, q0, v, mb) to the next (view, query tile) pair; start from vi = -1, and vi == g.count is the end.  A view without queries, or whose key range or skip
// range leaves nothing of the tile, is passed over; so is, with MASK, a view whose mask dropped the whole tile (mb, its mask bits of this key tile, is 0),
// before any of its Q / dO tiles is fetched.  The kernels take their steps ahead of the products in this order and add in it: the fixed order of additions
// of dK and dV, without atomics, is this function.
template <bool MASK>
__device__ __forceinline__ void ta_walk_next(const TaArgs& a, const TaGroup& g, int k0, int& vi, int& q0, AttnView& v, uint64_t& mb) {
    if (vi >= 0 && q0 + TA_T < v.nq) { q0 += TA_T; return; }
    q0 = 0;
    for (++vi; vi < g.count; ++vi) {
        const int id = a.list[g.first + vi];
        v = a.views[id];
        if (v.nq > 0 && !ta_tile_skipped(v, k0)) {
            if (!MASK) return;
            mb = ta_tile_bits(ta_mask_row<MASK>(a, id), k0, v.nk);
            if (mb) return;
        }
    }
}

// The three kernels of one family and instantiation, as ta_forward / ta_grad launch them: over the same arguments, grids and 256-thread blocks.
struct TaKernels {
    void (*fwd)(TaArgs);
    void (*dkv)(TaArgs);
    void (*dq)(TaArgs);
};
// train_attn16.hip: the calling thread's mode is MUST3R_TRAIN_ATTENTION_BF16 (must3r_hip_train_attention_mode), and the bf16 kernels; `masked` picks the
// MASK instantiations.
bool train_attention_bf16();
TaKernels ta_kernels_bf16(bool masked);

}  // namespace m3r
