// Device code that the training kernels share, fp32 and bf16 alike: the guarded 16-byte load, the zeroing of a wave's accumulators, the walk over a wave's
// 64 x 64 of a 128 x 128 / four-wave tile (linear_fwd_*, dgrad_*, wgrad_*), and the fragment code of the 16-bit MFMA (train_lin16.hip, train_attn16.hip).
// Everything here is forced inline and takes what it needs as values, so that a kernel's arguments reach its stores as the kernel itself wrote them.
#pragma once
#include "common.hpp"

namespace m3r {

// a tail is filled by a select on the load: nothing is read through p where ok is false
__device__ __forceinline__ f32x4 ld4_or_zero(const float* p, bool ok) { return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ bf16x8 cat8(bf16x4 lo, bf16x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

__device__ __forceinline__ void zero_acc(f32x4 (&x)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Four fragments of the 16-bit MFMA from a bf16 tile in LDS that lies [contraction][free] with rows of LD elements, transposed by the read: a fragment is two
// ds_read_b64_tr_b16 (common.hpp lds_read_tr4_x8).  p is the lane's chunk of fragment 0: row 4 (lane >> 4) + ((lane & 15) >> 2) of the 32-row step, columns
// 4 (lane & 3) ... + 3 of the fragment's sixteen; f[t] covers the free indices 16 t ... 16 t + 15 from there.
// The row-permutation contract: lane group g = lane >> 4 receives the tile rows 4 g ... 4 g + 3 and 16 + 4 g ... 16 + 4 g + 3 as its 8 contraction indices, not
// 8 g ... 8 g + 7.  A sum of products does not depend on the order of its terms' indices as long as BOTH operands of the MFMA name the same 8 rows per lane
// group: the other operand is read with frag_tr4 too (wgrad_bf16), or by rows as two 8-byte reads at 4 g and 16 + 4 g (dgrad_bf16), or is an accumulator of a
// product that left exactly these rows in the lane group (tb_pack of train_attn16.hip).
template <int LD>
__device__ __forceinline__ void frag_tr4(const bf16_t* p, bf16x8 (&f)[4]) {
    bf16x4 h[8];
    lds_read_tr4_x8<bf16_t>(p, p + 16 * LD, p + 16, p + 16 * LD + 16, p + 32, p + 16 * LD + 32, p + 48, p + 16 * LD + 48, h);
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = cat8(h[2 * t], h[2 * t + 1]);
}

// f(m, n, j, x) for every element x = acc[i][j][r] of a wave's 64 x 64 (4 x 4 accumulators of 16 x 16, origin (m0, n0)) that lies inside [0, M) x [0, N).
// C/D map of the 16 x 16 MFMAs: row 4 fk + r, column fr, with fr = lane & 15 and fk = lane >> 4 -- the kernel's own values: derived a second time here from
// the lane they changed the register allocation of wgrad_kernel's loop, 5 % on its largest partials (profiles/train_shared_ab.txt).  j, the column block,
// lets f use a per-column value loaded once (a bias).
// f is taken by value and must capture by value ([=]): through a reference the compiler no longer knows that a kernel's __restrict__ arguments do not alias
// and recomputes every row address after each store.
template <class F>
__device__ __forceinline__ void for_each_acc64(const f32x4 (&acc)[4][4], int m0, int n0, int M, int N, int fr, int fk, F f) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + i * 16 + fk * 4 + r;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + j * 16 + fr;
                if (n < N) f(m, n, j, acc[i][j][r]);
            }
        }
}

}  // namespace m3r
