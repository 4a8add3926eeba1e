// Checkpoint evaluation and the tail of a training step (eval.py:133-150; must3r/engine/losses.py Regr3D / ConfLoss;
// must3r/tools/geometry.py normalize_pointcloud): masked reductions over [B, V, H, W] pointmaps, and the gradient of the loss figures at
// the predictions (closed form, include/must3r_hip.h ABI 16), which recomputes the forward's per-pixel chain instead of saving it.
//
//   metrics_loss_kernel<PIX>    grid (blocks per view, B V): thread t of a block owns pixels 4t .. 4t+3 of a 1024-pixel chunk and walks the
//                               view in steps of gridDim.x chunks.  The mask bytes are read first; the points of a 4-pixel group with no
//                               selected pixel are not read at all.  Rigid transforms, scales, warp, log map and the L21 distance in fp32
//                               with every operation rounded (this file is built with -ffp-contract=off); sums in fp64 per thread, then
//                               wave (xor butterfly) and block (LDS, wave order) -> slab[view][block][6].  PIX: also the per-pixel values.
//   metrics_loss_final_kernel   one thread per view adds the view's partials in block order -> counts int64 [2], sums fp64 [4]
//   metrics_factor_kernel<MODE> grid (blocks per scene, B): the same walk over the V H W pixels of a scene; sum of d, log1p(d) or sqrt(d)
//                               over the valid pixels.  MEDIAN: writes d (NaN where not selected) and counts the top 11 bits of its pattern.
//   metrics_hist_kernel         radix-select passes 2 and 3 over the stored distances: the patterns that share the prefix found so far
//   metrics_select_kernel       one block per scene: the bin that holds the wanted rank -> longer prefix, smaller rank; clears the bins
//   metrics_factor_final_kernel one thread per scene: partials in block order -> norm_factor fp32, clipped at 1e-8
//   metrics_count_total_kernel  one block: the batch totals N_g, N_l of the forward's counts (integer sums) for the 'mean' weightings
//   metrics_grad_kernel<false>  the forward's walk; per block the fp64 sums of <g_y, y> of the global and of the local term at unit upstream
//                               weight -> slab[view][block][2]; blocks of scenes without a factor of their own return at once
//   metrics_scale_final_kernel  one thread per scene: partials in view / block order -> -(sum) / (pr_scale (n_b + 1e-8)) per term, the
//                               factor of the scale path that does not depend on the pixel (0 for scenes without one)
//   metrics_grad_kernel<true>   the forward's walk; direct term, scale-path term and conf gradient of 4 pixels per thread, every element
//                               of the outputs stored once (16-byte stores where aligned), zeros included
//
// Nothing here uses floating-point atomics; the histograms use integer ones, whose result does not depend on their order.  The block
// count of a view (scene) depends on H W (V H W) alone, so a scene's figures do not depend on the rest of the batch.
#include <cstdint>
#include "abi.hpp"
#include "common.hpp"

namespace m3r {
namespace {

constexpr int MET_T = 256;                       // threads per block
constexpr int MET_CHUNK = MET_T * 4;             // pixels per block and step
constexpr int MET_VIEW_BLOCKS = 32;              // at most, per view
constexpr int MET_SCENE_BLOCKS = 128;            // at most, per scene
constexpr int RS_BINS = 2048;

struct LossDev {
    must3r_hip_metrics_loss_args a;
    unsigned n_pix;
};

__device__ __forceinline__ void ld12(const float* __restrict__ q, const unsigned i, const unsigned n, float (&o)[12]) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 v = reinterpret_cast<const float4*>(q)[j];
            o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) o[j] = i + j / 3 < n ? q[j] : 0.f;
    }
}

__device__ __forceinline__ void ld4(const float* __restrict__ q, const unsigned i, const unsigned n, float (&o)[4]) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
        const float4 v = *reinterpret_cast<const float4*>(q);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = i + j < n ? q[j] : 0.f;
    }
}

// four mask bytes at q (pixel i of n): packed little-endian, 0 past the end
__device__ __forceinline__ unsigned ld4b(const unsigned char* __restrict__ q, const unsigned i, const unsigned n) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 3) == 0)) return *reinterpret_cast<const unsigned*>(q);
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (i + j < n ? (unsigned)q[j] : 0u) << (8 * j);
    return r;
}

__device__ __forceinline__ void st4f(float* __restrict__ q, const unsigned i, const unsigned n, const float (&v)[4]) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
        *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (i + j < n) q[j] = v[j];
    }
}

__device__ __forceinline__ float norm3(const float x, const float y, const float z) { return sqrtf((x * x + y * y) + z * z); }

// rows 0..2 of a row-major 4x4
__device__ __forceinline__ void rigid(const float (&T)[12], const float x, const float y, const float z, float (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
}

// normalize_pointcloud's warp and scale: x * (log1p(d) / max(d, 1e-8)) when warp, then / scale
__device__ __forceinline__ void warp_scale(float (&p)[3], const bool warp, const float scale) {
    if (warp) {
        const float d = norm3(p[0], p[1], p[2]);
        const float f = log1pf(d) / fmaxf(d, 1e-8f);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] *= f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] /= scale;
}

// apply_log_to_norm
__device__ __forceinline__ void log_map(float (&p)[3]) {
    const float d = norm3(p[0], p[1], p[2]);
    const float c = fmaxf(d, 1e-8f), l = log1pf(d);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = p[k] / c * l;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block total of K per-thread values in lane / wave order -> out[k] (thread 0 writes); s: K * MET_T / 64 doubles of LDS
template <int K>
__device__ __forceinline__ void block_sum_store(const double (&v)[K], double* s, double* __restrict__ out) {
    const unsigned wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum_f64(v[k]);
        if ((threadIdx.x & 63) == 0) s[wave * K + k] = w;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double r = s[threadIdx.x];
#pragma unroll
        for (int w = 1; w < MET_T / 64; ++w) r += s[w * K + threadIdx.x];
        out[threadIdx.x] = r;
    }
}

template <bool PIX>
__global__ void __launch_bounds__(MET_T) metrics_loss_kernel(const LossDev p, double* __restrict__ slab) {
    __shared__ double s_red[6 * MET_T / 64];
    const must3r_hip_metrics_loss_args& a = p.a;
    const unsigned bv = blockIdx.y, b = bv / (unsigned)a.n_views, n = p.n_pix;
    const size_t base = (size_t)bv * n;
    const bool local = a.pr_local != nullptr, use_sky = a.sky != nullptr && a.sky_loss_value > 0.f, has_conf = a.conf != nullptr;
    float T0[12], T1[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        T0[k] = a.in_camera0[16 * (size_t)b + k];
        T1[k] = local ? a.w2c[16 * (size_t)bv + k] : 0.f;
    }
    const float gs = a.gt_scale ? a.gt_scale[b] : 1.f, ps = a.pr_scale ? a.pr_scale[b] : 1.f;
    const bool gwarp = a.gt_warp != 0, pwarp = a.pr_warp && a.pr_warp[b] != 0;
    const bool log_g = a.loss_in_log != 0, log_l = a.loss_in_log == 1;
    double acc[6] = {0, 0, 0, 0, 0, 0};           // l global, l local, cl global, cl local, count global, count local
    for (unsigned i0 = (blockIdx.x * MET_T + threadIdx.x) * 4; i0 < n; i0 += gridDim.x * MET_CHUNK) {
        const unsigned vm = ld4b(a.valid + base + i0, i0, n);
        const unsigned sm = use_sky ? ld4b(a.sky + base + i0, i0, n) : 0u;
        float og[4], ol[4];
        unsigned mg = 0, ml = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) og[j] = ol[j] = __uint_as_float(0x7fc00000u);
        if (vm | sm) {
            float g[12], q[12], ql[12], c[4];
            // ground truth is only needed (and only trusted) under the valid mask
            if (vm) ld12(a.gt_pts + 3 * (base + i0), i0, n, g);
            if (vm) ld12(a.pr_pts + 3 * (base + i0), i0, n, q);
            if (vm && local) ld12(a.pr_local + 3 * (base + i0), i0, n, ql);
            if (has_conf) ld4(a.conf + base + i0, i0, n, c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool v = (vm >> (8 * j)) & 0xff, s = (sm >> (8 * j)) & 0xff;
                if (!v && !s) continue;
                float wg[3] = {0.f, 0.f, 0.f}, wl[3] = {0.f, 0.f, 0.f};
                bool vg = v, vl = v;
                if (v) {
                    rigid(T0, g[3 * j], g[3 * j + 1], g[3 * j + 2], wg);
                    if (a.has_dist_clip) vg = norm3(wg[0], wg[1], wg[2]) <= a.dist_clip;
                    if (local) {
                        rigid(T1, g[3 * j], g[3 * j + 1], g[3 * j + 2], wl);
                        if (a.has_dist_clip) vl = norm3(wl[0], wl[1], wl[2]) <= a.dist_clip;
                    }
                }
                const bool sg = s && !vg, sl = s && !vl;
                const float cj = has_conf ? c[j] : 1.f;
                const float lc = has_conf ? a.alpha * logf(cj) : 0.f;
                if (vg || sg) {
                    float l = a.sky_loss_value;
                    if (!sg) {
                        float pr[3] = {q[3 * j], q[3 * j + 1], q[3 * j + 2]};
                        warp_scale(wg, gwarp, gs);
                        warp_scale(pr, pwarp, ps);
                        if (log_g) { log_map(wg); log_map(pr); }
                        l = norm3(pr[0] - wg[0], pr[1] - wg[1], pr[2] - wg[2]);
                    }
                    acc[0] += (double)l;
                    if (has_conf) acc[2] += (double)(l * cj - lc);
                    acc[4] += 1.0;
                    og[j] = l;
                    mg |= 1u << (8 * j);
                }
                if (local && (vl || sl)) {
                    float l = a.sky_loss_value;
                    if (!sl) {
                        float pr[3] = {ql[3 * j], ql[3 * j + 1], ql[3 * j + 2]};
                        warp_scale(wl, false, gs);
                        warp_scale(pr, false, ps);
                        if (log_l) { log_map(wl); log_map(pr); }
                        l = norm3(pr[0] - wl[0], pr[1] - wl[1], pr[2] - wl[2]);
                    }
                    acc[1] += (double)l;
                    if (has_conf) acc[3] += (double)(l * cj - lc);
                    acc[5] += 1.0;
                    ol[j] = l;
                    ml |= 1u << (8 * j);
                }
            }
        }
        if (PIX) {
            st4f(a.pix_g + base + i0, i0, n, og);
            st4f(a.pix_l + base + i0, i0, n, ol);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j < n) {
                    a.msk_g[base + i0 + j] = (unsigned char)((mg >> (8 * j)) & 1u);
                    a.msk_l[base + i0 + j] = (unsigned char)((ml >> (8 * j)) & 1u);
                }
            }
        }
    }
    block_sum_store<6>(acc, s_red, slab + ((size_t)bv * gridDim.x + blockIdx.x) * 6);
}

__global__ void __launch_bounds__(64) metrics_loss_final_kernel(const double* __restrict__ slab, const int n_bv, const int n_blocks,
                                                                long long* __restrict__ counts, double* __restrict__ sums) {
    const int bv = blockIdx.x * 64 + threadIdx.x;
    if (bv >= n_bv) return;
    double r[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n_blocks; ++k) {
#pragma unroll
        for (int j = 0; j < 6; ++j) r[j] += slab[((size_t)bv * n_blocks + k) * 6 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sums[4 * (size_t)bv + j] = r[j];
    counts[2 * (size_t)bv] = (long long)r[4];
    counts[2 * (size_t)bv + 1] = (long long)r[5];
}

struct SelState {                                // radix select, per scene
    unsigned prefix;
    unsigned pad;
    unsigned long long rank, count;
};

// MODE: MUST3R_NORM_*
template <int MODE>
__global__ void __launch_bounds__(MET_T) metrics_factor_kernel(const float* __restrict__ pts, const float* __restrict__ trf,
                                                               const unsigned char* __restrict__ valid, const unsigned n,
                                                               float* __restrict__ dist, double* __restrict__ slab,
                                                               unsigned* __restrict__ hist) {
    constexpr bool MEDIAN = MODE == MUST3R_NORM_MEDIAN_DIS;
    __shared__ double s_red[2 * MET_T / 64];
    __shared__ unsigned s_hist[MEDIAN ? RS_BINS : 1];
    const unsigned b = blockIdx.y;
    const size_t base = (size_t)b * n;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = trf ? trf[16 * (size_t)b + k] : 0.f;
    if (MEDIAN) {
        for (int k = threadIdx.x; k < RS_BINS; k += MET_T) s_hist[k] = 0;
        __syncthreads();
    }
    double acc[2] = {0, 0};
    for (unsigned i0 = (blockIdx.x * MET_T + threadIdx.x) * 4; i0 < n; i0 += gridDim.x * MET_CHUNK) {
        const unsigned vm = ld4b(valid + base + i0, i0, n);
        float od[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) od[j] = __uint_as_float(0x7fc00000u);
        if (vm) {
            float g[12];
            ld12(pts + 3 * (base + i0), i0, n, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((vm >> (8 * j)) & 0xff)) continue;
                float w[3] = {g[3 * j], g[3 * j + 1], g[3 * j + 2]};
                if (trf) rigid(T, g[3 * j], g[3 * j + 1], g[3 * j + 2], w);
                const float d = norm3(w[0], w[1], w[2]);
                if (MODE == MUST3R_NORM_AVG_DIS) { acc[0] += (double)d; acc[1] += 1.0; }
                if (MODE == MUST3R_NORM_AVG_LOG1P) { acc[0] += (double)log1pf(d); acc[1] += 1.0; }
                // nanmean / nanmedian skip the NaN distances of valid pixels too
                if (MODE == MUST3R_NORM_SQRT_DIS && d == d) { acc[0] += (double)sqrtf(d); acc[1] += 1.0; }
                if (MEDIAN && d == d) {
                    od[j] = d;
                    atomicAdd(&s_hist[__float_as_uint(d) >> 21], 1u);
                }
            }
        }
        if (MEDIAN) st4f(dist + base + i0, i0, n, od);
    }
    if (MEDIAN) {
        __syncthreads();
        for (int k = threadIdx.x; k < RS_BINS; k += MET_T) {
            const unsigned c = s_hist[k];
            if (c) atomicAdd(&hist[(size_t)b * RS_BINS + k], c);
        }
    } else {
        block_sum_store<2>(acc, s_red, slab + ((size_t)b * gridDim.x + blockIdx.x) * 2);
    }
}

// distances whose pattern >> (shift + bits) equals the scene's prefix: count bin (pattern >> shift) & (2^bits - 1)
__global__ void __launch_bounds__(MET_T) metrics_hist_kernel(const float* __restrict__ dist, const unsigned n, const SelState* __restrict__ state,
                                                             const int shift, const int bits, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[RS_BINS];
    const unsigned b = blockIdx.y;
    const size_t base = (size_t)b * n;
    const unsigned prefix = state[b].prefix, mask = (1u << bits) - 1u;
    for (int k = threadIdx.x; k < RS_BINS; k += MET_T) s_hist[k] = 0;
    __syncthreads();
    for (unsigned i0 = (blockIdx.x * MET_T + threadIdx.x) * 4; i0 < n; i0 += gridDim.x * MET_CHUNK) {
        float d[4];
        ld4(dist + base + i0, i0, n, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = __float_as_uint(d[j]);
            if (i0 + j < n && d[j] == d[j] && (u >> (shift + bits)) == prefix) atomicAdd(&s_hist[(u >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < RS_BINS; k += MET_T) {
        const unsigned c = s_hist[k];
        if (c) atomicAdd(&hist[(size_t)b * RS_BINS + k], c);
    }
}

// first: the rank wanted is that of the lower median of all counted elements
__global__ void __launch_bounds__(MET_T) metrics_select_kernel(unsigned* __restrict__ hist, SelState* __restrict__ state, const int bits,
                                                               const int first) {
    constexpr int PER = RS_BINS / MET_T;
    __shared__ unsigned long long s_pre[MET_T + 1];
    unsigned* h = hist + (size_t)blockIdx.x * RS_BINS;
    unsigned c[PER];
    unsigned long long tot = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = h[threadIdx.x * PER + k]; tot += c[k]; }
    s_pre[threadIdx.x + 1] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        s_pre[0] = 0;
        for (int t = 1; t <= MET_T; ++t) s_pre[t] += s_pre[t - 1];
    }
    __syncthreads();
    SelState st = state[blockIdx.x];
    if (first) {
        st.count = s_pre[MET_T];
        st.rank = st.count ? (st.count - 1) / 2 : 0;
        st.prefix = 0;
    }
    __syncthreads();                               // every thread has read the state
    if (st.count && s_pre[threadIdx.x] <= st.rank && st.rank < s_pre[threadIdx.x + 1]) {
        unsigned long long cum = s_pre[threadIdx.x];
        int k = 0;
        while (cum + c[k] <= st.rank) { cum += c[k]; ++k; }
        st.prefix = (st.prefix << bits) | (unsigned)(threadIdx.x * PER + k);
        st.rank -= cum;
        st.pad = 0;
        state[blockIdx.x] = st;
    } else if (!st.count && threadIdx.x == 0) {
        st.pad = 0;
        state[blockIdx.x] = st;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) h[threadIdx.x * PER + k] = 0;
}

__global__ void __launch_bounds__(64) metrics_factor_final_kernel(const double* __restrict__ slab, const SelState* __restrict__ state,
                                                                  const int n_scenes, const int n_blocks, const int mode,
                                                                  float* __restrict__ factor) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_scenes) return;
    float f;
    if (mode == MUST3R_NORM_MEDIAN_DIS) {
        f = state[b].count ? __uint_as_float(state[b].prefix) : __uint_as_float(0x7fc00000u);
    } else {
        double s = 0, c = 0;
        for (int k = 0; k < n_blocks; ++k) { s += slab[((size_t)b * n_blocks + k) * 2]; c += slab[((size_t)b * n_blocks + k) * 2 + 1]; }
        if (mode == MUST3R_NORM_SQRT_DIS) {
            const float m = (float)(s / c);          // 0 / 0 = NaN, as nanmean of nothing
            f = m * m;
        } else {
            f = (float)(s / (c + 1e-8));
        }
    }
    factor[b] = f < 1e-8f ? 1e-8f : f;             // clip(min=1e-8); NaN stays NaN
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
struct GradDev {
    must3r_hip_metrics_loss_args a;
    must3r_hip_metrics_loss_grad_args g;
    unsigned n_pix;
    const long long* totals;                     // [2] batch totals of counts (W_MEAN / W_CONF)
    const float* scale_co;                       // [B][2] metrics_scale_final_kernel's output, or nullptr: no scale path
};

__device__ __forceinline__ void st12(float* __restrict__ q, const unsigned i, const unsigned n, const float (&v)[12]) {
    if (i + 4 <= n && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) reinterpret_cast<float4*>(q)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) if (i + j / 3 < n) q[j] = v[j];
    }
}

// v <- J(x) v, J the Jacobian of x -> x / max(|x|, 1e-8) * log1p(|x|): (log1p(d) / d)(I - x^ x^T) + x^ x^T / (1 + d), symmetric; below the
// clip the derivative of the clipped expression, 0 at d = 0
__device__ __forceinline__ void log_map_jac(const float (&x)[3], float (&v)[3]) {
    const float d = norm3(x[0], x[1], x[2]);
    if (d == 0.f) { v[0] = v[1] = v[2] = 0.f; return; }
    const float c = fmaxf(d, 1e-8f);
    const float h = log1pf(d) / c;
    const float b = d >= 1e-8f ? 1.f / (1.f + d) - h : d / (c * (1.f + d));
    const float s = ((x[0] * v[0] + x[1] * v[1]) + x[2] * v[2]) / d * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = h * v[k] + s * (x[k] / d);
}

// One regression term of one pixel, forward and backward: x the prediction as stored, t the ground truth in the term's frame (before
// warp and scale), w the weight of the term's loss.  Returns l = |y' - t'| as the forward computes it; gx = dl/dx w (direct term) and
// dot = <g_y, y> with y = warp(x) / ps and g_y the gradient at y (the scale path's summand).
__device__ __forceinline__ float term_grad(const float (&x)[3], float (&t)[3], const bool pwarp, const bool gwarp, const float ps, const float gs,
                                           const bool lg, const float w, float (&gx)[3], float& dot) {
    float y[3] = {x[0], x[1], x[2]};
    warp_scale(t, gwarp, gs);
    warp_scale(y, pwarp, ps);
    float yl[3] = {y[0], y[1], y[2]};
    if (lg) { log_map(t); log_map(yl); }
    const float r[3] = {yl[0] - t[0], yl[1] - t[1], yl[2] - t[2]};
    const float l = norm3(r[0], r[1], r[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] = l == 0.f ? 0.f : w * (r[k] / l);          // the norm's subgradient at 0 is 0, as torch has it
    if (lg) log_map_jac(y, gx);
    dot = (gx[0] * y[0] + gx[1] * y[1]) + gx[2] * y[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] /= ps;
    if (pwarp) log_map_jac(x, gx);
    return l;
}

__global__ void __launch_bounds__(MET_T) metrics_count_total_kernel(const long long* __restrict__ counts, const int n_bv, long long* __restrict__ totals) {
    __shared__ long long s[2 * MET_T];
    long long g = 0, l = 0;
    for (int k = threadIdx.x; k < n_bv; k += MET_T) { g += counts[2 * (size_t)k]; l += counts[2 * (size_t)k + 1]; }
    s[2 * threadIdx.x] = g;
    s[2 * threadIdx.x + 1] = l;
    __syncthreads();
    if (threadIdx.x < 2) {
        long long r = 0;
        for (int k = 0; k < MET_T; ++k) r += s[2 * k + threadIdx.x];
        totals[threadIdx.x] = r;
    }
}

// GRAD false: the scale path's sums (slab [view][block][2]); true: the gradients
template <bool GRAD>
__global__ void __launch_bounds__(MET_T) metrics_grad_kernel(const GradDev p, double* __restrict__ slab) {
    __shared__ double s_red[2 * MET_T / 64];
    const must3r_hip_metrics_loss_args& a = p.a;
    const must3r_hip_metrics_loss_grad_args& ga = p.g;
    const unsigned bv = blockIdx.y, b = bv / (unsigned)a.n_views, n = p.n_pix;
    const size_t base = (size_t)bv * n;
    const bool own = ga.n_own > 0 && ga.own_factor[b] != 0;
    if (!GRAD && !own) return;                    // metrics_scale_final_kernel does not read this scene's partials
    const bool local = a.pr_local != nullptr, use_sky = a.sky != nullptr && a.sky_loss_value > 0.f;
    const int wm = ga.weighting;
    const bool wconf = wm == MUST3R_LOSS_W_CONF, wpix = wm == MUST3R_LOSS_W_PIXEL;
    float T0[12], T1[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        T0[k] = a.in_camera0[16 * (size_t)b + k];
        T1[k] = local ? a.w2c[16 * (size_t)bv + k] : 0.f;
    }
    const float gs = a.gt_scale ? a.gt_scale[b] : 1.f, ps = a.pr_scale ? a.pr_scale[b] : 1.f;
    const bool gwarp = a.gt_warp != 0, pwarp = a.pr_warp && a.pr_warp[b] != 0;
    const bool log_g = a.loss_in_log != 0, log_l = a.loss_in_log == 1;
    // unit weights of the two terms (everything but the upstream scalars), and the upstream scalars, applied last
    float ug = 1.f, ul = 1.f, wg = 1.f, wl = 1.f;
    if (wm == MUST3R_LOSS_W_MEAN || wconf) {
        const long long ng = p.totals[0], nl = p.totals[1];
        ug = ng > 0 ? 1.f / (float)ng : 0.f;
        ul = nl > 0 ? 1.f / (float)nl : 0.f;
    }
    if (!wpix) { wg = ga.w_g[0]; wl = local ? ga.w_l[0] : wg; }
    const bool same = wg == wl;
    float sg_co = 0.f, sl_co = 0.f;               // the scale path's per-scene factors
    if (GRAD && own && p.scale_co) { sg_co = p.scale_co[2 * b]; sl_co = p.scale_co[2 * b + 1]; }
    const bool scale_path = sg_co != 0.f || sl_co != 0.f;
    double acc[2] = {0, 0};
    for (unsigned i0 = (blockIdx.x * MET_T + threadIdx.x) * 4; i0 < n; i0 += gridDim.x * MET_CHUNK) {
        const unsigned vm = ld4b(a.valid + base + i0, i0, n);
        const unsigned sm = GRAD && use_sky ? ld4b(a.sky + base + i0, i0, n) : 0u;
        float op[12], ol[12], oc[4];
#pragma unroll
        for (int j = 0; j < 12; ++j) op[j] = ol[j] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) oc[j] = 0.f;
        if (vm | (GRAD ? sm : 0u)) {
            float g[12], q[12], ql[12], c[4], pwg[4], pwl[4];
            if (vm) ld12(a.gt_pts + 3 * (base + i0), i0, n, g);
            if (vm) ld12(a.pr_pts + 3 * (base + i0), i0, n, q);
            if (vm && local) ld12(a.pr_local + 3 * (base + i0), i0, n, ql);
            if (wconf) ld4(a.conf + base + i0, i0, n, c);
            if (wpix && vm) {
                ld4(ga.w_g + base + i0, i0, n, pwg);
                if (local) ld4(ga.w_l + base + i0, i0, n, pwl);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool v = (vm >> (8 * j)) & 0xff, s = (sm >> (8 * j)) & 0xff;
                if (!v && !s) continue;
                float tg[3] = {0.f, 0.f, 0.f}, tl[3] = {0.f, 0.f, 0.f};
                bool vg = v, vl = v;
                if (v) {
                    rigid(T0, g[3 * j], g[3 * j + 1], g[3 * j + 2], tg);
                    if (a.has_dist_clip) vg = norm3(tg[0], tg[1], tg[2]) <= a.dist_clip;
                    if (local) {
                        rigid(T1, g[3 * j], g[3 * j + 1], g[3 * j + 2], tl);
                        if (a.has_dist_clip) vl = norm3(tl[0], tl[1], tl[2]) <= a.dist_clip;
                    }
                }
                const bool sg = s && !vg, sl = s && !vl;
                const float cj = wconf ? c[j] : 1.f;
                float dp[3] = {0.f, 0.f, 0.f}, dl[3] = {0.f, 0.f, 0.f}, cg = 0.f, cl = 0.f;
                if (vg) {
                    const float x[3] = {q[3 * j], q[3 * j + 1], q[3 * j + 2]};
                    const float w = wpix ? pwg[j] : (wconf ? ug * cj : ug);
                    float dot;
                    const float l = term_grad(x, tg, pwarp, gwarp, ps, gs, log_g, w, dp, dot);
                    acc[0] += (double)dot;
                    if (wconf) cg = (l - a.alpha / cj) * ug;
                } else if (sg && wconf) {
                    cg = (a.sky_loss_value - a.alpha / cj) * ug;
                }
                if (local && vl) {
                    const float x[3] = {ql[3 * j], ql[3 * j + 1], ql[3 * j + 2]};
                    const float w = wpix ? pwl[j] : (wconf ? ul * cj : ul);
                    float dot;
                    const float l = term_grad(x, tl, false, false, ps, gs, log_l, w, dl, dot);
                    acc[1] += (double)dot;
                    if (wconf) cl = (l - a.alpha / cj) * ul;
                } else if (local && sl && wconf) {
                    cl = (a.sky_loss_value - a.alpha / cj) * ul;
                }
                if (GRAD) {
                    float dir[3] = {0.f, 0.f, 0.f};  // dps/dx without its per-scene factor, on every valid pixel (within the clip or not)
                    if (v && scale_path) {
                        const float x[3] = {q[3 * j], q[3 * j + 1], q[3 * j + 2]};
                        const float d = norm3(x[0], x[1], x[2]);
                        if (d != 0.f) {
                            const float f = ga.factor_mode == MUST3R_NORM_AVG_DIS ? 1.f : (ga.factor_mode == MUST3R_NORM_AVG_LOG1P ? 1.f + d : sqrtf(d));
#pragma unroll
                            for (int k = 0; k < 3; ++k) dir[k] = x[k] / d / f;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        op[3 * j + k] = same ? wg * (dp[k] + (sg_co + sl_co) * dir[k]) : wg * (dp[k] + sg_co * dir[k]) + wl * (sl_co * dir[k]);
                        ol[3 * j + k] = wl * dl[k];
                    }
                    oc[j] = same ? wg * (cg + cl) : wg * cg + wl * cl;
                }
            }
        }
        if (GRAD) {
            st12(ga.grad_pts + 3 * (base + i0), i0, n, op);
            if (local) st12(ga.grad_local + 3 * (base + i0), i0, n, ol);
            if (ga.grad_conf) st4f(ga.grad_conf + base + i0, i0, n, oc);
        }
    }
    if (!GRAD) block_sum_store<2>(acc, s_red, slab + ((size_t)bv * gridDim.x + blockIdx.x) * 2);
}

__global__ void __launch_bounds__(64) metrics_scale_final_kernel(const double* __restrict__ slab, const int n_scenes, const int n_views,
                                                                 const int n_blocks, const int mode, const unsigned char* __restrict__ own,
                                                                 const long long* __restrict__ n_valid, const float* __restrict__ pr_scale,
                                                                 float* __restrict__ scale_co) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_scenes) return;
    double r[2] = {0, 0};
    const float ps = pr_scale[b];
    const long long nv = n_valid[b];
    if (own[b] && nv > 0 && ps > 1e-8f) {          // a factor at the clip has zero derivative
        double s[2] = {0, 0};
        const size_t k0 = (size_t)b * n_views * n_blocks;
        for (size_t k = 0; k < (size_t)n_views * n_blocks; ++k) { s[0] += slab[(k0 + k) * 2]; s[1] += slab[(k0 + k) * 2 + 1]; }
        // S_b = -sum / ps, times the part of dps/dx that is the same for every pixel of the scene
        const double co = mode == MUST3R_NORM_SQRT_DIS ? sqrt((double)ps) / (double)nv : 1.0 / ((double)nv + 1e-8);
        r[0] = -s[0] / (double)ps * co;
        r[1] = -s[1] / (double)ps * co;
    }
    scale_co[2 * (size_t)b] = (float)r[0];
    scale_co[2 * (size_t)b + 1] = (float)r[1];
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int blocks_for(long long n, int cap) {
    const long long c = (n + MET_CHUNK - 1) / MET_CHUNK;
    return (int)(c < cap ? c : cap);
}

int check_sizes(const char* who, int n_scenes, int n_views, int H, int W) {
    const char* what = nullptr;
    if (n_scenes <= 0) what = "n_scenes must be positive";
    else if (n_views <= 0) what = "n_views must be positive";
    else if (H <= 0 || W <= 0) what = "H and W must be positive";
    else if ((long long)n_views * H * W >= (1LL << 31)) what = "a scene has 2^31 or more pixels";
    else if ((long long)n_scenes * n_views > 65535) what = "more than 65535 views in a batch";
    return what ? fail("%s: %s", who, what) : 0;
}

struct GradPlan { int n_blocks; size_t off_co, off_slab, bytes; };

void grad_plan(int n_scenes, int n_views, int H, int W, GradPlan* p) {
    p->n_blocks = blocks_for((long long)H * W, MET_VIEW_BLOCKS);
    p->off_co = align256(2 * sizeof(long long));                                  // after the two totals
    p->off_slab = align256(p->off_co + (size_t)n_scenes * 2 * sizeof(float));
    p->bytes = align256(p->off_slab + (size_t)n_scenes * n_views * p->n_blocks * 2 * sizeof(double));
}

struct FactorPlan { int n_blocks; size_t off_hist, off_state, bytes; };

void factor_plan(int n_scenes, int n_views, int H, int W, FactorPlan* p) {
    p->n_blocks = blocks_for((long long)n_views * H * W, MET_SCENE_BLOCKS);
    size_t off = align256((size_t)n_scenes * p->n_blocks * 2 * sizeof(double));
    p->off_hist = off;
    off = align256(off + (size_t)n_scenes * RS_BINS * sizeof(unsigned));
    p->off_state = off;
    off = align256(off + (size_t)n_scenes * sizeof(SelState));
    p->bytes = off;
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_metrics_loss_scratch_bytes(int n_scenes, int n_views, int H, int W) {
    if (check_sizes("metrics_loss", n_scenes, n_views, H, W)) return 0;
    return align256((size_t)n_scenes * n_views * blocks_for((long long)H * W, MET_VIEW_BLOCKS) * 6 * sizeof(double));
}

extern "C" int must3r_hip_metrics_loss(const must3r_hip_metrics_loss_args* a, void* scratch, size_t scratch_bytes, void* stream) {
    if (!a) return fail("metrics_loss: null argument block");
    if (check_sizes("metrics_loss", a->n_scenes, a->n_views, a->H, a->W)) return 1;
    if (!a->gt_pts || !a->in_camera0 || !a->pr_pts || !a->valid || !a->counts || !a->sums || !scratch) return fail("metrics_loss: null argument");
    if (a->pr_local && !a->w2c) return fail("metrics_loss: the local term needs w2c");
    if (a->loss_in_log < 0 || a->loss_in_log > 2) return fail("metrics_loss: loss_in_log must be 0, 1 or 2");
    const int n_pix_out = (a->pix_g != nullptr) + (a->pix_l != nullptr) + (a->msk_g != nullptr) + (a->msk_l != nullptr);
    if (n_pix_out != 0 && n_pix_out != 4) return fail("metrics_loss: the per-pixel outputs come all four or not at all");
    if (scratch_bytes < must3r_hip_metrics_loss_scratch_bytes(a->n_scenes, a->n_views, a->H, a->W)) return fail("metrics_loss: scratch too small");
    LossDev p;
    p.a = *a;
    p.n_pix = (unsigned)((long long)a->H * a->W);
    const int n_bv = a->n_scenes * a->n_views, nb = blocks_for(p.n_pix, MET_VIEW_BLOCKS);
    double* slab = reinterpret_cast<double*>(scratch);
    const dim3 g((unsigned)nb, (unsigned)n_bv), t(MET_T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_pix_out) hipLaunchKernelGGL(metrics_loss_kernel<true>, g, t, 0, s, p, slab);
    else hipLaunchKernelGGL(metrics_loss_kernel<false>, g, t, 0, s, p, slab);
    hipLaunchKernelGGL(metrics_loss_final_kernel, dim3((unsigned)((n_bv + 63) / 64)), dim3(64), 0, s, slab, n_bv, nb,
                       reinterpret_cast<long long*>(a->counts), a->sums);
    if (hipGetLastError() != hipSuccess) return fail("metrics_loss: launch failed");
    return 0;
}

extern "C" size_t must3r_hip_metrics_factor_scratch_bytes(int n_scenes, int n_views, int H, int W, int mode) {
    if (check_sizes("metrics_factor", n_scenes, n_views, H, W)) return 0;
    if (mode < MUST3R_NORM_AVG_DIS || mode > MUST3R_NORM_MEDIAN_DIS) { fail("metrics_factor: unknown mode"); return 0; }
    FactorPlan p;
    factor_plan(n_scenes, n_views, H, W, &p);
    return p.bytes;
}

extern "C" int must3r_hip_metrics_factor(const float* pts, const float* trf, const uint8_t* valid, int n_scenes, int n_views, int H, int W, int mode,
                                         float* factor, float* dist, void* scratch, size_t scratch_bytes, void* stream) {
    if (check_sizes("metrics_factor", n_scenes, n_views, H, W)) return 1;
    if (mode < MUST3R_NORM_AVG_DIS || mode > MUST3R_NORM_MEDIAN_DIS) return fail("metrics_factor: unknown mode");
    if (!pts || !valid || !factor || !scratch) return fail("metrics_factor: null argument");
    if (mode == MUST3R_NORM_MEDIAN_DIS && !dist) return fail("metrics_factor: median_dis needs the distance buffer");
    FactorPlan p;
    factor_plan(n_scenes, n_views, H, W, &p);
    if (scratch_bytes < p.bytes) return fail("metrics_factor: scratch too small");
    char* sc = reinterpret_cast<char*>(scratch);
    double* slab = reinterpret_cast<double*>(sc);
    unsigned* hist = reinterpret_cast<unsigned*>(sc + p.off_hist);
    SelState* state = reinterpret_cast<SelState*>(sc + p.off_state);
    const unsigned n = (unsigned)((long long)n_views * H * W);
    const dim3 g((unsigned)p.n_blocks, (unsigned)n_scenes), t(MET_T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mode == MUST3R_NORM_MEDIAN_DIS) {
        if (hipMemsetAsync(sc + p.off_hist, 0, p.bytes - p.off_hist, s) != hipSuccess) return fail("metrics_factor: clearing the bins failed");
        hipLaunchKernelGGL(metrics_factor_kernel<MUST3R_NORM_MEDIAN_DIS>, g, t, 0, s, pts, trf, valid, n, dist, slab, hist);
        hipLaunchKernelGGL(metrics_select_kernel, dim3((unsigned)n_scenes), t, 0, s, hist, state, 11, 1);
        hipLaunchKernelGGL(metrics_hist_kernel, g, t, 0, s, dist, n, state, 10, 11, hist);
        hipLaunchKernelGGL(metrics_select_kernel, dim3((unsigned)n_scenes), t, 0, s, hist, state, 11, 0);
        hipLaunchKernelGGL(metrics_hist_kernel, g, t, 0, s, dist, n, state, 0, 10, hist);
        hipLaunchKernelGGL(metrics_select_kernel, dim3((unsigned)n_scenes), t, 0, s, hist, state, 10, 0);
    } else if (mode == MUST3R_NORM_AVG_DIS) {
        hipLaunchKernelGGL(metrics_factor_kernel<MUST3R_NORM_AVG_DIS>, g, t, 0, s, pts, trf, valid, n, dist, slab, hist);
    } else if (mode == MUST3R_NORM_AVG_LOG1P) {
        hipLaunchKernelGGL(metrics_factor_kernel<MUST3R_NORM_AVG_LOG1P>, g, t, 0, s, pts, trf, valid, n, dist, slab, hist);
    } else {
        hipLaunchKernelGGL(metrics_factor_kernel<MUST3R_NORM_SQRT_DIS>, g, t, 0, s, pts, trf, valid, n, dist, slab, hist);
    }
    hipLaunchKernelGGL(metrics_factor_final_kernel, dim3((unsigned)((n_scenes + 63) / 64)), dim3(64), 0, s, slab, state, n_scenes, p.n_blocks, mode,
                       factor);
    if (hipGetLastError() != hipSuccess) return fail("metrics_factor: launch failed");
    return 0;
}

extern "C" size_t must3r_hip_metrics_loss_grad_scratch_bytes(int n_scenes, int n_views, int H, int W) {
    if (check_sizes("metrics_loss_grad", n_scenes, n_views, H, W)) return 0;
    GradPlan p;
    grad_plan(n_scenes, n_views, H, W, &p);
    return p.bytes;
}

extern "C" int must3r_hip_metrics_loss_grad(const must3r_hip_metrics_loss_args* a, const must3r_hip_metrics_loss_grad_args* g, void* scratch,
                                            size_t scratch_bytes, void* stream) {
    if (!a || !g) return fail("metrics_loss_grad: null argument block");
    if (check_sizes("metrics_loss_grad", a->n_scenes, a->n_views, a->H, a->W)) return 1;
    if (!a->gt_pts || !a->in_camera0 || !a->pr_pts || !a->valid || !scratch) return fail("metrics_loss_grad: null argument");
    if (a->pr_local && !a->w2c) return fail("metrics_loss_grad: the local term needs w2c");
    if (a->loss_in_log < 0 || a->loss_in_log > 2) return fail("metrics_loss_grad: loss_in_log must be 0, 1 or 2");
    if (g->weighting < MUST3R_LOSS_W_SCALAR || g->weighting > MUST3R_LOSS_W_PIXEL) return fail("metrics_loss_grad: unknown weighting %d", g->weighting);
    if (!g->w_g || (a->pr_local && !g->w_l)) return fail("metrics_loss_grad: null weight");
    if (!g->grad_pts || (a->pr_local != nullptr) != (g->grad_local != nullptr)) return fail("metrics_loss_grad: grad_pts is needed, and grad_local exactly with pr_local");
    const bool mean = g->weighting == MUST3R_LOSS_W_MEAN || g->weighting == MUST3R_LOSS_W_CONF;
    if (mean && !g->counts) return fail("metrics_loss_grad: the 'mean' weightings need the forward's counts");
    if (g->weighting == MUST3R_LOSS_W_CONF && (!a->conf || !g->grad_conf)) return fail("metrics_loss_grad: the conf weighting needs conf and grad_conf");
    if (g->n_own < 0 || g->n_own > a->n_scenes) return fail("metrics_loss_grad: n_own = %d is not a number of scenes", g->n_own);
    if (g->n_own > 0) {
        if (g->factor_mode != MUST3R_NORM_AVG_DIS && g->factor_mode != MUST3R_NORM_AVG_LOG1P && g->factor_mode != MUST3R_NORM_SQRT_DIS)
            return fail("metrics_loss_grad: factor mode %d has no scale path", g->factor_mode);
        if (!g->own_factor || !g->n_valid || !a->pr_scale) return fail("metrics_loss_grad: the scale path needs own_factor, n_valid and pr_scale");
    }
    GradPlan pl;
    grad_plan(a->n_scenes, a->n_views, a->H, a->W, &pl);
    if (scratch_bytes < pl.bytes) return fail("metrics_loss_grad: scratch too small");
    char* sc = reinterpret_cast<char*>(scratch);
    long long* totals = reinterpret_cast<long long*>(sc);
    float* scale_co = reinterpret_cast<float*>(sc + pl.off_co);
    double* slab = reinterpret_cast<double*>(sc + pl.off_slab);
    GradDev p;
    p.a = *a;
    p.g = *g;
    p.n_pix = (unsigned)((long long)a->H * a->W);
    p.totals = totals;
    p.scale_co = g->n_own > 0 ? scale_co : nullptr;
    const int n_bv = a->n_scenes * a->n_views;
    const dim3 grid((unsigned)pl.n_blocks, (unsigned)n_bv), t(MET_T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mean) hipLaunchKernelGGL(metrics_count_total_kernel, dim3(1), t, 0, s, reinterpret_cast<const long long*>(g->counts), n_bv, totals);
    if (g->n_own > 0) {
        hipLaunchKernelGGL(metrics_grad_kernel<false>, grid, t, 0, s, p, slab);
        hipLaunchKernelGGL(metrics_scale_final_kernel, dim3((unsigned)((a->n_scenes + 63) / 64)), dim3(64), 0, s, slab, a->n_scenes, a->n_views,
                           pl.n_blocks, g->factor_mode, g->own_factor, reinterpret_cast<const long long*>(g->n_valid), a->pr_scale, scale_co);
    }
    hipLaunchKernelGGL(metrics_grad_kernel<true>, grid, t, 0, s, p, slab);
    if (hipGetLastError() != hipSuccess) return fail("metrics_loss_grad: launch failed");
    return 0;
}
