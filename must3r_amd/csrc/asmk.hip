// ASMK back-end of the retrieval mode (must3r/demo/inference.py:31-60 MUSt3R_Retriever, must3r/retrieval/processor.py:83-96):
// binary kernel, no idf, multiple assignment 1 (database) / 5 (query), similarity_threshold tau, alpha.  The reference runs
// asmk's build_ivf / query_ivf with a faiss L2 index; here the same scores come from three kernels.
//
//   csq_kernel              |c|^2 per centroid (once per codebook), fp32 in index order.
//   quantize_kernel<KK>     the KK nearest centroids of each feature row by the ranking value |c|^2 - 2 x.c, ascending, ties to the
//                           lower centroid id.  128 rows x 128 centroids per tile, 16-deep K steps through LDS, 4 waves of 64 x 64
//                           on v_mfma_f32_16x16x4_f32 (exact fp32 products, k-ordered fmaf chain).  The tile's values go through
//                           LDS to a running top-KK per (row, half of the columns) in registers.  blockIdx.y splits the centroid
//                           range so that a few hundred rows still fill the device; quantize_merge_kernel merges the per-split
//                           lists in split order.  Both orders are total ((value, id) lexicographic), so the ids do not depend
//                           on the split.
//   aggregate_kernel        per image: stable bitonic sort of the (word, row) pairs in LDS, run starts by wave ballots, residual
//                           r_w = sum_j (x_j - c_w) in fp32 in ascending row order (each difference rounded, then added: the
//                           reference's (des[mask] - centroid).sum(0) on float32), bits r_w[d] > 0 packed by ballots.  An image
//                           with an id outside [0, K) is refused (count -1) before any centroid row is read.
//   scores_kernel           per (query image, database image): merge-join of the ascending word lists (binary search of each
//                           database word in the query's list in LDS), h = popcount(xor), s = 1 - 2h/D, sigma = s^alpha if
//                           s >= tau else 0 in fp32, summed in fp64 in ascending word order, then / sqrt(|W_d|) / sqrt(|W_q|).
// No atomics: every output element has one writer and a fixed order of operations.
#include "abi.hpp"
#include "common.hpp"

namespace m3r {

constexpr int QM = 128, QN = 128, QK = 16, QPAD = 20, QTS = QN + 2;   // QTS: row stride of the ranking tile (conflict-free scan)
constexpr int QUANT_TARGET_BLOCKS = 1024;
constexpr int AGG_MAX_PAIRS = 4096;   // (word, row) pairs one image's LDS sort holds

__device__ __forceinline__ bool rank_before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }
// a NaN ranking value (a non-finite feature or centroid) ranks as +inf: it sorts after every number and still before the (+inf, INT_MAX)
// placeholders, so the k ids of a row are always real centroids in [0, K)
__device__ __forceinline__ float rank_value(float v) { return v == v ? v : INFINITY; }

template <int KK>
__device__ __forceinline__ void topk_insert(float (&d)[KK], int (&id)[KK], float cd, int cid) {
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        if (rank_before(cd, cid, d[j], id[j])) {
            const float td = d[j];
            const int ti = id[j];
            d[j] = cd; id[j] = cid;
            cd = td; cid = ti;
        }
    }
}

__global__ void __launch_bounds__(256) csq_kernel(const float* __restrict__ C, int K, int D, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= K) return;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = C[(size_t)row * D + c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

template <int KK>
__global__ void __launch_bounds__(256) quantize_kernel(const float* __restrict__ X, const float* __restrict__ Cb, const float* __restrict__ csq,
                                                       int M, int K, int D, int tiles_per_split, float* __restrict__ part_d,
                                                       int* __restrict__ part_i) {
    __shared__ __attribute__((aligned(16))) float As[QM * QPAD];
    __shared__ __attribute__((aligned(16))) float Bs[QN * QPAD];
    __shared__ float Ts[QM * QTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int m0 = blockIdx.x * QM, split = blockIdx.y;
    const int n_tiles = (K + QN - 1) / QN;
    const int t_lo = split * tiles_per_split, t_hi = min(n_tiles, t_lo + tiles_per_split);
    const int srow = tid >> 1, half = tid & 1;   // top-k owner: one row, every other column of each tile
    float bd[KK];
    int bi[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { bd[j] = INFINITY; bi[j] = 0x7fffffff; }
    // operand staging: 128 rows x 16 floats = 512 float4 per operand, two per thread
    int lr[2], lc[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) { const int idx = e * 256 + tid; lr[e] = idx >> 2; lc[e] = (idx & 3) * 4; }
    for (int t = t_lo; t < t_hi; ++t) {
        const int n0 = t * QN;
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 ra[2], rb[2];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int gm = m0 + lr[e], gn = n0 + lr[e];
                ra[e] = gm < M ? *reinterpret_cast<const f32x4*>(X + (size_t)gm * D + k0 + lc[e]) : f32x4{0.f, 0.f, 0.f, 0.f};
                rb[e] = gn < K ? *reinterpret_cast<const f32x4*>(Cb + (size_t)gn * D + k0 + lc[e]) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < D; k0 += QK) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                *reinterpret_cast<f32x4*>(As + lr[e] * QPAD + lc[e]) = ra[e];
                *reinterpret_cast<f32x4*>(Bs + lr[e] * QPAD + lc[e]) = rb[e];
            }
            __syncthreads();
            if (k0 + QK < D) fetch(k0 + QK);
#pragma unroll
            for (int ks = 0; ks < QK / 4; ++ks) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = As[(wm * 64 + i * 16 + fr) * QPAD + ks * 4 + fk];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = Bs[(wn * 64 + j * 16 + fr) * QPAD + ks * 4 + fk];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        // ranking values -> LDS (C/D map: row 4*(lane/16) + r, column lane & 15).  The previous tile's scan finished before the
        // barriers of this tile's K loop.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wn * 64 + j * 16 + fr;
            const float cs = n0 + col < K ? csq[n0 + col] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ts[(wm * 64 + i * 16 + fk * 4 + r) * QTS + col] = rank_value(cs - 2.0f * acc[i][j][r]);
        }
        __syncthreads();
        const int valid = min(QN, K - n0);
        for (int c = half; c < valid; c += 2) {
            const float v = Ts[srow * QTS + c];
            if (rank_before(v, n0 + c, bd[KK - 1], bi[KK - 1])) topk_insert<KK>(bd, bi, v, n0 + c);
        }
    }
    // merge the two halves of each row through LDS (As / Bs are free: the last K step's reads finished before the scan barrier)
    float* hd = As;
    int* hi = reinterpret_cast<int*>(Bs);
    if (half == 1) {
#pragma unroll
        for (int j = 0; j < KK; ++j) { hd[srow * KK + j] = bd[j]; hi[srow * KK + j] = bi[j]; }
    }
    __syncthreads();
    if (half == 0 && m0 + srow < M) {
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            const float v = hd[srow * KK + j];
            const int id = hi[srow * KK + j];
            if (rank_before(v, id, bd[KK - 1], bi[KK - 1])) topk_insert<KK>(bd, bi, v, id);
        }
        const size_t o = ((size_t)split * M + m0 + srow) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) { part_d[o + j] = bd[j]; part_i[o + j] = bi[j]; }
    }
}

template <int KK>
__global__ void __launch_bounds__(256) quantize_merge_kernel(const float* __restrict__ part_d, const int* __restrict__ part_i, int M, int S,
                                                             int* __restrict__ ids) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float bd[KK];
    int bi[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { bd[j] = INFINITY; bi[j] = 0x7fffffff; }
    for (int s = 0; s < S; ++s) {
        const size_t o = ((size_t)s * M + m) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) {
            const float v = rank_value(part_d[o + j]);
            const int id = part_i[o + j];
            if (rank_before(v, id, bd[KK - 1], bi[KK - 1])) topk_insert<KK>(bd, bi, v, id);
        }
    }
#pragma unroll
    for (int j = 0; j < KK; ++j) ids[(size_t)m * KK + j] = bi[j];
}

// one block (16 waves) per image
__global__ void __launch_bounds__(1024) aggregate_kernel(const float* __restrict__ X, const float* __restrict__ Cb, int K, int D,
                                                         const int* __restrict__ ids, int k_ids, int k_use, const int* __restrict__ offsets,
                                                         int* __restrict__ words,
                                                         unsigned* __restrict__ bits, int* __restrict__ counts) {
    __shared__ unsigned long long key[AGG_MAX_PAIRS];
    __shared__ int run_start[AGG_MAX_PAIRS + 1];
    __shared__ int n_runs;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = offsets[img], nr = offsets[img + 1] - r0;
    const int P = nr * k_use;
    if (nr < 0 || P > AGG_MAX_PAIRS) {   // the host checks this too; never index past the LDS arrays
        if (tid == 0) counts[img] = -1;
        return;
    }
    int Pp = 1;
    while (Pp < P) Pp <<= 1;
    int bad = 0;
    for (int i = tid; i < Pp; i += 1024) {
        unsigned long long v = ~0ull;
        if (i < P) {
            const int row = i / k_use, j = i - row * k_use;
            const int w = ids[(size_t)(r0 + row) * k_ids + j];
            bad |= (w < 0 || w >= K);
            v = ((unsigned long long)(unsigned)w << 32) | (unsigned)row;
        }
        key[i] = v;
    }
    if (__syncthreads_or(bad)) {          // a word outside the codebook: refuse the image before any centroid row is read
        if (tid == 0) counts[img] = -1;
        return;
    }
    for (int size = 2; size <= Pp; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < Pp / 2; i += 1024) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = ((lo & size) == 0);
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == asc) { key[lo] = b; key[hi] = a; }
            }
            __syncthreads();
        }
    if (wave == 0) {
        int cnt = 0;
        for (int b = 0; b < P; b += 64) {
            const int i = b + lane;
            const bool f = i < P && (i == 0 || (key[i] >> 32) != (key[i - 1] >> 32));
            const unsigned long long m = __ballot(f);
            const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            if (f) run_start[cnt + below] = i;
            cnt += __popcll(m);
        }
        if (lane == 0) { run_start[cnt] = P; n_runs = cnt; counts[img] = cnt; }
    }
    __syncthreads();
    const int nw = D / 32;
    const size_t slot = (size_t)r0 * k_use;
    for (int r = wave; r < n_runs; r += 16) {
        const int e0 = run_start[r], e1 = run_start[r + 1];
        const int w = (int)(key[e0] >> 32);
        if (lane == 0) words[slot + r] = w;
        for (int base = 0; base < D; base += 1024) {
            float c[16], acc[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int d = base + t * 64 + lane;
                c[t] = d < D ? Cb[(size_t)w * D + d] : 0.f;
                acc[t] = 0.f;
            }
            for (int e = e0; e < e1; ++e) {
                const float* xr = X + (size_t)(r0 + (int)(key[e] & 0xffffffffu)) * D;
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int d = base + t * 64 + lane;
                    if (d < D) acc[t] += xr[d] - c[t];
                }
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int d0 = base + t * 64;
                if (d0 >= D) break;
                const unsigned long long m = __ballot(acc[t] > 0.f);
                if (lane < 2) bits[(slot + r) * nw + d0 / 32 + lane] = lane ? (unsigned)(m >> 32) : (unsigned)m;
            }
        }
    }
}

// one block (4 waves) per query image x a slice of the database images; one wave per (query, database) pair
__global__ void __launch_bounds__(256) scores_kernel(const int* __restrict__ wq, const unsigned* __restrict__ bq, const int* __restrict__ cq,
                                                     const int* __restrict__ oq, int kq, const int* __restrict__ wd,
                                                     const unsigned* __restrict__ bdb, const int* __restrict__ cd, const int* __restrict__ od,
                                                     int kd, int n_d, int D, float alpha, float tau, int normalize,
                                                     double* __restrict__ out) {
    __shared__ int qw[AGG_MAX_PAIRS];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = max(0, min(cq[q], AGG_MAX_PAIRS));
    const size_t sq = (size_t)oq[q] * kq;
    for (int i = tid; i < nq; i += 256) qw[i] = wq[sq + i];
    __syncthreads();
    const int nw = D / 32;
    for (int d = blockIdx.y * 4 + wave; d < n_d; d += gridDim.y * 4) {
        const int nd = max(0, cd[d]);
        const size_t sd = (size_t)od[d] * kd;
        double total = 0.0;
        for (int b = 0; b < nd; b += 64) {
            const int i = b + lane;
            float sig = 0.f;
            if (i < nd) {
                const int w = wd[sd + i];
                int lo = 0, hi = nq;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (qw[mid] < w) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < nq && qw[lo] == w) {
                    const unsigned* x = bq + (sq + lo) * nw;
                    const unsigned* y = bdb + (sd + i) * nw;
                    int h = 0;
                    for (int c = 0; c < nw; ++c) h += __builtin_popcount(x[c] ^ y[c]);
                    const float s = 1.0f - (2.0f * (float)h) / (float)D;
                    sig = s >= tau ? powf(s, alpha) : 0.f;
                }
            }
            // fp64 sum in ascending word order; lanes without a shared word add nothing (x + 0.0 == x)
            unsigned long long m = __ballot(sig != 0.f);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                total += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(sig), j));
                m &= m - 1;
            }
        }
        if (lane == 0) {
            double v = total;
            if (normalize) v = (nd > 0 && nq > 0) ? (v / sqrt((double)nd)) / sqrt((double)nq) : 0.0;
            out[(size_t)q * n_d + d] = v;
        }
    }
}

static void quant_plan(int M, int K, int* tiles_per_split, int* S) {
    const int row_tiles = (M + QM - 1) / QM, n_tiles = (K + QN - 1) / QN;
    int target = (QUANT_TARGET_BLOCKS + row_tiles - 1) / row_tiles;
    target = max(1, min(target, n_tiles));
    *tiles_per_split = (n_tiles + target - 1) / target;
    *S = (n_tiles + *tiles_per_split - 1) / *tiles_per_split;
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_asmk_quantize_scratch_bytes(int M, int K, int k) {
    if (M <= 0 || K <= 0 || k <= 0) return 0;
    int tps, S;
    quant_plan(M, K, &tps, &S);
    return (size_t)S * M * k * (sizeof(float) + sizeof(int));
}

extern "C" int must3r_hip_asmk_centroid_sqnorm(const float* C, int K, int D, float* out, void* stream) {
    if (K < 0 || D <= 0) return fail("asmk_centroid_sqnorm: bad shape");
    if (K == 0) return 0;
    if (!C || !out) return fail("asmk_centroid_sqnorm: null argument");
    hipLaunchKernelGGL(csq_kernel, dim3((K + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), C, K, D, out);
    if (hipGetLastError() != hipSuccess) return fail("asmk_centroid_sqnorm: launch failed");
    return 0;
}

template <int KK>
static void launch_quant_k(const float* X, int M, const float* C, const float* csq, int K, int D, int tps, int S, float* pd, int* pi,
                           int* ids, hipStream_t s) {
    hipLaunchKernelGGL(quantize_kernel<KK>, dim3((M + QM - 1) / QM, S), dim3(256), 0, s, X, C, csq, M, K, D, tps, pd, pi);
    hipLaunchKernelGGL(quantize_merge_kernel<KK>, dim3((M + 255) / 256), dim3(256), 0, s, pd, pi, M, S, ids);
}

extern "C" int must3r_hip_asmk_quantize(const float* X, int M, const float* C, const float* csq, int K, int D, int k, int32_t* ids, void* scratch,
                                        size_t scratch_bytes, void* stream) {
    if (M < 0 || K <= 0 || D <= 0) return fail("asmk_quantize: bad shape");
    if (M == 0) return 0;
    if (!X || !C || !csq || !ids) return fail("asmk_quantize: null argument");
    if (D <= 0 || D % 64) return fail("asmk_quantize: D must be a positive multiple of 64");
    if (k < 1 || k > 8) return fail("asmk_quantize: k must be in [1, 8]");
    if (k > K) return fail("asmk_quantize: k exceeds the number of centroids");
    if (((size_t)X | (size_t)C) & 15) return fail("asmk_quantize: feat and centroids must be 16-byte aligned");
    if (!scratch || scratch_bytes < must3r_hip_asmk_quantize_scratch_bytes(M, K, k)) return fail("asmk_quantize: scratch too small");
    int tps, S;
    quant_plan(M, K, &tps, &S);
    float* pd = reinterpret_cast<float*>(scratch);
    int* pi = reinterpret_cast<int*>(pd + (size_t)S * M * k);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (k) {
        case 1: launch_quant_k<1>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 2: launch_quant_k<2>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 3: launch_quant_k<3>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 4: launch_quant_k<4>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 5: launch_quant_k<5>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 6: launch_quant_k<6>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        case 7: launch_quant_k<7>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
        default: launch_quant_k<8>(X, M, C, csq, K, D, tps, S, pd, pi, ids, s); break;
    }
    if (hipGetLastError() != hipSuccess) return fail("asmk_quantize: launch failed");
    return 0;
}

extern "C" int must3r_hip_asmk_aggregate(const float* X, const float* C, int K, int D, const int32_t* ids, int k_ids, int k_use,
                                         const int32_t* offsets, int n_images, int max_rows, int32_t* words, uint32_t* bits, int32_t* counts,
                                         void* stream) {
    if (n_images < 0 || K <= 0 || D <= 0) return fail("asmk_aggregate: bad shape");
    if (n_images == 0) return 0;
    if (!X || !C || !ids || !offsets || !words || !bits || !counts) return fail("asmk_aggregate: null argument");
    if (D <= 0 || D % 64) return fail("asmk_aggregate: D must be a positive multiple of 64");
    if (k_use < 1 || k_use > k_ids) return fail("asmk_aggregate: k_use must be in [1, k_ids]");
    if (max_rows < 0 || (long long)max_rows * k_use > AGG_MAX_PAIRS)
        return fail("asmk_aggregate: an image has more (word, row) pairs than the per-image LDS sort holds (rows * k_use <= 4096)");
    hipLaunchKernelGGL(aggregate_kernel, dim3(n_images), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), X, C, K, D, ids, k_ids, k_use,
                       offsets, words, bits, counts);
    if (hipGetLastError() != hipSuccess) return fail("asmk_aggregate: launch failed");
    return 0;
}

extern "C" int must3r_hip_asmk_scores(const int32_t* wq, const uint32_t* bq, const int32_t* cq, const int32_t* oq, int kq, int n_q,
                                      const int32_t* wd, const uint32_t* bd, const int32_t* cd, const int32_t* od, int kd, int n_d, int D,
                                      float alpha, float tau, int normalize, double* out, void* stream) {
    if (n_q < 0 || n_d < 0 || D <= 0 || kq < 1 || kd < 1) return fail("asmk_scores: bad shape");
    if (n_q == 0 || n_d == 0) return 0;
    if (!wq || !bq || !cq || !oq || !wd || !bd || !cd || !od || !out) return fail("asmk_scores: null argument");
    if (D <= 0 || D % 64) return fail("asmk_scores: D must be a positive multiple of 64");
    const int slices = max(1, min(64, (n_d + 31) / 32));   // up to 32 database images per block
    hipLaunchKernelGGL(scores_kernel, dim3(n_q, slices), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), wq, bq, cq, oq, kq, wd, bd, cd, od, kd,
                       n_d, D, alpha, tau, normalize, out);
    if (hipGetLastError() != hipSuccess) return fail("asmk_scores: launch failed");
    return 0;
}
