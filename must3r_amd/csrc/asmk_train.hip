// Learning the two artefacts of the retrieval mode on the device: the k-means update behind the ASMK codebook and the covariance behind the PCA whitening
// (must3r/retrieval/model.py:18-35 pcawhitenlearn_shrinkage).  The assignment step of k-means is must3r_hip_asmk_quantize with k = 1 (asmk.hip).
//
//   km_check_kernel     every id in [0, K) and every entry of the order in [0, M); the ids in order (`sid`), or the bad flag of the record.  Every later
//                       kernel leaves at once when the flag is set: nothing is read through a bad id and no output is written.
//   km_bounds_kernel    per cluster: its segment of `sid` by two binary searches, counts[c], the number of empty clusters (an integer atomic: orderless)
//   km_update_kernel    one block per cluster: the fp64 sum of its rows, SEQUENTIAL in ascending row index (four rows loaded ahead, added one after the other),
//                       one thread per column; new = fp32(sum / count); an empty cluster copies its old centroid
//   km_dist_kernel      one wave per row: dist[j] = sum_d (double(x) - double(c))^2, lane l over the columns l, l + 64, ... in order, then the xor tree
//   km_objective_kernel one block: thread t sums dist[t], dist[t + 1024], ... in order, then a tree in LDS: the order depends on M alone
//   cov_tile_kernel     one block per (tile pair on or below the diagonal, split of the rows): S_tile = sum_r u_r[a] u_r[b] on v_mfma_f64_16x16x4_f64, u = double(x) -
//                       shift formed while staging.  Both operands have the contraction (the rows) as their slow dimension in memory: a 16-row slab of each
//                       column tile lies in LDS as it lies in memory, and the fragment read As[k][i] takes the transpose (as wgrad_bf16, train_lin16.hip).
//                       A diagonal block also sums the columns of its slab.  Partials in fp64, one writer each.
//   cov_reduce_kernel   S[a][b] += the partials in split order, written to (a, b) and to its mirror (b, a): S is exactly symmetric; s += column partials; n += M
// No floating-point atomics anywhere: every floating-point output has one writer and a fixed order of operations.
#include "abi.hpp"
#include "common.hpp"

namespace m3r {

typedef double f64x4t __attribute__((ext_vector_type(4)));

struct KmRecord {   // device record of one update; the entry point copies it to the host
    int bad, n_empty;
    double objective;
};

__global__ void __launch_bounds__(256) km_check_kernel(const int* __restrict__ ids, long long ids_stride, const long long* __restrict__ order, int M, int K,
                                                       int* __restrict__ sid, KmRecord* __restrict__ rec) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    const int own = ids[(long long)p * ids_stride];
    const long long o = order[p];
    bool bad = own < 0 || own >= K || o < 0 || o >= M;
    if (!bad) {
        const int v = ids[o * ids_stride];
        bad = v < 0 || v >= K;
        if (!bad) sid[p] = v;
    }
    if (bad) rec->bad = 1;   // every writer stores the same value
}

__global__ void __launch_bounds__(256) km_bounds_kernel(const int* __restrict__ sid, int M, int K, int* __restrict__ start, int* __restrict__ counts,
                                                        KmRecord* __restrict__ rec) {
    if (rec->bad) return;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    int b[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {   // lower bound of c and of c + 1
        int lo = 0, hi = M;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sid[mid] < c + e) lo = mid + 1;
            else hi = mid;
        }
        b[e] = lo;
    }
    const int n = max(b[1] - b[0], 0);
    start[c] = b[0];
    counts[c] = n;
    if (n == 0) atomicAdd(&rec->n_empty, 1);
}

__global__ void __launch_bounds__(256) km_update_kernel(const float* __restrict__ X, const float* __restrict__ Cb, const long long* __restrict__ order,
                                                        const int* __restrict__ start, const int* __restrict__ counts, int D, float* __restrict__ out,
                                                        const KmRecord* __restrict__ rec) {
    if (rec->bad) return;
    const int c = blockIdx.x;
    const int p0 = start[c], n = counts[c];
    for (int d = threadIdx.x; d < D; d += 256) {
        if (n == 0) {
            out[(size_t)c * D + d] = Cb[(size_t)c * D + d];
            continue;
        }
        double acc = 0.0;
        int p = p0;
        for (; p + 4 <= p0 + n; p += 4) {
            const float v0 = X[(size_t)order[p] * D + d], v1 = X[(size_t)order[p + 1] * D + d];
            const float v2 = X[(size_t)order[p + 2] * D + d], v3 = X[(size_t)order[p + 3] * D + d];
            acc += (double)v0;
            acc += (double)v1;
            acc += (double)v2;
            acc += (double)v3;
        }
        for (; p < p0 + n; ++p) acc += (double)X[(size_t)order[p] * D + d];
        out[(size_t)c * D + d] = (float)(acc / (double)n);
    }
}

__global__ void __launch_bounds__(256) km_dist_kernel(const float* __restrict__ X, const float* __restrict__ Cb, const int* __restrict__ ids,
                                                      long long ids_stride, int M, int D, double* __restrict__ dist, const KmRecord* __restrict__ rec) {
    if (rec->bad) return;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int c = ids[(long long)row * ids_stride];
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double t = (double)X[(size_t)row * D + d] - (double)Cb[(size_t)c * D + d];
        s += t * t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) dist[row] = s;
}

__global__ void __launch_bounds__(1024) km_objective_kernel(const double* __restrict__ dist, int M, double* __restrict__ objective, KmRecord* __restrict__ rec) {
    __shared__ double part[1024];
    if (rec->bad) return;
    double s = 0.0;
    for (int j = threadIdx.x; j < M; j += 1024) s += dist[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        objective[0] = part[0];
        rec->objective = part[0];
    }
}

// ---- covariance
constexpr int CT = 64, CK = 16, CLD = CT + 16;   // tile width, rows per slab, LDS row stride in doubles (the four k rows of a fragment read fall in different banks)
constexpr int COV_TARGET_BLOCKS = 1024, COV_MIN_ROWS = 512, COV_MAX_SPLITS = 64;

// the split rule: a function of (M, D) alone
static void cov_plan(int M, int D, int* nt, int* T, int* nsplit, int* rows_per_split) {
    *nt = (D + CT - 1) / CT;
    *T = *nt * (*nt + 1) / 2;
    int s = max(1, COV_TARGET_BLOCKS / *T);
    s = min(s, max(1, (M + COV_MIN_ROWS - 1) / COV_MIN_ROWS));
    s = min(s, COV_MAX_SPLITS);
    int rps = (M + s - 1) / s;
    rps = (rps + CK - 1) / CK * CK;
    *rows_per_split = max(rps, CK);
    *nsplit = max(1, (M + *rows_per_split - 1) / *rows_per_split);
}

__global__ void __launch_bounds__(256) cov_tile_kernel(const float* __restrict__ X, const double* __restrict__ shift, int M, int D, int rows_per_split,
                                                       int T, int Dp, double* __restrict__ partS, double* __restrict__ parts) {
    __shared__ double As[CK * CLD];
    __shared__ double Bs[CK * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int t = blockIdx.x, split = blockIdx.y;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int a0 = ti * CT, b0 = tj * CT;
    const int r_lo = split * rows_per_split, r_hi = min(M, r_lo + rows_per_split);
    // staging: 16 rows x 64 columns per operand, element (k = e * 4 + wave, column = lane): four per thread and operand
    const int ca = a0 + lane, cb = b0 + lane;
    const double sa = ca < D ? shift[ca] : 0.0, sb = cb < D ? shift[cb] : 0.0;
    f64x4t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4t{0, 0, 0, 0};
    double colsum = 0.0;
    double ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = k0 + e * 4 + wave;
            const bool in = r < r_hi;   // a row behind the split contributes u = 0, not -shift
            ra[e] = (in && ca < D) ? (double)X[(size_t)r * D + ca] - sa : 0.0;
            rb[e] = (in && cb < D) ? (double)X[(size_t)r * D + cb] - sb : 0.0;
        }
    };
    if (r_lo < r_hi) fetch(r_lo);
    for (int k0 = r_lo; k0 < r_hi; k0 += CK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            As[(e * 4 + wave) * CLD + lane] = ra[e];
            Bs[(e * 4 + wave) * CLD + lane] = rb[e];
            colsum += ra[e];
        }
        __syncthreads();
        if (k0 + CK < r_hi) fetch(k0 + CK);
#pragma unroll
        for (int ks = 0; ks < CK / 4; ++ks) {
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[(ks * 4 + fk) * CLD + wm * 32 + i * 16 + fr];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[(ks * 4 + fk) * CLD + wn * 32 + j * 16 + fr];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // D layout of the f64 16x16x4: row 4 * r + lane / 16, column lane & 15
    double* P = partS + ((size_t)split * T + t) * (CT * CT);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(wm * 32 + i * 16 + r * 4 + fk) * CT + wn * 32 + j * 16 + fr] = acc[i][j][r];
    if (ti == tj) {   // the column sums of this slab: the four waves' shares of a column, added in wave order
        __syncthreads();
        As[wave * CT + lane] = colsum;
        __syncthreads();
        if (wave == 0) parts[(size_t)split * Dp + a0 + lane] = ((As[lane] + As[CT + lane]) + As[2 * CT + lane]) + As[3 * CT + lane];
    }
}

__global__ void __launch_bounds__(256) cov_reduce_kernel(const double* __restrict__ partS, const double* __restrict__ parts, int M, int D, int nsplit, int T,
                                                         int Dp, double* __restrict__ S, double* __restrict__ s, double* __restrict__ n) {
    const int ti = blockIdx.y, tj = blockIdx.z;
    if (tj > ti) return;
    const int t = ti * (ti + 1) / 2 + tj;
    const int e = blockIdx.x * 256 + threadIdx.x;   // element of the tile
    const int al = e >> 6, bl = e & 63;
    const int a = ti * CT + al, b = tj * CT + bl;
    if (a < D && b < D && (ti != tj || bl <= al)) {
        double tot = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) tot += partS[((size_t)sp * T + t) * (CT * CT) + e];
        const double v = S[(size_t)a * D + b] + tot;
        S[(size_t)a * D + b] = v;
        if (a != b) S[(size_t)b * D + a] = v;
    }
    if (ti == tj && al == 0 && b < D) {
        double tot = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) tot += parts[(size_t)sp * Dp + b];
        s[b] += tot;
    }
    if (ti == 0 && tj == 0 && e == 0) n[0] += (double)M;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_kmeans_update_scratch_bytes(int M, int K) {
    if (M <= 0 || K <= 0) return 0;
    return 256 + align256((size_t)M * sizeof(int)) + align256((size_t)K * sizeof(int));
}

extern "C" int must3r_hip_kmeans_update(const float* feat, int M, int D, const float* centroids, int K, const int32_t* ids, int64_t ids_stride,
                                        const int64_t* order, float* new_centroids, int32_t* counts, double* dist, double* objective, double* host_record,
                                        void* stream, void* scratch, size_t scratch_bytes) {
    if (M < 1 || D < 1) return fail("kmeans_update: bad shape (M %d, D %d)", M, D);
    if (K < 1) return fail("kmeans_update: K must be at least 1, got %d", K);
    if (D % 16) return fail("kmeans_update: D must be a multiple of 16, got %d", D);
    if (ids_stride < 1) return fail("kmeans_update: the row stride of ids must be at least 1");
    if (!feat || !centroids || !ids || !order || !new_centroids || !counts || !dist || !objective || !scratch) return fail("kmeans_update: null argument");
    if (((size_t)feat | (size_t)centroids | (size_t)new_centroids) & 15) return fail("kmeans_update: feat, centroids and new_centroids must be 16-byte aligned");
    if (((size_t)order | (size_t)dist | (size_t)objective | (size_t)scratch) & 7) return fail("kmeans_update: order, dist, objective and scratch must be 8-byte aligned");
    if (((size_t)ids | (size_t)counts) & 3) return fail("kmeans_update: ids and counts must be 4-byte aligned");
    if (scratch_bytes < must3r_hip_kmeans_update_scratch_bytes(M, K)) return fail("kmeans_update: scratch too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(scratch);
    KmRecord* rec = reinterpret_cast<KmRecord*>(base);
    int* sid = reinterpret_cast<int*>(base + 256);
    int* start = reinterpret_cast<int*>(base + 256 + align256((size_t)M * sizeof(int)));
    if (hipMemsetAsync(rec, 0, sizeof(KmRecord), s) != hipSuccess) return fail("kmeans_update: memset failed");
    const long long* ord = reinterpret_cast<const long long*>(order);
    hipLaunchKernelGGL(km_check_kernel, dim3((M + 255) / 256), dim3(256), 0, s, ids, (long long)ids_stride, ord, M, K, sid, rec);
    hipLaunchKernelGGL(km_bounds_kernel, dim3((K + 255) / 256), dim3(256), 0, s, sid, M, K, start, counts, rec);
    hipLaunchKernelGGL(km_update_kernel, dim3(K), dim3(256), 0, s, feat, centroids, ord, start, counts, D, new_centroids, rec);
    hipLaunchKernelGGL(km_dist_kernel, dim3((M + 3) / 4), dim3(256), 0, s, feat, centroids, ids, (long long)ids_stride, M, D, dist, rec);
    hipLaunchKernelGGL(km_objective_kernel, dim3(1), dim3(1024), 0, s, dist, M, objective, rec);
    if (hipGetLastError() != hipSuccess) return fail("kmeans_update: launch failed");
    KmRecord host;
    if (hipMemcpyAsync(&host, rec, sizeof(KmRecord), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail("kmeans_update: reading the record back failed");
    if (host.bad) return fail("kmeans_update: an id outside [0, %d) or an order entry outside [0, %d); nothing was read through it and no output was written", K, M);
    if (host_record) {
        host_record[0] = host.objective;
        host_record[1] = (double)host.n_empty;
    }
    return 0;
}

extern "C" size_t must3r_hip_cov_accumulate_scratch_bytes(int M, int D) {
    if (M <= 0 || D <= 0 || D % 16) return 0;
    int nt, T, nsplit, rps;
    cov_plan(M, D, &nt, &T, &nsplit, &rps);
    return (size_t)nsplit * ((size_t)T * CT * CT + (size_t)nt * CT) * sizeof(double);
}

extern "C" int must3r_hip_cov_accumulate(const float* x, int M, int D, const double* shift, double* S, double* s, double* n, void* stream, void* scratch,
                                         size_t scratch_bytes) {
    if (M < 0 || D < 1) return fail("cov_accumulate: bad shape (M %d, D %d)", M, D);
    if (D % 16) return fail("cov_accumulate: D must be a multiple of 16, got %d", D);
    if (M == 0) return 0;
    if (!x || !shift || !S || !s || !n || !scratch) return fail("cov_accumulate: null argument");
    if ((size_t)x & 15) return fail("cov_accumulate: x must be 16-byte aligned");
    if (((size_t)shift | (size_t)S | (size_t)s | (size_t)n | (size_t)scratch) & 7) return fail("cov_accumulate: shift, S, s, n and scratch must be 8-byte aligned");
    if (scratch_bytes < must3r_hip_cov_accumulate_scratch_bytes(M, D)) return fail("cov_accumulate: scratch too small");
    int nt, T, nsplit, rps;
    cov_plan(M, D, &nt, &T, &nsplit, &rps);
    const int Dp = nt * CT;
    double* partS = reinterpret_cast<double*>(scratch);
    double* parts = partS + (size_t)nsplit * T * CT * CT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cov_tile_kernel, dim3(T, nsplit), dim3(256), 0, st, x, shift, M, D, rps, T, Dp, partS, parts);
    hipLaunchKernelGGL(cov_reduce_kernel, dim3(CT * CT / 256, nt, nt), dim3(256), 0, st, partS, parts, M, D, nsplit, T, Dp, S, s, n);
    if (hipGetLastError() != hipSuccess) return fail("cov_accumulate: launch failed");
    return 0;
}
