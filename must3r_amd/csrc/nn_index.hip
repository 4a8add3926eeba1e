// Exact 1-NN index over a growing point set: the SLAM keyframe test's map (must3r/slam/nns.py:40-92) without a full scan per query.
// The reference rebuilds a scipy KD-tree after every keyframe (nns.py:47-50); nn.hip scans every point of the map for every query.
// Here the map is sorted once per change of the point set and a query walks a bounding-box hierarchy of its quadrant only:
//
//   build (all on the device, no host sync, into caller-owned buffers)
//     nn_bbox_partial_kernel / nn_bbox_final_kernel   box of the finite points (two-stage min / max reduction) + the index header
//     nn_key_kernel        key = quadrant id << shift | Morton code of the point on cubic cells of the box; non-finite points and
//                          ids outside [0, Q) get the key 0xffffffff and sort behind every quadrant (dropped: nn.hip never lets them win)
//     nn_rs_hist_kernel / nn_rs_scan_kernel / nn_rs_scatter_kernel
//                          stable LSD radix sort of (key, point index), 4 passes of 8-bit digits; per-block digit counts (LDS counters,
//                          order-free), one exclusive scan digit-major / block-minor, scatter ranked by wave ballots in element order:
//                          the output is a function of the input alone
//     nn_segments_kernel   quadrant segments [seg[q], seg[q+1]) by binary search; per quadrant ceil(count / L) leaves padded to a power
//                          of two P_q and a heap of 2 P_q - 1 fp32 AABBs (node 1 = root, children 2k, 2k + 1, leaves P_q .. 2 P_q - 1)
//     nn_gather_kernel     points in key order as float4
//     nn_tree_level_kernel leaf boxes, then the levels above: one launch per tree height over every quadrant's nodes at that height
//                          (a leaf never straddles two quadrants)
//   query
//     quadrant ids of the queries by nn.hip's quadrant_id_kernel (must3r_hip_quadrant_ids), written into out_dist and read back by
//     nn_index_query_kernel<G>: G lanes per query walk its quadrant's heap together, nearer child first, a node pruned when its box
//     bound is >= the best d2 so far; stackless (the path is the node number, a bit per level says the far sibling was taken):
//     registers only.  A query with another divider than the build's gets NaN.
//
// Exactness: the leaf computes d2 = fma(dz,dz, fma(dy,dy, dx*dx)) in fp32 as nn_query_kernel does.  The box bound is the same chain on
// the per-axis gaps max(lo - q, q - hi, 0), and fl() is monotone and sign-symmetric, so |fl(q - p)| >= gap for every p in the box and the
// bound never exceeds the d2 of any of its points: a pruned subtree cannot hold a value below the minimum, the minimum is the brute
// force's minimum over the same points, and sqrtf of it is bit-identical.  Empty quadrant / non-finite query: +inf as nn.hip gives.
#include "abi.hpp"
#include "common.hpp"
#include "nn_walk.hpp"
#include "options.hpp"

namespace m3r {

namespace {

constexpr int NNI_MIN_LEAF_LOG2 = 4;   // the node area is sized for leaves of 16 points, the smallest NN_LEAF_LOG2 allows
constexpr int RS_T = 256;              // radix sort: threads per block
constexpr int RS_ITEMS = 32;           // elements per thread and block tile
constexpr int RS_TILE = RS_T * RS_ITEMS;
constexpr int BB_BLOCKS = 1024;        // partial boxes of the bounding-box reduction
constexpr long long NNI_MAX_N = 1LL << 30;

// NnIndexHeader: nn_walk.hpp
constexpr size_t NNI_HEADER_BYTES = (sizeof(NnIndexHeader) + 255) / 256 * 256;

int n_quads_of(int divider) { return divider == 0 ? 1 : 2 * divider * divider; }
long long node_cap_of(long long n, int Q) { return 4 * (((n + (1 << NNI_MIN_LEAF_LOG2) - 1) >> NNI_MIN_LEAF_LOG2) + Q) + 4; }
long long rs_blocks_of(long long n) { return (n + RS_TILE - 1) / RS_TILE; }
long long next_pow2(long long v) { long long p = 1; while (p < v) p <<= 1; return p; }

// --------------------------------------------------------------------------------------------------------------------------------
// bounding box of the finite points
// --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_minmax6(float* v, float (*red)[6]) {   // v[0..2] min, v[3..5] max over the block -> red[0]
    const int t = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 6; ++a) red[t][a] = v[a];
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[t][a] = fminf(red[t][a], red[t + s][a]);
                red[t][a + 3] = fmaxf(red[t][a + 3], red[t + s][a + 3]);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) nn_bbox_partial_kernel(const float* __restrict__ xyz, const long long n, float* __restrict__ part) {
    __shared__ float red[256][6];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
        if (!finite3(x, y, z)) continue;
        v[0] = fminf(v[0], x); v[1] = fminf(v[1], y); v[2] = fminf(v[2], z);
        v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y); v[5] = fmaxf(v[5], z);
    }
    block_minmax6(v, red);
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = red[0][threadIdx.x];
}

__global__ void __launch_bounds__(256) nn_bbox_final_kernel(const float* __restrict__ part, const int n_part, NnIndexHeader* __restrict__ h,
                                                            const int divider, const int Q, const int leaf_log2, const int key_shift,
                                                            const int morton_bits, const int n, const long long pts_off,
                                                            const long long nodes_off, const long long node_cap) {
    __shared__ float red[256][6];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < n_part; b += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] = fminf(v[a], part[b * 6 + a]);
            v[a + 3] = fmaxf(v[a + 3], part[b * 6 + a + 3]);
        }
    }
    block_minmax6(v, red);
    if (threadIdx.x == 0) {
        h->divider = divider; h->n_quads = Q; h->leaf_log2 = leaf_log2; h->key_shift = key_shift;
        h->morton_bits = morton_bits; h->n_points = n;
        h->pts_off = pts_off; h->nodes_off = nodes_off; h->node_cap = node_cap;
        for (int a = 0; a < 3; ++a) { h->lo[a] = red[0][a]; h->hi[a] = red[0][a + 3]; }
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
// keys
// --------------------------------------------------------------------------------------------------------------------------------
// Cubic cells: one cell size on all three axes (the map's box is far from a cube: a camera path is long and the scene is shallow), as
// many bits per axis as its extent needs at that size, the largest axis getting as many as fit in the key_shift bits below the
// quadrant.  Bits are interleaved from the top level down, an axis joining once the level is within its bit count.  The key only
// orders the points: the tree built on it is exact whatever the order.
__global__ void __launch_bounds__(256) nn_key_kernel(const float* __restrict__ xyz, const int* __restrict__ qid, const int n,
                                                     const NnIndexHeader* __restrict__ h, unsigned* __restrict__ keys,
                                                     unsigned* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[(long long)i * 3 + 0], y = xyz[(long long)i * 3 + 1], z = xyz[(long long)i * 3 + 2];
    const int q = qid ? qid[i] : 0;
    unsigned key = 0xffffffffu;
    if (finite3(x, y, z) && q >= 0 && q < h->n_quads) {
        const int total = h->key_shift;
        const float lo[3] = {h->lo[0], h->lo[1], h->lo[2]};
        const float ext[3] = {h->hi[0] - lo[0], h->hi[1] - lo[1], h->hi[2] - lo[2]};
        const float emax = fmaxf(fmaxf(ext[0], ext[1]), ext[2]);
        unsigned m = 0;
        if (emax > 0.f && emax < INFINITY) {
            int d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = ext[a] > 0.f ? max(0, ilogbf(emax) - ilogbf(ext[a]) - 1) : 64;   // bits fewer than the largest axis
            int bmax = total < 30 ? total : 30;
            while (bmax > 0 && max(0, bmax - d[0]) + max(0, bmax - d[1]) + max(0, bmax - d[2]) > total) --bmax;
            const float scale = ldexpf(1.0f, bmax) / emax;   // cells per unit of length
            const float p[3] = {x, y, z};
            unsigned c[3];
            int bits[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                bits[a] = max(0, bmax - d[a]);
                const float top = (float)((1u << bits[a]) - 1u);
                c[a] = (unsigned)fminf(fmaxf((p[a] - lo[a]) * scale, 0.f), top);   // NaN (0 * inf) -> 0: the order only loses quality
            }
            int pos = total;
            for (int b = bmax - 1; b >= 0; --b) {
#pragma unroll
                for (int a = 2; a >= 0; --a) {
                    if (b < bits[a]) {
                        --pos;
                        m |= ((c[a] >> b) & 1u) << pos;
                    }
                }
            }
        }
        key = ((unsigned)q << total) | m;
    }
    keys[i] = key;
    vals[i] = (unsigned)i;
}

// --------------------------------------------------------------------------------------------------------------------------------
// stable LSD radix sort, 8-bit digits
// --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RS_T) nn_rs_hist_kernel(const unsigned* __restrict__ keys, const int n, const int shift,
                                                          unsigned* __restrict__ hist, const int nblocks) {
    __shared__ unsigned cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * RS_TILE;
    const int end = base + RS_TILE < n ? base + RS_TILE : n;
    for (int i = base + threadIdx.x; i < end; i += RS_T) atomicAdd(&cnt[(keys[i] >> shift) & 255u], 1u);   // a count: order-free
    __syncthreads();
    hist[threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of hist[0 .. m) in place, one block of 1024 threads, 16 consecutive elements per thread and round
__global__ void __launch_bounds__(1024) nn_rs_scan_kernel(unsigned* __restrict__ hist, const int m) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int r0 = 0; r0 < m; r0 += 1024 * 16) {
        unsigned v[16], s = 0;
        const int i0 = r0 + t * 16;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            v[k] = i0 + k < m ? hist[i0 + k] : 0u;
            s += v[k];
        }
        unsigned incl = s;   // inclusive wave scan of the thread sums
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned before = carry_s;
        for (int k = 0; k < w; ++k) before += wsum[k];
        unsigned run = before + incl - s;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (i0 + k < m) hist[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (t == 1023) carry_s = run;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(RS_T) nn_rs_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                             unsigned* __restrict__ kout, unsigned* __restrict__ vout, const int n,
                                                             const int shift, const unsigned* __restrict__ hist, const int nblocks) {
    __shared__ unsigned run[256];
    __shared__ unsigned wcnt[RS_T / 64][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    run[t] = hist[t * nblocks + blockIdx.x];
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int base = blockIdx.x * RS_TILE;
    for (int c = 0; c < RS_ITEMS; ++c) {
        const int i = base + c * RS_T + t;   // element order = (chunk, wave, lane): ranks below follow it
        const bool valid = i < n;
        const unsigned key = valid ? kin[i] : 0u, val = valid ? vin[i] : 0u;
        const unsigned d = (key >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const unsigned rank = (unsigned)__popcll(peers & lt);
        const unsigned total = (unsigned)__popcll(peers);
#pragma unroll
        for (int k = 0; k < RS_T / 64; ++k) wcnt[k][t] = 0u;
        __syncthreads();
        if (valid && rank + 1 == total) wcnt[w][d] = total;   // one writer per (wave, digit)
        __syncthreads();
        if (valid) {
            unsigned pos = run[d] + rank;
            for (int k = 0; k < w; ++k) pos += wcnt[k][d];
            kout[pos] = key;
            vout[pos] = val;
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int k = 0; k < RS_T / 64; ++k) add += wcnt[k][t];
        run[t] += add;
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
// segments, points in key order, boxes
// --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nn_segments_kernel(const unsigned* __restrict__ keys, const int n, NnIndexHeader* __restrict__ h) {
    const int Q = h->n_quads, shift = h->key_shift;
    for (int q = threadIdx.x; q <= Q; q += 256) {   // seg[q] = lower_bound(keys, q << shift); q = Q: the finite count
        const unsigned target = (unsigned)q << shift;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < target) lo = mid + 1; else hi = mid;
        }
        h->seg[q] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int L = 1 << h->leaf_log2;
        int base = 0;
        for (int q = 0; q < Q; ++q) {
            const int cnt = h->seg[q + 1] - h->seg[q];
            const int leaves = (cnt + L - 1) / L;
            int p = 0, dpt = 0;
            if (leaves > 0) { p = 1; while (p < leaves) { p <<= 1; ++dpt; } }
            h->pow2[q] = p;
            h->depth[q] = dpt;
            h->node_base[q] = base;
            base += p > 0 ? 2 * p - 1 : 0;
        }
    }
}

__global__ void __launch_bounds__(256) nn_gather_kernel(const float* __restrict__ xyz, const unsigned* __restrict__ vals, const int n,
                                                        const long long pts_off, char* __restrict__ index) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = vals[i];
    reinterpret_cast<f32x4*>(index + pts_off)[i] = f32x4{xyz[j * 3 + 0], xyz[j * 3 + 1], xyz[j * 3 + 2], 0.f};
}

// One launch per tree height (0: the leaves), over the nodes of every quadrant at that height only: a thread maps its global index to
// (quadrant, node) through the per-quadrant prefix of node counts, which each block builds in LDS from the header.
__global__ void __launch_bounds__(256) nn_tree_level_kernel(char* __restrict__ index, const int height) {
    __shared__ int base[NNI_MAXQ + 1];
    const NnIndexHeader* h = reinterpret_cast<const NnIndexHeader*>(index);
    const int Q = h->n_quads;
    if (threadIdx.x == 0) {
        int b = 0;
        for (int q = 0; q < Q; ++q) {
            base[q] = b;
            b += h->pow2[q] >> height;
        }
        base[Q] = b;
    }
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= base[Q]) return;
    int lo = 0, hi = Q;   // the last q with base[q] <= j (empty quadrants share their successor's base)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= j) lo = mid; else hi = mid;
    }
    const int q = lo, P = h->pow2[q];
    const int width = P >> height, k = width + (j - base[q]);   // nodes at this height: k = width .. 2 width - 1
    f32x4* nb = reinterpret_cast<f32x4*>(index + h->nodes_off) + 2LL * h->node_base[q];
    f32x4 lo3 = {INFINITY, INFINITY, INFINITY, 0.f}, hi3 = {-INFINITY, -INFINITY, -INFINITY, 0.f};   // empty leaf: every bound is +inf
    if (height == 0) {
        const int L = 1 << h->leaf_log2;
        const int s0 = h->seg[q] + (k - P) * L, s1 = min(s0 + L, h->seg[q + 1]);
        const f32x4* pts = reinterpret_cast<const f32x4*>(index + h->pts_off);
        for (int s = s0; s < s1; ++s) {
            const f32x4 p = pts[s];
            lo3[0] = fminf(lo3[0], p[0]); lo3[1] = fminf(lo3[1], p[1]); lo3[2] = fminf(lo3[2], p[2]);
            hi3[0] = fmaxf(hi3[0], p[0]); hi3[1] = fmaxf(hi3[1], p[1]); hi3[2] = fmaxf(hi3[2], p[2]);
        }
    } else {
        const f32x4 alo = nb[2 * (2 * k - 1)], ahi = nb[2 * (2 * k - 1) + 1], blo = nb[2 * (2 * k)], bhi = nb[2 * (2 * k) + 1];
        lo3 = f32x4{fminf(alo[0], blo[0]), fminf(alo[1], blo[1]), fminf(alo[2], blo[2]), 0.f};
        hi3 = f32x4{fmaxf(ahi[0], bhi[0]), fmaxf(ahi[1], bhi[1]), fmaxf(ahi[2], bhi[2]), 0.f};
    }
    nb[2 * (k - 1)] = lo3;
    nb[2 * (k - 1) + 1] = hi3;
}

// --------------------------------------------------------------------------------------------------------------------------------
// query
// --------------------------------------------------------------------------------------------------------------------------------
// G lanes per query walk its quadrant's heap together (nn_walk.hpp, shared with slam.hip).
template <int G>
__global__ void __launch_bounds__(256) nn_index_query_kernel(const char* __restrict__ index, const float* __restrict__ q, const int n_q,
                                                             const int divider, float* out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / G), sub = (int)(t % G);   // a group never straddles a wave (G divides 64)
    if (i >= n_q) return;
    const int quad = divider > 0 ? reinterpret_cast<const int*>(out)[i] : 0;   // must3r_hip_quadrant_ids wrote the id here; read before the write
    const float qx = q[(long long)i * 3 + 0], qy = q[(long long)i * 3 + 1], qz = q[(long long)i * 3 + 2];
    const float best = nn_walk<G>(index, divider, quad, qx, qy, qz, sub);
    if (sub == 0) out[i] = sqrtf(best);   // sqrt(+inf) = +inf
}

template <int G>
void launch_query_g(const char* index, const float* q, long long n_q, int divider, float* out, hipStream_t s) {
    hipLaunchKernelGGL(nn_index_query_kernel<G>, dim3((unsigned)((n_q * G + 255) / 256)), dim3(256), 0, s, index, q, (int)n_q, divider, out);
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_nn_index_bytes(int64_t n, int divider) {
    if (n < 0 || n > NNI_MAX_N || divider < 0 || n_quads_of(divider) > NNI_MAXQ) return 0;
    const int Q = n_quads_of(divider);
    return NNI_HEADER_BYTES + (size_t)n * 16 + (size_t)node_cap_of(n, Q) * 32;
}

extern "C" size_t must3r_hip_nn_index_scratch_bytes(int64_t n) {
    if (n < 0 || n > NNI_MAX_N) return 0;
    return (size_t)n * 16 + (size_t)rs_blocks_of(n) * 256 * 4 + BB_BLOCKS * 6 * 4 + 256;
}

extern "C" int must3r_hip_nn_index_build(const float* xyz, const int32_t* qid, int64_t n, int divider, void* index, void* scratch, void* stream) {
    if (n < 0) return fail("nn_index_build: negative count");
    if (!index || (n > 0 && (!xyz || !scratch))) return fail("nn_index_build: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n < 0 || n > NNI_MAX_N) return fail("nn_index_build: point count outside [0, 2^30]");
    if (divider < 0 || n_quads_of(divider) > NNI_MAXQ) return fail("nn_index_build: divider outside [0, 8]");
    if (divider > 0 && n > 0 && !qid) return fail("nn_index_build: quadrant ids are needed when divider > 0");
    const int Q = n_quads_of(divider);
    const int leaf_log2 = opt(OPT_NN_LEAF_LOG2);
    int qbits = 0;
    while ((1 << qbits) <= Q) ++qbits;        // values 0 .. Q (Q: the dropped points' quadrant never appears as a real one)
    const int key_shift = 32 - qbits;
    const int morton_bits = key_shift;   // recorded in the header: the key's bits below the quadrant
    const long long node_cap = node_cap_of(n, Q);
    const long long pts_off = NNI_HEADER_BYTES, nodes_off = pts_off + n * 16;
    char* idx = reinterpret_cast<char*>(index);
    NnIndexHeader* h = reinterpret_cast<NnIndexHeader*>(idx);
    if (hipMemsetAsync(idx, 0, must3r_hip_nn_index_bytes(n, divider), s) != hipSuccess) return fail("nn_index_build: memset failed");
    const int ni = (int)n;
    unsigned* kA = reinterpret_cast<unsigned*>(scratch);
    unsigned* vA = kA + n;
    unsigned* kB = vA + n;
    unsigned* vB = kB + n;
    const int nblocks = (int)rs_blocks_of(n);
    unsigned* hist = vB + n;
    float* part = reinterpret_cast<float*>(hist + (size_t)nblocks * 256);
    // n = 0: scratch may be NULL and is not touched (no partial boxes; the header and the empty segments are still written)
    const int n_part = (int)((n + 255) / 256 < BB_BLOCKS ? (n + 255) / 256 : BB_BLOCKS);
    if (n > 0) hipLaunchKernelGGL(nn_bbox_partial_kernel, dim3(n_part), dim3(256), 0, s, xyz, n, part);
    hipLaunchKernelGGL(nn_bbox_final_kernel, dim3(1), dim3(256), 0, s, part, n_part, h, divider, Q, leaf_log2, key_shift, morton_bits, ni,
                       pts_off, nodes_off, node_cap);
    if (n > 0) {
        const unsigned g = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(nn_key_kernel, dim3(g), dim3(256), 0, s, xyz, divider > 0 ? qid : nullptr, ni, h, kA, vA);
        for (int pass = 0; pass < 4; ++pass) {
            const unsigned* ki = pass & 1 ? kB : kA;
            const unsigned* vi = pass & 1 ? vB : vA;
            unsigned* ko = pass & 1 ? kA : kB;
            unsigned* vo = pass & 1 ? vA : vB;
            hipLaunchKernelGGL(nn_rs_hist_kernel, dim3(nblocks), dim3(RS_T), 0, s, ki, ni, pass * 8, hist, nblocks);
            hipLaunchKernelGGL(nn_rs_scan_kernel, dim3(1), dim3(1024), 0, s, hist, nblocks * 256);
            hipLaunchKernelGGL(nn_rs_scatter_kernel, dim3(nblocks), dim3(RS_T), 0, s, ki, vi, ko, vo, ni, pass * 8, hist, nblocks);
        }
        // 4 passes: the sorted (key, index) pairs are back in (kA, vA)
        hipLaunchKernelGGL(nn_gather_kernel, dim3(g), dim3(256), 0, s, xyz, vA, ni, pts_off, idx);
    }
    hipLaunchKernelGGL(nn_segments_kernel, dim3(1), dim3(256), 0, s, kA, ni, h);
    if (n > 0) {
        // sum over quadrants of P_q (leaves padded to a power of two) < 2 (ceil(n / L) + Q); at height h the nodes number at most that >> h
        const long long leaves = (n + (1LL << leaf_log2) - 1) >> leaf_log2;
        const long long bound = 2 * (leaves + Q), maxP = next_pow2(leaves);
        for (int height = 0; (maxP >> height) > 0; ++height) {
            const long long nodes = (bound + (1LL << height) - 1) >> height;
            hipLaunchKernelGGL(nn_tree_level_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, s, idx, height);
        }
    }
    if (hipGetLastError() != hipSuccess) return fail("nn_index_build: launch failed");
    return 0;
}

extern "C" int must3r_hip_nn_index_query(const void* index, const float* q, int64_t n_q, const float* cam_center_host, int divider, float* out_dist,
                                         void* stream) {
    if (n_q < 0) return fail("nn_index_query: negative count");
    if (n_q == 0) return 0;
    if (!index || !q || !out_dist || (divider > 0 && !cam_center_host)) return fail("nn_index_query: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_q > NNI_MAX_N) return fail("nn_index_query: query count above 2^30");
    if (divider < 0 || n_quads_of(divider) > NNI_MAXQ) return fail("nn_index_query: divider outside [0, 8]");
    if (divider > 0 && must3r_hip_quadrant_ids(q, n_q, cam_center_host, divider, reinterpret_cast<int32_t*>(out_dist), stream)) return 1;
    const char* idx = reinterpret_cast<const char*>(index);
    switch (opt(OPT_NN_QUERY_LANES_LOG2)) {
        case 0: launch_query_g<1>(idx, q, n_q, divider, out_dist, s); break;
        case 1: launch_query_g<2>(idx, q, n_q, divider, out_dist, s); break;
        case 2: launch_query_g<4>(idx, q, n_q, divider, out_dist, s); break;
        case 3: launch_query_g<8>(idx, q, n_q, divider, out_dist, s); break;
        default: launch_query_g<16>(idx, q, n_q, divider, out_dist, s); break;
    }
    if (hipGetLastError() != hipSuccess) return fail("nn_index_query: launch failed");
    return 0;
}
