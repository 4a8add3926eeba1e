// Scene export (demo/gradio.py:75-156 get_3D_model_from_scene / _convert_scene_output_to_glb; dust3r.viz.pts3d_to_trimesh + cat_meshes):
// ordered stream compaction of the confident points (or of the surviving triangles) plus one fp64 affine map, written in file layout.
//
//   export_count_kernel<MESH>   one read of conf: per block of EXP_BLOCK pixels and per threshold k the number of passing pixels
//                               (MESH: of quads whose (a,b,c') resp. (b,c',d) corners all pass) -> counts[channel][block]
//   export_scan_kernel          one 1024-thread block per channel: exclusive prefix over the blocks in view-major order, in place,
//                               the channel's total at index n_blocks and in totals[channel]
//   export_points_kernel<PLY, ALL>  thread t of a block owns pixels 4t .. 4t+3: four ballots give the lane rank (popcount of the lower
//                               lanes' bits), the wave offsets go through LDS, so the output order is the pixel order.  Position in fp64
//                               with every operation rounded (this file is built with -ffp-contract=off), one rounding to fp32; colour
//                               rint(clip(c) * 255) in fp32.  Per-block min / max partials of the written positions (plain vector stores).
//                               ALL: every pixel, index = vertex base + pixel (the mesh's vertex planes).
//   export_minmax_kernel        the partials -> 6 floats
//   export_faces_kernel         the same ordered compaction over the two triangle kinds; each kind writes its two windings
//
// Bandwidth kernels: 16-byte loads where the view's planes are 16-byte aligned (conf: 4 pixels = one float4; pts / rgb: 4 pixels = three
// float4), scalar loads otherwise and at a view's tail.  Scratch layout (export_plan): [device view table][prefix channels x (n_blocks+1)
// uint32][totals channels x int64][partials n_blocks x 6 float].
#include <vector>
#include <cstdint>
#include "abi.hpp"
#include "common.hpp"
#include "scene_load.hpp"

namespace m3r {
namespace {

constexpr int EXP_T = 256;                       // threads per block
constexpr int EXP_PPT = 4;                       // consecutive pixels per thread
constexpr int EXP_BLOCK = EXP_T * EXP_PPT;       // pixels per block
static_assert(EXP_BLOCK == MUST3R_EXPORT_BLOCK, "header and kernel disagree on the block size");
constexpr int EXP_MAXK = MUST3R_EXPORT_MAX_THR;

struct ExpView {                                 // device view table entry
    const float* conf;
    const float* pts;
    const float* rgb;
    int H, W;
    unsigned block_base;                         // first block of the view
    unsigned n_pix;
    unsigned long long vert_base;                // pixels of the views before
    double M[12];
};

struct ExpThr { float v[EXP_MAXK]; };

struct ExpPlan {
    long long n_blocks, n_pix;
    int channels;
    size_t off_prefix, off_totals, off_partials, bytes;
};

// view of a block: the last view whose block_base <= b
__device__ __forceinline__ int view_of_block(const ExpView* __restrict__ views, const int n_views, const unsigned b) {
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].block_base <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long lanemask_lt() {
    const unsigned lane = threadIdx.x & 63;
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// Ordered ranks inside a block for four flags per thread, in thread-major order (thread t's four flags come before thread t+1's): returns
// the number of set flags before this thread's first one.  The four ballots of the lower lanes summed are exactly the flags of the
// threads before this one in its wave; the waves before it add their totals through s_wave (EXP_T / 64 unsigned of LDS).  Every thread
// of the block must call it.
__device__ __forceinline__ unsigned block_rank4(const bool (&f)[4], unsigned* s_wave) {
    const unsigned long long lt = lanemask_lt();
    unsigned below = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long b = __ballot(f[j]);
        below += __popcll(b & lt);
        wave_total += __popcll(b);
    }
    const unsigned wave = threadIdx.x >> 6;
    __syncthreads();                              // s_wave may still be read from the call before
    if ((threadIdx.x & 63) == 0) s_wave[wave] = wave_total;
    __syncthreads();
    unsigned off = 0;
#pragma unroll
    for (int w = 0; w < EXP_T / 64; ++w) off += w < (int)wave ? s_wave[w] : 0u;
    return off + below;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// corners of the quad anchored at pixel i of a view (r < H-1, c < W-1): a = i, b = i+1, c' = i+W, d = i+W+1
template <bool MESH>
__global__ void __launch_bounds__(EXP_T) export_count_kernel(const ExpView* __restrict__ views, const int n_views, const ExpThr thr, const int K,
                                                             unsigned* __restrict__ prefix, const long long stride) {
    constexpr int NCH = MESH ? 2 * EXP_MAXK : EXP_MAXK;     // channels: mesh counts two triangle kinds per threshold
    __shared__ unsigned s_cnt[EXP_T / 64][NCH];
    const unsigned b = blockIdx.x;
    const ExpView& v = views[view_of_block(views, n_views, b)];
    const unsigned n = v.n_pix, i0 = (b - v.block_base) * EXP_BLOCK + threadIdx.x * EXP_PPT;
    unsigned cnt[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) cnt[k] = 0;
    if (!MESH) {
        float c[4];
        load4(v.conf, i0, n, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < n;
#pragma unroll
            for (int k = 0; k < EXP_MAXK; ++k) cnt[k] += (k < K && in && c[j] >= thr.v[k]) ? 1u : 0u;
        }
    } else {
        const unsigned W = (unsigned)v.W, H = (unsigned)v.H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = i0 + j;
            if (i >= n) continue;
            const unsigned r = i / W, c = i - r * W;
            if (r + 1 >= H || c + 1 >= W) continue;
            const float ca = v.conf[i], cb = v.conf[i + 1], cc = v.conf[i + W], cd = v.conf[i + W + 1];
#pragma unroll
            for (int k = 0; k < EXP_MAXK; ++k) {
                if (k >= K) continue;
                const float t = thr.v[k];
                const bool bc = cb >= t && cc >= t;
                cnt[2 * k] += (bc && ca >= t) ? 1u : 0u;
                cnt[2 * k + 1] += (bc && cd >= t) ? 1u : 0u;
            }
        }
    }
    const int C = MESH ? 2 * K : K;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned s = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < EXP_T / 64; ++w) s += s_cnt[w][threadIdx.x];
        prefix[threadIdx.x * stride + b] = s;
    }
}

// exclusive prefix of one channel's n counts, in place; p[n] and totals[channel] = the sum
__global__ void __launch_bounds__(1024) export_scan_kernel(unsigned* __restrict__ prefix, const long long stride, const long long n,
                                                           long long* __restrict__ totals) {
    __shared__ unsigned s_wave[16];
    __shared__ unsigned s_carry;
    unsigned* p = prefix + blockIdx.x * stride;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + threadIdx.x;
        const unsigned x = i < n ? p[i] : 0u;
        unsigned inc = x;                         // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(inc, o, 64);
            if (lane >= (unsigned)o) inc += y;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned off = s_carry, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned c = s_wave[w];
            if (w < (int)wave) off += c;
            tot += c;
        }
        if (i < n) p[i] = off + inc - x;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        p[n] = s_carry;
        totals[blockIdx.x] = (long long)s_carry;
    }
}

__device__ __forceinline__ float affine_row(const double* __restrict__ m, const float x, const float y, const float z) {
    // ((m0 x + m1 y) + m2 z) + m3, each operation rounded in fp64 (no contraction in this file), then one rounding to fp32
    const double a = m[0] * (double)x, b = m[1] * (double)y, c = m[2] * (double)z;
    return (float)(((a + b) + c) + m[3]);
}

template <bool PLY, bool ALL>
__global__ void __launch_bounds__(EXP_T) export_points_kernel(const ExpView* __restrict__ views, const int n_views, const float thr,
                                                              const unsigned* __restrict__ prefix, float* __restrict__ out_pos,
                                                              unsigned* __restrict__ out_col, float* __restrict__ partials) {
    __shared__ unsigned s_wave[EXP_T / 64];
    __shared__ float s_mm[EXP_T / 64][6];
    const unsigned b = blockIdx.x;
    const ExpView& v = views[view_of_block(views, n_views, b)];
    const unsigned n = v.n_pix, i0 = (b - v.block_base) * EXP_BLOCK + threadIdx.x * EXP_PPT;
    bool f[4];
    if (ALL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = i0 + j < n;
    } else {
        float c[4];
        load4(v.conf, i0, n, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = i0 + j < n && c[j] >= thr;
    }
    unsigned long long o;
    if (ALL) {
        o = v.vert_base + i0;
    } else {
        o = (unsigned long long)prefix[b] + block_rank4(f, s_wave);
    }
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (f[0] || f[1] || f[2] || f[3]) {
        float p[12], c[12];
        load12(v.pts, i0, n, p);
        load12(v.rgb, i0, n, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!f[j]) continue;
            float q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                q[a] = affine_row(v.M + 4 * a, p[3 * j], p[3 * j + 1], p[3 * j + 2]);
                mn[a] = fminf(mn[a], q[a]);
                mx[a] = fmaxf(mx[a], q[a]);
            }
            const unsigned col = quant8(c[3 * j]) | (quant8(c[3 * j + 1]) << 8) | (quant8(c[3 * j + 2]) << 16) | 0xff000000u;
            if (PLY) {
                uint4 rec;
                rec.x = __float_as_uint(q[0]); rec.y = __float_as_uint(q[1]); rec.z = __float_as_uint(q[2]); rec.w = col;
                reinterpret_cast<uint4*>(out_pos)[o] = rec;
            } else {
                out_pos[3 * o] = q[0]; out_pos[3 * o + 1] = q[1]; out_pos[3 * o + 2] = q[2];
                out_col[o] = col;
            }
            ++o;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], s, 64));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], s, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_mm[threadIdx.x >> 6][a] = mn[a]; s_mm[threadIdx.x >> 6][3 + a] = mx[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = s_mm[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EXP_T / 64; ++w) r = threadIdx.x < 3 ? fminf(r, s_mm[w][threadIdx.x]) : fmaxf(r, s_mm[w][threadIdx.x]);
        partials[6ull * b + threadIdx.x] = r;
    }
}

__global__ void __launch_bounds__(1024) export_minmax_kernel(const float* __restrict__ partials, const long long n_blocks, float* __restrict__ out) {
    __shared__ float s_mm[16][6];
    float r[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (long long i = threadIdx.x; i < n_blocks; i += 1024) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            r[a] = fminf(r[a], partials[6 * i + a]);
            r[3 + a] = fmaxf(r[3 + a], partials[6 * i + 3 + a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float y = __shfl_xor(r[a], s, 64);
            r[a] = a < 3 ? fminf(r[a], y) : fmaxf(r[a], y);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 6; ++a) s_mm[threadIdx.x >> 6][a] = r[a];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float x = s_mm[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) x = threadIdx.x < 3 ? fminf(x, s_mm[w][threadIdx.x]) : fmaxf(x, s_mm[w][threadIdx.x]);
        out[threadIdx.x] = x;
    }
}

// prefix1 / prefix2: the scanned channels of the two triangle kinds at this threshold
__global__ void __launch_bounds__(EXP_T) export_faces_kernel(const ExpView* __restrict__ views, const int n_views, const float thr,
                                                             const unsigned* __restrict__ prefix1, const unsigned* __restrict__ prefix2,
                                                             unsigned* __restrict__ out) {
    __shared__ unsigned s_wave[EXP_T / 64];
    const unsigned b = blockIdx.x;
    const int vi = view_of_block(views, n_views, b);
    const ExpView& v = views[vi];
    const unsigned n = v.n_pix, i0 = (b - v.block_base) * EXP_BLOCK + threadIdx.x * EXP_PPT;
    const unsigned W = (unsigned)v.W, H = (unsigned)v.H;
    bool f1[4], f2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned i = i0 + j;
        f1[j] = f2[j] = false;
        if (i >= n) continue;
        const unsigned r = i / W, c = i - r * W;
        if (r + 1 >= H || c + 1 >= W) continue;
        const bool bc = v.conf[i + 1] >= thr && v.conf[i + W] >= thr;
        f1[j] = bc && v.conf[i] >= thr;
        f2[j] = bc && v.conf[i + W + 1] >= thr;
    }
    const unsigned r1 = block_rank4(f1, s_wave);
    const unsigned r2 = block_rank4(f2, s_wave);
    // the view's first and one-past-last blocks bound its counts; the views before hold 2 (n1 + n2) faces
    const unsigned bb = v.block_base, be = vi + 1 < n_views ? views[vi + 1].block_base : gridDim.x;
    const unsigned long long p1 = prefix1[bb], p2 = prefix2[bb];
    const unsigned long long n1 = prefix1[be] - p1, n2 = prefix2[be] - p2;
    const unsigned long long face0 = 2ull * (p1 + p2);
    unsigned long long o1 = face0 + (prefix1[b] - p1) + r1;
    unsigned long long o2 = face0 + 2ull * n1 + (prefix2[b] - p2) + r2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned ia = (unsigned)(v.vert_base + i0 + j), ib = ia + 1, ic = ia + W, id = ic + 1;
        if (f1[j]) {
            unsigned* t = out + 3ull * o1;
            t[0] = ia; t[1] = ib; t[2] = ic;
            t = out + 3ull * (o1 + n1);
            t[0] = ic; t[1] = ib; t[2] = ia;
            ++o1;
        }
        if (f2[j]) {
            unsigned* t = out + 3ull * o2;
            t[0] = ib; t[1] = ic; t[2] = id;
            t = out + 3ull * (o2 + n2);
            t[0] = id; t[1] = ic; t[2] = ib;
            ++o2;
        }
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates the table and lays the scratch out; 0 = fine
int export_plan(const must3r_hip_export_view* views, int n_views, int n_thr, int mesh, ExpPlan* p) {
    if (!views) return fail("export: null view table");
    if (n_views <= 0) return fail("export: the view table is empty");
    if (n_thr < 1 || n_thr > EXP_MAXK) return fail("export: the number of thresholds is outside [1, 8]");
    long long blocks = 0, pix = 0;
    for (int i = 0; i < n_views; ++i) {
        const must3r_hip_export_view& v = views[i];
        if (v.H <= 0 || v.W <= 0) return fail("export: a view has a non-positive size");
        const long long n = (long long)v.H * v.W;
        if (n >= (1LL << 31)) return fail("export: a view has 2^31 or more pixels");
        pix += n;
        blocks += (n + EXP_BLOCK - 1) / EXP_BLOCK;
        if (pix >= (1LL << 32)) return fail("export: the scene has 2^32 or more vertices (uint32 indices)");
    }
    p->n_blocks = blocks;
    p->n_pix = pix;
    p->channels = mesh ? 2 * n_thr : n_thr;
    size_t off = align256((size_t)n_views * sizeof(ExpView));
    p->off_prefix = off;
    off = align256(off + (size_t)p->channels * (size_t)(blocks + 1) * sizeof(unsigned));
    p->off_totals = off;
    off = align256(off + (size_t)p->channels * sizeof(long long));
    p->off_partials = off;
    off = align256(off + (size_t)blocks * 6 * sizeof(float));
    p->bytes = off;
    return 0;
}

int check_pointers(const must3r_hip_export_view* views, int n_views) {
    for (int i = 0; i < n_views; ++i)
        if (!views[i].conf || !views[i].pts || !views[i].rgb) return fail("export: a view has a null plane");
    return 0;
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_export_scratch_bytes(const must3r_hip_export_view* views, int n_views, int n_thr, int mesh) {
    ExpPlan p;
    if (export_plan(views, n_views, n_thr, mesh, &p)) return 0;
    return p.bytes;
}

extern "C" int must3r_hip_export_count(const must3r_hip_export_view* views, int n_views, const float* thr, int n_thr, int mesh, void* scratch,
                                       size_t scratch_bytes, int64_t* totals_host, void* stream) {
    if (!totals_host) return fail("export_count: null argument");
    ExpPlan p;
    if (export_plan(views, n_views, n_thr, mesh, &p)) return 1;
    if (!thr || !scratch) return fail("export_count: null argument");
    if (check_pointers(views, n_views)) return 1;
    if (scratch_bytes < p.bytes) return fail("export_count: scratch too small");
    std::vector<ExpView> table((size_t)n_views);
    unsigned bb = 0;
    unsigned long long vb = 0;
    for (int i = 0; i < n_views; ++i) {
        ExpView& d = table[i];
        d.conf = views[i].conf; d.pts = views[i].pts; d.rgb = views[i].rgb;
        d.H = views[i].H; d.W = views[i].W;
        d.n_pix = (unsigned)((long long)d.H * d.W);
        d.block_base = bb; d.vert_base = vb;
        for (int j = 0; j < 12; ++j) d.M[j] = views[i].M[j];
        bb += (d.n_pix + EXP_BLOCK - 1) / EXP_BLOCK;
        vb += d.n_pix;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* sc = reinterpret_cast<char*>(scratch);
    ExpView* dv = reinterpret_cast<ExpView*>(sc);
    unsigned* prefix = reinterpret_cast<unsigned*>(sc + p.off_prefix);
    long long* totals = reinterpret_cast<long long*>(sc + p.off_totals);
    if (hipMemcpyAsync(dv, table.data(), table.size() * sizeof(ExpView), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail("export_count: view table upload failed");
    ExpThr t;
    for (int k = 0; k < EXP_MAXK; ++k) t.v[k] = k < n_thr ? thr[k] : INFINITY;
    const long long stride = p.n_blocks + 1;
    if (mesh) hipLaunchKernelGGL(export_count_kernel<true>, dim3((unsigned)p.n_blocks), dim3(EXP_T), 0, s, dv, n_views, t, n_thr, prefix, stride);
    else hipLaunchKernelGGL(export_count_kernel<false>, dim3((unsigned)p.n_blocks), dim3(EXP_T), 0, s, dv, n_views, t, n_thr, prefix, stride);
    hipLaunchKernelGGL(export_scan_kernel, dim3(p.channels), dim3(1024), 0, s, prefix, stride, p.n_blocks, totals);
    if (hipGetLastError() != hipSuccess) return fail("export_count: launch failed");
    long long tot[2 * EXP_MAXK];
    // the table vector must outlive its upload: the stream is drained here, before it goes out of scope
    if (hipMemcpyAsync(tot, totals, (size_t)p.channels * sizeof(long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail("export_count: reading the totals failed");
    for (int k = 0; k < n_thr; ++k) totals_host[k] = mesh ? 2 * (tot[2 * k] + tot[2 * k + 1]) : tot[k];
    return 0;
}

// the points that pass threshold k in either layout (all = 0), or every vertex of the mesh in the GLB layout (all = 1)
static int launch_export_points(const must3r_hip_export_view* views, int n_views, const float* thr, int n_thr, int k, int layout, int all,
                                const void* scratch, void* out_pos, void* out_col, float* minmax, void* stream) {
    ExpPlan p;
    const int mesh = all ? 1 : 0;
    if (export_plan(views, n_views, n_thr, mesh, &p)) return 1;
    if (!scratch || !out_pos || !minmax || (!all && !thr)) return fail("export_scatter: null argument");
    if (!all && (k < 0 || k >= n_thr)) return fail("export_scatter: threshold index outside the count's");
    if (layout != MUST3R_EXPORT_GLB && layout != MUST3R_EXPORT_PLY) return fail("export_scatter: unknown layout");
    if (layout == MUST3R_EXPORT_GLB && !out_col) return fail("export_scatter: the GLB layout needs a colour plane");
    if (layout == MUST3R_EXPORT_PLY && (reinterpret_cast<uintptr_t>(out_pos) & 15)) return fail("export_scatter: PLY records must be 16-byte aligned");
    const char* sc = reinterpret_cast<const char*>(scratch);
    const ExpView* dv = reinterpret_cast<const ExpView*>(sc);
    const unsigned* prefix = reinterpret_cast<const unsigned*>(sc + p.off_prefix) + (all ? 0 : (size_t)k * (size_t)(p.n_blocks + 1));
    float* partials = const_cast<float*>(reinterpret_cast<const float*>(sc + p.off_partials));
    const float t = all ? 0.f : thr[k];
    const dim3 g((unsigned)p.n_blocks), b(EXP_T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* op = reinterpret_cast<float*>(out_pos);
    unsigned* oc = reinterpret_cast<unsigned*>(out_col);
    if (all) hipLaunchKernelGGL((export_points_kernel<false, true>), g, b, 0, s, dv, n_views, t, prefix, op, oc, partials);
    else if (layout == MUST3R_EXPORT_PLY) hipLaunchKernelGGL((export_points_kernel<true, false>), g, b, 0, s, dv, n_views, t, prefix, op, oc, partials);
    else hipLaunchKernelGGL((export_points_kernel<false, false>), g, b, 0, s, dv, n_views, t, prefix, op, oc, partials);
    hipLaunchKernelGGL(export_minmax_kernel, dim3(1), dim3(1024), 0, s, partials, p.n_blocks, minmax);
    if (hipGetLastError() != hipSuccess) return fail("export_scatter: launch failed");
    return 0;
}

extern "C" int must3r_hip_export_scatter_points(const must3r_hip_export_view* views, int n_views, const float* thr, int n_thr, int k, int layout,
                                                const void* scratch, void* out_pos, void* out_col, float* minmax, void* stream) {
    return launch_export_points(views, n_views, thr, n_thr, k, layout, 0, scratch, out_pos, out_col, minmax, stream);
}

extern "C" int must3r_hip_export_vertices(const must3r_hip_export_view* views, int n_views, int n_thr, void* scratch, float* out_pos, void* out_col,
                                          float* minmax, void* stream) {
    return launch_export_points(views, n_views, nullptr, n_thr, 0, MUST3R_EXPORT_GLB, 1, scratch, out_pos, out_col, minmax, stream);
}

extern "C" int must3r_hip_export_scatter_faces(const must3r_hip_export_view* views, int n_views, const float* thr, int n_thr, int k,
                                               const void* scratch, uint32_t* out_faces, void* stream) {
    ExpPlan p;
    if (export_plan(views, n_views, n_thr, 1, &p)) return 1;
    if (!scratch || !out_faces || !thr) return fail("export_scatter_faces: null argument");
    if (k < 0 || k >= n_thr) return fail("export_scatter_faces: threshold index outside the count's");
    const char* sc = reinterpret_cast<const char*>(scratch);
    const ExpView* dv = reinterpret_cast<const ExpView*>(sc);
    const size_t stride = (size_t)(p.n_blocks + 1);
    const unsigned* prefix = reinterpret_cast<const unsigned*>(sc + p.off_prefix);
    hipLaunchKernelGGL(export_faces_kernel, dim3((unsigned)p.n_blocks), dim3(EXP_T), 0, reinterpret_cast<hipStream_t>(stream), dv, n_views, thr[k],
                       prefix + (size_t)(2 * k) * stride, prefix + (size_t)(2 * k + 1) * stride, out_faces);
    if (hipGetLastError() != hipSuccess) return fail("export_scatter_faces: launch failed");
    return 0;
}
