// postprocess(compute_cam=True) -- must3r/engine/inference.py:16-48 -- as ONE launch per group of views.
//
// Per view: activation (norm_exp on ch 0:3 and 3:6, conf = 1 + exp(ch 6), tools/geometry.py:14-18), focal by the
// Weiszfeld / IRLS scheme of dust3r's estimate_focal_knowing_depth (closed-form L2 start + 10 re-weighted steps), and the
// weighted rigid registration pts3d_local -> pts3d of roma.rigid_points_registration (weights conf - 1), assembled
// into c2w.  oracle/cam_ref.py states both third-party algorithms.
//
// HBM-bound: 28 B read + 28 B written per pixel, once.  The 11 global reductions of the focal iteration are what the
// reference pays 11 full passes over H*W for; here a view is spread over G persistent blocks (cooperative launch, all
// co-resident), every block keeps the (x/z, y/z) of its <= 16 x 1024 pixels in LDS (128 KB), and an iteration costs one
// block reduction + one per-view barrier (arrive counter + partials through agent-scope atomics) + a fixed-order sum of G partials
// (deterministic; no floating-point atomics).  All sums are accumulated in fp64 -- the reference's are fp32.  The
// per-pixel terms of the focal iteration are the reference's fp32 expressions.  Those of the registration are NOT:
// the reference centres x and y before it forms M = sum w (y - ybar)(x - xbar)^T; here the data pass (which cannot
// know the means yet) accumulates the uncentred moments sum fl(w y_i) x_j and subtracts ybar xbar^T in the solve.
// The fp32 rounding of w * y_i therefore scales with |y|, not with |y - ybar|, and the centring does not take it
// out again: the rotation's error grows linearly with the distance of the world points from the origin, in units
// of the scene's extent.  Emulated at 64x96 and 384x512 (tests/cam_cases.py), rotation error against fp64:
//   offset 0: 3e-8, the fp32 rounding of the stored R (fp32 reference 3e-7 .. 8e-7),
//   offset 100 extents: 2e-8 .. 2.5e-7 (2e-7 .. 7e-7), offset 10 000 extents: 1.6e-6 .. 2.5e-5 (1e-7 .. 3e-7).
// Up to some hundred extents this is inside the fp32 reference's own error (tests/test_cam_gpu.py pins offset 100);
// at 10 000 it is not.  The cure, should such scenes appear, is a per-view pilot point (e.g. the view's first y)
// subtracted from every y before the products and added back to ybar: M is invariant under that shift.
// The 3x3 Procrustes problem is solved by one thread per view
// with Horn's quaternion form (largest eigenvector of a 4x4 symmetric matrix, cyclic Jacobi in fp64), which equals
// U diag(1,1,det(UV^T)) V^T of the SVD form without the sign case analysis.
#include "abi.hpp"
#include "cam_solve.hpp"
#include "common.hpp"

namespace m3r {

constexpr int CAM_T = 1024;        // threads per block
constexpr int CAM_PPT = 16;        // pixels cached per thread (upper bound; CAM_T * CAM_PPT * 8 B = 128 KB of LDS)
constexpr int CAM_NSUM = 18;       // sum w, w*x[3], w*y[3], w*y*x^T[9], sum a, sum b
constexpr int CAM_ITERS = 10;
typedef double dbl2 __attribute__((ext_vector_type(2)));

struct CamArgs {
    const float* pm;      // [V, P, 7]
    float* p3;            // [V, P, 3]
    float* pl;            // [V, P, 3]
    float* cf;            // [V, P]
    double* sums;         // [V] final focal (input of cam_solve_kernel, which also reads buffer 0 of `partial`)
    double* partial;      // [V][G][16] per-block partial registration sums (summed by cam_solve_kernel)
    dbl2* slots;       // [V][3][G] pair exchange slots, all-ones before the launch
    int V, G, H, W, ppt;
    int linear;           // ActivationType.LINEAR (head.py:13-21): channels 0:3 / 3:6 pass through; conf = 1 + exp(ch 6) either way
};

__device__ __forceinline__ void norm_exp3c(const float* v, float* o) {
    const float d = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float sc = expm1f(d) / fmaxf(d, 1e-8f);
    o[0] = v[0] * sc;
    o[1] = v[1] * sc;
    o[2] = v[2] * sc;
}

// sum over the block of n (<= CAM_NSUM) doubles per thread; result valid in red[0..n) for every thread after return
template <int N>
__device__ __forceinline__ void block_sum(double* vals, double* red /* [16][N] */, double* out /* [N] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = vals[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave * N + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < CAM_T / 64; ++w) s += red[w * N + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// Exchange of one (a, b) pair per block per step between the G blocks of a view, without a counter and without fences.
// Block g owns slot g of the step's buffer (3 buffers, step n uses n % 3): it publishes its pair with ONE 16-byte
// L2-bypassing store (sc1: agent-coherent across the 8 XCDs); thread t of every block polls slot t until both halves
// differ from the all-ones sentinel the host memset left there, so all G slots are polled in parallel and a torn store
// cannot be mistaken for data.  After consuming step n a block re-arms its slot of buffer (n + 2) % 3 = buffer of step
// n - 1, which every block has finished reading (they all published step n); it is written again at step n + 2, two
// __syncthreads (vmcnt(0)) later.  The fenced alternative -- agent-scope release/acquire around an arrive counter --
// costs a full L2 write-back / invalidate scan per wave per step on gfx950 and measured 20x the data pass.
// The cooperative launch guarantees the peers are resident; the spin bound only turns a broken guarantee (e.g. a
// CU-masked stream) into wrong numbers instead of a hung device.
constexpr long long CAM_SENTINEL = -1LL;

__device__ __forceinline__ void slot_store(dbl2* p, dbl2 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ dbl2 slot_load(const dbl2* p) {
    dbl2 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// publish this block's pair for `step`, collect everybody's, sum in block order (deterministic); result in out[0..1]
__device__ __forceinline__ void exchange_pair(dbl2* slots /* [3][G] of the view */, int G, int g, int step, const double* mine,
                                              dbl2* stage /* [G] */, double* out) {
    dbl2* buf = slots + (size_t)(step % 3) * G;
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-arm store of this slot (two steps ago) has landed
        slot_store(buf + g, dbl2{mine[0], mine[1]});
    }
    for (int idx = threadIdx.x; idx < G; idx += CAM_T) {
        dbl2 d = slot_load(buf + idx);
        for (unsigned spins = 0; (__double_as_longlong(d.x) == CAM_SENTINEL || __double_as_longlong(d.y) == CAM_SENTINEL) && spins < (1u << 22); ++spins) {
            __builtin_amdgcn_s_sleep(1);
            d = slot_load(buf + idx);
        }
        stage[idx] = d;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int b = 0; b < G; ++b) s += threadIdx.x ? stage[b].y : stage[b].x;
        out[threadIdx.x] = s;
    }
    if (threadIdx.x == 0 && step >= 1)   // re-arm the slot of step - 1 for step + 2
        slot_store(slots + (size_t)((step + 2) % 3) * G + g, dbl2{__longlong_as_double(CAM_SENTINEL), __longlong_as_double(CAM_SENTINEL)});
    __syncthreads();
}

__device__ __forceinline__ void put(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One block (64 threads) per view: lanes 0..15 add up the G per-block partials of the registration sums in block
// order, lane 0 solves (cam_solve.hpp, shared with slam.hip).
__global__ void __launch_bounds__(64) cam_solve_kernel(const double* __restrict__ partial, const double* __restrict__ focal_in, int G,
                                                       float* __restrict__ focal_out, float* __restrict__ c2w_out) {
    __shared__ double S4[4][16];
    __shared__ double S[16];
    const int v = blockIdx.x;
    cam_sum_partials(partial + (size_t)v * G * 16, G, S4, S);
    if (threadIdx.x != 0) return;
    cam_register<false>(S, 1.0, c2w_out + (size_t)v * 16);
    focal_out[v] = (float)focal_in[v];
}

__global__ void __launch_bounds__(CAM_T) cam_kernel(const CamArgs p) {
    __shared__ float2 qs[CAM_PPT * CAM_T];   // (x/z, y/z) of this block's pixels: slot k * CAM_T + thread
    __shared__ double red[(CAM_T / 64) * CAM_NSUM];
    __shared__ double tot[CAM_NSUM];
    __shared__ dbl2 stage[512];           // exchange_pair staging (G <= 512)
    const int v = blockIdx.x / p.G, g = blockIdx.x - v * p.G;
    const int P = p.H * p.W;
    const size_t base = (size_t)v * P;
    const float ppx = 0.5f * (float)p.W, ppy = 0.5f * (float)p.H;
    const int stride = p.G * CAM_T;

    double acc[CAM_NSUM];
#pragma unroll
    for (int k = 0; k < CAM_NSUM; ++k) acc[k] = 0.0;
    for (int k = 0; k < p.ppt; ++k) {
        const int i = g * CAM_T + threadIdx.x + k * stride;
        if (i < P) {
            const float* src = p.pm + (base + i) * 7;
            float r[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) r[c] = src[c];
            float y[3], x[3];
            if (p.linear) {            // block-uniform
#pragma unroll
                for (int k = 0; k < 3; ++k) { y[k] = r[k]; x[k] = r[3 + k]; }
            } else {
                norm_exp3c(r, y);          // pts3d (world)
                norm_exp3c(r + 3, x);      // pts3d_local (camera)
            }
            const float conf = 1.0f + expf(r[6]);
            float* o3 = p.p3 + (base + i) * 3;
            float* ol = p.pl + (base + i) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o3[c] = y[c];
                ol[c] = x[c];
            }
            p.cf[base + i] = conf;
            const float w = conf - 1.0f;           // the reference's weight: (1 + e^v) - 1 in fp32
            float a = x[0] / x[2], b = x[1] / x[2];
            a = (fabsf(a) <= 3.402823466e38f) ? a : 0.f;   // nan_to_num(nan=0, posinf=0, neginf=0)
            b = (fabsf(b) <= 3.402823466e38f) ? b : 0.f;
            qs[k * CAM_T + threadIdx.x] = make_float2(a, b);
            const float u = (float)(i % p.W) - ppx, vv = (float)(i / p.W) - ppy;
            acc[0] += (double)w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[1 + c] += (double)(w * x[c]);
                acc[4 + c] += (double)(w * y[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int d = 0; d < 3; ++d) acc[7 + c * 3 + d] += (double)(w * y[c]) * (double)x[d];
            acc[16] += (double)(a * u + b * vv);
            acc[17] += (double)(a * a + b * b);
        }
    }
    double* part = p.partial + ((size_t)v * p.G + g) * 16;
    dbl2* slots = p.slots + (size_t)v * 3 * p.G;
    block_sum<CAM_NSUM>(acc, red, tot);
    if (threadIdx.x < 16) put(part + threadIdx.x, tot[threadIdx.x]);
    __shared__ double pair[2];
    exchange_pair(slots, p.G, g, 0, tot + 16, stage, pair);
    float focal = (float)(pair[0] / pair[1]);   // mean(a)/mean(b): the 1/P cancels

    // pixel (column, row) of slot k advances by a fixed (dcol, drow) -- no integer division in the iteration loop
    const int i0 = g * CAM_T + threadIdx.x;
    const int col0 = i0 % p.W, row0 = i0 / p.W, dcol = stride % p.W, drow = stride / p.W;
    for (int it = 0; it < CAM_ITERS; ++it) {
        // per-thread partial sums of <= 16 terms in fp32, everything across threads / blocks in fp64
        float sa = 0.f, sb = 0.f;
        int col = col0, row = row0, i = i0;
        for (int k = 0; k < p.ppt; ++k) {
            if (i < P) {
                const float2 q = qs[k * CAM_T + threadIdx.x];
                const float u = (float)col - ppx, vv = (float)row - ppy;
                const float dx = u - focal * q.x, dy = vv - focal * q.y;
                // w = 1 / max(|d|, 1e-8) = rsqrt(max(|d|^2, 1e-16))
                const float w = __builtin_amdgcn_rsqf(fmaxf(dx * dx + dy * dy, 1e-16f));
                sa += w * (q.x * u + q.y * vv);
                sb += w * (q.x * q.x + q.y * q.y);
            }
            i += stride;
            col += dcol;
            row += drow;
            if (col >= p.W) {
                col -= p.W;
                ++row;
            }
        }
        double it_acc[2] = {(double)sa, (double)sb};
        block_sum<2>(it_acc, red, tot);
        exchange_pair(slots, p.G, g, it + 1, tot, stage, pair);
        focal = (float)(pair[0] / pair[1]);
    }
    if (g == 0 && threadIdx.x == 0) p.sums[v] = (double)focal;
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_postprocess_cam_scratch_bytes(int n_views, int H, int W) {
    if (n_views <= 0 || H <= 0 || W <= 0) return 0;
    const int P = H * W;
    const int gmax = (P + CAM_T - 1) / CAM_T;
    // partials sized for the largest G any launch can pick, + one counter per view
    // [V][3][gmax] slots (16 B) + [V][gmax][16] partial sums + [V] focal
    return (size_t)n_views * gmax * (3 * 16 + 16 * 8) + (size_t)n_views * 8 + 256;
}

int m3r::cam_data_pass(const char* who, const float* pm, int activation, int n_views, int H, int W, float* p3, float* pl, float* cf, void* scratch,
                       size_t scratch_bytes, hipStream_t s, cam_solve_fn solve, void* user) {
    if (n_views < 0 || H <= 0 || W <= 0) return fail("%s: bad shape", who);
    if (activation != MUST3R_ACT_NORM_EXP && activation != MUST3R_ACT_LINEAR) return fail("%s: unknown activation %d", who, activation);
    if (n_views == 0) return 0;
    if (!pm || !p3 || !pl || !cf || !scratch) return fail("%s: null argument", who);
    const int P = H * W;
    if (P <= 0) return fail("%s: empty image", who);
    if (scratch_bytes < must3r_hip_postprocess_cam_scratch_bytes(n_views, H, W)) return fail("%s: scratch too small", who);
    int dev = 0, ncu = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cam_kernel, CAM_T, 0) != hipSuccess || per_cu < 1)
        return fail("%s: occupancy query failed", who);
    const int slots = ncu * per_cu;                                   // blocks that can be resident together
    const int gmin = (P + CAM_T * CAM_PPT - 1) / (CAM_T * CAM_PPT);   // fewest blocks per view (register cache bound)
    const int gmax = (P + CAM_T - 1) / CAM_T;
    if (gmin > slots) return fail("%s: image too large for the per-view register cache", who);
    const int vmax = slots / gmin;                                    // views per launch
    // scratch: [slots | partial | focal]; the slots must read all-ones (the "not yet published" sentinel)
    const size_t slot_bytes = (size_t)n_views * 3 * gmax * 16;
    dbl2* slot_base = reinterpret_cast<dbl2*>(scratch);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + slot_bytes);
    double* sums = partial + (size_t)n_views * gmax * 16;
    if (hipMemsetAsync(slot_base, 0xFF, slot_bytes, s) != hipSuccess) return fail("%s: memset failed", who);
    for (int v0 = 0; v0 < n_views; v0 += vmax) {
        const int nv = (n_views - v0 < vmax) ? n_views - v0 : vmax;
        int G = slots / nv;
        G = G > gmax ? gmax : G;
        // more than ~64 blocks per view only lengthens every exchange step (G slots to poll and add): measured 78 us
        // at G = 192 vs 66 us at G = 64 for one 384x512 view
        const int gcap = gmin > 64 ? gmin : 64;
        G = G > gcap ? gcap : G;
        CamArgs a;
        a.pm = pm + (size_t)v0 * P * 7;
        a.p3 = p3 + (size_t)v0 * P * 3;
        a.pl = pl + (size_t)v0 * P * 3;
        a.cf = cf + (size_t)v0 * P;
        a.sums = sums + v0;
        a.partial = partial + (size_t)v0 * gmax * 16;
        a.slots = slot_base + (size_t)v0 * 3 * gmax;
        a.V = nv; a.G = G; a.H = H; a.W = W; a.linear = activation == MUST3R_ACT_LINEAR;
        a.ppt = (P + G * CAM_T - 1) / (G * CAM_T);
        void* args[] = {&a};
        if (hipLaunchCooperativeKernel(reinterpret_cast<const void*>(cam_kernel), dim3(nv * G), dim3(CAM_T), args, 0, s) != hipSuccess) {
            (void)hipGetLastError();
            return fail("%s: cooperative launch failed", who);
        }
        if (solve(user, v0, nv, G, a.partial, a.sums, s)) return 1;
    }
    return 0;
}

namespace {
struct CamOut {
    float* focal;
    float* c2w;
};
int cam_solve_launch(void* user, int v0, int nv, int G, const double* partial, const double* focal, hipStream_t s) {
    const CamOut* o = static_cast<const CamOut*>(user);
    hipLaunchKernelGGL(cam_solve_kernel, dim3(nv), dim3(64), 0, s, partial, focal, G, o->focal + v0, o->c2w + (size_t)v0 * 16);
    if (hipGetLastError() != hipSuccess) return fail("postprocess_cam: solve launch failed");
    return 0;
}
}  // namespace

extern "C" int must3r_hip_postprocess_cam_act(const float* pm, int activation, int n_views, int H, int W, float* p3, float* pl, float* cf,
                                              float* focal, float* c2w, void* scratch, size_t scratch_bytes, void* stream) {
    if (n_views > 0 && H > 0 && W > 0 && (activation == MUST3R_ACT_NORM_EXP || activation == MUST3R_ACT_LINEAR) && (!focal || !c2w))
        return fail("postprocess_cam: null argument");
    CamOut o{focal, c2w};
    return cam_data_pass("postprocess_cam", pm, activation, n_views, H, W, p3, pl, cf, scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream),
                         cam_solve_launch, &o);
}

extern "C" int must3r_hip_postprocess_cam(const float* pm, int n_views, int H, int W, float* p3, float* pl, float* cf, float* focal, float* c2w,
                                          void* scratch, size_t scratch_bytes, void* stream) {
    return must3r_hip_postprocess_cam_act(pm, MUST3R_ACT_NORM_EXP, n_views, H, W, p3, pl, cf, focal, c2w, scratch, scratch_bytes, stream);
}
