// The per-frame step of the SLAM agent (must3r/slam/model.py) between the decoder call and the keyframe decision, as device work without a host read:
// include/must3r_hip.h ("the per-frame step of the SLAM agent") has the contract, must3r_amd/slam.py the caller.
//
//   must3r_hip_slam_pose      cam.hip's data pass (cam_kernel, cooperative: activation, Weiszfeld focal, registration sums -- reused unchanged through
//                             cam_data_pass) + slam_solve_kernel (one block of 64 per view: the partial sums in cam_solve_kernel's order; lane 0 reads
//                             seq_focal = sum f c / sum c from the agent's device state, forms ratio = fp32(fp32(seq_focal) / focal), solves the
//                             registration of the RECTIFIED points from the unrectified sums (cam_solve.hpp) and, asked to, advances the running
//                             fp64 sums and the (f_i, c_i) log) + slam_rectify_kernel (z <- fp32(z * ratio), 8 B per pixel).
//   must3r_hip_slam_keyframe  slam_select_kernel    2 blocks of 1024.  Block 0 walks the ::subsamp grid in row-major chunks of 1024 candidates: ballot of
//                                                   conf > min_conf, rank inside the wave by popcount, wave totals through LDS, a running offset: the
//                                                   selected world points and depths land in grid order and n_sel is exact.  Block 1: mean of conf (fp64,
//                                                   fixed order) and its lower median (4 x 8-bit radix select on the order-preserving bit pattern).
//                             slam_walk_kernel<G>   G lanes per selected point: quadrant id against the device's camera centre (nn_walk.hpp's quadrant_of,
//                                                   the text of must3r_hip_quadrant_ids), nn_walk (the text of must3r_hip_nn_index_query), fp64 quotient.
//                                                   The launch covers every candidate; groups past the device's n_sel return at once.
//                             slam_rank_kernel      2 blocks of 1024: block b selects the b-th of the two order statistics of the n_sel fp64 values by an
//                                                   8 x 8-bit radix select (exact: a rank among bit patterns).
//                             slam_record_kernel    one thread: numpy's _lerp, the record.
// The LDS bin counts are the only atomics; they are integer counts and decide no order.  The file is built with the flags of nn.hip, nn_index.hip and
// cam.hip, whose device routines it shares, so that the shared text contracts alike; the virtual index and the _lerp expressions are compiled with
// contraction off (a pragma in their two routines).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "abi.hpp"
#include "cam_solve.hpp"
#include "common.hpp"
#include "nn_walk.hpp"
#include "options.hpp"

namespace m3r {
namespace {

constexpr int SL_T = 1024;   // threads of the single-block passes
constexpr int REC_N = MUST3R_SLAM_RECORD_DOUBLES;

// ---------------------------------------------------------------------------------------------------------------------------------
// pose
// ---------------------------------------------------------------------------------------------------------------------------------
struct SolveDev {
    float* focal;          // [B]
    float* c2w;            // [B][4][4]
    float* ratio;          // [B] scratch
    double* state;         // focal_state or null
    double* log;           // focal_log or null
    int log_cap, is_first, use_seq, update;
    double inv_pixels;     // 1 / (H W)
};

__global__ void __launch_bounds__(64) slam_solve_kernel(const double* __restrict__ partial, const double* __restrict__ focal_in, const int G, const int v0,
                                                        const SolveDev p) {
    __shared__ double S4[4][16];
    __shared__ double S[16];
    const int v = blockIdx.x;
    cam_sum_partials(partial + (size_t)v * G * 16, G, S4, S);
    if (threadIdx.x != 0) return;
    const float focal = (float)focal_in[v];
    float ratio = 1.0f;
    if (p.use_seq && p.state && p.state[2] > 0.0) ratio = (float)(p.state[0] / p.state[1]) / focal;
    float* c2w = p.c2w + (size_t)(v0 + v) * 16;
    if (p.is_first) {
        ratio = 1.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) c2w[i] = (i % 5 == 0) ? 1.f : 0.f;
    } else {
        cam_register<true>(S, (double)ratio, c2w);
    }
    p.focal[v0 + v] = focal;
    p.ratio[v0 + v] = ratio;
    if (p.update) {   // one view (checked by the entry point): read-modify-write by this thread alone
        const double f = (double)focal, c = S[0] * p.inv_pixels;
        const double sfc = p.state[0] + f * c, sc = p.state[1] + c;
        const long long n = (long long)p.state[2];
        if (p.log && n < p.log_cap) {
            p.log[2 * n] = f;
            p.log[2 * n + 1] = c;
        }
        p.state[0] = sfc;
        p.state[1] = sc;
        p.state[2] = (double)(n + 1);
        p.state[3] = sfc / sc;
    }
}

__global__ void __launch_bounds__(256) slam_rectify_kernel(float* __restrict__ pl, const float* __restrict__ ratio, const int P) {
    const int v = blockIdx.y;
    const float r = ratio[v];
    float* z = pl + (size_t)v * P * 3 + 2;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) z[(size_t)i * 3] = z[(size_t)i * 3] * r;
}

int slam_solve_launch(void* user, int v0, int nv, int G, const double* partial, const double* focal, hipStream_t s) {
    const SolveDev* p = static_cast<const SolveDev*>(user);
    hipLaunchKernelGGL(slam_solve_kernel, dim3(nv), dim3(64), 0, s, partial, focal, G, v0, *p);
    if (hipGetLastError() != hipSuccess) return fail("slam_pose: solve launch failed");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// keyframe
// ---------------------------------------------------------------------------------------------------------------------------------
struct KfStats {          // head of the scratch
    int n_sel, pad;
    float conf_median, pad1;
    double conf_mean;
    double os[2];         // order statistics below / above the virtual index
};

struct KfDev {
    const float* p3;
    const float* pl;
    const float* cf;
    const float* c2w;
    const float* focal;
    const double* state;
    const char* index;
    float* sel;
    float* dist;
    double* record;
    KfStats* stats;
    float* zsel;          // [cand]
    double* dval;         // [cand]
    double quantile;
    float min_conf;
    int H, W, s, Hs, Ws, cand, divider, mode;
};

__device__ __forceinline__ unsigned key32(const float v) {   // unsigned order = float order (-0 below +0)
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey32(const unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ unsigned long long key64(const double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey64(const unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// The key of rank `rank` (0-based, ascending) among n keys, KEY(i) the i-th: BITS / 8 passes of 8-bit digits from the top.  One block of SL_T threads;
// hist[256] and sh[2] are LDS.  Every thread returns the key.
template <int BITS, class K, class F>
__device__ __forceinline__ K radix_select(const int n, long long rank, unsigned* hist, unsigned long long* sh, F key_of) {
    K prefix = 0, mask = 0;
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += SL_T) {
            const K k = key_of(i);
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)((k >> shift) & 255)], 1u);   // a count: order-free
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long r = rank;
            int b = 0;
            for (; b < 255; ++b) {
                if (r < (long long)hist[b]) break;
                r -= hist[b];
            }
            sh[0] = (unsigned long long)b;
            sh[1] = (unsigned long long)r;
        }
        __syncthreads();
        prefix |= (K)sh[0] << shift;
        mask |= (K)255 << shift;
        rank = (long long)sh[1];
        __syncthreads();
    }
    return prefix;
}

__global__ void __launch_bounds__(SL_T) slam_select_kernel(const KfDev p) {
    __shared__ unsigned wcnt[SL_T / 64];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh[2];
    __shared__ double red[SL_T / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (blockIdx.x == 0) {
        const unsigned long long lt = (1ull << lane) - 1ull;
        unsigned running = 0;
        for (int base = 0; base < p.cand; base += SL_T) {
            const int i = base + t;
            bool on = false;
            size_t pix = 0;
            if (i < p.cand) {
                const int r = i / p.Ws, c = i - r * p.Ws;
                pix = (size_t)(r * p.s) * p.W + (size_t)c * p.s;
                on = p.cf[pix] > p.min_conf;
            }
            const unsigned long long b = __ballot(on);
            if (lane == 0) wcnt[w] = (unsigned)__popcll(b);
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < SL_T / 64; ++k) {
                const unsigned c = wcnt[k];
                before += k < w ? c : 0u;
                total += c;
            }
            if (on) {
                const unsigned o = running + before + (unsigned)__popcll(b & lt);   // o <= i < cand
                p.sel[(size_t)o * 3 + 0] = p.p3[pix * 3 + 0];
                p.sel[(size_t)o * 3 + 1] = p.p3[pix * 3 + 1];
                p.sel[(size_t)o * 3 + 2] = p.p3[pix * 3 + 2];
                p.zsel[o] = p.pl[pix * 3 + 2];
            }
            running += total;
            __syncthreads();
        }
        if (t == 0) p.stats->n_sel = (int)running;
        return;
    }
    // block 1: mean and lower median of the full conf map
    const int P = p.H * p.W;
    double acc = 0.0;
    for (int i = t; i < P; i += SL_T) acc += (double)p.cf[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int k = 0; k < SL_T / 64; ++k) s += red[k];
        p.stats->conf_mean = s / (double)P;
    }
    const float* cf = p.cf;
    const unsigned k = radix_select<32, unsigned>(P, (long long)(P - 1) / 2, hist, sh, [cf](int i) { return key32(cf[i]); });
    if (t == 0) p.stats->conf_median = unkey32(k);
}

template <int G>
__global__ void __launch_bounds__(256) slam_walk_kernel(const KfDev p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / G), sub = (int)(t % G);   // a group never straddles a wave (G divides 64)
    if (i >= p.stats->n_sel) return;                  // n_sel <= cand: every read below is inside sel / zsel
    const float qx = p.sel[(size_t)i * 3 + 0], qy = p.sel[(size_t)i * 3 + 1], qz = p.sel[(size_t)i * 3 + 2];
    float best = INFINITY;
    if (p.index) {
        const int quad = p.divider > 0 ? quadrant_of(qx, qy, qz, p.c2w[3], p.c2w[7], p.c2w[11], p.divider) : 0;
        best = nn_walk<G>(p.index, p.divider, quad, qx, qy, qz, sub);
    }
    if (sub != 0) return;
    const float dist = sqrtf(best);   // sqrt(+inf) = +inf
    if (p.dist) p.dist[i] = dist;
    double d = (double)dist;
    if (p.mode & MUST3R_SLAM_MODE_NORM) d = d / (double)(p.zsel[i] + 1e-9f);
    if (d == (double)INFINITY) d = DBL_MAX;   // an unseen quadrant / an empty map (slam/model.py:87-88)
    p.dval[i] = d;
}

// previous and next index of numpy's linear method (_get_indexes): virtual index vi = (n - 1) q; at or above n - 1 both are the last element
__device__ __forceinline__ void quantile_indexes(const int n, const double q, double* vi, long long* prev, long long* next, double* gamma) {
#pragma clang fp contract(off)   // the product is rounded before the floor is subtracted, as numpy's two ufuncs round it
    *vi = (double)(n - 1) * q;
    const double fl = floor(*vi);
    if (*vi >= (double)(n - 1)) {
        *prev = *next = n - 1;
        *gamma = *vi - (-1.0);   // numpy indexes the last element as -1 and forms gamma from it; both neighbours are equal there
    } else {
        *prev = (long long)fl;
        *next = *prev + 1;
        *gamma = *vi - fl;
    }
}

// numpy's _lerp, every operation rounded (no FMA)
__device__ __forceinline__ double lerp(const double a, const double b, const double g) {
#pragma clang fp contract(off)
    const double diff = b - a;
    const double up = diff * g, down = diff * (1.0 - g);
    return g >= 0.5 ? b - down : a + up;
}

__global__ void __launch_bounds__(SL_T) slam_rank_kernel(const KfDev p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh[2];
    const int n = p.stats->n_sel;
    if (n <= 0) return;   // uniform
    double vi, g;
    long long prev, next;
    quantile_indexes(n, p.quantile, &vi, &prev, &next, &g);
    const double* dv = p.dval;
    const unsigned long long k = radix_select<64, unsigned long long>(n, blockIdx.x == 0 ? prev : next, hist, sh, [dv](int i) { return key64(dv[i]); });
    if (threadIdx.x == 0) p.stats->os[blockIdx.x] = unkey64(k);
}

__global__ void __launch_bounds__(64) slam_record_kernel(const KfDev p) {
    if (threadIdx.x != 0) return;
    double* r = p.record;
    for (int i = 0; i < REC_N; ++i) r[i] = 0.0;
    const int n = p.stats->n_sel;
    const double med = (double)p.stats->conf_median, mean = p.stats->conf_mean;
    double score = 0.0;
    if (p.mode & MUST3R_SLAM_MODE_NN) {
        if (n > 0) {
            double vi, g;
            long long prev, next;
            quantile_indexes(n, p.quantile, &vi, &prev, &next, &g);
            const double a = p.stats->os[0], b = p.stats->os[1];
            score = lerp(a, b, g);
            r[1] = a;
            r[2] = b;
            r[27] = vi;
        }
    } else {
        score = (p.mode & MUST3R_SLAM_MODE_MEANCONF) ? mean : med;
    }
    r[0] = (double)n;
    r[3] = score;
    r[4] = med;
    r[5] = mean;
    r[6] = p.focal ? (double)p.focal[0] : 0.0;
    r[7] = p.state ? p.state[3] : 0.0;
    r[8] = (double)p.c2w[3];
    r[9] = (double)p.c2w[7];
    r[10] = (double)p.c2w[11];
    for (int i = 0; i < 16; ++i) r[11 + i] = (double)p.c2w[i];
}

inline bool off8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; }
inline int grid_of(int n, int s) { return s <= 1 ? n : (n + s - 1) / s; }
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

const char* pose_args_error(const must3r_hip_slam_pose_args* a) {
    if (!a->pm || !a->pts3d || !a->pts3d_local || !a->conf || !a->focal || !a->c2w || !a->scratch) return "null argument (pm, pts3d, pts3d_local, conf, focal, c2w, scratch)";
    if (a->B < 1 || a->H <= 0 || a->W <= 0) return "B must be at least 1, H and W positive";
    if (a->activation != MUST3R_ACT_NORM_EXP && a->activation != MUST3R_ACT_LINEAR) return "unknown activation";
    if (a->update_focal && a->B != 1) return "update_focal takes one view (B = 1)";
    if (a->update_focal && !a->focal_state) return "update_focal needs focal_state";
    if (a->focal_log_cap < 0 || (a->focal_log_cap > 0 && !a->focal_log)) return "focal_log_cap is negative, or positive without focal_log";
    if (a->scratch_bytes < must3r_hip_slam_pose_scratch_bytes(a->B, a->H, a->W)) return "scratch too small";
    return nullptr;
}

const char* keyframe_args_error(const must3r_hip_slam_keyframe_args* a) {
    if (!a->pts3d || !a->pts3d_local || !a->conf || !a->c2w || !a->sel || !a->record || !a->scratch)
        return "null argument (pts3d, pts3d_local, conf, c2w, sel, record, scratch)";
    if (a->H <= 0 || a->W <= 0 || (long long)a->H * a->W > (1LL << 24)) return "H and W must be positive, at most 2^24 pixels";
    if (a->subsamp < 0) return "subsamp must not be negative";
    if (a->divider < 0 || a->divider > 8) return "divider outside [0, 8]";
    if (!(a->quantile >= 0.0 && a->quantile <= 1.0)) return "quantile outside [0, 1]";
    const int m = a->mode, conf_modes = MUST3R_SLAM_MODE_MEANCONF | MUST3R_SLAM_MODE_MEDIANCONF;
    if (m <= 0 || (m & ~(MUST3R_SLAM_MODE_NN | MUST3R_SLAM_MODE_NORM | conf_modes))) return "mode: no bit or an unknown bit";
    if ((m & MUST3R_SLAM_MODE_NORM) && !(m & MUST3R_SLAM_MODE_NN)) return "mode: NORM goes with NN";
    if ((m & MUST3R_SLAM_MODE_NN) && (m & conf_modes)) return "mode: NN and a conf mode exclude each other";
    if ((m & conf_modes) == conf_modes) return "mode: MEANCONF and MEDIANCONF exclude each other";
    if (a->scratch_bytes < must3r_hip_slam_keyframe_scratch_bytes(a->H, a->W, a->subsamp)) return "scratch too small";
    if (off8(a->sel) || off8(a->record) || off8(a->scratch)) return "sel, record and scratch must be 8-byte aligned";
    return nullptr;
}

template <int G>
void launch_walk(const KfDev& p, hipStream_t s) {
    hipLaunchKernelGGL(slam_walk_kernel<G>, dim3((unsigned)(((long long)p.cand * G + 255) / 256)), dim3(256), 0, s, p);
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_slam_pose_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return align256(must3r_hip_postprocess_cam_scratch_bytes(B, H, W)) + align256((size_t)B * 4);
}

extern "C" int must3r_hip_slam_pose(const must3r_hip_slam_pose_args* a) {
    const char* who = "slam_pose";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = pose_args_error(a)) return fail("%s: %s", who, e);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    const size_t cam_bytes = align256(must3r_hip_postprocess_cam_scratch_bytes(a->B, a->H, a->W));
    SolveDev p{};
    p.focal = a->focal; p.c2w = a->c2w;
    p.ratio = reinterpret_cast<float*>(static_cast<char*>(a->scratch) + cam_bytes);
    p.state = a->focal_state; p.log = a->focal_log; p.log_cap = a->focal_log_cap;
    p.is_first = a->is_first != 0; p.use_seq = a->use_seq_focal != 0; p.update = a->update_focal != 0;
    p.inv_pixels = 1.0 / ((double)a->H * (double)a->W);
    if (cam_data_pass(who, a->pm, a->activation, a->B, a->H, a->W, a->pts3d, a->pts3d_local, a->conf, a->scratch, cam_bytes, s, slam_solve_launch, &p)) return 1;
    if (!p.is_first && p.use_seq && p.state) {
        const int P = a->H * a->W;
        const unsigned blocks = (unsigned)((P + 255) / 256 < 256 ? (P + 255) / 256 : 256);
        hipLaunchKernelGGL(slam_rectify_kernel, dim3(blocks, (unsigned)a->B), dim3(256), 0, s, a->pts3d_local, p.ratio, P);
        if (hipGetLastError() != hipSuccess) return fail("%s: rectify launch failed", who);
    }
    return 0;
}

extern "C" size_t must3r_hip_slam_keyframe_scratch_bytes(int H, int W, int subsamp) {
    if (H <= 0 || W <= 0 || subsamp < 0 || (long long)H * W > (1LL << 24)) return 0;
    const size_t cand = (size_t)grid_of(H, subsamp) * grid_of(W, subsamp);
    return 256 + align256(cand * 8) + align256(cand * 4);
}

extern "C" int must3r_hip_slam_keyframe(const must3r_hip_slam_keyframe_args* a) {
    const char* who = "slam_keyframe";
    if (!a) return fail("%s: null argument", who);
    if (const char* e = keyframe_args_error(a)) return fail("%s: %s", who, e);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    static_assert(sizeof(KfStats) <= 256, "the statistics head of the scratch");
    KfDev p{};
    p.p3 = a->pts3d; p.pl = a->pts3d_local; p.cf = a->conf; p.c2w = a->c2w; p.focal = a->focal; p.state = a->focal_state;
    p.index = static_cast<const char*>(a->index); p.sel = a->sel; p.dist = a->dist; p.record = a->record;
    p.quantile = a->quantile; p.min_conf = a->min_conf;
    p.H = a->H; p.W = a->W; p.s = a->subsamp <= 1 ? 1 : a->subsamp;
    p.Hs = grid_of(a->H, a->subsamp); p.Ws = grid_of(a->W, a->subsamp); p.cand = p.Hs * p.Ws;
    p.divider = a->divider; p.mode = a->mode;
    char* sc = static_cast<char*>(a->scratch);
    p.stats = reinterpret_cast<KfStats*>(sc);
    p.dval = reinterpret_cast<double*>(sc + 256);
    p.zsel = reinterpret_cast<float*>(sc + 256 + align256((size_t)p.cand * 8));
    hipLaunchKernelGGL(slam_select_kernel, dim3(2), dim3(SL_T), 0, s, p);
    if (a->mode & MUST3R_SLAM_MODE_NN) {
        switch (opt(OPT_NN_QUERY_LANES_LOG2)) {
            case 0: launch_walk<1>(p, s); break;
            case 1: launch_walk<2>(p, s); break;
            case 2: launch_walk<4>(p, s); break;
            case 3: launch_walk<8>(p, s); break;
            default: launch_walk<16>(p, s); break;
        }
        hipLaunchKernelGGL(slam_rank_kernel, dim3(2), dim3(SL_T), 0, s, p);
    }
    hipLaunchKernelGGL(slam_record_kernel, dim3(1), dim3(64), 0, s, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}
