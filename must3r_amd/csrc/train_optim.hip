// The optimizer step of the training recipe (torch.optim.AdamW under croco's NativeScalerWithGradNormCount): one table of all parameter tensors, one pass over
// the gradients (global L2 norm, non-finite test, clip coefficient, GradScaler.update) and one pass over parameters and moments, all on the caller's stream and
// without a host synchronisation.  fp32 storage; the norm accumulates in fp64.  Per element, with coef = inv_scale * clip (1 without a control record):
//
//   g' = g coef                 p = p (1 - lr wd)
//   m  = b1 m + (1 - b1) g'     v = b2 v + (1 - b2) g' g'
//   p  = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)           bc1 = 1 - b1^t, bc2 = 1 - b2^t, t = the tensor's step count after this step
//
// g is never written: the unscale and the clip live in coef.
//
// The host cuts every tensor into chunks of MUST3R_OPTIM_CHUNK elements (a multiple of 4, so that a chunk of a 16-byte aligned tensor starts 16-byte aligned) and
// uploads tensors and chunk list in ONE copy into the caller's scratch, through a ring of pinned buffers per calling thread (as train_attention.hip's table
// upload: a slot is reused only after the event recorded behind its copy).  Offsets are 64-bit: there is no limit on the total.
//
//   optim_sumsq     grid = min(chunks, OPT_MAX_BLOCKS) blocks of 256 walking the chunk list; a thread adds the squares of its float4 loads (16 B per lane) into one
//                   fp64 accumulator, the block reduces in a fixed order and writes ONE partial per chunk.  A chunk's partial does not depend on the block that
//                   computed it.  The last chunk of a tensor whose n is not a multiple of 4 ends in a scalar tail.
//   optim_finish    one block: adds the partials (thread t the partials t, t + 256, ... in ascending order, then a fixed tree), thread 0 writes the control record
//                   and applies GradScaler.update() to the scaler state.  No atomics anywhere: the result repeats bit for bit.
//   optim_prepare   one block: nothing on found_inf; else step += 1 per tensor and the tensor's lr / bc1 and sqrt(bc2), computed in fp64 and rounded once.
//   optim_adamw     the same grid over the same chunk list; returns at once on found_inf (one uniform load and branch).
#include <math.h>
#include <string.h>

#include <vector>

#include "abi.hpp"
#include "common.hpp"
#include "train_common.hpp"

namespace m3r {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_BLOCKS = 4096;                         // a few thousand blocks walk the chunk list
constexpr long long OPT_CHUNK = MUST3R_OPTIM_CHUNK;
constexpr int OPT_BATCH = 4;                                 // optim_sumsq: float4 loads a lane issues before it uses the first
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is a whole number of float4 rounds of a block");

// what the kernels read of a tensor: the caller's record and its group's numbers, the fp32 ones rounded once on the host
struct OptTensor {
    float* p; const float* g; float* m; float* v; float* step;
    long long n;
    double lr, beta1, beta2;                                 // prepare: the bias corrections in fp64
    float decay, b1, omb1, b2, omb2, eps;                    // 1 - lr wd, b1, 1 - b1, b2, 1 - b2, eps
};
struct OptChunk { long long off; int tensor, count; };       // elements [off, off + count) of a tensor of the table
struct OptBc { float step_size, sqrt_bc2; };                 // lr / bc1, sqrt(bc2)
static_assert(sizeof(OptTensor) == 96 && sizeof(OptChunk) == 16 && sizeof(OptBc) == 8, "the scratch formula of include/must3r_hip.h");

struct OptArgs {
    const OptTensor* tensors; const OptChunk* chunks;
    int n_tensors, n_chunks;
    double* partials; OptBc* bc;
    must3r_hip_optim_control* control;
    float* scale; int* tracker;
    float max_norm, growth, backoff;
    int growth_interval;
};

// the sum over the block of one fp64 value per thread, in a fixed order; valid in thread 0
__device__ __forceinline__ double opt_block_sum(double x, double* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(OPT_THREADS) __attribute__((amdgpu_waves_per_eu(8))) optim_sumsq(OptArgs a) {
    __shared__ double red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const OptChunk ch = a.chunks[c];
        const float* __restrict__ g = a.tensors[ch.tensor].g + ch.off;
        const int nvec = ch.count >> 2;
        const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
        double acc = 0.0;
        int i = tid;
        // OPT_BATCH loads in flight per lane (one load per trip leaves the kernel waiting on latency, at a quarter of the copy rate); the squares are added in
        // the order of the plain loop below, so that the batching does not show in the bits
        for (; i + (OPT_BATCH - 1) * OPT_THREADS < nvec; i += OPT_BATCH * OPT_THREADS) {
            f32x4 x[OPT_BATCH];
#pragma unroll
            for (int b = 0; b < OPT_BATCH; ++b) x[b] = g4[i + b * OPT_THREADS];
#pragma unroll
            for (int b = 0; b < OPT_BATCH; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fma((double)x[b][e], (double)x[b][e], acc);
        }
        for (; i < nvec; i += OPT_THREADS) {
            const f32x4 x = g4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fma((double)x[e], (double)x[e], acc);
        }
        const int j = 4 * nvec + tid;                        // the scalar tail: at most 3 elements
        if (j < ch.count) acc = fma((double)g[j], (double)g[j], acc);
        const double s = opt_block_sum(acc, red);
        if (tid == 0) a.partials[c] = s;
    }
}

__global__ void __launch_bounds__(OPT_THREADS) optim_finish(OptArgs a) {
    __shared__ double red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c = tid; c < a.n_chunks; c += OPT_THREADS) acc += a.partials[c];
    const double total = opt_block_sum(acc, red);
    if (tid != 0) return;
    const float inv_scale = a.scale ? 1.0f / *a.scale : 1.0f;
    const float norm = (float)(sqrt(total) * (double)inv_scale);
    const bool found_inf = !isfinite(total);
    float clip = 1.0f;
    if (a.max_norm > 0.f) clip = fminf(1.0f, a.max_norm / (norm + 1e-6f));
    a.control->norm = norm;
    a.control->coef = inv_scale * clip;
    a.control->found_inf = found_inf ? 1 : 0;
    a.control->reserved = 0;
    if (a.scale) {
        if (found_inf) {
            *a.scale *= a.backoff;
            *a.tracker = 0;
        } else {
            const int t = *a.tracker + 1;
            if (t == a.growth_interval) {
                *a.scale *= a.growth;
                *a.tracker = 0;
            } else {
                *a.tracker = t;
            }
        }
    }
}

__global__ void __launch_bounds__(OPT_THREADS) optim_prepare(OptArgs a) {
    if (a.control && a.control->found_inf) return;
    for (int i = threadIdx.x; i < a.n_tensors; i += OPT_THREADS) {
        const OptTensor t = a.tensors[i];
        const float st = *t.step + 1.0f;
        *t.step = st;
        const double bc1 = 1.0 - pow(t.beta1, (double)st), bc2 = 1.0 - pow(t.beta2, (double)st);
        a.bc[i] = OptBc{(float)(t.lr / bc1), (float)sqrt(bc2)};
    }
}

__device__ __forceinline__ void opt_update(float& p, float g, float& m, float& v, const OptTensor& t, const OptBc bc, float coef) {
    const float gs = g * coef;
    p = p * t.decay;
    m = t.b1 * m + t.omb1 * gs;
    v = t.b2 * v + t.omb2 * gs * gs;
    const float denom = sqrtf(v) / bc.sqrt_bc2 + t.eps;
    p = p - bc.step_size * (m / denom);
}

// A chunk's numbers are the same for the whole block, but they are loaded from memory that the kernel also writes (as far as the compiler can tell), so they
// would sit in vector registers, some 30 of them; taking them from the first lane puts them into scalar registers.
__device__ __forceinline__ int opt_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float opt_uni(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
template <class T>
__device__ __forceinline__ T* opt_uni(T* x) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(x);
    const unsigned lo = (unsigned)opt_uni((int)(unsigned)u), hi = (unsigned)opt_uni((int)(unsigned)(u >> 32));
    return reinterpret_cast<T*>((unsigned long long)hi << 32 | lo);
}

// 8 waves per SIMD (at most 64 registers): a streaming kernel lives on the loads it has in flight
__global__ void __launch_bounds__(OPT_THREADS) __attribute__((amdgpu_waves_per_eu(8))) optim_adamw(OptArgs a) {
    float coef = 1.0f;
    if (a.control) {
        if (a.control->found_inf) return;
        coef = opt_uni(a.control->coef);
    }
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const OptChunk ch = a.chunks[c];
        const int ti = opt_uni(ch.tensor), count = opt_uni(ch.count);
        const OptTensor& src = a.tensors[ti];
        OptTensor t;
        t.decay = opt_uni(src.decay); t.b1 = opt_uni(src.b1); t.omb1 = opt_uni(src.omb1);
        t.b2 = opt_uni(src.b2); t.omb2 = opt_uni(src.omb2); t.eps = opt_uni(src.eps);
        const OptBc bc{opt_uni(a.bc[ti].step_size), opt_uni(a.bc[ti].sqrt_bc2)};
        float* __restrict__ p = opt_uni(src.p + ch.off);
        const float* __restrict__ g = opt_uni(src.g + ch.off);
        float* __restrict__ m = opt_uni(src.m + ch.off);
        float* __restrict__ v = opt_uni(src.v + ch.off);
        const int nvec = count >> 2;
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            f32x4 xp = reinterpret_cast<f32x4*>(p)[i];
            const f32x4 xg = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 xm = reinterpret_cast<f32x4*>(m)[i];
            f32x4 xv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sp = xp[e], sm = xm[e], sv = xv[e];
                opt_update(sp, xg[e], sm, sv, t, bc, coef);
                xp[e] = sp; xm[e] = sm; xv[e] = sv;
            }
            reinterpret_cast<f32x4*>(p)[i] = xp;
            reinterpret_cast<f32x4*>(m)[i] = xm;
            reinterpret_cast<f32x4*>(v)[i] = xv;
        }
        const int j = 4 * nvec + tid;
        if (j < count) {
            float sp = p[j], sm = m[j], sv = v[j];
            opt_update(sp, g[j], sm, sv, t, bc, coef);
            p[j] = sp; m[j] = sm; v[j] = sv;
        }
    }
}

// ---- host ----

// scratch: [tensors | chunks] (one upload) | partials fp64 [chunks] | bias corrections [tensors], each part a multiple of 256 bytes.  The scratch query sizes the
// chunk parts for the most chunks a table of n_tensors tensors and total elements can have, total / CHUNK + n_tensors.
struct OptLayout { size_t tensors, chunks, upload_bytes, partials, bc, total; };
static OptLayout opt_layout(long long n_tensors, long long max_chunks) {
    OptLayout L{};
    ScratchCursor c;
    L.tensors = c.take((size_t)n_tensors * sizeof(OptTensor));
    L.chunks = c.take((size_t)max_chunks * sizeof(OptChunk));
    L.upload_bytes = c.off;
    L.partials = c.take((size_t)max_chunks * sizeof(double));
    L.bc = c.take((size_t)n_tensors * sizeof(OptBc));
    L.total = c.off;
    return L;
}
static long long opt_max_chunks(long long n_tensors, long long total) { return total / OPT_CHUNK + n_tensors; }

static const char* opt_shape_error(long long n_tensors, long long total) {
    if (n_tensors < 1 || n_tensors > (1 << 24)) return "n_tensors must be in [1, 2^24]";
    if (total < n_tensors) return "total_elems must be at least n_tensors (every tensor has n >= 1)";
    if (total > (1LL << 46)) return "total_elems must not exceed 2^46";
    return nullptr;
}

// The table of a call: nullptr and the device records and chunk list, or why the call is refused.  Reads host memory only.
struct OptPlan {
    std::vector<OptTensor> tensors;
    std::vector<OptChunk> chunks;
    long long total = 0;
};
static const char* opt_plan(const must3r_hip_optim_args* a, bool step, OptPlan& P) {
    if (!a->tensors) return "null argument (tensors)";
    if (a->n_tensors < 1 || a->n_tensors > (1 << 24)) return "n_tensors must be in [1, 2^24]";
    if (step) {
        if (!a->groups) return "null argument (groups)";
        if (a->n_groups < 1) return "n_groups must be positive";
        for (int i = 0; i < a->n_groups; ++i) {
            const must3r_hip_optim_group& q = a->groups[i];
            if (!(q.beta1 >= 0.0 && q.beta1 < 1.0) || !(q.beta2 >= 0.0 && q.beta2 < 1.0)) return "a beta outside [0, 1)";
            if (!(q.eps >= 0.0)) return "eps must not be negative";
            if (!(q.lr >= 0.0)) return "lr must not be negative";
            if (!(q.weight_decay >= 0.0)) return "weight_decay must not be negative";
        }
    }
    P.tensors.resize((size_t)a->n_tensors);
    for (int i = 0; i < a->n_tensors; ++i) {
        const must3r_hip_optim_tensor& t = a->tensors[i];
        if (!t.g) return "null argument (g of a tensor)";
        if (step && (!t.p || !t.m || !t.v || !t.step)) return "null argument (p, m, v or step of a tensor)";
        if (misaligned(t.g) || (step && (misaligned(t.p) || misaligned(t.m) || misaligned(t.v)))) return "tensors must be 16-byte aligned";
        if (step && ((size_t)t.step & 3)) return "step must be 4-byte aligned";
        if (t.n <= 0) return "n of a tensor must be positive";
        if (t.n > (1LL << 46) || P.total + t.n > (1LL << 46)) return "total_elems must not exceed 2^46";
        OptTensor& d = P.tensors[(size_t)i];
        d = OptTensor{};
        d.p = t.p; d.g = t.g; d.m = t.m; d.v = t.v; d.step = t.step; d.n = t.n;
        if (step) {
            if (t.group < 0 || t.group >= a->n_groups) return "a group index outside the group table";
            const must3r_hip_optim_group& q = a->groups[t.group];
            d.lr = q.lr; d.beta1 = q.beta1; d.beta2 = q.beta2;
            d.decay = (float)(1.0 - q.lr * q.weight_decay);
            d.b1 = (float)q.beta1; d.omb1 = (float)(1.0 - q.beta1);
            d.b2 = (float)q.beta2; d.omb2 = (float)(1.0 - q.beta2);
            d.eps = (float)q.eps;
        }
        for (long long off = 0; off < t.n; off += OPT_CHUNK) P.chunks.push_back(OptChunk{off, i, (int)std::min(OPT_CHUNK, t.n - off)});
        P.total += t.n;
    }
    return nullptr;
}

// the pinned ring of the table uploads (train_attention.hip's ta_upload, image.hip's staging): with one buffer a second call would wait on the host for the
// first call's copy, which is queued behind everything the stream still has to do
struct OptPin {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
};
constexpr int kOptPinSlots = 4;
static thread_local OptPin opt_pins[kOptPinSlots];
static thread_local int opt_pin_next = 0;

static int opt_upload(const OptPlan& P, const OptLayout& L, char* scratch, hipStream_t s, const char* who) {
    const size_t bytes = L.chunks + P.chunks.size() * sizeof(OptChunk);
    OptPin& pin = opt_pins[opt_pin_next];
    opt_pin_next = (opt_pin_next + 1) % kOptPinSlots;
    if (pin.ev) {
        if (hipEventSynchronize(pin.ev) != hipSuccess) return fail("%s: waiting for the previous table upload failed", who);
        (void)hipEventDestroy(pin.ev);
        pin.ev = nullptr;
    }
    if (pin.cap < bytes) {
        if (pin.host) (void)hipHostFree(pin.host);
        pin.host = nullptr; pin.cap = 0;
        if (hipHostMalloc(&pin.host, bytes, hipHostMallocDefault) != hipSuccess) { pin.host = nullptr; return fail("%s: no pinned memory for the tables", who); }
        pin.cap = bytes;
    }
    char* h = reinterpret_cast<char*>(pin.host);
    memcpy(h, P.tensors.data(), P.tensors.size() * sizeof(OptTensor));
    memset(h + P.tensors.size() * sizeof(OptTensor), 0, L.chunks - P.tensors.size() * sizeof(OptTensor));
    memcpy(h + L.chunks, P.chunks.data(), P.chunks.size() * sizeof(OptChunk));
    if (hipMemcpyAsync(scratch, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("%s: the table upload failed", who);
    if (hipEventCreateWithFlags(&pin.ev, hipEventDisableTiming) != hipSuccess) { pin.ev = nullptr; return fail("%s: no event", who); }
    if (hipEventRecord(pin.ev, s) != hipSuccess) return fail("%s: no event", who);
    return 0;
}

// the checks both entry points make after their own, the upload and the kernel arguments
static int opt_begin(const char* who, const must3r_hip_optim_args* a, bool step, void* scratch, size_t scratch_bytes, OptArgs& k, hipStream_t s) {
    OptPlan P;
    if (const char* e = opt_plan(a, step, P)) return fail("%s: %s", who, e);
    if (misaligned(a->control)) return fail("%s: control must be 16-byte aligned", who);
    const OptLayout L = opt_layout(a->n_tensors, opt_max_chunks(a->n_tensors, P.total));
    if (!scratch || misaligned(scratch) || scratch_bytes < L.total) return fail("%s: scratch too small", who);
    char* p = reinterpret_cast<char*>(scratch);
    if (opt_upload(P, L, p, s, who)) return 1;
    k = OptArgs{};
    k.tensors = reinterpret_cast<const OptTensor*>(p + L.tensors);
    k.chunks = reinterpret_cast<const OptChunk*>(p + L.chunks);
    k.n_tensors = a->n_tensors; k.n_chunks = (int)P.chunks.size();
    k.partials = reinterpret_cast<double*>(p + L.partials);
    k.bc = reinterpret_cast<OptBc*>(p + L.bc);
    k.control = a->control;
    return 0;
}

}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_optim_scratch_bytes(int64_t n_tensors, int64_t total_elems) {
    if (const char* e = opt_shape_error(n_tensors, total_elems)) {
        fail("optim_scratch_bytes: %s", e);
        return 0;
    }
    return opt_layout(n_tensors, opt_max_chunks(n_tensors, total_elems)).total;
}

extern "C" int must3r_hip_optim_norm(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "optim_norm";
    if (!a) return fail("%s: null argument", who);
    if (!a->control) return fail("%s: null argument (control)", who);
    if (!a->scale != !a->growth_tracker) return fail("%s: scale and growth_tracker come together (both NULL: no scaler state)", who);
    if (a->scale && (((size_t)a->scale & 3) || ((size_t)a->growth_tracker & 3))) return fail("%s: scale and growth_tracker must be 4-byte aligned", who);
    if (a->scale && (!(a->growth_factor > 0.f) || !(a->backoff_factor > 0.f) || a->growth_interval < 1))
        return fail("%s: growth_factor and backoff_factor must be positive and growth_interval at least 1", who);
    if (a->max_norm != a->max_norm) return fail("%s: max_norm is NaN", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    OptArgs k;
    if (opt_begin(who, a, false, scratch, scratch_bytes, k, s)) return 1;
    k.scale = a->scale; k.tracker = a->growth_tracker;
    k.max_norm = a->max_norm; k.growth = a->growth_factor; k.backoff = a->backoff_factor; k.growth_interval = a->growth_interval;
    hipLaunchKernelGGL(optim_sumsq, dim3(std::min(k.n_chunks, OPT_MAX_BLOCKS)), dim3(OPT_THREADS), 0, s, k);
    hipLaunchKernelGGL(optim_finish, dim3(1), dim3(OPT_THREADS), 0, s, k);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

extern "C" int must3r_hip_optim_adamw(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes) {
    const char* who = "optim_adamw";
    if (!a) return fail("%s: null argument", who);
    hipStream_t s = reinterpret_cast<hipStream_t>(a->stream);
    OptArgs k;
    if (opt_begin(who, a, true, scratch, scratch_bytes, k, s)) return 1;
    hipLaunchKernelGGL(optim_prepare, dim3(1), dim3(OPT_THREADS), 0, s, k);
    hipLaunchKernelGGL(optim_adamw, dim3(std::min(k.n_chunks, OPT_MAX_BLOCKS)), dim3(OPT_THREADS), 0, s, k);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}
