// Native host runtime of libmust3r_hip: context, weight store, workspace arena and the two forwards
// (per-view ViT-L encoder, ViT-B memory decoder) expressed as launches of the gfx950 kernels in
// gemm.hip / attention.hip / misc.hip on the caller's HIP stream.  C ABI: include/must3r_hip.h.
//
// Algorithm citations are to the reference tree (must3r/model/...):
//   encoder.py:46-52, blocks/layers.py:51-54,90-99, blocks/attention.py:37-149, decoder.py:158-350,
//   feedback_mechanism.py:39-53, blocks/head.py:63-72, tools/image.py:9-14.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "abi.hpp"
#include "encode_plan.hpp"
#include "kernels.hpp"
#include "options.hpp"

using namespace m3r;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int m3r::fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
#define HIP_OK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
#define M3R_OK(expr)                  \
    do {                              \
        int rc__ = (expr);            \
        if (rc__) return rc__;        \
    } while (0)

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct Param {
    std::vector<int64_t> shape;
    size_t n = 0;
    float* d = nullptr;       // fp32 master on device
    void* h16[2] = {nullptr, nullptr};   // packed 16-bit copy per dtype (lazy)
    void* l16[2] = {nullptr, nullptr};   // low part (split precision), lazy, only where needed
    void* x2[2] = {nullptr, nullptr};    // [rows][hi(K) | lo(K)] layout for the split-weight GEMM, lazy
    void* x3[2] = {nullptr, nullptr};    // [rows][hi | hi | lo] layout: one K = 3 in launch of the split-precision head, lazy
    void* sp_vals = nullptr;             // r05: 2:4-sparse copy of the fp16 low part (GemmArgs::Wlo_sp / Widx_sp), built with x2[DT_F16] where the shape allows
    void* sp_idx = nullptr;
    bool loaded = false;
    bool derived = false;     // built by finalize, not loaded
    bool optional = false;    // may legitimately be absent (feedback layer variants)
};

// softmax scale folded into q by the projection epilogues: 1/sqrt(64) * log2(e)
static const float kQScale = 0.125f * 1.44269504088896340736f;

struct ProfEntry { hipEvent_t a, b; int cat; double flops; char kern[40]; };
struct ProfKern { double ms = 0, flops = 0; long long calls = 0; };
enum ProfCat { PC_GEMM128 = 0, PC_GEMM64, PC_ATTN_SA, PC_ATTN_CA, PC_ATTN_COMBINE, PC_LN, PC_MISC, PC_COUNT };
static const char* kProfNames[PC_COUNT] = {"gemm128", "gemm64", "attn_self", "attn_cross", "attn_combine", "layernorm", "misc"};

// parameters of one transformer block, resolved to Param* once per context
enum LayerField { LF_N1W, LF_N1B, LF_QKVW, LF_QKVB, LF_PROJW, LF_PROJB, LF_N2W, LF_N2B, LF_FC1W, LF_FC1B, LF_FC2W, LF_FC2B, LF_NYW, LF_NYB, LF_PQW, LF_PQB, LF_PKVW, LF_PKVB, LF_CPW, LF_CPB, LF_N3W, LF_N3B, LF_QKVLN_W, LF_QKVLN_S, LF_QKVLN_C, LF_PQLN_W, LF_PQLN_S, LF_PQLN_C, LF_FC1LN_W, LF_FC1LN_S, LF_FC1LN_C, LF_COUNT };
static const char* kLayerFieldNames[LF_COUNT] = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "norm_y.weight", "norm_y.bias", "cross_attn.projq.weight", "cross_attn.projq.bias", "cross_attn.projkv.weight", "cross_attn.projkv.bias", "cross_attn.proj.weight", "cross_attn.proj.bias", "norm3.weight", "norm3.bias", "attn.qkv_ln.weight", "attn.qkv_ln.s", "attn.qkv_ln.c", "cross_attn.projq_ln.weight", "cross_attn.projq_ln.s", "cross_attn.projq_ln.c", "mlp.fc1_ln.weight", "mlp.fc1_ln.s", "mlp.fc1_ln.c"};

struct must3r_hip_ctx {
    must3r_hip_config cfg;
    int device = 0;
    std::map<std::string, Param> params;
    bool fin_enc = false, fin_dec = false;
    // per-layer parameter tables (resolved once: no string building / map lookups per launch); entries of absent parameters are null
    std::vector<std::vector<struct Param*>> enc_tab, dec_tab;
    DType dt = DT_F16;         // operand type of the running forward's kernels; this and the next three: set_mode()
    int wsplit = 0;            // 2 while a forward runs in MUST3R_F16_W2 / MUST3R_F16_WA mode
    int mlp_plain = 0;         // 1 in MUST3R_F16_WA mode: the Mlp Linears take plain fp16 weights (one MFMA pass)
    int attn8 = 0;             // 1 while a forward runs with MUST3R_ATTN_FP8 (e4m3 attention operands)
    float* rope_tab = nullptr;
    int rope_npos = 0;
    // workspace arena (grow-only)
    char* ws = nullptr;
    size_t ws_cap = 0;
    // pinned staging for per-call view tables
    static constexpr int kSlots = 32;
    static constexpr size_t kSlotBytes = 64 * 1024;
    char* pin = nullptr;
    char* pin_dev = nullptr;
    hipEvent_t slot_ev[kSlots];
    bool slot_used[kSlots];
    int slot_next = 0;
    // profiling
    bool prof = false;
    std::vector<ProfEntry> prof_entries;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[PC_COUNT] = {0}, prof_flops[PC_COUNT] = {0};
    long long prof_calls[PC_COUNT] = {0};
    std::map<std::string, ProfKern> prof_kern;   // per kernel symbol (GEMM: family / epilogue / weight layout / tile width; attention: kernel + self / cross)
    // r05: split-weight matrix ([hi | lo] rows, Param::x2) -> its 2:4-sparse low part; the gemm() wrapper hands it to the launcher, which uses it in the
    // chip-filling kernel only (every other split-weight kernel reads the dense low half of the rows)
    struct SparseLo { const void* vals; const void* idx; int rows; };
    std::map<const void*, SparseLo> sparse_lo;
};

// The entry points run on the context's device and leave the caller's current device as they found it (a process that
// drives several GPUs keeps its own current device; torch's notion of it is not changed behind its back).
struct DeviceGuard {
    int prev = -1, want;
    explicit DeviceGuard(int d) : want(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) (void)hipSetDevice(want);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static int ws_reserve(must3r_hip_ctx* c, size_t bytes, hipStream_t s) {
    if (bytes <= c->ws_cap) return 0;
    if (c->ws) {
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(c->ws));
        c->ws = nullptr;
    }
    const size_t cap = align_up(bytes + bytes / 8, 1 << 20);
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&c->ws), cap));
    c->ws_cap = cap;
    return 0;
}
// Workspace planner of one forward: every buffer is requested ONCE, typed by its pointer; commit() sums the requests, reserves the arena and only then
// assigns the pointers (nothing may capture a buffer before it).  Each buffer starts at the next multiple of 256 bytes, in request order; a count of 0
// leaves the pointer null.
struct Workspace {
    struct Req { void* ptr; size_t bytes; };   // ptr: address of the caller's T* variable
    std::vector<Req> reqs;
    template <class T> void want(T*& p, size_t count) { p = nullptr; reqs.push_back(Req{&p, count * sizeof(T)}); }
    int commit(must3r_hip_ctx* c, hipStream_t s) {
        size_t need = 0, off = 0;
        for (const Req& r : reqs) need = align_up(need, 256) + r.bytes;
        M3R_OK(ws_reserve(c, need, s));
        for (const Req& r : reqs) {
            char* const at = c->ws + (off = align_up(off, 256));
            if (r.bytes) memcpy(r.ptr, &at, sizeof(at));
            off += r.bytes;
        }
        return 0;
    }
};

// upload a small host table to device memory that stays valid until the stream has consumed it
static int upload_table(must3r_hip_ctx* c, const void* host, size_t bytes, void** dev, hipStream_t s) {
    if (bytes > must3r_hip_ctx::kSlotBytes) return fail("view table too large (%zu bytes)", bytes);
    const int i = c->slot_next;
    c->slot_next = (i + 1) % must3r_hip_ctx::kSlots;
    if (c->slot_used[i]) HIP_OK(hipEventSynchronize(c->slot_ev[i]));
    char* h = c->pin + (size_t)i * must3r_hip_ctx::kSlotBytes;
    char* d = c->pin_dev + (size_t)i * must3r_hip_ctx::kSlotBytes;
    memcpy(h, host, bytes);
    // (r06, measured and dropped: a one-block copy KERNEL reading the pinned slot instead of this copy-engine transfer -- the 28 gaps of ~35 us per one-scene pass that
    // surround these uploads became ~40 gaps of 6-40 us, 59.3 vs 58.7 ms per pass: scripts/r06_runs/c08_tables.sh, profiles/r06_single_scene_seams.txt)
    HIP_OK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(c->slot_ev[i], s));
    c->slot_used[i] = true;
    *dev = d;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// profiling helpers
// ------------------------------------------------------------------------------------------------
static hipEvent_t ev_get(must3r_hip_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
struct ProfScope {
    must3r_hip_ctx* c; hipStream_t s; ProfEntry e; bool on;
    ProfScope(must3r_hip_ctx* c_, hipStream_t s_, int cat, double flops) : c(c_), s(s_), on(c_ && c_->prof) {
        if (on) { e.a = ev_get(c); e.b = ev_get(c); e.cat = cat; e.flops = flops; e.kern[0] = 0; (void)hipEventRecord(e.a, s); }
    }
    void kernel(const char* name, const char* suffix = "") { if (on) snprintf(e.kern, sizeof(e.kern), "%s%s", name, suffix); }
    ~ProfScope() { if (on) { (void)hipEventRecord(e.b, s); c->prof_entries.push_back(e); } }
};
static void prof_flush(must3r_hip_ctx* c) {
    for (auto& e : c->prof_entries) {
        (void)hipEventSynchronize(e.b);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e.a, e.b);
        c->prof_ms[e.cat] += ms;
        c->prof_flops[e.cat] += e.flops;
        c->prof_calls[e.cat] += 1;
        if (e.kern[0]) {
            ProfKern& k = c->prof_kern[e.kern];
            k.ms += ms; k.flops += e.flops; k.calls += 1;
        }
        c->ev_pool.push_back(e.a);
        c->ev_pool.push_back(e.b);
    }
    c->prof_entries.clear();
}

// ------------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------------
// ws_override >= 0: the caller chose the weight layout of THIS launch (wmlp below); otherwise the context's mode decides
static int gemm(must3r_hip_ctx* c, DType dt, Epi epi, GemmArgs a, hipStream_t s, int ws_override = -1) {
    const char* err = "";
    const long nbat = a.batch > 1 ? a.batch : 1;
    const int ws = ws_override >= 0 ? ws_override : ((c && epi != EPI_HEAD) ? c->wsplit : a.wsplit);
    const long tiles128 = (long)((a.M + 127) / 128) * (a.N / 128) * nbat;
    const int cat = ws == 2 ? (((long)((a.M + 127) / 128) * (a.N / 64) * nbat >= 384) ? PC_GEMM128 : PC_GEMM64)
                            : ((a.N % 128 == 0 && tiles128 >= 192) ? PC_GEMM128 : PC_GEMM64);
    if (ws_override >= 0) a.wsplit = ws_override;
    else if (c && epi != EPI_HEAD) a.wsplit = c->wsplit;
    if (c && a.wsplit == 2 && c->mlp_plain && epi != EPI_HEAD && !c->sparse_lo.empty() && opt(OPT_SPARSE_LO) != 0) {   // (the sparse copies of an earlier MUST3R_F16_WA forward are not for MUST3R_F16_W2)
        auto it = c->sparse_lo.find(a.W);
        if (it != c->sparse_lo.end()) { a.Wlo_sp = it->second.vals; a.Widx_sp = it->second.idx; a.wsp_rows = it->second.rows; }
    }
    ProfScope ps(c, s, cat, 2.0 * a.M * a.N * a.K * (a.batch > 1 ? a.batch : 1));
    if (launch_gemm(dt, epi, a, s, &err)) return fail("%s (M=%d N=%d K=%d epi=%d)", err, a.M, a.N, a.K, (int)epi);
    ps.kernel(gemm_last_kernel());
    return 0;
}
static GemmArgs gargs(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int lda, int ldc) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc;
    return a;
}
static LnArgs lnargs(const float* x, const float* add, const float* w, const float* b, void* o16, void* o16lo, float* o32,
                     float* copy, int M, int C, float eps) {
    LnArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.add = add; a.w = w; a.b = b; a.out16 = o16; a.out16_lo = o16lo; a.out32 = o32; a.copy32 = copy;
    a.M = M; a.C = C; a.eps = eps;
    return a;
}
static int layernorm_a(must3r_hip_ctx* c, DType dt, const LnArgs& a, hipStream_t s) {
    const char* err = "";
    ProfScope ps(c, s, PC_LN, 0.0);
    if (launch_layernorm(dt, a, s, &err)) return fail("%s", err);
    return 0;
}
// The two launches of the prediction head, shared by must3r_hip_decode and the training forward (train_head.hip; c = nullptr there: no profiling):
// LayerNorm of the residual stream into the [y_hi | y_lo | y_hi] rows of 3 D (+ the fp32 y of return_feats), then ONE plain GEMM over K = 3 D against the
// pixel-shuffle-ordered [W_hi | W_hi | W_lo] rows, scattered to [views][H][W][7].
int m3r::head_layernorm(must3r_hip_ctx* c, DType dt, const float* x, const float* gamma, const float* beta, void* hcat, float* y32, int R, int D, float eps,
                        hipStream_t s) {
    uint16_t* h = reinterpret_cast<uint16_t*>(hcat);
    LnArgs la = lnargs(x, nullptr, gamma, beta, h, h + D, y32, nullptr, R, D, eps);
    la.out16_dup = h + 2 * D;
    la.ld16 = 3 * D;
    return layernorm_a(c, dt, la, s);
}
int m3r::head_linear(must3r_hip_ctx* c, DType dt, const void* hcat, const void* wcat, const float* bias_ps, float* pointmaps, int rows, int D, int OUT, int ntok,
                     int gw, int H, int Wimg, int head_views, long long head_scene_skip, hipStream_t s) {
    GemmArgs ga = gargs(hcat, wcat, bias_ps, pointmaps, rows, OUT, 3 * D, 3 * D, 0);
    ga.ntok = ntok; ga.gw = gw; ga.H = H; ga.Wimg = Wimg;
    ga.head_views = head_views; ga.head_scene_skip = head_scene_skip;
    return gemm(c, dt, EPI_HEAD, ga, s);
}
static int quant8(must3r_hip_ctx* c, DType dt, const void* in16, int ld_in, void* out8, int ld_out, void* const* out_table,
                  int rows_per_group, size_t rows, int cols, int tail_cols, hipStream_t s) {
#ifdef M3R_ATTN_FP8
    const char* err = "";
    ProfScope ps(c, s, PC_MISC, 0.0);
    if (launch_quant8(dt, in16, ld_in, out8, ld_out, out_table, rows_per_group, rows, cols, tail_cols, s, &err)) return fail("%s", err);
    return 0;
#else
    return fail("quant8: the e4m3 attention path is an experiment build (make EXTRA=-DM3R_ATTN_FP8)");
#endif
}
static int attention(must3r_hip_ctx* c, DType dt, const AttnArgs& a, double flops, int cat, hipStream_t s) {
    const char* err = "";
    if (a.nsplit > 1 && !a.dense_rows) {
        ProfScope ps(c, s, PC_ATTN_COMBINE, 0.0);
        if (launch_attention_phase(dt, a, 0, s, &err)) return fail("%s", err);
    }
    {
        ProfScope ps(c, s, cat, flops);   // the attention kernel alone: what rocprofv3 reports under its symbol
        if (launch_attention_phase(dt, a, 1, s, &err)) return fail("%s", err);
        ps.kernel(attention_last_kernel(), cat == PC_ATTN_SA ? "/self" : "/cross");
    }
    if (a.nsplit > 1) {
        ProfScope ps(c, s, PC_ATTN_COMBINE, 0.0);
        if (launch_attention_phase(dt, a, 2, s, &err)) return fail("%s", err);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// parameters
// ------------------------------------------------------------------------------------------------
static void expect(must3r_hip_ctx* c, const std::string& name, std::vector<int64_t> shape, bool optional = false) {
    Param p;
    p.optional = optional;
    p.shape = shape;
    p.n = 1;
    for (auto d : shape) p.n *= (size_t)d;
    c->params[name] = p;
}
static void expect_linear(must3r_hip_ctx* c, const std::string& pfx, int64_t out, int64_t in, bool optional = false) {
    expect(c, pfx + ".weight", {out, in}, optional);
    expect(c, pfx + ".bias", {out}, optional);
}
static void expect_ln(must3r_hip_ctx* c, const std::string& pfx, int64_t dim, bool optional = false) {
    expect(c, pfx + ".weight", {dim}, optional);
    expect(c, pfx + ".bias", {dim}, optional);
}
static bool is_loaded(must3r_hip_ctx* c, const std::string& name) {
    auto it = c->params.find(name);
    return it != c->params.end() && it->second.loaded;
}

static void build_expected(must3r_hip_ctx* c) {
    const must3r_hip_config& g = c->cfg;
    const int64_t C = g.enc_dim, D = g.dec_dim, p = g.patch_size, r = g.mlp_ratio;
    expect(c, "encoder.patch_embed.proj.weight", {C, 3, p, p});
    expect(c, "encoder.patch_embed.proj.bias", {C});
    for (int i = 0; i < g.enc_depth; ++i) {
        const std::string b = "encoder.blocks_enc." + std::to_string(i);
        expect_ln(c, b + ".norm1", C);
        expect_linear(c, b + ".attn.qkv", 3 * C, C);
        expect_linear(c, b + ".attn.proj", C, C);
        expect_ln(c, b + ".norm2", C);
        expect_linear(c, b + ".mlp.fc1", r * C, C);
        expect_linear(c, b + ".mlp.fc2", C, r * C);
    }
    expect_ln(c, "encoder.norm_enc", C);
    expect(c, "decoder.image2_embed", {1, 1, D});
    expect_linear(c, "decoder.feat_embed_enc_to_dec", D, C);
    for (int i = 0; i < g.dec_depth; ++i) {
        const std::string b = "decoder.blocks_dec." + std::to_string(i);
        expect_ln(c, b + ".norm1", D);
        expect_linear(c, b + ".attn.qkv", 3 * D, D);
        expect_linear(c, b + ".attn.proj", D, D);
        expect_ln(c, b + ".norm2", D);
        expect_ln(c, b + ".norm_y", D);
        expect_linear(c, b + ".cross_attn.projq", D, D);
        expect_linear(c, b + ".cross_attn.projk", D, D);
        expect_linear(c, b + ".cross_attn.projv", D, D);
        expect_linear(c, b + ".cross_attn.proj", D, D);
        expect_ln(c, b + ".norm3", D);
        expect_linear(c, b + ".mlp.fc1", r * D, D);
        expect_linear(c, b + ".mlp.fc2", D, r * D);
    }
    // feedback_mechanism.py:11-22: 'single_mlp' (fc1/fc2 + norm), 'single_linear' (weight/bias + norm) or no feedback layer:
    // all optional here, told apart by which keys were loaded; finalize rejects incomplete or mixed sets
    expect_linear(c, "decoder.feedback_layer.fc1", 4 * D, D, true);
    expect_linear(c, "decoder.feedback_layer.fc2", D, 4 * D, true);
    expect_linear(c, "decoder.feedback_layer", D, D, true);
    expect_ln(c, "decoder.feedback_norm", D, true);
    expect_ln(c, "decoder.norm_dec", D);
    expect_linear(c, "decoder.head_dec.proj", p * p * 7, D);
}

static Param* param(must3r_hip_ctx* c, const std::string& name) {
    auto it = c->params.find(name);
    return it == c->params.end() ? nullptr : &it->second;
}
static const float* p32(must3r_hip_ctx* c, const std::string& name) { return c->params.at(name).d; }

// packed 16-bit copy (and optional low part) of a parameter, created on first use for a dtype
static int p16p(must3r_hip_ctx* c, Param& p, DType dt, bool want_lo, const void** hi, const void** lo, hipStream_t s);
static int w16p(must3r_hip_ctx* c, Param& p, DType dt, const void** hi, hipStream_t s);
static int p16(must3r_hip_ctx* c, const std::string& name, DType dt, bool want_lo, const void** hi, const void** lo,
               hipStream_t s) {
    return p16p(c, c->params.at(name), dt, want_lo, hi, lo, s);
}
static int w16(must3r_hip_ctx* c, const std::string& name, DType dt, const void** hi, hipStream_t s) {
    return w16p(c, c->params.at(name), dt, hi, s);
}

// Param-based forms of p16 / w16 (the per-layer loops use the tables below instead of building the parameter name per launch)
static int p16p(must3r_hip_ctx* c, Param& p, DType dt, bool want_lo, const void** hi, const void** lo, hipStream_t s) {
    const char* err = "";
    if (!p.h16[dt] || (want_lo && !p.l16[dt])) {
        if (!p.h16[dt]) HIP_OK(hipMalloc(&p.h16[dt], p.n * 2));
        if (want_lo && !p.l16[dt]) HIP_OK(hipMalloc(&p.l16[dt], p.n * 2));
        if (launch_split16(dt, p.d, p.h16[dt], want_lo ? p.l16[dt] : nullptr, p.n, s, &err)) return fail("%s", err);
    }
    *hi = p.h16[dt];
    if (lo) *lo = p.l16[dt];
    return 0;
}
static int w16p(must3r_hip_ctx* c, Param& p, DType dt, const void** hi, hipStream_t s) {
    if (c->wsplit != 2) return p16p(c, p, dt, false, hi, nullptr, s);
    if (!p.x2[dt]) {
        const void *h, *l;
        M3R_OK(p16p(c, p, dt, true, &h, &l, s));
        const size_t rows = (size_t)p.shape[0], K = p.n / rows;
        HIP_OK(hipMalloc(&p.x2[dt], p.n * 4));
        HIP_OK(hipMemcpy2DAsync(p.x2[dt], K * 4, h, K * 2, K * 2, rows, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpy2DAsync(reinterpret_cast<char*>(p.x2[dt]) + K * 2, K * 4, l, K * 2, K * 2, rows, hipMemcpyDeviceToDevice, s));
        // the separate hi / lo copies are dead once the interleaved rows exist (they are rebuilt from the fp32 master if a later call
        // asks for the plain 16-bit mode): 4 of the 16 bytes per parameter.  hipFree waits for the copies above (first use only).
        (void)hipFree(p.h16[dt]); p.h16[dt] = nullptr;
        (void)hipFree(p.l16[dt]); p.l16[dt] = nullptr;
    }
    // r05: the 2:4-sparse low part for the chip-filling kernels -- MUST3R_F16_WA only (mlp_plain): there the error budget is the plain Mlp weights' and the
    // dropped half of W_lo is invisible (scripts/emul/sparse_lo.py: 5.99e-4 vs 6.05e-4); MUST3R_F16_W2 exists for its 4e-4 and keeps the dense low part
    // (all-sparse would be 4.4e-4 against 3.4e-4).  fp16; M3R_SPARSE_LO=0: never.  rows x K / 2 values + rows x K / 8 bytes of positions, built on first use.
    const bool sparse_on = opt(OPT_SPARSE_LO) != 0;
    if (sparse_on && c->mlp_plain && dt == DT_F16 && !p.sp_vals) {
        const size_t rows = (size_t)p.shape[0], K = p.n / rows;
        if (rows % 128 == 0 && K % 64 == 0) {
            const char* err = "";
            HIP_OK(hipMalloc(&p.sp_vals, rows * K));
            HIP_OK(hipMalloc(&p.sp_idx, rows * K / 8));
            if (launch_sparse24_pack(p.d, (int)rows, (int)K, p.sp_vals, p.sp_idx, s, &err)) return fail("%s", err);
            c->sparse_lo[p.x2[dt]] = {p.sp_vals, p.sp_idx, (int)rows};
        }
    }
    *hi = p.x2[dt];
    return 0;
}
// weight operand of an Mlp Linear (fc1, fc2, the feedback Mlp): the plain 16-bit copy in MUST3R_F16_WA mode -- the launch then runs
// one MFMA pass (*ws = 0) -- and the context's layout otherwise
static int wmlp(must3r_hip_ctx* c, Param& p, DType dt, const void** w, int* ws, hipStream_t s) {
    if (c->wsplit == 2 && c->mlp_plain) { *ws = 0; return p16p(c, p, dt, false, w, nullptr, s); }
    *ws = c->wsplit;
    return w16p(c, p, dt, w, s);
}
static void build_layer_tables(must3r_hip_ctx* c, bool decoder) {
    std::vector<std::vector<Param*>>& tab = decoder ? c->dec_tab : c->enc_tab;
    const int depth = decoder ? c->cfg.dec_depth : c->cfg.enc_depth;
    tab.assign(depth, std::vector<Param*>(LF_COUNT, nullptr));
    for (int l = 0; l < depth; ++l) {
        const std::string b = (decoder ? "decoder.blocks_dec." : "encoder.blocks_enc.") + std::to_string(l) + ".";
        for (int f = 0; f < LF_COUNT; ++f) tab[l][f] = param(c, b + kLayerFieldNames[f]);
    }
}

// [W_hi | W_hi | W_lo] rows: with the activation laid out as [y_hi | y_lo | y_hi] the three products of the split-precision head
// (y_hi W_hi + y_lo W_hi + y_hi W_lo) are ONE plain GEMM over K = 3 in
static int w3(must3r_hip_ctx* c, const std::string& name, DType dt, const void** out, hipStream_t s) {
    Param& p = c->params.at(name);
    if (!p.x3[dt]) {
        const void *h, *l;
        M3R_OK(p16(c, name, dt, true, &h, &l, s));
        const size_t rows = (size_t)p.shape[0], K = p.n / rows;
        HIP_OK(hipMalloc(&p.x3[dt], p.n * 6));
        char* d = reinterpret_cast<char*>(p.x3[dt]);
        HIP_OK(hipMemcpy2DAsync(d, K * 6, h, K * 2, K * 2, rows, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpy2DAsync(d + K * 2, K * 6, h, K * 2, K * 2, rows, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpy2DAsync(d + K * 4, K * 6, l, K * 2, K * 2, rows, hipMemcpyDeviceToDevice, s));
    }
    *out = p.x3[dt];
    return 0;
}

extern "C" int must3r_hip_rope_table(float freq, float f0, int npos, float* out) {
    // angle(p, i) = p * f0 * freq^(-i/16), i in [0,16)  (croco RoPE2D, head dim 64)
    for (int p = 0; p < npos; ++p)
        for (int i = 0; i < 16; ++i) {
            const float inv = f0 / powf(freq, (float)i / 16.0f);
            const float ang = (float)p * inv;
            out[(p * 16 + i) * 2 + 0] = cosf(ang);
            out[(p * 16 + i) * 2 + 1] = sinf(ang);
        }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: lifetime / weights
// ------------------------------------------------------------------------------------------------
extern "C" int must3r_hip_abi_version(void) { return MUST3R_HIP_ABI_VERSION; }
extern "C" int must3r_hip_set_option(const char* name, long long value) {
    const char* err = "";
    if (opt_set(name, value, &err)) return fail("%s", err);
    return 0;
}
extern "C" const char* must3r_hip_last_error(void) { return g_err; }

extern "C" int must3r_hip_create(const must3r_hip_config* cfg, int device, must3r_hip_ctx** out) {
    if (!cfg || !out) return fail("create: null argument");
    if (cfg->patch_size != 16) return fail("create: patch_size must be 16");
    if (cfg->enc_dim != cfg->enc_heads * 64 || cfg->dec_dim != cfg->dec_heads * 64)
        return fail("create: head dim must be 64 (enc %d/%d, dec %d/%d)", cfg->enc_dim, cfg->enc_heads, cfg->dec_dim, cfg->dec_heads);
    if (cfg->enc_dim % 64 || cfg->dec_dim % 64 || cfg->enc_dim > 1024 || cfg->dec_dim > 1024)
        return fail("create: feature dims must be multiples of 64 and <= 1024");
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("create: no HIP device visible (the HIP path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("create: bad device %d", device);
    DeviceGuard dev_guard(device);
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("create: device is %s, this library is built for gfx950 only", prop.gcnArchName);
    must3r_hip_ctx* c = new must3r_hip_ctx();
    c->cfg = *cfg;
    c->device = device;
    build_expected(c);
    if (hipHostMalloc(reinterpret_cast<void**>(&c->pin), must3r_hip_ctx::kSlots * must3r_hip_ctx::kSlotBytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->pin_dev), must3r_hip_ctx::kSlots * must3r_hip_ctx::kSlotBytes) != hipSuccess) {
        delete c;
        return fail("create: staging allocation failed");
    }
    for (int i = 0; i < must3r_hip_ctx::kSlots; ++i) {
        (void)hipEventCreateWithFlags(&c->slot_ev[i], hipEventDisableTiming);
        c->slot_used[i] = false;
    }
    *out = c;
    return 0;
}

// drop the packed copies of a parameter (they are rebuilt from the fp32 master on next use)
static void free_packed(must3r_hip_ctx* c, Param& p) {
    for (int i = 0; i < 2; ++i) {
        if (p.x2[i]) c->sparse_lo.erase(p.x2[i]);
        for (void** q : {&p.h16[i], &p.l16[i], &p.x2[i], &p.x3[i]})
            if (*q) { (void)hipFree(*q); *q = nullptr; }
    }
    for (void** q : {&p.sp_vals, &p.sp_idx})
        if (*q) { (void)hipFree(*q); *q = nullptr; }
}

extern "C" void must3r_hip_destroy(must3r_hip_ctx* c) {
    if (!c) return;
    DeviceGuard dev_guard(c->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : c->params) {
        free_packed(c, kv.second);
        if (kv.second.d) (void)hipFree(kv.second.d);
    }
    if (c->rope_tab) (void)hipFree(c->rope_tab);
    if (c->ws) (void)hipFree(c->ws);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->pin_dev) (void)hipFree(c->pin_dev);
    for (int i = 0; i < must3r_hip_ctx::kSlots; ++i) (void)hipEventDestroy(c->slot_ev[i]);
    prof_flush(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
}

extern "C" int must3r_hip_load_weight(must3r_hip_ctx* c, const char* name, const float* data, int is_device, int ndim,
                                      const int64_t* shape) {
    if (!c || !name || !data) return fail("load_weight: null argument");
    Param* p = param(c, name);
    if (!p || p->derived) return fail("load_weight: unexpected key '%s'", name);
    bool same = (int)p->shape.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = p->shape[i] == shape[i];
    if (!same) return fail("load_weight: shape mismatch for '%s'", name);
    DeviceGuard dev_guard(c->device);
    if (!p->d) HIP_OK(hipMalloc(reinterpret_cast<void**>(&p->d), p->n * sizeof(float)));
    HIP_OK(hipMemcpy(p->d, data, p->n * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    free_packed(c, *p);
    p->loaded = true;
    if (strncmp(name, "encoder.", 8) == 0) c->fin_enc = false; else c->fin_dec = false;
    return 0;
}

static int derive(must3r_hip_ctx* c, const std::string& name, std::vector<int64_t> shape, const std::vector<float>& host) {
    Param& p = c->params[name];
    if (p.d) { (void)hipFree(p.d); p.d = nullptr; }
    free_packed(c, p);
    p.shape = shape;
    p.n = host.size();
    p.derived = true;
    p.loaded = true;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&p.d), p.n * sizeof(float)));
    HIP_OK(hipMemcpy(p.d, host.data(), p.n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
static int fetch(must3r_hip_ctx* c, const std::string& name, std::vector<float>& host) {
    Param& p = c->params.at(name);
    host.resize(p.n);
    HIP_OK(hipMemcpy(host.data(), p.d, p.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// "LN fold" operands of a Linear that follows a LayerNorm: W' = gamma (.) W, s_n = sum_k W'[n][k], c_n = (W beta + b)_n, so that
// LN(x) W^T + b = rstd (x W'^T - mu s) + c.  Derived parameters <block>.<linear>_ln.{weight, s, c}.
static int derive_ln_fold(must3r_hip_ctx* c, const std::string& pb, const char* norm, const char* lin) {
    std::vector<float> w, bb, gam, bet;
    M3R_OK(fetch(c, pb + lin + ".weight", w));
    M3R_OK(fetch(c, pb + lin + ".bias", bb));
    M3R_OK(fetch(c, pb + norm + ".weight", gam));
    M3R_OK(fetch(c, pb + norm + ".bias", bet));
    const size_t K = gam.size(), N = bb.size();
    if (w.size() != N * K || bet.size() != K) return fail("finalize: LN-fold shapes of %s%s", pb.c_str(), lin);
    std::vector<float> sn(N), cn(N);
    for (size_t n = 0; n < N; ++n) {
        double ss = 0.0, cc = bb[n];
        float* row = &w[n * K];
        for (size_t k = 0; k < K; ++k) {
            cc += (double)bet[k] * row[k];
            row[k] *= gam[k];
            ss += row[k];
        }
        sn[n] = (float)ss;
        cn[n] = (float)cc;
    }
    M3R_OK(derive(c, pb + lin + "_ln.weight", {(int64_t)N, (int64_t)K}, w));
    M3R_OK(derive(c, pb + lin + "_ln.s", {(int64_t)N}, sn));
    M3R_OK(derive(c, pb + lin + "_ln.c", {(int64_t)N}, cn));
    return 0;
}

extern "C" int must3r_hip_finalize_weights(must3r_hip_ctx* c, int parts) {
    if (!c) return fail("finalize: null context");
    if (!(parts & 3)) return fail("finalize: parts must include MUST3R_PART_ENCODER and/or MUST3R_PART_DECODER");
    DeviceGuard dev_guard(c->device);
    for (auto& kv : c->params) {
        const bool is_enc = kv.first.compare(0, 8, "encoder.") == 0;
        if (!((is_enc && (parts & 1)) || (!is_enc && (parts & 2)))) continue;
        if (!kv.second.loaded && !kv.second.derived && !kv.second.optional) return fail("finalize: missing key '%s'", kv.first.c_str());
    }
    if (parts & 2) {
        int mlp = 0, lin = 0, nrm = 0;
        for (const char* k : {"decoder.feedback_layer.fc1.weight", "decoder.feedback_layer.fc1.bias", "decoder.feedback_layer.fc2.weight",
                              "decoder.feedback_layer.fc2.bias"}) mlp += is_loaded(c, k);
        for (const char* k : {"decoder.feedback_layer.weight", "decoder.feedback_layer.bias"}) lin += is_loaded(c, k);
        for (const char* k : {"decoder.feedback_norm.weight", "decoder.feedback_norm.bias"}) nrm += is_loaded(c, k);
        const bool ok = (mlp == 4 && lin == 0 && nrm == 2) || (mlp == 0 && lin == 2 && nrm == 2) || (mlp == 0 && lin == 0 && nrm == 0);
        if (!ok) return fail("finalize: inconsistent feedback layer keys (single_mlp: fc1/fc2 + feedback_norm; single_linear: "
                             "weight/bias + feedback_norm; none: neither)");
    }
    // RoPE table for positions up to 256 (4096-pixel side), shared by both halves
    {
        c->rope_npos = 256;
        std::vector<float> t((size_t)c->rope_npos * 32);
        must3r_hip_rope_table(c->cfg.rope_freq, c->cfg.rope_f0, c->rope_npos, t.data());
        if (!c->rope_tab) HIP_OK(hipMalloc(reinterpret_cast<void**>(&c->rope_tab), t.size() * sizeof(float)));
        HIP_OK(hipMemcpy(c->rope_tab, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (parts & 1) {
        // r06: LN-fold operands of the encoder blocks (norm1 -> attn.qkv, norm2 -> mlp.fc1) for the chip-filling launches (GemmArgs::fold256)
        for (int l = 0; l < c->cfg.enc_depth; ++l) {
            const std::string pb = "encoder.blocks_enc." + std::to_string(l) + ".";
            M3R_OK(derive_ln_fold(c, pb, "norm1", "attn.qkv"));
            M3R_OK(derive_ln_fold(c, pb, "norm2", "mlp.fc1"));
        }
        c->enc_tab.clear();
        c->fin_enc = true;
    }
    if (!(parts & 2)) return 0;
    const must3r_hip_config& g = c->cfg;
    const int D = g.dec_dim;
    std::vector<float> a, b, o;
    // fused K|V projection per decoder layer: rows [0,D) = projk, [D,2D) = projv  (layers.py:87-88 cat([k,v],-1))
    for (int l = 0; l < g.dec_depth; ++l) {
        const std::string pb = "decoder.blocks_dec." + std::to_string(l) + ".cross_attn.";
        M3R_OK(fetch(c, pb + "projk.weight", a));
        M3R_OK(fetch(c, pb + "projv.weight", b));
        o = a; o.insert(o.end(), b.begin(), b.end());
        M3R_OK(derive(c, pb + "projkv.weight", {2 * D, D}, o));
        M3R_OK(fetch(c, pb + "projk.bias", a));
        M3R_OK(fetch(c, pb + "projv.bias", b));
        o = a; o.insert(o.end(), b.begin(), b.end());
        M3R_OK(derive(c, pb + "projkv.bias", {2 * D}, o));
    }
    // all layers' K|V projections and norm_y affine parameters stacked, for the grouped post-feedback projection
    {
        std::vector<float> wall, ball, nw, nb;
        for (int l = 0; l < g.dec_depth; ++l) {
            const std::string pb = "decoder.blocks_dec." + std::to_string(l);
            M3R_OK(fetch(c, pb + ".cross_attn.projkv.weight", a)); wall.insert(wall.end(), a.begin(), a.end());
            M3R_OK(fetch(c, pb + ".cross_attn.projkv.bias", a)); ball.insert(ball.end(), a.begin(), a.end());
            M3R_OK(fetch(c, pb + ".norm_y.weight", a)); nw.insert(nw.end(), a.begin(), a.end());
            M3R_OK(fetch(c, pb + ".norm_y.bias", a)); nb.insert(nb.end(), a.begin(), a.end());
        }
        M3R_OK(derive(c, "decoder.projkv_all.weight", {(int64_t)g.dec_depth * 2 * D, D}, wall));
        M3R_OK(derive(c, "decoder.projkv_all.bias", {(int64_t)g.dec_depth * 2 * D}, ball));
        M3R_OK(derive(c, "decoder.norm_y_all.weight", {(int64_t)g.dec_depth * D}, nw));
        M3R_OK(derive(c, "decoder.norm_y_all.bias", {(int64_t)g.dec_depth * D}, nb));
    }
    // pixel-shuffled head: new row (i*16+j)*7 + ch <- old row ch*256 + i*16 + j  (tools/image.py:9-14)
    {
        M3R_OK(fetch(c, "decoder.head_dec.proj.weight", a));
        M3R_OK(fetch(c, "decoder.head_dec.proj.bias", b));
        const int P = 256;
        std::vector<float> w2(a.size()), b2(b.size());
        for (int ch = 0; ch < 7; ++ch)
            for (int ij = 0; ij < P; ++ij) {
                const size_t nr = (size_t)ij * 7 + ch, orow = (size_t)ch * P + ij;
                memcpy(&w2[nr * D], &a[orow * D], sizeof(float) * D);
                b2[nr] = b[orow];
            }
        M3R_OK(derive(c, "decoder.head_dec.proj_ps.weight", {7 * P, D}, w2));
        M3R_OK(derive(c, "decoder.head_dec.proj_ps.bias", {7 * P}, b2));
    }
    // "LN fold" operands of the decoder blocks (one-view memory updates since r02, chip-filling batched calls since r06): the three Linears that follow a LayerNorm
    for (int l = 0; l < g.dec_depth; ++l) {
        const std::string pb = "decoder.blocks_dec." + std::to_string(l) + ".";
        M3R_OK(derive_ln_fold(c, pb, "norm1", "attn.qkv"));
        M3R_OK(derive_ln_fold(c, pb, "norm2", "cross_attn.projq"));
        M3R_OK(derive_ln_fold(c, pb, "norm3", "mlp.fc1"));
    }
    c->dec_tab.clear();   // rebuilt on the next decode (the derived entries above may be new)
    c->fin_dec = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// what the two forwards share: the precision mode, the LN-fold state, the two sublayers every block has
// ------------------------------------------------------------------------------------------------
// the ABI's dtype word -> c->dt (operand type of the kernels), c->wsplit, c->mlp_plain, c->attn8; false: not one of the four dtypes
static bool set_mode(must3r_hip_ctx* c, int dtype) {
    const int d = dtype & ~MUST3R_ATTN_FP8;
    if (d != MUST3R_BF16 && d != MUST3R_F16 && d != MUST3R_F16_W2 && d != MUST3R_F16_WA) return false;
    c->attn8 = (dtype & MUST3R_ATTN_FP8) ? 1 : 0;
    c->wsplit = (d == MUST3R_F16_W2 || d == MUST3R_F16_WA) ? 2 : 0;
    c->mlp_plain = d == MUST3R_F16_WA ? 1 : 0;
    c->dt = c->wsplit == 2 ? DT_F16 : (DType)d;
    return true;
}

// LN fold (kernels.hpp GemmArgs "LN fold") of one forward: the LayerNorm launches of the blocks are not issued; a residual GEMM leaves the 16-bit rows +
// per-fragment sums (out), the Linear behind the folded norm reads them with the gamma-scaled weight and normalises after its product (in)
struct Fold {
    uint16_t* x16 = nullptr;   // the residual stream rounded to fp16 (fold256: the shifted rows); null: this forward does not fold
    float* stats = nullptr;    // per row and 16-column fragment (fold256: 64-column wave tile) (sum, sum of squares)
    float* shift = nullptr;    // per row: the mean the last consumer measured (shift of the next rows)
    bool f256 = false;         // the chip-filling form (GemmArgs::fold256): shift is zeroed up front, the consumers add to it, its first producer reads zeros
    bool fresh = true;         // nothing measured yet in this call: the first consumer starts the estimate
    bool on() const { return x16 != nullptr; }
    void in(GemmArgs& g, const Param* s, const Param* c) {
        g.A = x16; g.ln_stats = stats; g.ln_s = s->d; g.bias = c->d; g.ln_eps = 1e-6f;
        g.ln_shift = shift; g.ln_shift_init = (fresh && !f256) ? 1 : 0; g.fold256 = f256 ? 1 : 0;
        fresh = false;
    }
    void out(GemmArgs& g, float* copy32) const { g.x16_out = x16; g.stats_out = stats; g.copy32_out = copy32; g.ln_shift = shift; g.fold256 = f256 ? 1 : 0; }   // copy32: the memorised input of the next block (decoder.py:304-305)
};

// rows and scratch of the block sublayers: R rows of width C (hidden width F) in the fp32 residual stream x
struct BlockRows {
    int R, C, heads, F;
    float* x; uint16_t *h16, *qkv, *a16, *g16;
    uint8_t* q8;               // e4m3 copies of q | k (fp8 attention build only)
    const int64_t* pos;        // [R, 2]
};
// the views of a self attention: device table, count, longest view, FLOPs, and (one view) the view itself to pass inline
struct SelfViews { const AttnView* dev; int n, max_n; double flops; const AttnView* inline0; };

// x += proj(attention(rope(qkv(norm1(x)))))  (layers.py:51-54 / :91).  fold_n1: norm1 is folded into qkv; otherwise its kernel runs, leaves copy32 (the
// block's memorised input) and mean_out (the row means: the shift of this block's proj producer) where given
static int self_attention_sublayer(must3r_hip_ctx* c, DType dt, const std::vector<Param*>& LP, const BlockRows& b, const SelfViews& v, Fold& fold, bool fold_n1,
                                   float* copy32, float* mean_out, hipStream_t s) {
    const int R = b.R, C = b.C;
    const bool a8 = kAttnFp8Built && c->attn8 != 0;   // (compiles out of the default build, kernels.hpp)
    const void* w;
    if (!fold_n1) {
        LnArgs la = lnargs(b.x, nullptr, LP[LF_N1W]->d, LP[LF_N1B]->d, b.h16, nullptr, nullptr, copy32, R, C, 1e-6f);
        if (mean_out) { la.mean_out = mean_out; fold.fresh = false; }
        M3R_OK(layernorm_a(c, dt, la, s));
    }
    M3R_OK(w16p(c, *LP[fold_n1 ? LF_QKVLN_W : LF_QKVW], dt, &w, s));
    GemmArgs ga = gargs(b.h16, w, LP[LF_QKVB]->d, b.qkv, R, 3 * C, C, C, 3 * C);
    if (fold_n1) fold.in(ga, LP[LF_QKVLN_S], LP[LF_QKVLN_C]);
    ga.pos = b.pos; ga.rope_tab = c->rope_tab; ga.rope_cols = 2 * C; ga.rope_npos = c->rope_npos;
    ga.out_scale = kQScale; ga.scale_cols = C;   // q *= 1/sqrt(64) * log2(e)
    M3R_OK(gemm(c, dt, EPI_QKV_ROPE, ga, s));
    AttnArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.Q = b.qkv; aa.K = b.qkv + C; aa.V = b.qkv + 2 * C; aa.O = b.a16;
    aa.ldq = aa.ldk = aa.ldv = 3 * C; aa.ldo = C; aa.heads = b.heads;
    aa.views = v.dev; aa.nviews = v.n; aa.max_nq = v.max_n; aa.scale = 0.125f; aa.q_prescaled = 1;
    if (v.inline0) { aa.view0_inline = 1; aa.view0 = *v.inline0; }
    if (a8 && !attention_is_small(v.n, b.heads, v.max_n, 1)) {   // e4m3 copies of q | k (one byte per element); V stays 16-bit
        M3R_OK(quant8(c, dt, b.qkv, 3 * C, b.q8, 2 * C, nullptr, 0, (size_t)R, 2 * C, 0, s));
        aa.Q = b.q8; aa.K = b.q8 + C; aa.ldq = aa.ldk = 2 * C; aa.fp8 = 1;
    }
    aa.max_nk = v.max_n;
    M3R_OK(attention(c, dt, aa, v.flops, PC_ATTN_SA, s));
    M3R_OK(w16p(c, *LP[LF_PROJW], dt, &w, s));
    GemmArgs gp = gargs(b.a16, w, LP[LF_PROJB]->d, b.x, R, C, C, C, C);
    if (fold.on()) fold.out(gp, nullptr);
    return gemm(c, dt, EPI_RESID_F32, gp, s);
}

// x += fc2(gelu(fc1(norm(x))))  (layers.py:54 / :98); norm_w: the block's last norm (LF_N2W in the encoder, LF_N3W in the decoder), folded into fc1 when the
// forward folds.  leave_rows: fc2 leaves the rows for the next block's norm1 (+ copy32, that block's memorised input)
static int mlp_sublayer(must3r_hip_ctx* c, DType dt, const std::vector<Param*>& LP, int norm_w, const BlockRows& b, Fold& fold, bool leave_rows, float* copy32,
                        hipStream_t s) {
    const int R = b.R, C = b.C, F = b.F;
    const bool folded = fold.on();
    const void* w;
    int ws;
    if (!folded) M3R_OK(layernorm_a(c, dt, lnargs(b.x, nullptr, LP[norm_w]->d, LP[norm_w + 1]->d, b.h16, nullptr, nullptr, nullptr, R, C, 1e-6f), s));
    M3R_OK(wmlp(c, *LP[folded ? LF_FC1LN_W : LF_FC1W], dt, &w, &ws, s));
    GemmArgs g1 = gargs(b.h16, w, LP[LF_FC1B]->d, b.g16, R, F, C, C, F);
    if (folded) fold.in(g1, LP[LF_FC1LN_S], LP[LF_FC1LN_C]);
    M3R_OK(gemm(c, dt, EPI_STORE16_GELU, g1, s, ws));
    M3R_OK(wmlp(c, *LP[LF_FC2W], dt, &w, &ws, s));
    GemmArgs g2 = gargs(b.g16, w, LP[LF_FC2B]->d, b.x, R, C, F, F, C);
    if (leave_rows) fold.out(g2, copy32);
    return gemm(c, dt, EPI_RESID_F32, g2, s, ws);
}

// ------------------------------------------------------------------------------------------------
// encoder  (Dust3rEncoder.forward encoder.py:46-52)
// ------------------------------------------------------------------------------------------------
static int encode_chunk(must3r_hip_ctx* c, DType dt, const float* img, int V, int H, int W, float* out_tokens,
                        int64_t* out_pos, hipStream_t s) {
    const must3r_hip_config& g = c->cfg;
    const int C = g.enc_dim, gh = H / 16, gw = W / 16, N = gh * gw, R = V * N, F = g.mlp_ratio * C;
    const char* err = "";
    const bool a8 = kAttnFp8Built && c->attn8 != 0;   // (compiles out of the default build, kernels.hpp)
    // r06, LN fold on the chip-filling launches (GemmArgs::fold256; MUST3R_F16_WA): norm1 of blocks 1.. and norm2 of every block are not launched -- the residual
    // GEMM in front of them (fc2 of the previous block / proj) leaves the shifted rows in fp16 + per-wave-tile sums, qkv / fc1 normalise after their product.
    // Block 0's norm1 keeps its kernel (its rows come from the patch embedding, an EPI_F32 launch).  Only when every Linear of the block lands on the fold kernels.
    if (c->enc_tab.empty()) build_layer_tables(c, false);
    const bool f256 = opt(OPT_LNFOLD256) != 0 && dt == DT_F16 && c->wsplit == 2 && c->mlp_plain && !a8 && (C == 768 || C == 1024) &&
                      c->enc_tab[0][LF_QKVLN_W] && c->enc_tab[0][LF_FC1LN_W] &&
                      gemm_fold256_shape_ok(R, 3 * C, C, true) && gemm_fold256_shape_ok(R, C, C, true) &&
                      gemm_fold256_shape_ok(R, F, C, false) && gemm_fold256_shape_ok(R, C, F, false);
    Workspace ws; uint16_t* P16;
    BlockRows b{R, C, g.enc_heads, F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_pos};
    Fold fold; fold.f256 = f256;
    ws.want(P16, (size_t)R * 768);
    ws.want(b.x, (size_t)R * C);
    ws.want(b.h16, (size_t)R * C);
    ws.want(b.qkv, (size_t)R * 3 * C);
    ws.want(b.a16, (size_t)R * C);
    ws.want(b.g16, (size_t)R * F);
    ws.want(b.q8, a8 ? (size_t)R * 2 * C : 0);
    ws.want(fold.x16, f256 ? (size_t)R * C : 0);                  // the shifted residual rows in fp16
    ws.want(fold.stats, f256 ? (size_t)R * (C / 64) * 2 : 0);     // per row and 64-column wave tile (sum, sum of squares)
    ws.want(fold.shift, f256 ? (size_t)R : 0);                    // per row: the current mean (GemmArgs::ln_shift)
    M3R_OK(ws.commit(c, s));
    if (f256) HIP_OK(hipMemsetAsync(fold.shift, 0, (size_t)R * sizeof(float), s));

    {
        ProfScope ps(c, s, PC_MISC, 0.0);
        if (launch_fill_pos(out_pos, V, gh, gw, s, &err)) return fail("%s", err);
        if (launch_im2col(dt, img, P16, V, H, W, s, &err)) return fail("%s", err);
    }
    std::vector<AttnView> views(V);
    for (int v = 0; v < V; ++v) views[v] = AttnView{v * N, N, v * N, N, 0, 0};
    void* views_dev = nullptr;
    M3R_OK(upload_table(c, views.data(), sizeof(AttnView) * V, &views_dev, s));
    const SelfViews sv{reinterpret_cast<const AttnView*>(views_dev), V, N, 4.0 * V * (double)N * N * C, nullptr};   // (never inline: the encoder reads its table)

    const void* w;
    M3R_OK(w16(c, "encoder.patch_embed.proj.weight", dt, &w, s));
    M3R_OK(gemm(c, dt, EPI_F32, gargs(P16, w, p32(c, "encoder.patch_embed.proj.bias"), b.x, R, C, 768, 768, C), s));
    for (int l = 0; l < g.enc_depth; ++l) {
        const std::vector<Param*>& LP = c->enc_tab[l];
        M3R_OK(self_attention_sublayer(c, dt, LP, b, sv, fold, f256 && l > 0, nullptr, nullptr, s));
        M3R_OK(mlp_sublayer(c, dt, LP, LF_N2W, b, fold, f256 && l + 1 < g.enc_depth, nullptr, s));   // (leaves the next block's norm1 its rows)
    }
    return layernorm_a(c, dt, lnargs(b.x, nullptr, p32(c, "encoder.norm_enc.weight"), p32(c, "encoder.norm_enc.bias"), nullptr, nullptr,
                     out_tokens, nullptr, R, C, 1e-6f), s);
}

extern "C" int must3r_hip_encode(must3r_hip_ctx* c, int dtype, const float* img, int n_views, int H, int W,
                                 float* out_tokens, int64_t* out_pos, void* stream) {
    if (!c || !img || !out_tokens || !out_pos) return fail("encode: null argument");
    if (!c->fin_enc) return fail("encode: encoder weights not finalized");
    if ((dtype & MUST3R_ATTN_FP8) && !kAttnFp8Built) return fail("encode: MUST3R_ATTN_FP8 is an experiment build (make EXTRA=-DM3R_ATTN_FP8): measured outside the 1e-3 target for +0.4 %%");
    if (!set_mode(c, dtype)) return fail("encode: bad dtype %d", dtype & ~MUST3R_ATTN_FP8);
    if (n_views <= 0) return 0;
    if (H <= 0 || W <= 0 || H % 16 || W % 16) return fail("encode: H=%d W=%d must be positive multiples of 16", H, W);
    if (H / 16 > c->rope_npos || W / 16 > c->rope_npos) return fail("encode: image too large for the RoPE table");
    DeviceGuard dev_guard(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int N = (H / 16) * (W / 16);
    // rows per chunk: bounds the workspace (~32k token rows: the 16-bit activations of a chunk stay inside the 256 MB MALL between producer and
    // consumer launches).  M3R_ENC_CHUNK_ROWS: A/B instrument -- larger chunks lose less to the round quantisation of the
    // one-block-per-CU GEMMs (40 views: 93.75 % tile fill; 42 views: 98.4 %; 64 / 128 views: 100 %) but stream their activations through HBM.
    // Under the cap the chunk sizes come from encode_plan (encode_plan.hpp): the partition whose GEMM rounds are fullest, never more chunks than an equal split
    // makes (560 views of 768 tokens: 12 x 42 + 35 + 21 instead of 14 x 40; 80 views: 2 x 40 as before, 42 + 38 costs the same rounds and the tie goes to the even
    // split); shapes that are not on the 256-row kernels keep the equal split.  Every chunk sizes its own workspace, view table and positions (encode_chunk), the largest comes first.
    const std::vector<int> plan = encode_plan(n_views, N, c->cfg.enc_dim, c->cfg.mlp_ratio * c->cfg.enc_dim, opt(OPT_ENC_CHUNK_ROWS), gemm_route_opts());
    int v0 = 0;
    for (const int nv : plan) {
        M3R_OK(encode_chunk(c, c->dt, img +(size_t)v0 * 3 * H * W, nv, H, W, out_tokens + (size_t)v0 * N * c->cfg.enc_dim,
                            out_pos + (size_t)v0 * N * 2, s));
        v0 += nv;
    }
    if (v0 != n_views) return fail("encode: the chunk plan covers %d of %d views", v0, n_views);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// decoder  (MUSt3R.forward_list decoder.py:158-265; forward :267-350 is the single-group case)
// ------------------------------------------------------------------------------------------------
// one native call = one launch sequence (decode_impl, at the end of this section); must3r_hip_decode (below) validates the arguments and cuts oversize
// render calls.  Plan and state of one call; the plan (decode_plan) depends on cfg, the arguments and the options only:
struct Decode {
    must3r_hip_ctx* c; const must3r_hip_decode_args* A; void* stream; hipStream_t s; DType dt; bool a8;
    int C, D, Hh, F, L, Nm, mode;
    // row layout
    int S, Rs, R, total_views, max_n; long long mem_stride; std::vector<int> grow0; bool one_block;
    // the call's flags
    bool update, use_mask, lone_view, need_pre_kv, lnf, lnf_all, f256;
    const must3r_hip_cp* cp;
    int max_nk_ca, ca_split, memD; size_t split_bytes, memRB, kvs_rows1, kvs_rows, kv16_rows;
    // workspace (decode_workspace)
    BlockRows b; Fold fold;
    uint16_t *t16, *hcat, *q16, *yall, *kvs, *ytmp, *kv16; float *newmem, *off32; char* split_ws; uint8_t* kvs8;
    // per-call tables (decode_tables)
    std::vector<AttnView> tab; SelfViews sv; const AttnView* ca_views; double ca_flops; void* const* kvout;
};

static void decode_plan(Decode& d) {
    must3r_hip_ctx* c = d.c; const must3r_hip_decode_args* A = d.A;
    const must3r_hip_config& g = c->cfg;
    d.dt = c->dt;
    d.a8 = kAttnFp8Built && c->attn8 != 0;   // (the default build has no e4m3 attention path: every `a8` branch below compiles out)
    d.C = g.enc_dim; d.D = g.dec_dim; d.Hh = g.dec_heads; d.F = g.mlp_ratio * g.dec_dim; d.L = g.dec_depth; d.Nm = A->n_mem; d.mode = A->mem_mode;
    const int D = d.D, F = d.F, Nm = d.Nm;
    // ---- row layout: scenes (batch elements, decoder.py:170-186: B), then groups, then views, then tokens (x_cat order of a scene,
    //      decoder.py:211-214).  The S scenes of a call never interact (memory, labels and attention are per batch element): they
    //      share every launch -- M = S x rows-per-scene in the GEMMs, S x views in the attention tables -- and nothing else.
    const int S = d.S = A->n_scenes > 1 ? A->n_scenes : 1;
    d.mem_stride = S > 1 ? A->mem_scene_stride : 0;      // memory rows between two scenes' buffers
    int Rs = 0, views_s = 0;
    d.max_n = 0;
    d.grow0.resize(A->n_groups);
    for (int gi = 0; gi < A->n_groups; ++gi) {
        const must3r_hip_group& G = A->groups[gi];
        d.grow0[gi] = Rs;
        Rs += G.n_views * G.n_tokens;
        views_s += G.n_views;
        if (G.n_tokens > d.max_n) d.max_n = G.n_tokens;
    }
    const int R = S * Rs;
    d.Rs = Rs; d.R = R; d.total_views = S * views_s;
    d.one_block = A->n_groups == 1;                           // a group's [S, n_views, n_tokens] rows ARE the call's row order
    const bool update = d.update = !A->render;
    // r06, context-parallel cross attention (include/must3r_hip.h must3r_hip_cp): Nm = THIS rank's shard of the memory (possibly empty), the call's semantics
    // follow the GLOBAL row count (validated by must3r_hip_decode: one-view update of one scene, 'kv' memory, 16-bit attention)
    d.cp = A->cp;
    const int Nm_global = d.cp ? d.cp->n_mem_total : Nm;
    d.use_mask = update && (Nm_global > 0 || views_s > 1);    // decoder.py:199 / :293
    d.lone_view = update && views_s == 1 && Nm_global > 0;    // own tokens excluded -> keys = old memory only
    d.need_pre_kv = update && !d.lone_view;                   // pre-feedback K|V of the new tokens are attended
    // LN fold (one-view update calls, fp16 + split weights): the LayerNorm launches of the blocks are not issued; the residual GEMMs
    // leave 16-bit rows + per-fragment sums, the Linears that follow normalise after their product (kernels.hpp GemmArgs "LN fold").
    // Block 0's norm1 keeps its kernel (35 of the 36 launches go): a consumer multiplies the fp16 copy of x - shift, so its error grows with
    // |mean - shift| / sigma of the row, and the embedded tokens come with no estimate of their mean -- a common offset of 40 sigma in the embed
    // bias took the update pointmaps of a 48 x 64 scene from 4.9e-4 to 1.4e-3 (tests/test_lnfold_model_gpu.py; the bound per launch form:
    // tests/lnfold_forms.py).  The LayerNorm launch pays nothing for an offset and leaves the row means as the shift of block 0's first producer.  M3R_LNFOLD=2 (A/B instrument): block 0's norm1 folded too.
    // (S > 1: the consumers of the fold only exist on the small-M tile shapes; a batched call is past the launch floor the fold removes)
    d.lnf = opt(OPT_LNFOLD) != 0 && update && !d.need_pre_kv && c->wsplit == 2 && d.dt == DT_F16 && !d.a8 && !A->feats && A->n_groups == 1 &&
            S == 1 && D == 768 && F % 96 == 0;
    // r06: the same fold on the chip-filling launches of a batched call -- update or render -- (GemmArgs::fold256; MUST3R_F16_WA): block 0's norm1 keeps its kernel
    // (its rows come from an EPI_F32 launch), every other norm1 / norm2 / norm3 is folded.  Only when every Linear of the block lands on the fold kernels.
    d.f256 = !d.lnf && opt(OPT_LNFOLD256) != 0 && c->wsplit == 2 && c->mlp_plain && d.dt == DT_F16 && !d.a8 && !A->feats && !A->cp && (D == 768 || D == 1024) &&
             gemm_fold256_shape_ok(R, 3 * D, D, true) && gemm_fold256_shape_ok(R, D, D, true) &&
             gemm_fold256_shape_ok(R, F, D, false) && gemm_fold256_shape_ok(R, D, F, false);
    d.lnf_all = d.lnf && opt(OPT_LNFOLD) == 2;   // block 0's norm1 folded as well: its consumer reads unshifted rows
    // split-KV cross attention when the launch cannot fill the chip (sequential memory update: one view per call)
    d.max_nk_ca = A->render ? Nm : Nm + (d.lone_view ? 0 : Rs);
    // (context parallel: the local attention always leaves split-KV partials -- at least two splits, an empty one costs nothing -- for the partial merge)
    d.ca_split = attention_pick_split(d.total_views, d.Hh, d.max_n, d.max_nk_ca);
    if (d.cp) d.ca_split = Nm > 0 ? (d.ca_split > 2 ? d.ca_split : 2) : 0;
    d.split_bytes = attention_split_scratch_bytes(d.ca_split, R, d.Hh);
    // memory_mode 'norm_y' / 'raw': the memory holds (normalised / raw) tokens, K|V of ALL attended rows are projected
    // per layer per call into scratch (the reference re-projects them per query view, layers.py:92-96)
    d.memD = d.mode == MUST3R_MEM_KV ? 2 * D : D;
    // bytes of a memory row: 16-bit elements, except the K (e4m3, D bytes) | V (16-bit, 2 D bytes) rows of the fp8-attention mode
    d.memRB = (d.a8 && d.mode == MUST3R_MEM_KV) ? (size_t)3 * D : (size_t)d.memD * 2;
    d.kvs_rows1 = d.mode == MUST3R_MEM_KV ? 0 : (size_t)d.max_nk_ca;   // per scene
    d.kvs_rows = d.kvs_rows1 * S;
    // fp8 attention: 16-bit staging of freshly projected K|V rows before they are quantised into the memory
    d.kv16_rows = (d.a8 && d.mode == MUST3R_MEM_KV && update) ? (size_t)d.L * R : 0;
}

static int decode_workspace(Decode& d) {
    const size_t R = d.R, D = d.D, L = d.L;
    const bool update = d.update, lnF = d.lnf || d.f256, a8 = d.a8;
    d.b = BlockRows{d.R, d.D, d.Hh, d.F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d.A->groups[0].pos};   // single group: the caller's array is already [R,2]
    d.fold.f256 = d.f256;
    Workspace ws;
    ws.want(d.t16, R * d.C);
    ws.want(d.b.x, R * D);
    ws.want(d.b.h16, R * D);
    ws.want(d.hcat, R * 3 * D);                              // [y_hi | y_lo | y_hi] operand of the head
    ws.want(d.b.qkv, R * 3 * D);
    ws.want(d.q16, R * D);
    ws.want(d.b.a16, R * D);
    ws.want(d.b.g16, R * d.F);
    ws.want(d.newmem, update ? L * R * D : 0);               // memorised layer inputs
    ws.want(d.off32, update ? R * D : 0);                    // feedback offset
    ws.want(d.yall, update ? L * R * D : 0);                 // norm_y of all layers (grouped K|V projection)
    ws.want(d.fold.x16, lnF ? R * D : 0);
    ws.want(d.fold.stats, lnF ? R * (D / 16) * 2 : 0);
    ws.want(d.fold.shift, lnF ? R : 0);
    ws.want(d.split_ws, d.split_bytes);
    ws.want(d.kvs, d.kvs_rows * 2 * D);
    ws.want(d.ytmp, d.mode == MUST3R_MEM_RAW ? d.kvs_rows * D : 0);
    // fp8 attention: e4m3 copies of q|k|v (self) / q (cross), the 16-bit staging rows, e4m3 K of the per-call projection ('norm_y' / 'raw')
    ws.want(d.b.q8, a8 ? R * 2 * D : 0);
    ws.want(d.kv16, d.kv16_rows * 2 * D);
    ws.want(d.kvs8, a8 ? d.kvs_rows * D : 0);
    M3R_OK(ws.commit(d.c, d.s));
    if (d.f256) HIP_OK(hipMemsetAsync(d.fold.shift, 0, R * sizeof(float), d.s));   // (the fold256 consumers add to it; its first producer reads zeros)
    return 0;
}

// per-view tables: self-attention, cross-attention; the K|V destination table of an update
static int decode_tables(Decode& d) {
    const must3r_hip_decode_args* A = d.A;
    const int S = d.S, Rs = d.Rs, Nm = d.Nm, D = d.D, L = d.L, total_views = d.total_views;
    d.tab.resize(2 * (size_t)total_views);
    double sa_flops = 0;
    d.ca_flops = 0;
    // K|V rows a scene's cross attention reads: its own memory buffer ('kv': rows b * mem_stride of the layer's buffer) or its slice
    // of the per-call projection scratch ('norm_y' / 'raw')
    const long long kv_stride = d.mode == MUST3R_MEM_KV ? d.mem_stride : (long long)d.kvs_rows1;
    int vi = 0;
    for (int b = 0; b < S; ++b)
        for (int gi = 0; gi < A->n_groups; ++gi) {
            const must3r_hip_group& G = A->groups[gi];
            for (int j = 0; j < G.n_views; ++j, ++vi) {
                const int rl = d.grow0[gi] + j * G.n_tokens, n = G.n_tokens;   // row inside the scene
                const int r0 = b * Rs + rl;
                d.tab[vi] = AttnView{r0, n, r0, n, 0, 0};
                AttnView cv{r0, n, (int)(b * kv_stride), Nm, 0, 0};
                if (d.update) {
                    if (d.lone_view) { cv.nk = Nm; }
                    else if (d.use_mask && A->causal) {
                        // CausalMUSt3R.make_attn_mask (decoder.py:389-433): old memory + the new tokens of the views before this one = a PREFIX of the key rows;
                        // empty memory: view 0 attends view 1's tokens (labels < 2, != 0: decoder.py:399-402) = rows [n, 2n) behind an excluded [0, n)
                        if (Nm == 0 && j == 0) { cv.nk = 2 * n; cv.skip_lo = 0; cv.skip_hi = n; }
                        else { cv.nk = Nm + rl; }
                    }
                    else if (d.use_mask) { cv.nk = Nm + Rs; cv.skip_lo = Nm + rl; cv.skip_hi = Nm + rl + n; }
                    else { cv.nk = Nm + Rs; }  // first view alone: attends its own (pre-feedback) tokens
                }
                d.tab[total_views + vi] = cv;
                sa_flops += 4.0 * n * (double)n * D;
                d.ca_flops += 4.0 * n * (double)(cv.nk - (cv.skip_hi - cv.skip_lo)) * D;
            }
        }
    void* tab_dev = nullptr;
    M3R_OK(upload_table(d.c, d.tab.data(), sizeof(AttnView) * d.tab.size(), &tab_dev, d.s));
    const AttnView* sa_views = reinterpret_cast<const AttnView*>(tab_dev);
    d.ca_views = sa_views + total_views;
    d.sv = SelfViews{sa_views, total_views, d.max_n, sa_flops, total_views == 1 ? &d.tab[0] : nullptr};   // (a single view travels inline)

    // per-(layer, scene) destinations of freshly projected K|V rows: memory rows [Nm, Nm + Rs) of scene b in layer l's buffer;
    // second half: the 16-bit staging rows the fp8 memory is quantised from
    void* kvout_dev = nullptr;
    if (d.update && d.mode == MUST3R_MEM_KV) {
        std::vector<void*> outs(2 * (size_t)L * S);
        for (int l = 0; l < L; ++l)
            for (int b = 0; b < S; ++b) {
                void* memrow = reinterpret_cast<char*>(A->mem[l]) + ((size_t)b * d.mem_stride + Nm) * d.memRB;
                outs[(size_t)l * S + b] = d.a8 ? static_cast<void*>(d.kv16 + ((size_t)l * S + b) * Rs * 2 * D) : memrow;
                outs[(size_t)L * S + (size_t)l * S + b] = memrow;
            }
        M3R_OK(upload_table(d.c, outs.data(), sizeof(void*) * outs.size(), &kvout_dev, d.s));
    }
    d.kvout = reinterpret_cast<void* const*>(kvout_dev);
    return 0;
}

// tokens -> 16 bit, enc->dec projection + image2_embed  (decoder.py:172-181 / :275-287); several groups: their positions gathered into one [R,2] array
static int decode_embed(Decode& d) {
    must3r_hip_ctx* c = d.c; const must3r_hip_decode_args* A = d.A; hipStream_t s = d.s;
    const int S = d.S, Rs = d.Rs, C = d.C, D = d.D;
    const char* err = "";
    for (int b = 0; b < (d.one_block ? 1 : S); ++b)
        for (int gi = 0; gi < A->n_groups; ++gi) {
            const must3r_hip_group& G = A->groups[gi];
            const size_t rg = (size_t)G.n_views * G.n_tokens;   // rows of this group per scene
            ProfScope ps(c, s, PC_MISC, 0.0);
            if (launch_cast(d.dt, G.tokens + (size_t)b * rg * C, d.t16 + ((size_t)b * Rs + d.grow0[gi]) * C, nullptr, (d.one_block ? S : 1) * rg * C, s, &err))
                return fail("%s", err);
        }
    const void* w;
    M3R_OK(w16(c, "decoder.feat_embed_enc_to_dec.weight", d.dt, &w, s));
    GemmArgs ga = gargs(d.t16, w, p32(c, "decoder.feat_embed_enc_to_dec.bias"), d.b.x, d.R, D, C, C, D);
    ga.bias2 = p32(c, "decoder.image2_embed");
    ga.row_start2 = A->first_call ? A->groups[0].n_tokens : 0;  // reference view (group 0, view 0) of every scene gets no embed
    ga.row_period2 = S > 1 ? Rs : 0;
    if (d.lnf_all) { ga.x16_out = d.fold.x16; ga.stats_out = d.fold.stats; ga.copy32_out = d.newmem; }   // block 0's norm1 input (+ its memorised copy)
    M3R_OK(gemm(c, d.dt, EPI_F32, ga, s));
    // several aspect ratios: gather the positions of all rows into one [R,2] array.  t16 is dead after the
    // projection above (stream order) and is large enough (R*C*2 >= R*16 bytes).
    if (!d.one_block) {
        int64_t* pos_ws = reinterpret_cast<int64_t*>(d.t16);
        for (int b = 0; b < S; ++b)
            for (int gi = 0; gi < A->n_groups; ++gi) {
                const must3r_hip_group& G = A->groups[gi];
                const size_t rg = (size_t)G.n_views * G.n_tokens;
                HIP_OK(hipMemcpyAsync(pos_ws + ((size_t)b * Rs + d.grow0[gi]) * 2, G.pos + (size_t)b * rg * 2, rg * 16, hipMemcpyDeviceToDevice, s));
            }
        d.b.pos = pos_ws;
    }
    return 0;
}

// prepare_y (layers.py:81-88) of the R new token rows, written to memory rows [Nm, Nm+R) in the caller's mode:
//   'kv'     LN(norm_y) -> [projk | projv]       'norm_y'  LN(norm_y)        'raw'  the tokens themselves
static int kv_project(Decode& d, int l, const float* src, const float* add, float* copy) {
    must3r_hip_ctx* c = d.c; const must3r_hip_decode_args* A = d.A; hipStream_t s = d.s;
    const int S = d.S, Rs = d.Rs, R = d.R, D = d.D, Nm = d.Nm;
    const std::vector<Param*>& LP = c->dec_tab[l];
    if (d.mode != MUST3R_MEM_KV) {   // the LayerNorm itself writes the scene's memory rows (one launch per scene)
        for (int b = 0; b < S; ++b) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(A->mem[l]) + ((size_t)b * d.mem_stride + Nm) * d.memD;
            const size_t o = (size_t)b * Rs * D;
            LnArgs la = lnargs(src + o, add ? add + o : nullptr, LP[LF_NYW]->d, LP[LF_NYB]->d, nullptr, nullptr, nullptr, copy ? copy + o : nullptr, Rs, D, 1e-6f);
            if (d.mode == MUST3R_MEM_NORM_Y) la.out16 = dst; else la.raw16 = dst;
            M3R_OK(layernorm_a(c, d.dt, la, s));
        }
        return 0;
    }
    M3R_OK(layernorm_a(c, d.dt, lnargs(src, add, LP[LF_NYW]->d, LP[LF_NYB]->d, d.b.h16, nullptr, nullptr, copy, R, D, 1e-6f), s));
    const void* wk;
    M3R_OK(w16p(c, *LP[LF_PKVW], d.dt, &wk, s));
    // one problem per scene (same weights): rows [b Rs, (b+1) Rs) -> memory rows of scene b (fp8 memory: 16-bit staging rows first)
    GemmArgs gk = gargs(d.b.h16, wk, LP[LF_PKVB]->d, nullptr, Rs, 2 * D, D, D, 2 * D);
    gk.batch = S; gk.strideA = (long long)Rs * D; gk.out_table = d.kvout + (size_t)l * S;
    if (S == 1) { gk.batch = 0; gk.out_table = nullptr; gk.out = d.a8 ? static_cast<void*>(d.kv16) : reinterpret_cast<char*>(A->mem[l]) + (size_t)Nm * d.memRB; }
    M3R_OK(gemm(c, d.dt, EPI_STORE16, gk, s));
    if (!d.a8) return 0;
    // K -> e4m3, V copied: memory rows [K e4m3 | V 16-bit]
    return quant8(c, d.dt, d.kv16 + (size_t)l * S * Rs * 2 * D * (S > 1 ? 1 : 0), 2 * D, S == 1 ? reinterpret_cast<char*>(A->mem[l]) + (size_t)Nm * d.memRB : nullptr,
                  3 * D, S > 1 ? d.kvout + (size_t)d.L * S + (size_t)l * S : nullptr, Rs, (size_t)R, D, D, s);
}
// K|V rows the cross attention of layer l reads: the memory itself ('kv') or a projection of it into scratch
static int kv_source(Decode& d, int l, const void** kptr) {
    must3r_hip_ctx* c = d.c; hipStream_t s = d.s;
    const int D = d.D, rows = (int)d.kvs_rows1;
    if (d.mode == MUST3R_MEM_KV) { *kptr = d.A->mem[l]; return 0; }
    const std::vector<Param*>& LP = c->dec_tab[l];
    const void* wk;
    M3R_OK(w16p(c, *LP[LF_PKVW], d.dt, &wk, s));
    for (int b = 0; b < d.S; ++b) {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(d.A->mem[l]) + (size_t)b * d.mem_stride * D;
        if (d.mode == MUST3R_MEM_RAW) {  // y_ = norm_y(y) on the stored tokens (layers.py:92)
            LnArgs la = lnargs(nullptr, nullptr, LP[LF_NYW]->d, LP[LF_NYB]->d, d.ytmp, nullptr, nullptr, nullptr, rows, D, 1e-6f);
            la.x16 = src;
            M3R_OK(layernorm_a(c, d.dt, la, s));
            src = d.ytmp;
        }
        M3R_OK(gemm(c, d.dt, EPI_STORE16, gargs(src, wk, LP[LF_PKVB]->d, d.kvs + (size_t)b * rows * 2 * D, rows, 2 * D, D, D, 2 * D), s));
    }
    *kptr = d.kvs;
    if (d.a8) M3R_OK(quant8(c, d.dt, d.kvs, 2 * D, d.kvs8, D, nullptr, 0, (size_t)d.kvs_rows, D, 0, s));   // K -> e4m3 (V is read from kvs)
    return 0;
}

// context-parallel cross attention of layer l: this rank's keys -> ONE partial in its slot (fp32 un-normalised, or 16-bit normalised with
// must3r_hip_cp::partial16); all-gather of the slots (the caller's collective); merge of the world's partials into a16
static int cross_attention_cp(Decode& d, int l, AttnArgs& aa) {
    must3r_hip_ctx* c = d.c; hipStream_t s = d.s; const must3r_hip_cp* cp = d.cp;
    const int R = d.R, p16 = cp->partial16 ? 1 : 0;
    const char* err = "";
    char* const slot0 = reinterpret_cast<char*>(cp->slots);
    const size_t o_bytes = (size_t)R * d.D * (p16 ? 2 : 4);
    float* const my_o = reinterpret_cast<float*>(slot0 + (size_t)cp->rank * cp->slot_bytes);
    float* const my_ml = reinterpret_cast<float*>(slot0 + (size_t)cp->rank * cp->slot_bytes + o_bytes);
    if (d.Nm > 0) {
        {
            ProfScope ps(c, s, PC_ATTN_CA, d.ca_flops);
            if (launch_attention_phase(d.dt, aa, 1, s, &err)) return fail("%s", err);
            ps.kernel(attention_last_kernel(), "/cross");
        }
        ProfScope ps(c, s, PC_ATTN_COMBINE, 0.0);
        aa.total_q_rows = R;
        if (launch_attention_partial_merge(d.dt, aa, my_o, my_ml, p16, s, &err)) return fail("%s", err);
    } else {
        ProfScope ps(c, s, PC_ATTN_COMBINE, 0.0);
        if (launch_attention_partial_empty(my_o, my_ml, R, d.Hh, p16, s, &err)) return fail("%s", err);
    }
    if (cp->exchange(cp->user, l, cp->slots, cp->slot_bytes, cp->world, cp->rank, d.stream))
        return fail("decode: the context-parallel exchange of layer %d failed", l);
    ProfScope ps(c, s, PC_ATTN_COMBINE, 0.0);
    aa.total_q_rows = R;
    if (launch_attention_partial_final(d.dt, aa, reinterpret_cast<const float*>(slot0), reinterpret_cast<const float*>(slot0 + o_bytes),
                                       (long long)(cp->slot_bytes / (p16 ? 2 : 4)), (long long)(cp->slot_bytes / 4), cp->world, p16, s, &err)) return fail("%s", err);
    return 0;
}

// x += proj(attention(projq(norm2(x)), K|V of the memory))  (layers.py:92-97; attention.py:139-149)
static int cross_attention_sublayer(Decode& d, int l) {
    must3r_hip_ctx* c = d.c; hipStream_t s = d.s; const DType dt = d.dt;
    const BlockRows& b = d.b;
    const std::vector<Param*>& LP = c->dec_tab[l];
    const int R = d.R, D = d.D;
    const bool folded = d.fold.on();
    const void* w;
    if (!folded) M3R_OK(layernorm_a(c, dt, lnargs(b.x, nullptr, LP[LF_N2W]->d, LP[LF_N2B]->d, b.h16, nullptr, nullptr, nullptr, R, D, 1e-6f), s));
    M3R_OK(w16p(c, *LP[folded ? LF_PQLN_W : LF_PQW], dt, &w, s));
    GemmArgs gq = gargs(b.h16, w, LP[LF_PQB]->d, d.q16, R, D, D, D, D);
    if (folded) d.fold.in(gq, LP[LF_PQLN_S], LP[LF_PQLN_C]);
    gq.out_scale = kQScale; gq.scale_cols = D;
    M3R_OK(gemm(c, dt, EPI_STORE16, gq, s));
    const void* mk = nullptr;
    M3R_OK(kv_source(d, l, &mk));
    AttnArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.Q = d.q16; aa.K = mk; aa.V = reinterpret_cast<const uint16_t*>(mk) + D; aa.O = b.a16;
    aa.ldq = D; aa.ldk = aa.ldv = 2 * D; aa.ldo = D; aa.heads = d.Hh;
    if (d.a8) {   // e4m3 q and K; 'kv' memory rows are [K e4m3 (D bytes) | V 16-bit]: ldk in bytes, ldv in 16-bit elements
        M3R_OK(quant8(c, dt, d.q16, D, b.q8, D, nullptr, 0, (size_t)R, D, 0, s));
        aa.Q = b.q8; aa.fp8 = 1;
        if (d.mode == MUST3R_MEM_KV) { aa.ldk = 3 * D; aa.ldv = 3 * D / 2; aa.V = reinterpret_cast<const char*>(mk) + D; }
        else { aa.K = d.kvs8; aa.ldk = D; }   // per-call projection: K from its e4m3 copy, V from the 16-bit scratch rows
    }
    aa.max_nk = d.max_nk_ca;
    aa.views = d.ca_views; aa.nviews = d.total_views; aa.max_nq = d.max_n; aa.scale = 0.125f; aa.q_prescaled = 1;
    if (d.total_views == 1) { aa.view0_inline = 1; aa.view0 = d.tab[d.total_views]; }
    if (d.ca_split > 1) {
        aa.nsplit = d.ca_split; aa.total_q_rows = R; aa.dense_rows = 1;
        aa.part_o = reinterpret_cast<float*>(d.split_ws);
        aa.part_ml = aa.part_o + (size_t)d.ca_split * R * D;
    }
    if (d.cp) M3R_OK(cross_attention_cp(d, l, aa));
    else M3R_OK(attention(c, dt, aa, d.ca_flops, PC_ATTN_CA, s));
    M3R_OK(w16p(c, *LP[LF_CPW], dt, &w, s));
    GemmArgs gp = gargs(b.a16, w, LP[LF_CPB]->d, b.x, R, D, D, D, D);
    if (folded) d.fold.out(gp, nullptr);
    return gemm(c, dt, EPI_RESID_F32, gp, s);
}

// prediction head in split precision (fp32-equivalent; decoder.py:149-156 runs it in fp32):
//     y = LN(x); out = y_hi W_hi + y_lo W_hi + y_hi W_lo + b, pixel-shuffled to [n,H,W,7]
// (Measured and rejected in r02: forking this head onto a second stream so that it overlaps the feedback / memory-write chain that ends
// an update call -- the two chains are independent -- costs 2.5 ms per scene instead of saving 0.5: the head's blocks take CUs from
// the latency-critical chain.  273 vs 282 views/s, interleaved runs on one box.)
static int decode_head(Decode& d) {
    must3r_hip_ctx* c = d.c; const must3r_hip_decode_args* A = d.A;
    const int S = d.S, R = d.R, D = d.D, OUT = c->cfg.patch_size * c->cfg.patch_size * 7;
    M3R_OK(head_layernorm(c, d.dt, d.b.x, p32(c, "decoder.norm_dec.weight"), p32(c, "decoder.norm_dec.bias"), d.hcat,
                          A->feats ? A->feats + (size_t)(d.L - 1) * R * D : nullptr, R, D, 1e-6f, d.s));
    const void* wcat;
    M3R_OK(w3(c, "decoder.head_dec.proj_ps.weight", d.dt, &wcat, d.s));
    for (int b = 0; b < (d.one_block ? 1 : S); ++b)
        for (int gi = 0; gi < A->n_groups; ++gi) {
            const must3r_hip_group& G = A->groups[gi];
            const int rg = G.n_views * G.n_tokens;                       // rows of this group per scene
            const int Rg = d.one_block ? S * rg : rg;                    // one group: all scenes in one launch ([S, n, H, W, 7] is contiguous)
            const size_t scene_elems = (size_t)G.n_views * G.H * G.W * 7;
            const size_t scene_stride = G.pointmaps_scene_stride > 0 ? (size_t)G.pointmaps_scene_stride : scene_elems;
            const bool skip = d.one_block && scene_stride != scene_elems;
            M3R_OK(head_linear(c, d.dt, d.hcat + ((size_t)b * d.Rs + d.grow0[gi]) * 3 * D, wcat, p32(c, "decoder.head_dec.proj_ps.bias"),
                               G.pointmaps + (size_t)b * scene_stride, Rg, D, OUT, G.n_tokens, G.W / 16, G.H, G.W, skip ? G.n_views : 0,
                               skip ? (long long)(scene_stride - scene_elems) : 0, d.s));
        }
    return 0;
}

// the end of an update call: feedback, then the stored memory
static int decode_feedback_memory(Decode& d) {
    must3r_hip_ctx* c = d.c; hipStream_t s = d.s; const DType dt = d.dt;
    const int S = d.S, Rs = d.Rs, R = d.R, D = d.D, L = d.L;
    uint16_t* const h16 = d.b.h16;
    const void* w;
    // --- feedback (feedback_mechanism.py:39-53): offset = layer(LN_1e-5(new_mem[L-1])), added to layers 0..L-2;
    //     layer = Mlp ('single_mlp'), Linear ('single_linear') or nothing (feedback_type None: no offset)
    const bool fb_mlp = is_loaded(c, "decoder.feedback_layer.fc1.weight");
    const bool fb_lin = !fb_mlp && is_loaded(c, "decoder.feedback_layer.weight");
    float* const off32 = (fb_mlp || fb_lin) ? d.off32 : nullptr;
    if (fb_mlp || fb_lin)
        M3R_OK(layernorm_a(c, dt, lnargs(d.newmem + (size_t)(L - 1) * R * D, nullptr, p32(c, "decoder.feedback_norm.weight"),
                         p32(c, "decoder.feedback_norm.bias"), h16, nullptr, nullptr, nullptr, R, D, 1e-5f), s));
    if (fb_mlp) {
        int ws_fb;
        M3R_OK(wmlp(c, c->params.at("decoder.feedback_layer.fc1.weight"), dt, &w, &ws_fb, s));
        M3R_OK(gemm(c, dt, EPI_STORE16_GELU, gargs(h16, w, p32(c, "decoder.feedback_layer.fc1.bias"), d.b.g16, R, 4 * D, D, D, 4 * D), s, ws_fb));
        M3R_OK(wmlp(c, c->params.at("decoder.feedback_layer.fc2.weight"), dt, &w, &ws_fb, s));
        M3R_OK(gemm(c, dt, EPI_F32, gargs(d.b.g16, w, p32(c, "decoder.feedback_layer.fc2.bias"), off32, R, D, 4 * D, 4 * D, D), s, ws_fb));
    } else if (fb_lin) {
        M3R_OK(w16(c, "decoder.feedback_layer.weight", dt, &w, s));
        M3R_OK(gemm(c, dt, EPI_F32, gargs(h16, w, p32(c, "decoder.feedback_layer.bias"), off32, R, D, D, D, D), s));
    }
    // --- stored memory = prepare_y(new_mem + offset) (decoder.py:236-239 / :327-330)
    if (d.mode != MUST3R_MEM_KV) {
        for (int l = 0; l < L; ++l)
            M3R_OK(kv_project(d, l, d.newmem + (size_t)l * R * D, l < L - 1 ? off32 : nullptr, nullptr));
        return 0;
    }
    // the L projections are independent: ONE grouped LayerNorm over [L*R, D] (per-layer affine, offset on layers
    // < L-1) and ONE grouped GEMM writing each layer's K|V rows into its own memory buffer
    LnArgs la = lnargs(d.newmem, off32, p32(c, "decoder.norm_y_all.weight"), p32(c, "decoder.norm_y_all.bias"), d.yall, nullptr,
                       nullptr, nullptr, L * R, D, 1e-6f);
    la.rows_per_group = R; la.add_groups = L - 1;
    M3R_OK(layernorm_a(c, dt, la, s));
    // fp8 memory: the GEMM writes the 16-bit staging rows [L][S][Rs][2D], one grouped quantisation scatters them into the
    // layers' memory rows.  Problem g = l * S + b: rows of scene b, weights of layer l = g / S.
    const void* wk;
    M3R_OK(w16(c, "decoder.projkv_all.weight", dt, &wk, s));
    GemmArgs gk = gargs(d.yall, wk, p32(c, "decoder.projkv_all.bias"), nullptr, Rs, 2 * D, D, D, 2 * D);
    gk.batch = L * S; gk.wdiv = S; gk.strideA = (long long)Rs * D; gk.strideW = (long long)2 * D * D * (c->wsplit == 2 ? 2 : 1);
    gk.strideB = 2 * D; gk.out_table = d.kvout;
    M3R_OK(gemm(c, dt, EPI_STORE16, gk, s));
    if (d.a8) M3R_OK(quant8(c, dt, d.kv16, 2 * D, nullptr, 3 * D, d.kvout + (size_t)L * S, Rs, (size_t)L * R, D, D, s));
    return 0;
}

static int decode_impl(must3r_hip_ctx* c, const must3r_hip_decode_args* A, void* stream) {
    DeviceGuard dev_guard(c->device);
    if (c->dec_tab.empty()) build_layer_tables(c, true);
    Decode d; d.c = c; d.A = A; d.stream = stream; d.s = reinterpret_cast<hipStream_t>(stream);
    decode_plan(d);
    M3R_OK(decode_workspace(d));
    M3R_OK(decode_tables(d));
    M3R_OK(decode_embed(d));
    const size_t RD = (size_t)d.R * d.D;
    for (int l = 0; l < d.L; ++l) {
        const std::vector<Param*>& LP = c->dec_tab[l];
        if (d.need_pre_kv) M3R_OK(kv_project(d, l, d.b.x, nullptr, nullptr));
        // LN fold: norm1 is folded in every block but block 0 (M3R_LNFOLD=2: there too); its kernel leaves the memorised input of the block and, under the
        // one-view fold, the row means; fc2 leaves the next block's rows (+ their memorised copy, decoder.py:304-305)
        const bool fq = d.lnf_all || (d.fold.on() && l > 0);
        M3R_OK(self_attention_sublayer(c, d.dt, LP, d.b, d.sv, d.fold, fq, d.update ? d.newmem + l * RD : nullptr, d.lnf ? d.fold.shift : nullptr, d.s));
        M3R_OK(cross_attention_sublayer(d, l));
        M3R_OK(mlp_sublayer(c, d.dt, LP, LF_N3W, d.b, d.fold, d.fold.on() && l + 1 < d.L, d.update ? d.newmem + (l + 1) * RD : nullptr, d.s));
        if (A->feats && l < d.L - 1)   // return_feats: the residual stream after block l (decoder.py:321)
            HIP_OK(hipMemcpyAsync(A->feats + l * RD, d.b.x, RD * sizeof(float), hipMemcpyDeviceToDevice, d.s));
    }
    M3R_OK(decode_head(d));
    return d.update ? decode_feedback_memory(d) : 0;
}

// MUSt3R.forward / forward_list (decoder.py:158-350).  Validates everything the launches rely on (so that a non-Python caller
// cannot overrun a memory buffer or a table) and cuts render calls whose view tables would not fit the staging slot: rendered
// views (and scenes) are independent of each other, the pieces give the same pointmaps.
extern "C" int must3r_hip_has_fp8_attention(void) { return kAttnFp8Built ? 1 : 0; }

static size_t cp_slot_bytes(const must3r_hip_ctx* c, int rows, int partial16) {
    return align_up((size_t)rows * ((size_t)c->cfg.dec_dim * (partial16 ? 2 : 4) + 2 * (size_t)c->cfg.dec_heads * sizeof(float)), 256);
}
extern "C" size_t must3r_hip_cp_slot_bytes(const must3r_hip_ctx* c, int rows) {
    if (!c || rows <= 0) return 0;
    return cp_slot_bytes(c, rows, 0);
}
extern "C" size_t must3r_hip_cp_slot_bytes16(const must3r_hip_ctx* c, int rows) {
    if (!c || rows <= 0) return 0;
    return cp_slot_bytes(c, rows, 1);
}

extern "C" int must3r_hip_decode(must3r_hip_ctx* c, const must3r_hip_decode_args* A, void* stream) {
    if (!c || !A || !A->groups || !A->mem) return fail("decode: null argument");
    if (!c->fin_dec) return fail("decode: decoder weights not finalized");
    if (!set_mode(c, A->dtype)) return fail("decode: bad dtype %d", A->dtype);
    if ((A->dtype & MUST3R_ATTN_FP8) && !kAttnFp8Built) return fail("decode: MUST3R_ATTN_FP8 is an experiment build (make EXTRA=-DM3R_ATTN_FP8): measured outside the 1e-3 target for +0.4 %%");
    if (A->mem_mode != MUST3R_MEM_KV && A->mem_mode != MUST3R_MEM_NORM_Y && A->mem_mode != MUST3R_MEM_RAW)
        return fail("decode: bad mem_mode %d", A->mem_mode);
    if (A->n_groups <= 0) return fail("decode: no input group");
    if (A->n_mem < 0) return fail("decode: negative n_mem");
    if (A->render && (A->first_call || A->n_mem <= 0)) return fail("decode: render needs a memory (decoder.py:278)");
    if (A->first_call && A->n_mem != 0) return fail("decode: first_call with a non-empty memory");
    if (A->n_scenes < 0) return fail("decode: negative n_scenes");
    const int S = A->n_scenes > 1 ? A->n_scenes : 1;
    if (A->causal != 0 && A->causal != 1) return fail("decode: causal must be 0 or 1");
    if (A->causal && (A->n_groups != 1 || A->cp)) return fail("decode: the causal forward takes ONE group of views (CausalMUSt3R has no list dispatch) and no context parallelism");
    if (A->cp) {   // context-parallel cross attention: the one-view update of the streaming schedule, nothing else
        const must3r_hip_cp& P = *A->cp;
        if (P.world < 1 || P.rank < 0 || P.rank >= P.world) return fail("decode: context parallel: bad rank %d of %d", P.rank, P.world);
        if (A->render || A->first_call || S != 1 || A->n_groups != 1 || A->groups[0].n_views != 1)
            return fail("decode: context parallel is for memory-update calls of ONE view on ONE scene against an existing memory");
        if (A->mem_mode != MUST3R_MEM_KV || (A->dtype & MUST3R_ATTN_FP8)) return fail("decode: context parallel needs memory_mode 'kv' and 16-bit attention operands");
        if (P.n_mem_total <= 0 || A->n_mem > P.n_mem_total) return fail("decode: context parallel: n_mem_total %d with %d local rows", P.n_mem_total, A->n_mem);
        if (P.partial16 != 0 && P.partial16 != 1) return fail("decode: context parallel: partial16 must be 0 or 1");
        if (!P.exchange || !P.slots || (reinterpret_cast<uintptr_t>(P.slots) & 15) || (P.slot_bytes & 15) ||
            P.slot_bytes < cp_slot_bytes(c, A->groups[0].n_tokens, P.partial16))
            return fail("decode: context parallel: slots must be 16-byte aligned, world x slot_bytes with slot_bytes >= %zu, and an exchange function given",
                        cp_slot_bytes(c, A->groups[0].n_tokens, P.partial16));
    }
    long long Rs = 0, views_s = 0;
    for (int gi = 0; gi < A->n_groups; ++gi) {
        const must3r_hip_group& G = A->groups[gi];
        if (!G.tokens || !G.pos || !G.pointmaps) return fail("decode: null buffer in group %d", gi);
        if (G.n_views <= 0 || G.n_tokens <= 0) return fail("decode: empty group %d", gi);
        if (G.pointmaps_scene_stride != 0 && G.pointmaps_scene_stride < (long long)G.n_views * G.H * G.W * 7)
            return fail("decode: group %d: pointmaps_scene_stride %lld is smaller than one scene's pointmaps", gi, (long long)G.pointmaps_scene_stride);
        if (G.pointmaps_scene_stride % 4 != 0 || (reinterpret_cast<uintptr_t>(G.pointmaps) & 15) != 0)   // the head epilogue stores (and accumulates) f32x4 vectors
            return fail("decode: group %d: pointmaps must be 16-byte aligned and pointmaps_scene_stride (%lld) a multiple of 4 floats", gi, (long long)G.pointmaps_scene_stride);
        if (G.H % 16 || G.W % 16 || (G.H / 16) * (G.W / 16) != G.n_tokens)
            return fail("decode: group %d: %dx%d does not give %d tokens", gi, G.H, G.W, G.n_tokens);
        if (G.H / 16 > c->rope_npos || G.W / 16 > c->rope_npos) return fail("decode: group %d: image too large for the RoPE table", gi);
        Rs += (long long)G.n_views * G.n_tokens;
        views_s += G.n_views;
    }
    for (int l = 0; l < c->cfg.dec_depth; ++l)
        if (!A->mem[l]) return fail("decode: null memory buffer for layer %d", l);
    // capacity: rows [0, n_mem) are read, an update writes rows [n_mem, n_mem + Rs) of every scene's buffer
    const long long rows_needed = (long long)A->n_mem + (A->render ? 0 : Rs);
    if (A->mem_capacity <= 0) return fail("decode: mem_capacity must be given (rows each scene's memory buffer can hold)");
    if (rows_needed > A->mem_capacity)
        return fail("decode: memory buffers hold %d rows, this call needs %lld (n_mem %d + %lld new)", A->mem_capacity, rows_needed, A->n_mem,
                    A->render ? 0LL : Rs);
    if (S > 1 && A->mem_scene_stride < A->mem_capacity)
        return fail("decode: mem_scene_stride %lld < mem_capacity %d", (long long)A->mem_scene_stride, A->mem_capacity);
    if ((S - 1) * (S > 1 ? (long long)A->mem_scene_stride : 0) + rows_needed > 0x7fffffffLL || (long long)S * Rs > (1LL << 24))
        return fail("decode: call too large (row indices are 32-bit)");
    // cross-attention staging addresses K|V rows of one scene with 32-bit byte offsets (attention.hip, attn3_kernel)
    {
        const long long memD = A->mem_mode == MUST3R_MEM_KV ? 2LL * c->cfg.dec_dim : 1LL * c->cfg.dec_dim;
        if (rows_needed * 2LL * c->cfg.dec_dim * 2 >= 0x7fffffffLL || rows_needed * memD * 2 >= 0x7fffffffLL)
            return fail("decode: a scene memory of %lld rows exceeds the 2 GiB the attention staging can address per layer", rows_needed);
    }
    // the per-call view tables travel through one staging slot: 2 tables x 24 B per view
    const long long max_views = (long long)(must3r_hip_ctx::kSlotBytes / (2 * sizeof(AttnView)));
    // ... and so does an update's table of K|V destinations: 2 x dec_depth x S pointers ('kv' memory)
    if (!A->render && A->mem_mode == MUST3R_MEM_KV && (size_t)2 * c->cfg.dec_depth * S * sizeof(void*) > must3r_hip_ctx::kSlotBytes)
        return fail("decode: %d scenes in one memory update (limit %zu at decoder depth %d)", S,
                    must3r_hip_ctx::kSlotBytes / (2 * sizeof(void*) * c->cfg.dec_depth), c->cfg.dec_depth);
    if (S * views_s <= max_views) return decode_impl(c, A, stream);
    if (!A->render) return fail("decode: %lld views in one memory update (limit %lld)", S * views_s, max_views);
    if (A->feats) return fail("decode: return_feats with %lld rendered views in one call (limit %lld)", S * views_s, max_views);
    must3r_hip_decode_args sub = *A;
    if (S > 1) {   // cut the batch into ranges of scenes
        const int per = views_s <= max_views ? (int)(max_views / views_s) : 1;
        std::vector<must3r_hip_group> gs(A->n_groups);
        std::vector<void*> mems(c->cfg.dec_depth);
        const long long memRB = ((A->dtype & MUST3R_ATTN_FP8) && A->mem_mode == MUST3R_MEM_KV) ? 3LL * c->cfg.dec_dim
                                : (A->mem_mode == MUST3R_MEM_KV ? 4LL : 2LL) * c->cfg.dec_dim;
        for (int b0 = 0; b0 < S; b0 += per) {
            const int nb = S - b0 < per ? S - b0 : per;
            for (int gi = 0; gi < A->n_groups; ++gi) {
                gs[gi] = A->groups[gi];
                const size_t rg = (size_t)gs[gi].n_views * gs[gi].n_tokens;
                gs[gi].tokens += (size_t)b0 * rg * c->cfg.enc_dim;
                gs[gi].pos += (size_t)b0 * rg * 2;
                gs[gi].pointmaps += (size_t)b0 * (gs[gi].pointmaps_scene_stride > 0 ? (size_t)gs[gi].pointmaps_scene_stride
                                                                                       : (size_t)gs[gi].n_views * gs[gi].H * gs[gi].W * 7);
            }
            for (int l = 0; l < c->cfg.dec_depth; ++l)
                mems[l] = reinterpret_cast<char*>(A->mem[l]) + (size_t)b0 * A->mem_scene_stride * memRB;
            sub.groups = gs.data(); sub.mem = mems.data(); sub.n_scenes = nb;
            M3R_OK(must3r_hip_decode(c, &sub, stream));
        }
        return 0;
    }
    // one scene: cut every group into ranges of views
    for (int gi = 0; gi < A->n_groups; ++gi) {
        const must3r_hip_group& G = A->groups[gi];
        for (long long v0 = 0; v0 < G.n_views; v0 += max_views) {
            must3r_hip_group g1 = G;
            g1.n_views = (int)(G.n_views - v0 < max_views ? G.n_views - v0 : max_views);
            g1.tokens += (size_t)v0 * G.n_tokens * c->cfg.enc_dim;
            g1.pos += (size_t)v0 * G.n_tokens * 2;
            g1.pointmaps += (size_t)v0 * G.H * G.W * 7;
            sub.groups = &g1; sub.n_groups = 1;
            M3R_OK(decode_impl(c, &sub, stream));
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// operator-level entry points + profiling
// ------------------------------------------------------------------------------------------------
extern "C" int must3r_hip_op_gemm(int dtype, int epi, const void* A, const void* W, const float* bias, void* out, int M, int N,
                                  int K, int lda, int ldc, const int64_t* pos, const float* rope_tab, int rope_cols,
                                  int rope_npos, const float* bias2, int row_start2, int accumulate, int ntok, int gw, int H,
                                  int W_img, int wsplit, void* stream) {
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("op_gemm: bad dtype");
    if (epi < 0 || epi >= EPI_COUNT) return fail("op_gemm: bad epilogue");
    GemmArgs a = gargs(A, W, bias, out, M, N, K, lda, ldc);
    a.pos = pos; a.rope_tab = rope_tab; a.rope_cols = rope_cols; a.rope_npos = rope_npos;
    a.bias2 = bias2; a.row_start2 = row_start2; a.accumulate = accumulate;
    a.ntok = ntok; a.gw = gw; a.H = H; a.Wimg = W_img; a.wsplit = wsplit;
    const char* err = "";
    if (launch_gemm((DType)dtype, (Epi)epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

/* r05, ABI 7: the chip-filling split-weight GEMM with a 2:4-sparse low part (tests / probes): pack, then multiply */
extern "C" int must3r_hip_op_sparse24_pack(const float* w, int rows, int K, void* vals, void* idx, void* stream) {
    const char* err = "";
    if (launch_sparse24_pack(w, rows, K, vals, idx, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}
// r06: the LN fold on the chip-filling 256 x 256 tiles alone (tests): GemmArgs::fold256 with split weights + packed sparse low part (wsplit = 2) or plain fp16 weights
extern "C" int must3r_hip_op_gemm_fold256(int epi, int wsplit, const void* A, const void* W, const void* Wlo_sp, const void* Widx_sp, const float* bias, void* out,
                                          int M, int N, int K, int lda, int ldc, void* x16_out, float* copy32_out, float* stats_out, const float* ln_stats,
                                          const float* ln_s, float ln_eps, float* ln_shift, const int64_t* pos, const float* rope_tab, int rope_cols, int rope_npos,
                                          float out_scale, int scale_cols, void* stream) {
    if (epi < 0 || epi >= EPI_COUNT) return fail("op_gemm_fold256: bad epilogue");
    GemmArgs a = gargs(A, W, bias, out, M, N, K, lda, ldc);
    a.wsplit = wsplit == 2 ? 2 : 0; a.Wlo_sp = Wlo_sp; a.Widx_sp = Widx_sp; a.wsp_rows = N;
    a.x16_out = x16_out; a.copy32_out = copy32_out; a.stats_out = stats_out;
    a.ln_stats = ln_stats; a.ln_s = ln_s; a.ln_eps = ln_eps; a.ln_shift = ln_shift; a.fold256 = 1;
    a.pos = pos; a.rope_tab = rope_tab; a.rope_cols = rope_cols; a.rope_npos = rope_npos;
    a.out_scale = out_scale; a.scale_cols = scale_cols;
    const char* err = "";
    if (launch_gemm(DT_F16, (Epi)epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}
extern "C" int must3r_hip_op_gemm_sp(int epi, const void* A, const void* W2, const void* Wlo_sp, const void* Widx_sp, const float* bias, void* out, int M,
                                     int N, int K, int lda, int ldc, const int64_t* pos, const float* rope_tab, int rope_cols, int rope_npos, void* stream) {
    if (epi < 0 || epi >= EPI_COUNT) return fail("op_gemm_sp: bad epilogue");
    GemmArgs a = gargs(A, W2, bias, out, M, N, K, lda, ldc);
    a.wsplit = 2; a.Wlo_sp = Wlo_sp; a.Widx_sp = Widx_sp; a.wsp_rows = N;
    a.pos = pos; a.rope_tab = rope_tab; a.rope_cols = rope_cols; a.rope_npos = rope_npos;
    const char* err = "";
    if (launch_gemm(DT_F16, (Epi)epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

extern "C" int must3r_hip_op_gemm_lnfold(int dtype, int epi, const void* A, const void* W2, const float* bias, void* out, int M, int N, int K,
                                         int lda, int ldc, void* x16_out, float* copy32_out, float* stats_out, const float* ln_stats,
                                         const float* ln_s, float ln_eps, float* ln_shift, int ln_shift_init, const int64_t* pos,
                                         const float* rope_tab, int rope_cols, int rope_npos, float out_scale, int scale_cols, void* stream) {
    if (dtype != MUST3R_F16) return fail("op_gemm_lnfold: fp16 operands with split weights only");
    if (epi < 0 || epi >= EPI_COUNT) return fail("op_gemm_lnfold: bad epilogue");
    GemmArgs a = gargs(A, W2, bias, out, M, N, K, lda, ldc);
    a.wsplit = 2;
    a.x16_out = x16_out; a.copy32_out = copy32_out; a.stats_out = stats_out;
    a.ln_stats = ln_stats; a.ln_s = ln_s; a.ln_eps = ln_eps; a.ln_shift = ln_shift; a.ln_shift_init = ln_shift_init;
    a.pos = pos; a.rope_tab = rope_tab; a.rope_cols = rope_cols; a.rope_npos = rope_npos;
    a.out_scale = out_scale; a.scale_cols = scale_cols;
    const char* err = "";
    if (launch_gemm(DT_F16, (Epi)epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

// ABI 18 (tests): every launch form of the one-view LN fold -- plain or split weights, bias2 -- one launch through launch_gemm; what the kernels would misread is refused
extern "C" int must3r_hip_op_gemm_lnfold_ex(const must3r_hip_lnfold_op* d, void* stream) {
    if (!d) return fail("op_gemm_lnfold_ex: null descriptor");
    if (d->dtype != MUST3R_F16) return fail("op_gemm_lnfold_ex: the fold is built for fp16 operands (dtype)");
    if (d->epi < 0 || d->epi >= EPI_COUNT) return fail("op_gemm_lnfold_ex: bad epilogue");
    if (d->wsplit != 0 && d->wsplit != 2) return fail("op_gemm_lnfold_ex: wsplit = %d (0: plain weights, 2: split weights)", d->wsplit);
    if (!d->A || !d->W || !d->out) return fail("op_gemm_lnfold_ex: A, W and out are needed");
    if (d->M < 0 || d->N <= 0 || d->K <= 0) return fail("op_gemm_lnfold_ex: M >= 0, N > 0 and K > 0 are needed");
    const bool cons = d->ln_stats != nullptr, prod = d->x16_out || d->copy32_out || d->stats_out;
    if (cons && prod) return fail("op_gemm_lnfold_ex: ln_stats (consumer) and x16_out / copy32_out / stats_out (producer) exclude each other");
    if (cons) {
        if (d->epi != EPI_STORE16 && d->epi != EPI_STORE16_GELU && d->epi != EPI_QKV_ROPE) return fail("op_gemm_lnfold_ex: a consumer has a 16-bit-store epilogue");
        if (!d->ln_s || !d->bias || !d->ln_shift) return fail("op_gemm_lnfold_ex: a consumer needs ln_s, bias and ln_shift");
        if (d->K != 768) return fail("op_gemm_lnfold_ex: a consumer reads 48 fragment sums per row (K = 768), not K = %d", d->K);
    }
    if (prod) {
        if (d->epi != EPI_RESID_F32 && d->epi != EPI_F32) return fail("op_gemm_lnfold_ex: producer outputs belong to the RESID_F32 / F32 epilogues");
        if (d->stats_out && !d->x16_out) return fail("op_gemm_lnfold_ex: stats_out comes with x16_out");
        if (d->stats_out && d->N != 768) return fail("op_gemm_lnfold_ex: stats_out needs N = 768, not N = %d", d->N);
        if (d->ldc != d->N) return fail("op_gemm_lnfold_ex: producer outputs are addressed with out's stride: ldc = %d must equal N = %d", d->ldc, d->N);
    }
    if (d->bias2 && d->epi != EPI_F32) return fail("op_gemm_lnfold_ex: bias2 belongs to EPI_F32");
    if (d->row_start2 < 0) return fail("op_gemm_lnfold_ex: row_start2 must not be negative");
    if (d->out_scale != 0.f && d->epi != EPI_STORE16 && d->epi != EPI_QKV_ROPE) return fail("op_gemm_lnfold_ex: out_scale belongs to the STORE16 / QKV_ROPE epilogues");
    if (d->out_scale != 0.f && (d->scale_cols < 0 || d->scale_cols % 64 != 0)) return fail("op_gemm_lnfold_ex: scale_cols = %d must be a multiple of 64", d->scale_cols);
    GemmArgs a = gargs(d->A, d->W, d->bias, d->out, d->M, d->N, d->K, d->lda, d->ldc);
    a.wsplit = d->wsplit;
    a.x16_out = d->x16_out; a.copy32_out = d->copy32_out; a.stats_out = d->stats_out;
    a.ln_stats = d->ln_stats; a.ln_s = d->ln_s; a.ln_eps = d->ln_eps; a.ln_shift = d->ln_shift; a.ln_shift_init = d->ln_shift_init;
    a.pos = d->pos; a.rope_tab = d->rope_tab; a.rope_cols = d->rope_cols; a.rope_npos = d->rope_npos;
    a.out_scale = d->out_scale; a.scale_cols = d->scale_cols;
    a.bias2 = d->bias2; a.row_start2 = d->row_start2;
    const char* err = "";
    if (launch_gemm(DT_F16, (Epi)d->epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    if (d->picked && d->M > 0) *d->picked = gemm_last_kernel();
    return 0;
}

// ABI 17 (tests): the grouped and per-scene fields of GemmArgs, one launch through launch_gemm under the default dispatch; what the kernels would misread is refused
extern "C" int must3r_hip_op_gemm_ex(const must3r_hip_gemm_op* d, void* stream) {
    if (!d) return fail("op_gemm_ex: null descriptor");
    if (d->dtype != MUST3R_BF16 && d->dtype != MUST3R_F16) return fail("op_gemm_ex: bad dtype");
    if (d->epi < 0 || d->epi >= EPI_COUNT) return fail("op_gemm_ex: bad epilogue");
    if (!d->A || !d->W) return fail("op_gemm_ex: A and W are needed");
    if (d->M < 0 || d->N <= 0 || d->K <= 0) return fail("op_gemm_ex: M >= 0, N > 0 and K > 0 are needed");
    if (d->batch < 0 || d->wdiv < 0 || d->strideA < 0 || d->strideW < 0 || d->strideB < 0) return fail("op_gemm_ex: batch, wdiv and the strides must not be negative");
    if (d->batch > 1 && !d->out_table) return fail("op_gemm_ex: batch = %d needs out_table", d->batch);
    if (d->batch <= 1 && !d->out) return fail("op_gemm_ex: out is needed");
    if (d->wdiv > 1 && (d->batch <= 1 || d->batch % d->wdiv != 0)) return fail("op_gemm_ex: wdiv = %d must divide batch = %d", d->wdiv, d->batch);
    if (d->out_scale != 0.f && d->epi != EPI_STORE16 && d->epi != EPI_QKV_ROPE) return fail("op_gemm_ex: out_scale belongs to the STORE16 / QKV_ROPE epilogues");
    if (d->out_scale != 0.f && (d->scale_cols < 0 || d->scale_cols % 64 != 0)) return fail("op_gemm_ex: scale_cols = %d must be a multiple of 64", d->scale_cols);
    if (d->row_start2 < 0 || d->row_period2 < 0) return fail("op_gemm_ex: row_start2 and row_period2 must not be negative");
    if (d->row_period2 > 0 && !d->bias2) return fail("op_gemm_ex: row_period2 = %d needs bias2", d->row_period2);
    if ((d->head_views != 0 || d->head_scene_skip != 0) && d->epi != EPI_HEAD) return fail("op_gemm_ex: head_views / head_scene_skip belong to EPI_HEAD");
    if (d->head_views < 0 || d->head_scene_skip < 0) return fail("op_gemm_ex: head_views and head_scene_skip must not be negative");
    if (d->head_scene_skip % 4 != 0) return fail("op_gemm_ex: head_scene_skip = %lld must be a multiple of 4 floats", (long long)d->head_scene_skip);
    if ((d->Wlo_sp != nullptr) != (d->Widx_sp != nullptr)) return fail("op_gemm_ex: Wlo_sp and Widx_sp come together");
    if (d->Wlo_sp) {
        if (d->wsplit != 2 || d->dtype != MUST3R_F16) return fail("op_gemm_ex: the sparse low part belongs to fp16 split weights (wsplit = 2)");
        const long long ngroups = d->batch > 1 ? (d->wdiv > 1 ? d->batch / d->wdiv : d->batch) : 1;
        const long long need = (ngroups - 1) * (d->strideW / (2 * (long long)d->K)) + d->N;
        if (d->wsp_rows < need || d->wsp_rows % 32 != 0)
            return fail("op_gemm_ex: wsp_rows = %d, but the %lld weight groups index %lld rows of the packed low part (a multiple of 32)", d->wsp_rows, ngroups, need);
    }
    GemmArgs a = gargs(d->A, d->W, d->bias, d->out, d->M, d->N, d->K, d->lda, d->ldc);
    a.wsplit = d->wsplit == 2 ? 2 : 0; a.Wlo_sp = d->Wlo_sp; a.Widx_sp = d->Widx_sp; a.wsp_rows = d->wsp_rows;
    a.out_scale = d->out_scale; a.scale_cols = d->scale_cols;
    a.batch = d->batch; a.strideA = d->strideA; a.strideW = d->strideW; a.strideB = d->strideB; a.out_table = d->out_table; a.wdiv = d->wdiv;
    a.pos = d->pos; a.rope_tab = d->rope_tab; a.rope_cols = d->rope_cols; a.rope_npos = d->rope_npos;
    a.bias2 = d->bias2; a.row_start2 = d->row_start2; a.row_period2 = d->row_period2; a.accumulate = d->accumulate;
    a.ntok = d->ntok; a.gw = d->gw; a.H = d->H; a.Wimg = d->Wimg; a.head_views = d->head_views; a.head_scene_skip = d->head_scene_skip;
    const char* err = "";
    if (launch_gemm((DType)d->dtype, (Epi)d->epi, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    if (d->picked && d->M > 0) *d->picked = gemm_last_kernel();
    return 0;
}

extern "C" size_t must3r_hip_attention_scratch_bytes(int nsplit, int total_q_rows, int heads) {
    return attention_split_scratch_bytes(nsplit, total_q_rows, heads);
}

extern "C" int must3r_hip_op_attention(int dtype, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv,
                                       int ldo, int heads, const int32_t* views_dev, int n_views, int max_nq, int nsplit,
                                       void* scratch, int total_q_rows, void* stream) {
    const int fp8 = (dtype & MUST3R_ATTN_FP8) ? 1 : 0;   // Q, K, V are e4m3 bytes (strides in bytes); O in the 16-bit type
    if (fp8 && !kAttnFp8Built) return fail("op_attention: MUST3R_ATTN_FP8 is an experiment build (make EXTRA=-DM3R_ATTN_FP8)");
    dtype &= ~MUST3R_ATTN_FP8;
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("op_attention: bad dtype");
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.fp8 = fp8;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.heads = heads;
    a.views = reinterpret_cast<const AttnView*>(views_dev); a.nviews = n_views; a.max_nq = max_nq; a.scale = 0.125f;
    if (nsplit > 1) {
        if (!scratch || total_q_rows <= 0) return fail("op_attention: split-KV needs scratch and total_q_rows");
        a.nsplit = nsplit; a.total_q_rows = total_q_rows;
        a.part_o = reinterpret_cast<float*>(scratch);
        a.part_ml = a.part_o + (size_t)nsplit * total_q_rows * heads * 64;
    }
    const char* err = "";
    if (launch_attention((DType)dtype, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

// ABI 10 (tests): the launches of decode() one by one -- stage 0 = static attention(), stages 1 / 2 / 3 = the context-parallel local partial / empty partial / final merge
extern "C" int must3r_hip_op_attention_ex(const must3r_hip_attn_op* d, void* stream) {
    if (!d) return fail("op_attention_ex: null descriptor");
    if (d->dtype != MUST3R_BF16 && d->dtype != MUST3R_F16) return fail("op_attention_ex: bad dtype");
    if (d->stage < 0 || d->stage > 3) return fail("op_attention_ex: stage must be 0 .. 3");
    if (d->view0_inline && d->n_views != 1) return fail("op_attention_ex: view0_inline needs n_views = 1");
    const DType dt = (DType)d->dtype;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = d->Q; a.K = d->K; a.V = d->V; a.O = d->O;
    a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo; a.heads = d->heads;
    a.views = reinterpret_cast<const AttnView*>(d->views_dev); a.nviews = d->n_views;
    if (d->view0_inline) {
        a.view0_inline = 1;
        a.view0 = AttnView{d->view0[0], d->view0[1], d->view0[2], d->view0[3], d->view0[4], d->view0[5]};
    }
    a.max_nq = d->max_nq; a.max_nk = d->max_nk; a.scale = 0.125f; a.q_prescaled = d->q_prescaled ? 1 : 0;
    a.total_q_rows = d->total_q_rows; a.dense_rows = d->dense_rows ? 1 : 0;
    if (d->nsplit > 1) {
        if (!d->scratch || d->total_q_rows <= 0) return fail("op_attention_ex: split-KV needs scratch and total_q_rows");
        a.nsplit = d->nsplit;
        a.part_o = reinterpret_cast<float*>(d->scratch);
        a.part_ml = a.part_o + (size_t)d->nsplit * d->total_q_rows * d->heads * 64;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* err = "";
    switch (d->stage) {
    case 0:
        if (launch_attention(dt, a, s, &err)) return fail("%s", err);
        break;
    case 1:
        if (d->nsplit < 2) return fail("op_attention_ex: a local partial needs nsplit >= 2");
        if (launch_attention_phase(dt, a, 0, s, &err) || launch_attention_phase(dt, a, 1, s, &err) ||
            launch_attention_partial_merge(dt, a, reinterpret_cast<float*>(d->slot_o), d->slot_ml, d->p16, s, &err)) return fail("%s", err);
        break;
    case 2:
        if (launch_attention_partial_empty(reinterpret_cast<float*>(d->slot_o), d->slot_ml, d->total_q_rows, d->heads, d->p16, s, &err)) return fail("%s", err);
        break;
    default:
        if (launch_attention_partial_final(dt, a, reinterpret_cast<const float*>(d->slot_o), d->slot_ml, d->stride_o, d->stride_ml, d->nslots, d->p16, s, &err))
            return fail("%s", err);
    }
    if (d->picked && d->stage < 2) *d->picked = attention_last_kernel();
    return 0;
}

extern "C" int must3r_hip_op_layernorm(int dtype, const float* x, const float* add, const float* w, const float* b, void* out16,
                                       void* out16_lo, float* out32, float* copy32, int M, int C, float eps, void* stream) {
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("op_layernorm: bad dtype");
    LnArgs a = lnargs(x, add, w, b, out16, out16_lo, out32, copy32, M, C, eps);
    const char* err = "";
    if (launch_layernorm((DType)dtype, a, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

extern "C" int must3r_hip_op_im2col(int dtype, const float* img, void* out16, int n_views, int H, int W, void* stream) {
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("op_im2col: bad dtype");
    const char* err = "";
    if (launch_im2col((DType)dtype, img, out16, n_views, H, W, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

extern "C" int must3r_hip_op_cast(int dtype, const float* in, void* out16, void* out16_lo, size_t n, void* stream) {
    if (dtype != MUST3R_BF16 && dtype != MUST3R_F16) return fail("op_cast: bad dtype");
    const char* err = "";
    if (launch_cast((DType)dtype, in, out16, out16_lo, n, reinterpret_cast<hipStream_t>(stream), &err)) return fail("%s", err);
    return 0;
}

extern "C" int must3r_hip_debug_tr_probe(void* out256_i16_dev, void* stream) {
    if (!out256_i16_dev) return fail("tr_probe: null argument");
    if (launch_tr_probe(reinterpret_cast<short*>(out256_i16_dev), reinterpret_cast<hipStream_t>(stream))) return fail("tr_probe: launch failed");
    return 0;
}

extern "C" int must3r_hip_set_profiling(must3r_hip_ctx* c, int enabled) {
    if (!c) return fail("set_profiling: null context");
    prof_flush(c);
    c->prof = enabled != 0;
    return 0;
}

extern "C" int must3r_hip_get_profile(must3r_hip_ctx* c, must3r_hip_prof_record* out, int max, int reset) {
    if (!c || !out) return 0;
    prof_flush(c);
    int n = 0;
    for (int i = 0; i < PC_COUNT && n < max; ++i) {
        memset(&out[n], 0, sizeof(out[n]));
        strncpy(out[n].name, kProfNames[i], sizeof(out[n].name) - 1);
        out[n].ms = c->prof_ms[i];
        out[n].flops = c->prof_flops[i];
        out[n].calls = c->prof_calls[i];
        ++n;
    }
    // per-kernel rows behind the class rows, names prefixed "k:" (one rocprofv3 symbol each)
    for (auto& kv : c->prof_kern) {
        if (n >= max) break;
        memset(&out[n], 0, sizeof(out[n]));
        snprintf(out[n].name, sizeof(out[n].name), "k:%s", kv.first.c_str());
        out[n].ms = kv.second.ms;
        out[n].flops = kv.second.flops;
        out[n].calls = kv.second.calls;
        ++n;
    }
    if (reset) {
        for (int i = 0; i < PC_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_flops[i] = 0; c->prof_calls[i] = 0; }
        c->prof_kern.clear();
    }
    return n;
}
