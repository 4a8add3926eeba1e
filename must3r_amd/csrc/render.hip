// Scene rendering: a point rasteriser for headless previews of a scene (what the reference shows through demo/viser.py and the open3d PipelineView of
// slam/slam.py), from any pinhole camera into colour, depth and source-index images.
//
//   render_splat_kernel    thread t of a block owns source pixels 4t .. 4t+3 of one view (the export's 16-byte loads) and walks the block's cameras: the fp64
//                          projection with every operation rounded (this file is built with -ffp-contract=off), the drop tests before any conversion to an
//                          integer, then for every covered target pixel one 64-bit unsigned atomicMin of (bits(fp32 Z) << 32) | global source index.  A plain
//                          load of the key in front skips the atomic when it cannot win: a key only ever falls, so a stale read costs one needless atomic.
//   render_resolve_kernel  one thread per target pixel: the winning index located in its view by a search over the per-view pixel offsets, the colour bytes by
//                          the export's rule, the depth the fp32 in the key; an empty key gives the background, +inf and 0xFFFFFFFF.
//
// An integer minimum does not depend on arrival order: the images are repeatable bit for bit, and a tie in depth goes to the lower source index.
// Scratch layout (render_plan): [device view table][device camera table][A = w2c . M, n_cams x n_views x 12 fp64][keys n_cams x H x W uint64].
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "abi.hpp"
#include "common.hpp"
#include "scene_load.hpp"

namespace m3r {
namespace render {

constexpr int RN_T = 256;                        // threads per block
constexpr int RN_PPT = 4;                        // consecutive source pixels per thread
constexpr int RN_BLOCK = RN_T * RN_PPT;          // source pixels per block
// cameras a block walks with its four points per thread in registers.  More cameras per block read the points fewer times but keep more key planes in
// flight at once, and the key reads are what the launch waits for: measured at 120 cameras of 512 x 384 over 39.3 M points, 1 / 2 / 4 / 8 / 16 / 120 cameras
// per block take 63 / 48 / 38 / 32 / 35 / 73 ms at point size 1 and 385 / 346 / 325 / 315 / 363 / 990 ms at point size 4; 8 is also the best at 3.9 M and
// at 0.2 M points (profiles/render_scratch_builds.jsonl)
constexpr int RN_CAMS_PER_BLOCK = 8;
constexpr unsigned long long RN_EMPTY = ~0ull;   // bits(fp32 Z) = 0xFFFFFFFF is a NaN: no point writes this key

struct RnView {                                  // device view table entry, 40 bytes
    const float* conf;
    const float* pts;
    const float* rgb;
    unsigned n_pix;
    unsigned block_base;                         // first source block of the view
    unsigned pix_base;                           // pixels of the views before: the global source index of the view's first pixel
    unsigned pad;
};
static_assert(sizeof(RnView) == 40, "the header states the scratch size");

struct RnCam {                                   // device camera table entry, 40 bytes
    double fx, fy, cx, cy;
    float z_near, z_far;
};
static_assert(sizeof(RnCam) == 40, "the header states the scratch size");

struct RnPlan {
    long long n_blocks, n_pix, n_target;         // source blocks, source pixels, target pixels of all cameras
    int W, H;
    size_t off_cams, off_A, off_keys, bytes;
};

// view of a source block: the last view whose block_base <= b
__device__ __forceinline__ int view_of_block(const RnView* __restrict__ views, const int n_views, const unsigned b) {
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].block_base <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ((a0 x + a1 y) + a2 z) + a3 in fp64, every operation rounded
__device__ __forceinline__ double affine_row64(const double* __restrict__ a, const double x, const double y, const double z) {
    const double p = a[0] * x, q = a[1] * y, r = a[2] * z;
    return ((p + q) + r) + a[3];
}

// first column (row) of the square of `ps` pixels around u, clipped to [0, n): false when nothing is left.  Everything stays fp64 until the range is known
// to fit an int: u may be 1e30.
__device__ __forceinline__ bool span(const double u, const double half, const int ps, const int n, int& lo, int& hi) {
    const double f = floor(u - half);
    if (!(f < (double)n) || !(f + (double)ps > 0.0)) return false;
    const int i = (int)f;                        // in (-ps, n)
    lo = i < 0 ? 0 : i;
    hi = i + ps < n ? i + ps : n;
    return true;
}

// grid (source blocks, camera groups): block (b, g) takes cameras [g cams_per_block, (g + 1) cams_per_block)
__global__ void __launch_bounds__(RN_T) render_splat_kernel(const RnView* __restrict__ views, const int n_views, const RnCam* __restrict__ cams, const int n_cams,
                                                            const int cams_per_block, const double* __restrict__ A, const float thr, const int ps,
                                                            const int W, const int H, unsigned long long* __restrict__ keys) {
    const unsigned b = blockIdx.x;
    const int vi = view_of_block(views, n_views, b);
    const RnView& v = views[vi];
    const unsigned n = v.n_pix, i0 = (b - v.block_base) * RN_BLOCK + threadIdx.x * RN_PPT;
    float c[4];
    load4(v.conf, i0, n, c);
    bool f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = i0 + j < n && c[j] >= thr;
    if (!(f[0] || f[1] || f[2] || f[3])) return;
    float p[12];
    load12(v.pts, i0, n, p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = f[j] && isfinite(p[3 * j]) && isfinite(p[3 * j + 1]) && isfinite(p[3 * j + 2]);
    const double half = 0.5 * (double)(ps - 1);
    const size_t plane = (size_t)W * (size_t)H;
    const int c_lo = blockIdx.y * cams_per_block, c_hi = min(n_cams, c_lo + cams_per_block);
    for (int ci = c_lo; ci < c_hi; ++ci) {
        const double* a = A + ((size_t)ci * n_views + vi) * 12;
        const RnCam cam = cams[ci];
        unsigned long long* kc = keys + (size_t)ci * plane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!f[j]) continue;
            const double x = (double)p[3 * j], y = (double)p[3 * j + 1], z = (double)p[3 * j + 2];
            const double Z = affine_row64(a + 8, x, y, z);
            if (!(Z >= (double)cam.z_near && Z <= (double)cam.z_far)) continue;
            const double iz = 1.0 / Z;
            const double X = affine_row64(a, x, y, z), Y = affine_row64(a + 4, x, y, z);
            const double u = cam.fx * (X * iz) + cam.cx, w = cam.fy * (Y * iz) + cam.cy;
            if (!isfinite(u) || !isfinite(w)) continue;
            int x0, x1, y0, y1;
            if (!span(u, half, ps, W, x0, x1) || !span(w, half, ps, H, y0, y1)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)Z) << 32) | (unsigned long long)(v.pix_base + i0 + j);
            for (int r = y0; r < y1; ++r) {
                for (int q = x0; q < x1; ++q) {
                    unsigned long long* k = kc + (size_t)r * W + q;
                    if (*k > key) atomicMin(k, key);
                }
            }
        }
    }
}

// view of a global source index: the last view whose pix_base <= i
__device__ __forceinline__ int view_of_pixel(const RnView* __restrict__ views, const int n_views, const unsigned i) {
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].pix_base <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct RnBackground { unsigned char c[3]; };

__global__ void __launch_bounds__(RN_T) render_resolve_kernel(const RnView* __restrict__ views, const int n_views, const unsigned long long* __restrict__ keys,
                                                              const long long n_target, const RnBackground bg, unsigned char* __restrict__ rgb,
                                                              float* __restrict__ depth, unsigned* __restrict__ index) {
    const long long t = (long long)blockIdx.x * RN_T + threadIdx.x;
    if (t >= n_target) return;
    const unsigned long long key = keys[t];
    unsigned char col[3] = {bg.c[0], bg.c[1], bg.c[2]};
    float d = INFINITY;
    unsigned idx = 0xFFFFFFFFu;
    if (key != RN_EMPTY) {
        idx = (unsigned)key;
        d = __uint_as_float((unsigned)(key >> 32));
        if (rgb) {
            const RnView& v = views[view_of_pixel(views, n_views, idx)];
            const float* src = v.rgb + 3ull * (idx - v.pix_base);
#pragma unroll
            for (int a = 0; a < 3; ++a) col[a] = (unsigned char)quant8(src[a]);
        }
    }
    if (rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) rgb[3 * t + a] = col[a];
    }
    if (depth) depth[t] = d;
    if (index) index[t] = idx;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates everything of the descriptor but its scratch and lays the scratch out; 0 = fine.  No HIP call.
int render_plan(const must3r_hip_render_desc* d, RnPlan* p) {
    if (!d) return fail("render: null descriptor");
    if (!d->views) return fail("render: null view table");
    if (!d->cams) return fail("render: null camera table");
    if (d->n_views <= 0) return fail("render: the view table is empty");
    if (d->n_cams <= 0) return fail("render: the camera table is empty");
    if (d->point_size < 1 || d->point_size > MUST3R_RENDER_MAX_POINT_SIZE) return fail("render: point_size is outside [1, 8]");
    long long blocks = 0, pix = 0;
    for (int i = 0; i < d->n_views; ++i) {
        const must3r_hip_export_view& v = d->views[i];
        if (v.H <= 0 || v.W <= 0) return fail("render: a view has a non-positive size");
        const long long n = (long long)v.H * v.W;
        if (n >= (1LL << 31)) return fail("render: a view has 2^31 or more pixels");
        pix += n;
        blocks += (n + RN_BLOCK - 1) / RN_BLOCK;
        if (pix >= (1LL << 32)) return fail("render: the scene has 2^32 or more pixels (uint32 source indices)");
    }
    const int W = d->cams[0].W, H = d->cams[0].H;
    if (W <= 0 || H <= 0) return fail("render: a camera has a non-positive image size");
    for (int i = 0; i < d->n_cams; ++i) {
        const must3r_hip_render_camera& c = d->cams[i];
        if (c.W != W || c.H != H) return fail("render: the cameras of one call must share one image size");
        if (!(c.z_near > 0.f) || !(c.z_far >= c.z_near) || !std::isfinite(c.z_far)) return fail("render: a camera needs 0 < z_near <= z_far < inf");
    }
    const long long target = (long long)d->n_cams * W * H;
    if ((long long)W * H >= (1LL << 31) || target >= (1LL << 31)) return fail("render: 2^31 or more target pixels in one call");
    p->n_blocks = blocks;
    p->n_pix = pix;
    p->n_target = target;
    p->W = W;
    p->H = H;
    size_t off = align256((size_t)d->n_views * sizeof(RnView));
    p->off_cams = off;
    off = align256(off + (size_t)d->n_cams * sizeof(RnCam));
    p->off_A = off;
    off = align256(off + (size_t)d->n_cams * (size_t)d->n_views * 12 * sizeof(double));
    p->off_keys = off;
    off = align256(off + (size_t)target * sizeof(unsigned long long));
    p->bytes = off;
    return 0;
}

// pinned staging of the tables, a ring of slots per calling thread (as image.hip's and png.hip's): the copy is asynchronous, a slot is reused once its copy
// has completed
struct StageSlot {
    void* pin = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int dev = -1;
    bool used = false;
};
constexpr int kStageSlots = 4;

// hands out the slot's pinned buffer of `bytes` bytes for the caller to fill
static int stage_begin(size_t bytes, StageSlot** out) {
    static thread_local StageSlot slots[kStageSlots];
    static thread_local int next = 0;
    StageSlot& slot = slots[next];
    next = (next + 1) % kStageSlots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail("render: hipGetDevice failed");
    if (slot.used && hipEventSynchronize(slot.ev) != hipSuccess) return fail("render: staging event wait failed");
    slot.used = false;
    if (slot.dev != dev || slot.cap < bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        if (slot.ev) (void)hipEventDestroy(slot.ev);
        slot = StageSlot();
        const size_t cap = std::max(bytes, (size_t)1 << 16);
        if (hipHostMalloc(&slot.pin, cap) != hipSuccess) { slot.pin = nullptr; return fail("render: pinned staging allocation failed"); }
        if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) != hipSuccess) { slot.ev = nullptr; return fail("render: event creation failed"); }
        slot.cap = cap;
        slot.dev = dev;
    }
    *out = &slot;
    return 0;
}

static int stage_send(StageSlot* slot, void* dst, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(dst, slot->pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("render: table upload failed");
    if (hipEventRecord(slot->ev, s) != hipSuccess) return fail("render: staging event record failed");
    slot->used = true;
    return 0;
}

// A = w2c . M of a 3x4 by a 3x4 with the implied last row (0 0 0 1), in fp64: per element the three products summed in ascending k, then the translation
static void compose(const double* w2c, const double* M, double* A) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 4; ++b) {
            double s = w2c[4 * a] * M[b];
            s = s + w2c[4 * a + 1] * M[4 + b];
            s = s + w2c[4 * a + 2] * M[8 + b];
            if (b == 3) s = s + w2c[4 * a + 3];
            A[4 * a + b] = s;
        }
    }
}

}  // namespace render
}  // namespace m3r
using namespace m3r;
using namespace m3r::render;

extern "C" size_t must3r_hip_render_scratch_bytes(const must3r_hip_render_desc* d) {
    RnPlan p;
    if (render_plan(d, &p)) return 0;
    return p.bytes;
}

extern "C" int must3r_hip_render(const must3r_hip_render_desc* d) {
    RnPlan p;
    if (render_plan(d, &p)) return 1;
    if (!d->scratch) return fail("render: null scratch");
    if (d->scratch_bytes < p.bytes) return fail("render: scratch too small");
    if (reinterpret_cast<uintptr_t>(d->scratch) & 255) return fail("render: the scratch must be 256-byte aligned");
    for (int i = 0; i < d->n_views; ++i)
        if (!d->views[i].conf || !d->views[i].pts || (d->rgb && !d->views[i].rgb)) return fail("render: a view has a null plane");
    hipStream_t s = reinterpret_cast<hipStream_t>(d->stream);
    char* sc = reinterpret_cast<char*>(d->scratch);
    // the three tables are one contiguous piece of the scratch: one staging slot, one copy
    StageSlot* slot = nullptr;
    if (stage_begin(p.off_keys, &slot)) return 1;
    char* host = reinterpret_cast<char*>(slot->pin);
    std::memset(host, 0, p.off_keys);
    RnView* hv = reinterpret_cast<RnView*>(host);
    unsigned bb = 0, pb = 0;
    for (int i = 0; i < d->n_views; ++i) {
        const must3r_hip_export_view& v = d->views[i];
        hv[i].conf = v.conf; hv[i].pts = v.pts; hv[i].rgb = v.rgb;
        hv[i].n_pix = (unsigned)((long long)v.H * v.W);
        hv[i].block_base = bb; hv[i].pix_base = pb; hv[i].pad = 0;
        bb += (hv[i].n_pix + RN_BLOCK - 1) / RN_BLOCK;
        pb += hv[i].n_pix;
    }
    RnCam* hc = reinterpret_cast<RnCam*>(host + p.off_cams);
    double* hA = reinterpret_cast<double*>(host + p.off_A);
    for (int c = 0; c < d->n_cams; ++c) {
        const must3r_hip_render_camera& cam = d->cams[c];
        hc[c].fx = cam.fx; hc[c].fy = cam.fy; hc[c].cx = cam.cx; hc[c].cy = cam.cy;
        hc[c].z_near = cam.z_near; hc[c].z_far = cam.z_far;
        for (int i = 0; i < d->n_views; ++i) compose(cam.w2c, d->views[i].M, hA + ((size_t)c * d->n_views + i) * 12);
    }
    if (stage_send(slot, sc, p.off_keys, s)) return 1;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(sc + p.off_keys);
    if (hipMemsetAsync(keys, 0xFF, (size_t)p.n_target * sizeof(unsigned long long), s) != hipSuccess) return fail("render: clearing the keys failed");
    const RnView* dv = reinterpret_cast<const RnView*>(sc);
    const RnCam* dc = reinterpret_cast<const RnCam*>(sc + p.off_cams);
    const double* dA = reinterpret_cast<const double*>(sc + p.off_A);
    const int cpb = std::min(d->n_cams, RN_CAMS_PER_BLOCK);
    const unsigned groups = (unsigned)((d->n_cams + cpb - 1) / cpb);
    if (groups > 65535u) return fail("render: too many cameras in one call");
    hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)p.n_blocks, groups), dim3(RN_T), 0, s, dv, d->n_views, dc, d->n_cams, cpb, dA, d->thr,
                       d->point_size, p.W, p.H, keys);
    RnBackground bg;
    for (int a = 0; a < 3; ++a) bg.c[a] = d->background[a];
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((p.n_target + RN_T - 1) / RN_T)), dim3(RN_T), 0, s, dv, d->n_views, keys, p.n_target, bg,
                       d->rgb, d->depth, d->index);
    if (hipGetLastError() != hipSuccess) return fail("render: launch failed");
    return 0;
}
