// Scene rendering, triangles: the mesh the export writes (export.hip: two triangles per quad of every view's pixel grid), rasterised into the point path's
// three images under the point path's guarantees (render.hip; the rule is stated in include/must3r_hip.h and lives in render_tri.hpp).
//
//   render_mesh_splat_kernel    thread t of a block owns the anchors 4t .. 4t+3 of one view (the export's 16-byte loads) and reads the five pixels of its row
//                               piece and the five below it: ten corners, eight triangles.  Per camera of the block's group it projects the ten corners once,
//                               then each triangle whose candidate box holds at most RM_WAVE_AREA target pixels is walked by its own lane; the others are
//                               marked, and after the lane pass the wave takes them one at a time: a ballot per triangle slot, the chosen lane's nine fp64
//                               corner values and id read across the wave, the 64 lanes striding the box.  Every covered sample takes the 64-bit atomicMin
//                               of (bits(fp32 Zp) << 32) | triangle id behind a plain load of the key.
//   render_mesh_resolve_kernel  one thread per target pixel: from the winning id the anchor, its view and the three corners; their projections, the weights t
//                               and Zp at the pixel's own centre again, the colour from them; the depth is the fp32 in the key.
//
// The result is a minimum over a set of (pixel, key) pairs that does not depend on which path drew a triangle nor on arrival order.
// Scratch layout (mesh_plan), the sections of render.hip: [device view table][device camera table][A = w2c . M, n_cams x n_views x 12 fp64][keys].
// The host side (plan, staging ring, composition) repeats render.hip's, which this file leaves untouched.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "abi.hpp"
#include "common.hpp"
#include "scene_load.hpp"
#include "render_tri.hpp"

namespace m3r {
namespace render_mesh {

constexpr int RM_T = 256;                        // threads per block: four waves
constexpr int RM_PPT = 4;                        // consecutive anchors per thread
constexpr int RM_BLOCK = RM_T * RM_PPT;          // source pixels per block
constexpr int RM_CAMS_PER_BLOCK = 8;             // render.hip's RN_CAMS_PER_BLOCK, taken over and not swept again here: the corner floats stay in registers
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): splat 198 VGPRs, no scratch, no spill, 2 waves per SIMD -- the ten corners are 30 fp64 values
// and 30 fp32 source values per lane, and the per-corner flags are bit masks in one VGPR (as bools they were SGPR pairs and spilled 16 SGPRs); resolve 76 VGPRs,
// no scratch.  No LDS: a thread's corners come from its own loads.
// scratch builds (scripts/bench_render_mesh.py, profiles/render_mesh_scratch_builds.jsonl): -DRM_WAVE_AREA=<n> moves the split, -DRM_NO_WAVE_PATH leaves every
// triangle to its lane
#ifndef RM_WAVE_AREA
#define RM_WAVE_AREA MUST3R_RENDER_MESH_WAVE_AREA
#endif
constexpr unsigned long long RM_EMPTY = ~0ull;

struct RmView {                                  // device view table entry, 40 bytes
    const float* conf;
    const float* pts;
    const float* rgb;
    unsigned n_pix;
    unsigned block_base;                         // first source block of the view
    unsigned pix_base;                           // pixels of the views before
    unsigned W;                                  // row length: the corners below an anchor
};
static_assert(sizeof(RmView) == 40, "the header states the scratch size");

struct RmCam {                                   // device camera table entry, 40 bytes
    double fx, fy, cx, cy;
    float z_near, z_far;
};
static_assert(sizeof(RmCam) == 40, "the header states the scratch size");

struct RmPlan {
    long long n_blocks, n_pix, n_target;
    int W, H;
    size_t off_cams, off_A, off_keys, bytes;
};

// the last view whose block_base <= b
__device__ __forceinline__ int view_of_block(const RmView* __restrict__ views, const int n_views, const unsigned b) {
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].block_base <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the last view whose pix_base <= i
__device__ __forceinline__ int view_of_pixel(const RmView* __restrict__ views, const int n_views, const unsigned i) {
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].pix_base <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one sample point of one triangle: (q, r) is inside the image
__device__ __forceinline__ void sample(const tri::Corner& c0, const tri::Corner& c1, const tri::Corner& c2, const int q, const int r, const unsigned id,
                                       unsigned long long* __restrict__ kc, const int W) {
    double Zp, t[3];
    if (!tri::cover(c0, c1, c2, (double)q + 0.5, (double)r + 0.5, Zp, t)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)Zp) << 32) | (unsigned long long)id;
    unsigned long long* k = kc + (size_t)r * W + q;
    if (*k > key) atomicMin(k, key);
}

// x of lane `lane` (the same lane in every lane of the wave)
__device__ __forceinline__ double lane_read(const double x, const int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ tri::Corner lane_read(const tri::Corner& c, const int lane) {
    tri::Corner o;
    o.u = lane_read(c.u, lane);
    o.v = lane_read(c.v, lane);
    o.iz = lane_read(c.iz, lane);
    return o;
}

// grid (source blocks, camera groups).  No thread leaves early: the wave pass needs all 64 lanes.
__global__ void __launch_bounds__(RM_T) render_mesh_splat_kernel(const RmView* __restrict__ views, const int n_views, const RmCam* __restrict__ cams,
                                                                 const int n_cams, const int cams_per_block, const double* __restrict__ A, const float thr,
                                                                 const int W, const int H, unsigned long long* __restrict__ keys) {
    const unsigned b = blockIdx.x;
    const int vi = view_of_block(views, n_views, b);
    const RmView& v = views[vi];
    const unsigned n = v.n_pix, Wv = v.W, i0 = (b - v.block_base) * RM_BLOCK + threadIdx.x * RM_PPT;
    // anchors: column < Wv - 1 and a row below
    bool anchor[4];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned i = i0 + j;
        anchor[j] = i < n && i + Wv < n && i % Wv + 1 < Wv;
        any = any || anchor[j];
    }
    // the row piece i0 .. i0 + 4 and the one below it: confidence test and finite points per corner
    float pt[15], pb[15];
    unsigned fm = 0;                             // bit j: top corner j passes, bit 5 + j: bottom corner j (bit masks, not bools: a bool per lane is an SGPR pair)
    if (any) {
        float c[4], p[12];
        load4(v.conf, i0, n, c);
        load12(v.pts, i0, n, p);
#pragma unroll
        for (int j = 0; j < 4; ++j) fm |= (unsigned)(i0 + j < n && c[j] >= thr) << j;
#pragma unroll
        for (int j = 0; j < 12; ++j) pt[j] = p[j];
        const unsigned i4 = i0 + 4;
        fm |= (unsigned)(i4 < n && v.conf[i4] >= thr) << 4;
#pragma unroll
        for (int a = 0; a < 3; ++a) pt[12 + a] = i4 < n ? v.pts[3ull * i4 + a] : 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned i = i0 + Wv + j;
            fm |= (unsigned)(i < n && v.conf[i] >= thr) << (5 + j);
#pragma unroll
            for (int a = 0; a < 3; ++a) pb[3 * j + a] = i < n ? v.pts[3ull * i + a] : 0.f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 15; ++j) pt[j] = pb[j] = 0.f;
    }
    // corner masks of the eight triangles: kind 0 of anchor j = top j, top j + 1, bottom j; kind 1 = top j + 1, bottom j, bottom j + 1
    constexpr unsigned need[8] = {0x23, 0x62, 0x46, 0xC4, 0x8C, 0x188, 0x118, 0x310};
    unsigned can = 0;                            // the triangles this thread can draw at all
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (anchor[s >> 1] && (fm & need[s]) == need[s]) can |= 1u << s;
    const unsigned id0 = 2u * (v.pix_base + i0);
    const size_t plane = (size_t)W * (size_t)H;
    const int c_lo = blockIdx.y * cams_per_block, c_hi = min(n_cams, c_lo + cams_per_block);
    for (int ci = c_lo; ci < c_hi; ++ci) {
        const double* a = A + ((size_t)ci * n_views + vi) * 12;
        const RmCam cam = cams[ci];
        const double zn = (double)cam.z_near, zf = (double)cam.z_far;
        unsigned long long* kc = keys + (size_t)ci * plane;
        tri::Corner top[5], bot[5];
        unsigned om = 0;                         // fm's bits after the camera's tests
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            top[j].u = top[j].v = top[j].iz = 0.0;
            bot[j].u = bot[j].v = bot[j].iz = 0.0;
            if (can != 0 && tri::project(a, cam.fx, cam.fy, cam.cx, cam.cy, zn, zf, (fm >> j) & 1u, pt[3 * j], pt[3 * j + 1], pt[3 * j + 2], top[j])) om |= 1u << j;
            if (can != 0 && tri::project(a, cam.fx, cam.fy, cam.cx, cam.cy, zn, zf, (fm >> (5 + j)) & 1u, pb[3 * j], pb[3 * j + 1], pb[3 * j + 2], bot[j]))
                om |= 1u << (5 + j);
        }
        unsigned big = 0;                        // triangles left to the wave
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int j = s >> 1;
            const tri::Corner& c0 = (s & 1) ? top[j + 1] : top[j];
            const tri::Corner& c1 = (s & 1) ? bot[j] : top[j + 1];
            const tri::Corner& c2 = (s & 1) ? bot[j + 1] : bot[j];
            const bool ok = ((can >> s) & 1u) && (om & need[s]) == need[s];
            int x0, x1, y0, y1;
            if (!ok || !tri::box(c0, c1, c2, W, H, x0, x1, y0, y1)) continue;
#ifndef RM_NO_WAVE_PATH
            if ((unsigned)(x1 - x0 + 1) * (unsigned)(y1 - y0 + 1) > (unsigned)RM_WAVE_AREA) {
                big |= 1u << s;
                continue;
            }
#endif
            for (int r = y0; r <= y1; ++r)
                for (int q = x0; q <= x1; ++q) sample(c0, c1, c2, q, r, id0 + s, kc, W);
        }
#ifndef RM_NO_WAVE_PATH
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int j = s >> 1;
            unsigned long long m = __ballot((big >> s) & 1u);
            while (m) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                m &= m - 1;
                const tri::Corner c0 = lane_read((s & 1) ? top[j + 1] : top[j], src);
                const tri::Corner c1 = lane_read((s & 1) ? bot[j] : top[j + 1], src);
                const tri::Corner c2 = lane_read((s & 1) ? bot[j + 1] : bot[j], src);
                const unsigned id = (unsigned)__builtin_amdgcn_readlane((int)(id0 + s), src);
                int x0, x1, y0, y1;
                if (!tri::box(c0, c1, c2, W, H, x0, x1, y0, y1)) continue;       // the same for every lane: it held for lane `src`
                const unsigned bw = (unsigned)(x1 - x0 + 1), area = bw * (unsigned)(y1 - y0 + 1);
                for (unsigned k = (unsigned)lane; k < area; k += 64u) sample(c0, c1, c2, x0 + (int)(k % bw), y0 + (int)(k / bw), id, kc, W);
            }
        }
#endif
    }
}

struct RmBackground { unsigned char c[3]; };

__global__ void __launch_bounds__(RM_T) render_mesh_resolve_kernel(const RmView* __restrict__ views, const int n_views, const RmCam* __restrict__ cams,
                                                                   const double* __restrict__ A, const unsigned long long* __restrict__ keys,
                                                                   const long long n_target, const int W, const int H, const RmBackground bg,
                                                                   unsigned char* __restrict__ rgb, float* __restrict__ depth, unsigned* __restrict__ index) {
    const long long t = (long long)blockIdx.x * RM_T + threadIdx.x;
    if (t >= n_target) return;
    const unsigned long long key = keys[t];
    unsigned char col[3] = {bg.c[0], bg.c[1], bg.c[2]};
    float d = INFINITY;
    unsigned idx = 0xFFFFFFFFu;
    if (key != RM_EMPTY) {
        idx = (unsigned)key;
        d = __uint_as_float((unsigned)(key >> 32));
        if (rgb) {
            const long long plane = (long long)W * H;
            const int ci = (int)(t / plane);
            const int pix = (int)(t - (long long)ci * plane), r = pix / W, q = pix - r * W;
            const unsigned g = idx >> 1;
            const int vi = view_of_pixel(views, n_views, g);
            const RmView& v = views[vi];
            unsigned off[3];
            tri::corner_offsets((int)(idx & 1u), v.W, off);
            const double* a = A + ((size_t)ci * n_views + vi) * 12;
            const RmCam cam = cams[ci];
            tri::Corner c[3];
            const float* src[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned long long i = (unsigned long long)(g - v.pix_base) + off[k];
                const float* p = v.pts + 3ull * i;
                src[k] = v.rgb + 3ull * i;
                (void)tri::project(a, cam.fx, cam.fy, cam.cx, cam.cy, (double)cam.z_near, (double)cam.z_far, true, p[0], p[1], p[2], c[k]);
            }
            double Zp = 0.0, w[3] = {0.0, 0.0, 0.0};
            (void)tri::cover(c[0], c[1], c[2], (double)q + 0.5, (double)r + 0.5, Zp, w);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) col[ch] = (unsigned char)quant8(tri::shade(w, Zp, src[0][ch], src[1][ch], src[2][ch]));
        }
    }
    if (rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[3 * t + ch] = col[ch];
    }
    if (depth) depth[t] = d;
    if (index) index[t] = idx;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates everything of the descriptor but its scratch and lays the scratch out; 0 = fine.  No HIP call.
static int mesh_plan(const must3r_hip_render_mesh_desc* d, RmPlan* p) {
    if (!d) return fail("render_mesh: null descriptor");
    if (!d->views) return fail("render_mesh: null view table");
    if (!d->cams) return fail("render_mesh: null camera table");
    if (d->n_views <= 0) return fail("render_mesh: the view table is empty");
    if (d->n_cams <= 0) return fail("render_mesh: the camera table is empty");
    long long blocks = 0, pix = 0;
    for (int i = 0; i < d->n_views; ++i) {
        const must3r_hip_export_view& v = d->views[i];
        if (v.H <= 0 || v.W <= 0) return fail("render_mesh: a view has a non-positive size");
        const long long n = (long long)v.H * v.W;
        if (n >= (1LL << 31)) return fail("render_mesh: a view has 2^31 or more pixels");
        pix += n;
        blocks += (n + RM_BLOCK - 1) / RM_BLOCK;
        if (pix >= (1LL << 31)) return fail("render_mesh: the scene has 2^31 or more pixels (a triangle id is twice a source index plus the kind)");
    }
    const int W = d->cams[0].W, H = d->cams[0].H;
    if (W <= 0 || H <= 0) return fail("render_mesh: a camera has a non-positive image size");
    for (int i = 0; i < d->n_cams; ++i) {
        const must3r_hip_render_camera& c = d->cams[i];
        if (c.W != W || c.H != H) return fail("render_mesh: the cameras of one call must share one image size");
        if (!(c.z_near > 0.f) || !(c.z_far >= c.z_near) || !std::isfinite(c.z_far)) return fail("render_mesh: a camera needs 0 < z_near <= z_far < inf");
    }
    const long long target = (long long)d->n_cams * W * H;
    if ((long long)W * H >= (1LL << 31) || target >= (1LL << 31)) return fail("render_mesh: 2^31 or more target pixels in one call");
    p->n_blocks = blocks;
    p->n_pix = pix;
    p->n_target = target;
    p->W = W;
    p->H = H;
    size_t off = align256((size_t)d->n_views * sizeof(RmView));
    p->off_cams = off;
    off = align256(off + (size_t)d->n_cams * sizeof(RmCam));
    p->off_A = off;
    off = align256(off + (size_t)d->n_cams * (size_t)d->n_views * 12 * sizeof(double));
    p->off_keys = off;
    off = align256(off + (size_t)target * sizeof(unsigned long long));
    p->bytes = off;
    return 0;
}

// pinned staging of the tables, a ring of slots per calling thread (as render.hip's): the copy is asynchronous, a slot is reused once its copy has completed
struct StageSlot {
    void* pin = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int dev = -1;
    bool used = false;
};
constexpr int kStageSlots = 4;

static int stage_begin(size_t bytes, StageSlot** out) {
    static thread_local StageSlot slots[kStageSlots];
    static thread_local int next = 0;
    StageSlot& slot = slots[next];
    next = (next + 1) % kStageSlots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail("render_mesh: hipGetDevice failed");
    if (slot.used && hipEventSynchronize(slot.ev) != hipSuccess) return fail("render_mesh: staging event wait failed");
    slot.used = false;
    if (slot.dev != dev || slot.cap < bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        if (slot.ev) (void)hipEventDestroy(slot.ev);
        slot = StageSlot();
        const size_t cap = std::max(bytes, (size_t)1 << 16);
        if (hipHostMalloc(&slot.pin, cap) != hipSuccess) { slot.pin = nullptr; return fail("render_mesh: pinned staging allocation failed"); }
        if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) != hipSuccess) { slot.ev = nullptr; return fail("render_mesh: event creation failed"); }
        slot.cap = cap;
        slot.dev = dev;
    }
    *out = &slot;
    return 0;
}

static int stage_send(StageSlot* slot, void* dst, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(dst, slot->pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("render_mesh: table upload failed");
    if (hipEventRecord(slot->ev, s) != hipSuccess) return fail("render_mesh: staging event record failed");
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

}  // namespace render_mesh
}  // namespace m3r
using namespace m3r;
using namespace m3r::render_mesh;

extern "C" size_t must3r_hip_render_mesh_scratch_bytes(const must3r_hip_render_mesh_desc* d) {
    RmPlan p;
    if (mesh_plan(d, &p)) return 0;
    return p.bytes;
}

extern "C" int must3r_hip_render_mesh(const must3r_hip_render_mesh_desc* d) {
    RmPlan p;
    if (mesh_plan(d, &p)) return 1;
    if (!d->scratch) return fail("render_mesh: null scratch");
    if (d->scratch_bytes < p.bytes) return fail("render_mesh: scratch too small");
    if (reinterpret_cast<uintptr_t>(d->scratch) & 255) return fail("render_mesh: the scratch must be 256-byte aligned");
    for (int i = 0; i < d->n_views; ++i)
        if (!d->views[i].conf || !d->views[i].pts || (d->rgb && !d->views[i].rgb)) return fail("render_mesh: a view has a null plane");
    hipStream_t s = reinterpret_cast<hipStream_t>(d->stream);
    char* sc = reinterpret_cast<char*>(d->scratch);
    // the three tables are one contiguous piece of the scratch: one staging slot, one copy
    StageSlot* slot = nullptr;
    if (stage_begin(p.off_keys, &slot)) return 1;
    char* host = reinterpret_cast<char*>(slot->pin);
    std::memset(host, 0, p.off_keys);
    RmView* hv = reinterpret_cast<RmView*>(host);
    unsigned bb = 0, pb = 0;
    for (int i = 0; i < d->n_views; ++i) {
        const must3r_hip_export_view& v = d->views[i];
        hv[i].conf = v.conf; hv[i].pts = v.pts; hv[i].rgb = v.rgb;
        hv[i].n_pix = (unsigned)((long long)v.H * v.W);
        hv[i].block_base = bb; hv[i].pix_base = pb; hv[i].W = (unsigned)v.W;
        bb += (hv[i].n_pix + RM_BLOCK - 1) / RM_BLOCK;
        pb += hv[i].n_pix;
    }
    RmCam* hc = reinterpret_cast<RmCam*>(host + p.off_cams);
    double* hA = reinterpret_cast<double*>(host + p.off_A);
    for (int c = 0; c < d->n_cams; ++c) {
        const must3r_hip_render_camera& cam = d->cams[c];
        hc[c].fx = cam.fx; hc[c].fy = cam.fy; hc[c].cx = cam.cx; hc[c].cy = cam.cy;
        hc[c].z_near = cam.z_near; hc[c].z_far = cam.z_far;
        for (int i = 0; i < d->n_views; ++i) compose(cam.w2c, d->views[i].M, hA + ((size_t)c * d->n_views + i) * 12);
    }
    if (stage_send(slot, sc, p.off_keys, s)) return 1;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(sc + p.off_keys);
    if (hipMemsetAsync(keys, 0xFF, (size_t)p.n_target * sizeof(unsigned long long), s) != hipSuccess) return fail("render_mesh: clearing the keys failed");
    const RmView* dv = reinterpret_cast<const RmView*>(sc);
    const RmCam* dc = reinterpret_cast<const RmCam*>(sc + p.off_cams);
    const double* dA = reinterpret_cast<const double*>(sc + p.off_A);
    const int cpb = std::min(d->n_cams, RM_CAMS_PER_BLOCK);
    const unsigned groups = (unsigned)((d->n_cams + cpb - 1) / cpb);
    if (groups > 65535u) return fail("render_mesh: too many cameras in one call");
    hipLaunchKernelGGL(render_mesh_splat_kernel, dim3((unsigned)p.n_blocks, groups), dim3(RM_T), 0, s, dv, d->n_views, dc, d->n_cams, cpb, dA, d->thr, p.W,
                       p.H, keys);
    RmBackground bg;
    for (int a = 0; a < 3; ++a) bg.c[a] = d->background[a];
    hipLaunchKernelGGL(render_mesh_resolve_kernel, dim3((unsigned)((p.n_target + RM_T - 1) / RM_T)), dim3(RM_T), 0, s, dv, d->n_views, dc, dA, keys,
                       p.n_target, p.W, p.H, bg, d->rgb, d->depth, d->index);
    if (hipGetLastError() != hipSuccess) return fail("render_mesh: launch failed");
    return 0;
}
