// Training augmentation behind the resampler (include/must3r_hip.h "ABI 21, additive", must3r_amd/train_augment.py): what the reference's datasets do to a raw
// frame on the host with PIL, cv2 and torchvision -- dust3r's _crop_resize_if_necessary, ColorJitter + ImgNorm, transpose_to_landscape.  The crop and the
// Pillow resize of the image are must3r_hip_resample's; this file holds what follows it, one launch per pass for the whole batch, each reading a per-view table:
//
//   augment_color_kernel<SUMS>   the colour jitter on the resampler's fp32 ImgNorm planes: a value v is the byte u = int(127.5f v + 127.5f + 0.5f) (exact for the
//                                256 values of the table), the view's flagged operations run on (r, g, b) bytes in the view's order, each output a byte again,
//                                and the result leaves through (u / 255 - 0.5) / 0.5.  Brightness, saturation and contrast are Pillow's Image.blend against
//                                black, the pixel's L and the image's mean L; hue is Pillow's RGB -> HSV, h + shift mod 256, HSV -> RGB.  The arithmetic is
//                                Pillow's operation for operation (the header states it); this file is built with -ffp-contract=off so that each rounds alone.
//                                SUMS = true is the first pass, for the views that apply contrast alone: the operations in front of contrast, then L, summed
//                                as integers over the lanes (xor butterfly), the waves (LDS, wave order) -> partial[view][tile], a uint32.  The second pass adds a
//                                view's partials in tile order into a uint64 (integers: any order is exact) and takes m = int(sum / count + 0.5) in double.
//   augment_depth_kernel<T>      the nearest-neighbour gather of the depth map through the same crop, resize and window: window pixel (x, y) reads
//                                depth[t1 + sy][l1 + sx], sx = min(floor((x + l) * (W / resized_w)), W - 1) in double (the quotient is formed on the host).
//                                The values are moved, not computed with: sky (negative) and holes (0) pass through, fp32 and uint16 alike.
//
// Both walk a view in tiles of 64 x 64 STORED pixels, grid (tiles across, tiles down, V), four waves of 16 tile rows each, a lane per column: a wave reads and
// writes runs of 64 consecutive pixels.  A portrait view of a batch stored landscape is written with its axes swapped (stored (r, c) = true (row c, col r)):
// its tile is read along the TRUE rows, turned through LDS (a 64 x 65 array of 32-bit words: a 32-bit LDS read banks by word address mod 32 inside each
// 32-lane half of the wave, and the odd pitch puts the 32 rows a half reads down a column on 32 different banks; an rgb triple travels as one word)
// and written along the stored rows, so both sides stay runs of 64.  The branch is per view, hence per block.
// No atomics, one writer per element, 64-bit offsets, every load and store guarded by the view's own sizes; a view's bits do not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "abi.hpp"
#include "common.hpp"

namespace m3r {
namespace {

constexpr int AUG_TILE = MUST3R_AUG_TILE;   // 64: stored pixels per tile side, and the lanes of a wave
constexpr int AUG_T = 256;                  // threads per block: 4 waves x 16 tile rows
constexpr int AUG_ROWS = AUG_TILE / (AUG_T / 64);
static_assert(AUG_TILE == 64 && AUG_ROWS * (AUG_T / 64) == AUG_TILE, "a lane per tile column");

struct ColorDev {
    long long src_offset;   // elements: the view's planes [3][h][w]
    int h, w;               // the true image
    int portrait;
    int nops;               // flagged operations
    int ops;                // in order, two bits each from bit 0 (no array: the record stays in scalar registers)
    int contrast_at;        // contrast's place among them, -1: not applied
    int shift;              // hue: trunc(factor * 255) mod 256
    float fb, fc, fs;       // the factors of brightness, contrast and saturation
};

struct DepthDev {
    const void* src;
    long long row_stride;
    double rx, ry;          // W1 / resized_w, H1 / resized_h
    int l1, t1, W1, H1;     // the first crop
    int l, t, w, h;         // the window inside the rescaled image, and its size = the true size of the output
    int portrait, pad;
};

struct ColorArgs {
    const float* src;
    const ColorDev* views;
    uint32_t* partial;      // [V][tiles]
    float* out;
    int Hs, Ws;
};

struct DepthArgs {
    const DepthDev* views;
    void* out;
    int Hs, Ws;
};

__host__ __device__ __forceinline__ int blend8(const int a, const int b, const float f) {
    const float t = (float)a + f * (float)(b - a);   // two roundings: -ffp-contract=off
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__host__ __device__ __forceinline__ int luma8(const int r, const int g, const int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__host__ __device__ __forceinline__ int clip8(const int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__host__ __device__ __forceinline__ void hue8(int& r, int& g, int& b, const int shift) {
    const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
        float h;
        if (r == mx) h = bc - gc;
        else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        // fmod(x, 1) of x = h / 6 + 1 in [5/6, 11/6]: x - floor(x) is the same number, exactly (x < 1: x itself; else x - 1, which fp64 represents)
        const double x = (double)h / 6.0 + 1.0;
        h = (float)(x - floor(x));
        H = clip8((int)((double)h * 255.0));
        S = clip8((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double hh = (double)H * 6.0 / 255.0;
    const double fi = floor(hh), f = hh - fi, fs = (double)S / 255.0, v = (double)V;
    const int p = clip8((int)round(v * (1.0 - fs)));
    const int q = clip8((int)round(v * (1.0 - fs * f)));
    const int t = clip8((int)round(v * (1.0 - fs * (1.0 - f))));
    switch ((int)fi % 6) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

// the operations ops[first .. last) of a view on one pixel; m: the contrast mean
__device__ __forceinline__ void jitter(const ColorDev& v, const int first, const int last, const int m, int& r, int& g, int& b) {
    for (int i = first; i < last; ++i) {   // uniform over the block
        const int op = (v.ops >> (2 * i)) & 3;
        if (op == MUST3R_AUG_BRIGHTNESS) {
            r = blend8(0, r, v.fb); g = blend8(0, g, v.fb); b = blend8(0, b, v.fb);
        } else if (op == MUST3R_AUG_CONTRAST) {
            r = blend8(m, r, v.fc); g = blend8(m, g, v.fc); b = blend8(m, b, v.fc);
        } else if (op == MUST3R_AUG_SATURATION) {
            const int L = luma8(r, g, b);
            r = blend8(L, r, v.fs); g = blend8(L, g, v.fs); b = blend8(L, b, v.fs);
        } else {
            hue8(r, g, b, v.shift);
        }
    }
}

__host__ __device__ __forceinline__ int byte_of(const float x) { return clip8((int)(127.5f * x + 127.5f + 0.5f)); }   // three roundings; the clip guards foreign input
__host__ __device__ __forceinline__ float norm_of(const int u) { return ((float)u / 255.0f - 0.5f) / 0.5f; }          // image.hip's table entry

// true pixel (y, x) of the view as bytes
__device__ __forceinline__ void load_rgb(const float* __restrict__ src, const ColorDev& v, const int y, const int x, int& r, int& g, int& b) {
    const size_t plane = (size_t)v.h * (size_t)v.w;
    const float* q = src + (size_t)v.src_offset + (size_t)y * (size_t)v.w + (size_t)x;
    r = byte_of(q[0]);
    g = byte_of(q[plane]);
    b = byte_of(q[2 * plane]);
}

template <bool SUMS>
__global__ void __launch_bounds__(AUG_T) augment_color_kernel(const ColorArgs p) {
    __shared__ uint32_t tile[SUMS ? 1 : AUG_TILE][SUMS ? 1 : AUG_TILE + 1];
    __shared__ uint32_t s_red[AUG_T / 64];
    __shared__ int s_mean;
    const unsigned view = blockIdx.z;
    const ColorDev v = p.views[view];   // uniform address
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.y * AUG_TILE, c0 = blockIdx.x * AUG_TILE;
    const unsigned tiles = gridDim.x * gridDim.y, tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    if constexpr (SUMS) {
        if (v.contrast_at < 0) return;   // uniform over the block
        uint32_t acc = 0;
#pragma unroll 4
        for (int k = 0; k < AUG_ROWS; ++k) {
            // stored (r0 + .., c0 + lane); the sum does not care which way the tile is walked, so a portrait view is walked along its true rows
            const int a = (v.portrait ? c0 : r0) + wv * AUG_ROWS + k, bcol = (v.portrait ? r0 : c0) + lane;
            if (a < v.h && bcol < v.w) {
                int r, g, b;
                load_rgb(p.src, v, a, bcol, r, g, b);
                jitter(v, 0, v.contrast_at, 0, r, g, b);
                acc += (uint32_t)luma8(r, g, b);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) s_red[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = s_red[0];
#pragma unroll
            for (int w = 1; w < AUG_T / 64; ++w) total += s_red[w];
            p.partial[(size_t)view * tiles + tile_id] = total;
        }
        return;
    } else {
        int m = 0;
        if (v.contrast_at >= 0) {
            if (threadIdx.x == 0) {
                unsigned long long sum = 0;
                for (unsigned t = 0; t < tiles; ++t) sum += p.partial[(size_t)view * tiles + t];
                s_mean = (int)((double)sum / (double)((long long)v.h * (long long)v.w) + 0.5);
            }
            __syncthreads();
            m = s_mean;
        }
        const size_t plane = (size_t)p.Hs * (size_t)p.Ws;
        float* __restrict__ out = p.out + (size_t)view * 3 * plane;
        if (!v.portrait) {
#pragma unroll 4
            for (int k = 0; k < AUG_ROWS; ++k) {
                const int r_ = r0 + wv * AUG_ROWS + k, c_ = c0 + lane;
                if (r_ < p.Hs && c_ < p.Ws) {
                    int r, g, b;
                    load_rgb(p.src, v, r_, c_, r, g, b);
                    jitter(v, 0, v.nops, m, r, g, b);
                    float* q = out + (size_t)r_ * (size_t)p.Ws + (size_t)c_;
                    q[0] = norm_of(r); q[plane] = norm_of(g); q[2 * plane] = norm_of(b);
                }
            }
            return;
        }
        // portrait: true (y, x) = stored (col, row).  tile[stored col][stored row]
#pragma unroll 4
        for (int k = 0; k < AUG_ROWS; ++k) {
            const int y = c0 + wv * AUG_ROWS + k, x = r0 + lane;
            if (y < v.h && x < v.w) {
                int r, g, b;
                load_rgb(p.src, v, y, x, r, g, b);
                jitter(v, 0, v.nops, m, r, g, b);
                tile[wv * AUG_ROWS + k][lane] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < AUG_ROWS; ++k) {
            const int r_ = r0 + wv * AUG_ROWS + k, c_ = c0 + lane;
            if (r_ < p.Hs && c_ < p.Ws) {
                const uint32_t px = tile[lane][wv * AUG_ROWS + k];
                float* q = out + (size_t)r_ * (size_t)p.Ws + (size_t)c_;
                q[0] = norm_of((int)(px & 255u)); q[plane] = norm_of((int)((px >> 8) & 255u)); q[2 * plane] = norm_of((int)((px >> 16) & 255u));
            }
        }
    }
}

// window pixel (x, y) of the view: the raw value at its source
template <class T>
__device__ __forceinline__ T depth_at(const DepthDev& v, const int y, const int x) {
    const int sx = (int)fmin(floor((double)(x + v.l) * v.rx), (double)(v.W1 - 1));
    const int sy = (int)fmin(floor((double)(y + v.t) * v.ry), (double)(v.H1 - 1));
    return reinterpret_cast<const T*>(v.src)[(size_t)(v.t1 + sy) * (size_t)v.row_stride + (size_t)(v.l1 + sx)];
}

template <class T>
__global__ void __launch_bounds__(AUG_T) augment_depth_kernel(const DepthArgs p) {
    __shared__ T tile[AUG_TILE][AUG_TILE + (sizeof(T) == 4 ? 1 : 2)];   // an odd pitch in 32-bit words either way
    const unsigned view = blockIdx.z;
    const DepthDev v = p.views[view];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.y * AUG_TILE, c0 = blockIdx.x * AUG_TILE;
    T* __restrict__ out = reinterpret_cast<T*>(p.out) + (size_t)view * (size_t)p.Hs * (size_t)p.Ws;
    T vals[AUG_ROWS];   // all of a lane's gathers are issued before the first of them is used
    if (!v.portrait) {
#pragma unroll
        for (int k = 0; k < AUG_ROWS; ++k) {
            const int r_ = r0 + wv * AUG_ROWS + k, c_ = c0 + lane;
            vals[k] = r_ < p.Hs && c_ < p.Ws ? depth_at<T>(v, r_, c_) : T(0);
        }
#pragma unroll
        for (int k = 0; k < AUG_ROWS; ++k) {
            const int r_ = r0 + wv * AUG_ROWS + k, c_ = c0 + lane;
            if (r_ < p.Hs && c_ < p.Ws) out[(size_t)r_ * (size_t)p.Ws + (size_t)c_] = vals[k];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < AUG_ROWS; ++k) {
        const int y = c0 + wv * AUG_ROWS + k, x = r0 + lane;
        vals[k] = y < v.h && x < v.w ? depth_at<T>(v, y, x) : T(0);
    }
#pragma unroll
    for (int k = 0; k < AUG_ROWS; ++k) tile[wv * AUG_ROWS + k][lane] = vals[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < AUG_ROWS; ++k) {
        const int r_ = r0 + wv * AUG_ROWS + k, c_ = c0 + lane;
        if (r_ < p.Hs && c_ < p.Ws) out[(size_t)r_ * (size_t)p.Ws + (size_t)c_] = tile[lane][wv * AUG_ROWS + k];
    }
}

inline size_t up256(const size_t x) { return (x + 255) & ~(size_t)255; }
inline bool off(const void* q, const uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }
inline unsigned tiles_of(const int n) { return (unsigned)((n + AUG_TILE - 1) / AUG_TILE); }

const char* shape_error(const int V, const int Hs, const int Ws) {
    if (V <= 0 || V > 65535) return "V must be in 1 .. 65535";
    if (Hs <= 0 || Ws <= 0) return "Hs and Ws must be positive";
    if ((long long)Hs * Ws > 0x7fffffffLL) return "a view of more than 2^31 - 1 pixels";
    if (tiles_of(Hs) > 65535u) return "more than 65535 tiles down a view";
    return nullptr;
}

// the stored shape every view of a batch must have: (h, w), swapped for a portrait view
const char* stored_error(const int portrait, const int h, const int w, const int Hs, const int Ws) {
    if (portrait != 0 && portrait != 1) return "bad flags: a view's portrait flag must be 0 or 1";
    if (h <= 0 || w <= 0) return "a view's size must be positive";
    if ((portrait ? w : h) != Hs || (portrait ? h : w) != Ws) return "mixed stored shape: a view's (h, w), swapped where it is flagged portrait, is not (Hs, Ws)";
    return nullptr;
}

// nullptr and the device table, or why the descriptor is refused: nothing is read through a device pointer and nothing is launched before this has passed
const char* color_plan(const must3r_hip_augment_color_args* a, std::vector<ColorDev>& tab, bool& any_contrast) {
    if (!a->src || !a->views || !a->out || !a->scratch) return "null argument (src, views, out, scratch)";
    if (const char* e = shape_error(a->V, a->Hs, a->Ws)) return e;
    if (off(a->src, 3) || off(a->out, 3)) return "src and out must be 4-byte aligned";
    if (off(a->scratch, 255)) return "scratch must be 256-byte aligned";
    if (a->scratch_bytes < must3r_hip_augment_color_scratch_bytes(a->V, a->Hs, a->Ws)) return "scratch is smaller than must3r_hip_augment_color_scratch_bytes";
    if (a->src_elems <= 0) return "src_elems must be positive";
    tab.resize((size_t)a->V);
    any_contrast = false;
    for (int i = 0; i < a->V; ++i) {
        const must3r_hip_augment_color_view& s = a->views[i];
        ColorDev& d = tab[(size_t)i];
        if (const char* e = stored_error(s.portrait, s.h, s.w, a->Hs, a->Ws)) return e;
        if (s.src_offset < 0 || s.src_offset > a->src_elems - 3LL * s.h * s.w) return "a view's planes do not lie inside src";
        unsigned seen = 0;
        for (int k = 0; k < 4; ++k) {
            if (s.order[k] < 0 || s.order[k] > 3 || (seen >> s.order[k] & 1u)) return "bad order: a view's order must be a permutation of 0 .. 3";
            seen |= 1u << s.order[k];
            if (s.apply[k] != 0 && s.apply[k] != 1) return "bad flags: a view's apply flags must be 0 or 1";
            if (!std::isfinite(s.factor[k])) return "a view's factors must be finite";
        }
        if (s.apply[MUST3R_AUG_HUE] && !(s.factor[MUST3R_AUG_HUE] >= -0.5f && s.factor[MUST3R_AUG_HUE] <= 0.5f)) return "a view's hue factor must be in [-0.5, 0.5]";
        d.src_offset = s.src_offset; d.h = s.h; d.w = s.w; d.portrait = s.portrait;
        d.nops = 0; d.ops = 0; d.contrast_at = -1;
        for (int k = 0; k < 4; ++k) {
            const int op = s.order[k];
            if (!s.apply[op]) continue;
            if (op == MUST3R_AUG_CONTRAST) d.contrast_at = d.nops;
            d.ops |= op << (2 * d.nops++);
        }
        any_contrast = any_contrast || d.contrast_at >= 0;
        d.fb = s.factor[MUST3R_AUG_BRIGHTNESS]; d.fc = s.factor[MUST3R_AUG_CONTRAST]; d.fs = s.factor[MUST3R_AUG_SATURATION];
        const int sh = (int)std::trunc((double)s.factor[MUST3R_AUG_HUE] * 255.0) % 256;
        d.shift = s.apply[MUST3R_AUG_HUE] ? (sh + 256) % 256 : 0;
    }
    return nullptr;
}

const char* depth_plan(const must3r_hip_augment_depth_args* a, std::vector<DepthDev>& tab) {
    if (!a->views || !a->out || !a->scratch) return "null argument (views, out, scratch)";
    if (a->depth_u16 != 0 && a->depth_u16 != 1) return "bad flags: depth_u16 must be 0 or 1";
    if (const char* e = shape_error(a->V, a->Hs, a->Ws)) return e;
    const uintptr_t mask = a->depth_u16 ? 1 : 3;
    if (off(a->out, mask)) return "out must be aligned to its element";
    if (off(a->scratch, 255)) return "scratch must be 256-byte aligned";
    if (a->scratch_bytes < must3r_hip_augment_depth_scratch_bytes(a->V)) return "scratch is smaller than must3r_hip_augment_depth_scratch_bytes";
    tab.resize((size_t)a->V);
    for (int i = 0; i < a->V; ++i) {
        const must3r_hip_augment_depth_view& s = a->views[i];
        DepthDev& d = tab[(size_t)i];
        if (!s.src) return "null argument (a view's src)";
        if (off(s.src, mask)) return "a view's src must be aligned to its element";
        if (const char* e = stored_error(s.portrait, s.out_h, s.out_w, a->Hs, a->Ws)) return e;
        if (s.H <= 0 || s.W <= 0 || s.row_stride < s.W) return "a view's source size must be positive and its row stride at least W";
        if (s.crop_x < 0 || s.crop_y < 0 || s.crop_w <= 0 || s.crop_h <= 0 || s.crop_x > s.W - s.crop_w || s.crop_y > s.H - s.crop_h)
            return "a view's crop does not lie inside its source";
        if (s.resize_w <= 0 || s.resize_h <= 0) return "a view's resize must be positive";
        if (s.win_x < 0 || s.win_y < 0 || s.win_x > s.resize_w - s.out_w || s.win_y > s.resize_h - s.out_h) return "a view's window does not lie inside its resize";
        d.src = s.src; d.row_stride = s.row_stride;
        d.rx = (double)s.crop_w / (double)s.resize_w; d.ry = (double)s.crop_h / (double)s.resize_h;
        d.l1 = s.crop_x; d.t1 = s.crop_y; d.W1 = s.crop_w; d.H1 = s.crop_h;
        d.l = s.win_x; d.t = s.win_y; d.w = s.out_w; d.h = s.out_h;
        d.portrait = s.portrait; d.pad = 0;
    }
    return nullptr;
}

// the pinned ring of the table uploads (train_optim.hip's opt_upload, image.hip's staging): with one buffer a second call would wait on the host for the
// first call's copy, which is queued behind everything the stream still has to do
struct AugPin {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
};
constexpr int kAugPinSlots = 4;
thread_local AugPin aug_pins[kAugPinSlots];
thread_local int aug_pin_next = 0;

int aug_upload(const void* table, const size_t bytes, void* scratch, hipStream_t s, const char* who) {
    AugPin& pin = aug_pins[aug_pin_next];
    aug_pin_next = (aug_pin_next + 1) % kAugPinSlots;
    if (pin.ev) {
        if (hipEventSynchronize(pin.ev) != hipSuccess) return fail("%s: waiting for the previous table upload failed", who);
        (void)hipEventDestroy(pin.ev);
        pin.ev = nullptr;
    }
    if (pin.cap < bytes) {
        if (pin.host) (void)hipHostFree(pin.host);
        pin.host = nullptr; pin.cap = 0;
        if (hipHostMalloc(&pin.host, bytes, hipHostMallocDefault) != hipSuccess) { pin.host = nullptr; return fail("%s: no pinned memory for the table", who); }
        pin.cap = bytes;
    }
    memcpy(pin.host, table, bytes);
    if (hipMemcpyAsync(scratch, pin.host, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("%s: the table upload failed", who);
    if (hipEventCreateWithFlags(&pin.ev, hipEventDisableTiming) != hipSuccess) { pin.ev = nullptr; return fail("%s: no event", who); }
    if (hipEventRecord(pin.ev, s) != hipSuccess) return fail("%s: no event", who);
    return 0;
}

}  // namespace
}  // namespace m3r
using namespace m3r;

extern "C" size_t must3r_hip_augment_color_scratch_bytes(int V, int Hs, int Ws) {
    if (const char* e = shape_error(V, Hs, Ws)) { fail("augment_color_scratch_bytes: %s", e); return 0; }
    return up256((size_t)V * sizeof(ColorDev)) + up256((size_t)V * tiles_of(Hs) * tiles_of(Ws) * sizeof(uint32_t));
}

extern "C" int must3r_hip_augment_color(const must3r_hip_augment_color_args* a) {
    const char* who = "augment_color";
    if (!a) return fail("%s: null argument", who);
    std::vector<ColorDev> tab;
    bool any_contrast = false;
    if (const char* e = color_plan(a, tab, any_contrast)) return fail("%s: %s", who, e);
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (int rc = aug_upload(tab.data(), tab.size() * sizeof(ColorDev), a->scratch, stream, who)) return rc;
    ColorArgs p{};
    p.src = a->src; p.views = static_cast<const ColorDev*>(a->scratch);
    p.partial = reinterpret_cast<uint32_t*>(static_cast<char*>(a->scratch) + up256((size_t)a->V * sizeof(ColorDev)));
    p.out = a->out; p.Hs = a->Hs; p.Ws = a->Ws;
    const dim3 grid(tiles_of(a->Ws), tiles_of(a->Hs), (unsigned)a->V);
    if (any_contrast) {
        hipLaunchKernelGGL(augment_color_kernel<true>, grid, dim3(AUG_T), 0, stream, p);
        if (hipGetLastError() != hipSuccess) return fail("%s: launch failed (sums)", who);
    }
    hipLaunchKernelGGL(augment_color_kernel<false>, grid, dim3(AUG_T), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}

extern "C" size_t must3r_hip_augment_depth_scratch_bytes(int V) {
    if (V <= 0 || V > 65535) { fail("augment_depth_scratch_bytes: V must be in 1 .. 65535"); return 0; }
    return up256((size_t)V * sizeof(DepthDev));
}

extern "C" int must3r_hip_augment_depth(const must3r_hip_augment_depth_args* a) {
    const char* who = "augment_depth";
    if (!a) return fail("%s: null argument", who);
    std::vector<DepthDev> tab;
    if (const char* e = depth_plan(a, tab)) return fail("%s: %s", who, e);
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (int rc = aug_upload(tab.data(), tab.size() * sizeof(DepthDev), a->scratch, stream, who)) return rc;
    DepthArgs p{};
    p.views = static_cast<const DepthDev*>(a->scratch); p.out = a->out; p.Hs = a->Hs; p.Ws = a->Ws;
    const dim3 grid(tiles_of(a->Ws), tiles_of(a->Hs), (unsigned)a->V);
    if (a->depth_u16) hipLaunchKernelGGL(augment_depth_kernel<unsigned short>, grid, dim3(AUG_T), 0, stream, p);
    else hipLaunchKernelGGL(augment_depth_kernel<uint32_t>, grid, dim3(AUG_T), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
    return 0;
}
