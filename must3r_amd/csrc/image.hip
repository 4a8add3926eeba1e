// Image ingestion (include/must3r_hip.h, ABI 9): the reference's image loaders -- must3r/demo/inference.py:63-76 load_images with
// must3r/tools/image.py:55-97 get_resize_function, and must3r/slam/model.py:99-120 preproc_frame -- as one separable, batched resampler.
// uint8 RGB rows are uploaded as they are (a quarter of the bytes of the fp32 tensor the reference builds on the host) and the
// normalised fp32 NCHW model input is written straight into HBM.
//
//   resample_h_kernel<PIL>   one block = one source row x 256 output columns of one image (blockIdx.y).  The row segment the
//                            block's taps read is staged through LDS with 16-byte loads (uint8 RGB rows are 3-byte strided; a
//                            byte load per lane and tap would issue 3 x taps loads per pixel), in chunks of RS_LDS bytes when the
//                            segment is longer (huge shrink factors).  Every lane then sums its own taps in ascending order.
//                            Writes the intermediate [C][rows][ld]: fp32 (AA / NEAREST) or clip8'd uint8 (PIL).
//   resample_v_kernel<PIL>   one wave = one output row x 256 columns (4 per lane, 16- / 4-byte loads of the intermediate); the
//                            row's weights are wave-uniform (scalar loads).  Writes fp32 planes [C][out_h][out_w].
//
// Coefficients are built on the host in double / float exactly as the replaced library does (Pillow's precompute_coeffs +
// normalize_coeffs_8bpc; ATen's antialiased _compute_indices_min_size_weights_aa; ATen's nearest-exact source index), so that
// the integer path is bit-exact with Pillow and the fp32 paths sum the same products in the same order as torch on the CPU.
// An axis whose size does not change gets one tap of weight 1 per output (the replaced libraries skip that pass; a tap of
// weight 1 << 22 or 1.0f is an exact copy, clip8 included).
//
// Bandwidth-bound: source bytes + intermediate (written once, read once) + output bytes over ~6.3 TB/s.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "abi.hpp"
#include "common.hpp"

namespace m3r {

constexpr int RS_T = 256;        // threads per block (both passes)
constexpr int RS_LDS = 16384;    // staging bytes of the horizontal pass
constexpr int RS_VCOLS = 256;    // output columns per wave of the vertical pass (4 per lane)
constexpr int PREC = 22;         // Pillow PRECISION_BITS (32 - 8 - 2)

// per-image launch descriptor (built on the host, uploaded into the scratch)
struct ImgDev {
    const unsigned char* src;
    long long row_stride;        // bytes between source rows
    long long plane_stride;      // bytes between source planes (F32_CHW)
    float* out;                  // this image's [C][out_h][out_w]
    long long tmp;               // byte offset of the intermediate [C][rows][ld] in the scratch
    int fmt, C;
    int crop_y, crop_x;
    int out_y, out_x, out_h, out_w;
    int resize_w;
    int xb, xw, yb, yw, ky;      // int32-word offsets of the coefficient arrays; x weights transposed [kx][resize_w], y weights [resize_h][ky]
    int y_first, rows;           // crop rows [y_first, y_first + rows) feed the vertical pass
    int ld;                      // intermediate row stride in elements (multiple of 16)
    int tiles_h, tiles_v;        // horizontal blocks per row, vertical column tiles per row
};

// ------------------------------------------------------------------------------------------------------------------------------
// coefficients (host)
// ------------------------------------------------------------------------------------------------------------------------------
static double pil_bicubic(double x) {   // Pillow Resample.c bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double pil_lanczos(double x) {   // Pillow Resample.c lanczos_filter (truncated sinc, support 3)
    if (-3.0 <= x && x < 3.0) return pil_sinc(x) * pil_sinc(x / 3);
    return 0.0;
}

static int ksize_of(int mode, int in, int out) {
    if (in == out || mode == MUST3R_RESAMPLE_NEAREST_EXACT) return 1;
    if (mode == MUST3R_RESAMPLE_AA_BILINEAR) {
        const float scale = (float)in / (float)out;
        const float support = scale >= 1.0f ? (float)((2 * 0.5) * scale) : (float)(2 * 0.5);
        return (int)std::ceil(support) * 2 + 1;
    }
    const double filterscale = std::max((double)((float)in - 0.0f) / out, 1.0);
    const double support = (mode == MUST3R_RESAMPLE_PIL_LANCZOS ? 3.0 : 2.0) * filterscale;
    return (int)std::ceil(support) * 2 + 1;
}

// bounds [out][2] = (first tap, taps), weights [out][ksize] (int32 for the PIL modes, fp32 otherwise); unused taps are 0
static void build_coeffs(int mode, int in, int out, int ksize, int32_t* bounds, void* weights) {
    int32_t* wi = static_cast<int32_t*>(weights);
    float* wf = static_cast<float*>(weights);
    const bool pil = mode == MUST3R_RESAMPLE_PIL_LANCZOS || mode == MUST3R_RESAMPLE_PIL_BICUBIC;
    std::memset(weights, 0, (size_t)out * ksize * 4);
    if (in == out) {   // the replaced libraries skip this axis; one tap of weight 1 is an exact copy
        for (int i = 0; i < out; ++i) {
            bounds[2 * i] = i;
            bounds[2 * i + 1] = 1;
            if (pil) wi[(size_t)i * ksize] = 1 << PREC; else wf[(size_t)i * ksize] = 1.0f;
        }
        return;
    }
    if (mode == MUST3R_RESAMPLE_NEAREST_EXACT) {
        // ATen nearest_neighbor_exact_compute_source_index: min(floorf((dst + 0.5) * scale), in - 1), scale = (float)in / out
        const float scale = (float)in / (float)out;
        for (int i = 0; i < out; ++i) {
            const long long s = (long long)floorf((float)((i + 0.5) * scale));
            bounds[2 * i] = (int32_t)std::min(s, (long long)in - 1);
            bounds[2 * i + 1] = 1;
            wf[(size_t)i * ksize] = 1.0f;
        }
        return;
    }
    if (mode == MUST3R_RESAMPLE_AA_BILINEAR) {
        // ATen UpSampleKernel.cpp, HelperInterpLinear with antialias: _compute_indices_min_size_weights_aa in opmath (float),
        // with its float / double promotions kept (scale * (i + 0.5) and (j + xmin - center + 0.5) * invscale are double expressions)
        const float scale = (float)in / (float)out;
        const float support = scale >= 1.0f ? (float)((2 * 0.5) * scale) : (float)(2 * 0.5);
        const float invscale = scale >= 1.0f ? (float)(1.0 / scale) : 1.0f;
        const long long maxk = (long long)std::ceil(support) * 2 + 1;
        for (int i = 0; i < out; ++i) {
            const float center = (float)(scale * (i + 0.5));
            const long long xmin = std::max((long long)(center - support + 0.5), 0LL);
            long long xsize = std::min((long long)(center + support + 0.5), (long long)in) - xmin;
            xsize = std::min(std::max(xsize, 0LL), std::min(maxk, (long long)ksize));
            float* w = wf + (size_t)i * ksize;
            float total = 0.0f;
            for (long long j = 0; j < xsize; ++j) {
                float x = (float)(((float)(j + xmin) - center + 0.5) * invscale);
                x = std::fabs(x);
                const float v = x < 1.0f ? (float)(1.0 - x) : 0.0f;
                w[j] = v;
                total += v;
            }
            if (total != 0.0f)
                for (long long j = 0; j < xsize; ++j) w[j] /= total;
            bounds[2 * i] = (int32_t)xmin;
            bounds[2 * i + 1] = (int32_t)xsize;
        }
        return;
    }
    // Pillow Resample.c precompute_coeffs (box = (0, in)) + normalize_coeffs_8bpc
    double (*filter)(double) = mode == MUST3R_RESAMPLE_PIL_LANCZOS ? pil_lanczos : pil_bicubic;
    const double fsupport = mode == MUST3R_RESAMPLE_PIL_LANCZOS ? 3.0 : 2.0;
    const float in0 = 0.0f, in1 = (float)in;
    const double scale = (double)(in1 - in0) / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = fsupport * filterscale;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = 0; x < xmax; ++x)
            wi[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PREC)) : (int)(0.5 + k[x] * (1 << PREC));
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------------------
template <bool PIL>
__global__ void __launch_bounds__(RS_T) resample_h_kernel(const ImgDev* __restrict__ descs, const float* __restrict__ tab,
                                                          const int* __restrict__ coef, unsigned char* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[RS_LDS];
    __shared__ float ltab[256];
    const ImgDev& d = descs[blockIdx.y];
    const int nblk = d.rows * d.tiles_h;
    if ((int)blockIdx.x >= nblk) return;               // block-uniform, before any barrier
    const int r = blockIdx.x / d.tiles_h, t = blockIdx.x - r * d.tiles_h;
    const int j0 = t * RS_T, jn = min(RS_T, d.out_w - j0);
    const int C = d.C;
    const bool u8 = d.fmt == MUST3R_IMG_U8_HWC;
    const int* xb = coef + d.xb;
    const int i_first = d.out_x + j0, i_last = d.out_x + j0 + jn - 1;
    const int lo = xb[2 * i_first], hi = xb[2 * i_last] + xb[2 * i_last + 1];
    const int j = threadIdx.x;
    const bool active = j < jn;
    const int i = d.out_x + j0 + (active ? j : 0);
    const int xmin = xb[2 * i], n = active ? xb[2 * i + 1] : 0;
    if (!PIL && u8) ltab[threadIdx.x] = tab[threadIdx.x];   // RS_T == 256
    float accf[4] = {0.f, 0.f, 0.f, 0.f};
    int acci[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    const unsigned char* row = d.src + (long long)(d.crop_y + d.y_first + r) * d.row_stride;
    // chunk length in pixels: uint8 rows need <= px * C + 30 staged bytes; fp32 planes px + 6 floats each (16-byte alignment slop)
    const int CHP = u8 ? (RS_LDS - 32) / C : ((RS_LDS / 4 / C - 8) & ~3);
    const int PL = CHP + 8;                             // fp32: floats per staged plane
    const int* wt = coef + d.xw;                        // transposed [k][resize_w]
    for (int c0 = lo; c0 < hi; c0 += CHP) {
        const int c1 = min(c0 + CHP, hi);
        __syncthreads();                                // the previous chunk has been consumed
        int shift[4] = {0, 0, 0, 0};
        if (u8) {
            const unsigned char* b_lo = row + (long long)(d.crop_x + c0) * C;
            const unsigned char* b_hi = row + (long long)(d.crop_x + c1) * C;
            // 16-byte aligned loads that hold at least one byte of the segment: such a load never leaves the segment's pages
            const unsigned char* a_lo = (const unsigned char*)((uintptr_t)b_lo & ~(uintptr_t)15);
            const int nv = (int)((b_hi - a_lo + 15) >> 4);
            for (int v = threadIdx.x; v < nv; v += RS_T)
                *reinterpret_cast<u32x4*>(stage + 16 * v) = *reinterpret_cast<const u32x4*>(a_lo + 16 * v);
            shift[0] = (int)(b_lo - a_lo);
        } else {
            for (int c = 0; c < C; ++c) {
                const float* b_lo = reinterpret_cast<const float*>(row + c * d.plane_stride) + d.crop_x + c0;
                const float* b_hi = b_lo + (c1 - c0);
                const float* a_lo = (const float*)((uintptr_t)b_lo & ~(uintptr_t)15);
                const int nv = (int)((b_hi - a_lo + 3) >> 2);
                float* dst = reinterpret_cast<float*>(stage) + c * PL;
                for (int v = threadIdx.x; v < nv; v += RS_T)
                    *reinterpret_cast<f32x4*>(dst + 4 * v) = *reinterpret_cast<const f32x4*>(a_lo + 4 * v);
                shift[c] = (int)(b_lo - a_lo);
            }
        }
        __syncthreads();
        const int kb = max(c0 - xmin, 0), ke = min(c1 - xmin, n);
        for (int k = kb; k < ke; ++k) {
            const int x = xmin + k - c0;                // pixel within the chunk
            if (PIL) {
                const int w = wt[(size_t)k * d.resize_w + i];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) acci[c] += (int)stage[shift[0] + x * C + c] * w;
            } else {
                const float w = __int_as_float(wt[(size_t)k * d.resize_w + i]);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) {
                        const float v = u8 ? ltab[stage[shift[0] + x * C + c]] : reinterpret_cast<const float*>(stage)[c * PL + shift[c] + x];
                        accf[c] += v * w;
                    }
            }
        }
    }
    if (!active) return;
    const long long plane = (long long)d.rows * d.ld;
    const long long o = (long long)r * d.ld + j0 + j;
    if (PIL) {
        unsigned char* tmp = scratch + d.tmp;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) tmp[c * plane + o] = (unsigned char)min(max(acci[c] >> PREC, 0), 255);   // clip8
    } else {
        float* tmp = reinterpret_cast<float*>(scratch + d.tmp);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) tmp[c * plane + o] = accf[c];
    }
}

template <bool PIL>
__global__ void __launch_bounds__(RS_T) resample_v_kernel(const ImgDev* __restrict__ descs, const float* __restrict__ tab,
                                                          const int* __restrict__ coef, const unsigned char* __restrict__ scratch) {
    const ImgDev& d = descs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int unit = blockIdx.x * (RS_T / 64) + wave;   // (output row, column tile), one per wave
    if (unit >= d.out_h * d.tiles_v) return;
    const int orow = unit / d.tiles_v, t = unit - orow * d.tiles_v;
    const int j = t * RS_VCOLS + lane * 4;
    if (j >= d.out_w) return;
    const int i = d.out_y + orow;
    const int* yb = coef + d.yb;
    const int ymin = yb[2 * i] - d.y_first, n = yb[2 * i + 1];
    const int* wrow = coef + d.yw + (size_t)i * d.ky;
    const long long plane = (long long)d.rows * d.ld;
    const long long out_plane = (long long)d.out_h * d.out_w;
    const bool vec = (d.out_w & 3) == 0 && ((uintptr_t)d.out & 15) == 0 && j + 4 <= d.out_w;
    for (int c = 0; c < d.C; ++c) {
        float v[4];
        if (PIL) {
            const unsigned char* src = scratch + d.tmp + c * plane + (long long)ymin * d.ld + j;
            int acc[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
            for (int k = 0; k < n; ++k) {
                const unsigned p = *reinterpret_cast<const unsigned*>(src + (long long)k * d.ld);
                const int w = wrow[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (int)((p >> (8 * e)) & 255u) * w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = tab[min(max(acc[e] >> PREC, 0), 255)];   // clip8, then ToTensor + Normalize
        } else {
            const float* src = reinterpret_cast<const float*>(scratch + d.tmp) + c * plane + (long long)ymin * d.ld + j;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < n; ++k) {
                const f32x4 p = *reinterpret_cast<const f32x4*>(src + (long long)k * d.ld);
                const float w = __int_as_float(wrow[k]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += p[e] * w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[e];
        }
        float* o = d.out + c * out_plane + (long long)orow * d.out_w + j;
        if (vec) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < d.out_w) o[e] = v[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host: plan (scratch layout) and launch
// ------------------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct ResamplePlan {
    std::vector<unsigned char> host;   // [table 1 KiB | descriptors | coefficients], uploaded as one copy
    size_t desc_off = 0, coef_off = 0, tmp_off = 0, total = 0;
    int max_blocks_h = 0, max_blocks_v = 0;
};

// Coefficients of the axes this thread has resampled lately: a stream of frames of one size builds its LANCZOS tables (double precision,
// sin per tap) once, not once per call.
struct CoefEntry {
    std::vector<int32_t> words;   // bounds [out][2], then weights [out][ksize]
    int ksize;
};
static const CoefEntry& cached_coeffs(int mode, int in, int out) {
    static thread_local std::map<std::tuple<int, int, int>, CoefEntry> cache;
    const auto key = std::make_tuple(mode, in, out);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() >= 256) cache.clear();   // bounded: a folder of many different sizes does not grow it without end
    CoefEntry e;
    e.ksize = ksize_of(mode, in, out);
    e.words.resize((size_t)out * (2 + e.ksize));
    build_coeffs(mode, in, out, e.ksize, e.words.data(), e.words.data() + 2 * (size_t)out);
    return cache.emplace(key, std::move(e)).first->second;
}

// Pinned host staging for the table upload, a ring of slots per thread (as the forwards' view tables, model.hip upload_table): the copy is
// asynchronous, so the call does not wait for the work already queued on the stream; a slot is reused once the copy out of it has completed
// (its event).  A slot grows to the largest upload it has carried and is bound to the device that was current when it was allocated.
struct StageSlot {
    void* pin = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int dev = -1;
    bool used = false;
};
constexpr int kStageSlots = 4;

static int stage_upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    static thread_local StageSlot slots[kStageSlots];
    static thread_local int next = 0;
    StageSlot& slot = slots[next];
    next = (next + 1) % kStageSlots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail("resample: hipGetDevice failed");
    if (slot.used && hipEventSynchronize(slot.ev) != hipSuccess) return fail("resample: staging event wait failed");
    slot.used = false;
    if (slot.dev != dev || slot.cap < bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        if (slot.ev) (void)hipEventDestroy(slot.ev);
        slot.pin = nullptr;
        slot.ev = nullptr;
        slot.cap = 0;
        slot.dev = -1;
        const size_t cap = std::max(bytes, (size_t)1 << 16);
        if (hipHostMalloc(&slot.pin, cap) != hipSuccess) { slot.pin = nullptr; return fail("resample: pinned staging allocation failed"); }
        if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) != hipSuccess) { slot.ev = nullptr; return fail("resample: event creation failed"); }
        slot.cap = cap;
        slot.dev = dev;
    }
    std::memcpy(slot.pin, src, bytes);
    if (hipMemcpyAsync(dst, slot.pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("resample: table upload failed");
    if (hipEventRecord(slot.ev, s) != hipSuccess) return fail("resample: staging event record failed");
    slot.used = true;
    return 0;
}

static int plan_resample(int mode, const must3r_hip_image_desc* ds, int n, float* out, ResamplePlan& P) {
    if (mode < MUST3R_RESAMPLE_AA_BILINEAR || mode > MUST3R_RESAMPLE_NEAREST_EXACT) return fail("resample: unknown mode %d", mode);
    if (n < 0 || n > 65535) return fail("resample: %d images (0 ... 65535 per call)", n);
    const bool pil = mode == MUST3R_RESAMPLE_PIL_LANCZOS || mode == MUST3R_RESAMPLE_PIL_BICUBIC;
    // coefficient arrays, one per distinct (in, out) axis; words: bounds 2 x out, then weights ksize x out
    std::map<std::pair<int, int>, std::pair<int, int>> axes;   // (in, out) -> (word offset, ksize)
    std::vector<int32_t> coef;
    auto axis = [&](int in, int outsz) -> std::pair<int, int> {
        auto it = axes.find({in, outsz});
        if (it != axes.end()) return it->second;
        const CoefEntry& e = cached_coeffs(mode, in, outsz);
        const int off = (int)coef.size();
        const int k = e.ksize;
        coef.insert(coef.end(), e.words.begin(), e.words.end());
        axes[{in, outsz}] = {off, k};
        return {off, k};
    };
    std::vector<ImgDev> dev(n);
    std::map<int, int> xt;          // x array offset -> offset of its transposed weights
    size_t tmp_bytes = 0;
    for (int m = 0; m < n; ++m) {
        const must3r_hip_image_desc& s = ds[m];
        if (!s.src) return fail("resample: image %d has no source", m);
        if (s.src_format != MUST3R_IMG_U8_HWC && s.src_format != MUST3R_IMG_F32_CHW) return fail("resample: image %d: unknown source format %d", m, s.src_format);
        if (pil && s.src_format != MUST3R_IMG_U8_HWC) return fail("resample: image %d: the PIL modes resample uint8 images (MUST3R_IMG_U8_HWC)", m);
        if (s.channels < 1 || s.channels > 4) return fail("resample: image %d: %d channels (1 ... 4)", m, s.channels);
        if (s.H <= 0 || s.W <= 0) return fail("resample: image %d is empty (%d rows)", m, s.H);
        if (s.crop_h <= 0 || s.crop_w <= 0 || s.crop_y < 0 || s.crop_x < 0 || s.crop_y + s.crop_h > s.H || s.crop_x + s.crop_w > s.W)
            return fail("resample: image %d: crop box outside the %d-row source", m, s.H);
        if (s.resize_h <= 0 || s.resize_w <= 0) return fail("resample: image %d: empty target size", m);
        if (s.out_h <= 0 || s.out_w <= 0 || s.out_y < 0 || s.out_x < 0 || s.out_y + s.out_h > s.resize_h || s.out_x + s.out_w > s.resize_w)
            return fail("resample: image %d: output window outside the %d-row resampled image", m, s.resize_h);
        if (s.out_offset < 0) return fail("resample: image %d: negative output offset", m);
        const long long esz = s.src_format == MUST3R_IMG_U8_HWC ? 1 : 4;
        if (s.src_format == MUST3R_IMG_U8_HWC) {
            if (s.row_stride < (long long)s.W * s.channels) return fail("resample: image %d: row stride below W x channels bytes", m);
        } else {
            if (((uintptr_t)s.src & 3) != 0) return fail("resample: image %d: fp32 source not 4-byte aligned", m);
            if (s.row_stride < s.W) return fail("resample: image %d: row stride below W elements", m);
            if (s.channels > 1 && s.plane_stride < (long long)(s.H - 1) * s.row_stride + s.W) return fail("resample: image %d: plane stride too small", m);
        }
        const std::pair<int, int> X = axis(s.crop_w, s.resize_w), Y = axis(s.crop_h, s.resize_h);
        ImgDev& d = dev[m];
        d.src = static_cast<const unsigned char*>(s.src);
        d.row_stride = s.row_stride * esz;
        d.plane_stride = s.plane_stride * esz;
        d.out = out ? out + s.out_offset : nullptr;
        d.fmt = s.src_format;
        d.C = s.channels;
        d.crop_y = s.crop_y; d.crop_x = s.crop_x;
        d.out_y = s.out_y; d.out_x = s.out_x; d.out_h = s.out_h; d.out_w = s.out_w;
        d.resize_w = s.resize_w;
        d.xb = X.first;
        d.yb = Y.first; d.yw = Y.first + 2 * s.resize_h; d.ky = Y.second;
        auto t = xt.find(X.first);
        if (t == xt.end()) {   // transposed copy [k][resize_w] of the x weights: lane i reads consecutive words
            const int off = (int)coef.size();
            coef.resize(coef.size() + (size_t)X.second * s.resize_w);
            const int32_t* w = coef.data() + X.first + 2 * (size_t)s.resize_w;
            for (int i = 0; i < s.resize_w; ++i)
                for (int k = 0; k < X.second; ++k) coef[off + (size_t)k * s.resize_w + i] = w[(size_t)i * X.second + k];
            t = xt.emplace(X.first, off).first;
        }
        d.xw = t->second;
        // the crop rows the vertical pass reads for the output window (bounds are monotone; min / max all the same)
        const int32_t* yb = coef.data() + Y.first;
        int first = yb[2 * s.out_y], end = first + 1;
        for (int i = s.out_y; i < s.out_y + s.out_h; ++i) {
            first = std::min(first, (int)yb[2 * i]);
            end = std::max(end, (int)(yb[2 * i] + yb[2 * i + 1]));
        }
        d.y_first = first;
        d.rows = end - first;
        d.ld = (s.out_w + 15) & ~15;
        d.tmp = (long long)tmp_bytes;
        tmp_bytes += up256((size_t)s.channels * d.rows * d.ld * (pil ? 1 : 4));
        d.tiles_h = (s.out_w + RS_T - 1) / RS_T;
        d.tiles_v = (s.out_w + RS_VCOLS - 1) / RS_VCOLS;
        const long long bh = (long long)d.rows * d.tiles_h, bv = ((long long)s.out_h * d.tiles_v + RS_T / 64 - 1) / (RS_T / 64);
        if (bh > 0x7fffffffLL || bv > 0x7fffffffLL) return fail("resample: image %d too large", m);
        P.max_blocks_h = std::max(P.max_blocks_h, (int)bh);
        P.max_blocks_v = std::max(P.max_blocks_v, (int)bv);
    }
    if (coef.size() > 0x7fffffffULL) return fail("resample: coefficient tables too large");
    P.desc_off = 1024;
    P.coef_off = up256(P.desc_off + sizeof(ImgDev) * n);
    P.tmp_off = up256(P.coef_off + coef.size() * 4);
    P.total = P.tmp_off + tmp_bytes;
    P.host.assign(P.tmp_off, 0);
    float* tab = reinterpret_cast<float*>(P.host.data());
    for (int u = 0; u < 256; ++u) tab[u] = ((float)u / 255.0f - 0.5f) / 0.5f;   // ToTensor (x / 255) then Normalize(0.5, 0.5), fp32
    if (n) std::memcpy(P.host.data() + P.desc_off, dev.data(), sizeof(ImgDev) * n);
    if (!coef.empty()) std::memcpy(P.host.data() + P.coef_off, coef.data(), coef.size() * 4);
    // the device descriptors point into the scratch: fix up the intermediate offsets relative to the scratch base
    ImgDev* hd = reinterpret_cast<ImgDev*>(P.host.data() + P.desc_off);
    for (int m = 0; m < n; ++m) hd[m].tmp += (long long)P.tmp_off;
    return 0;
}

}  // namespace m3r
using namespace m3r;

extern "C" int must3r_hip_resample_coeffs(int mode, int in, int out, int* ksize, int32_t* bounds, void* weights) {
    if (mode < MUST3R_RESAMPLE_AA_BILINEAR || mode > MUST3R_RESAMPLE_NEAREST_EXACT) return fail("resample_coeffs: unknown mode");
    if (in <= 0 || out <= 0) return fail("resample_coeffs: sizes must be positive");
    const int k = ksize_of(mode, in, out);
    if (ksize) *ksize = k;
    if (bounds && weights) build_coeffs(mode, in, out, k, bounds, weights);
    else if (bounds || weights) return fail("resample_coeffs: pass both bounds and weights, or neither (ksize query)");
    return 0;
}

extern "C" size_t must3r_hip_image_scratch_bytes(int mode, const must3r_hip_image_desc* descs, int n) {
    ResamplePlan P;
    if (n <= 0 || !descs || plan_resample(mode, descs, n, nullptr, P)) return 0;
    return P.total;
}

extern "C" int must3r_hip_resample(int mode, const must3r_hip_image_desc* descs, int n, float* out, void* scratch, size_t scratch_bytes,
                                   void* stream) {
    if (n < 0) return fail("resample: negative image count");
    if (n == 0) return 0;
    if (!descs || !out) return fail("resample: null argument");
    ResamplePlan P;
    if (plan_resample(mode, descs, n, out, P)) return 1;
    if (!scratch) return fail("resample: null scratch");
    if (scratch_bytes < P.total) return fail("resample: scratch of %zu bytes < %zu (must3r_hip_image_scratch_bytes)", scratch_bytes, P.total);
    if (((uintptr_t)scratch & 255) != 0) return fail("resample: scratch must be 256-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stage_upload(scratch, P.host.data(), P.host.size(), s)) return 1;
    unsigned char* base = static_cast<unsigned char*>(scratch);
    const ImgDev* dd = reinterpret_cast<const ImgDev*>(base + P.desc_off);
    const float* tab = reinterpret_cast<const float*>(base);
    const int* coef = reinterpret_cast<const int*>(base + P.coef_off);
    const bool pil = mode == MUST3R_RESAMPLE_PIL_LANCZOS || mode == MUST3R_RESAMPLE_PIL_BICUBIC;
    const dim3 gh((unsigned)P.max_blocks_h, (unsigned)n), gv((unsigned)P.max_blocks_v, (unsigned)n);
    if (pil) {
        hipLaunchKernelGGL(resample_h_kernel<true>, gh, dim3(RS_T), 0, s, dd, tab, coef, base);
        hipLaunchKernelGGL(resample_v_kernel<true>, gv, dim3(RS_T), 0, s, dd, tab, coef, base);
    } else {
        hipLaunchKernelGGL(resample_h_kernel<false>, gh, dim3(RS_T), 0, s, dd, tab, coef, base);
        hipLaunchKernelGGL(resample_v_kernel<false>, gv, dim3(RS_T), 0, s, dd, tab, coef, base);
    }
    if (hipGetLastError() != hipSuccess) return fail("resample: launch failed");
    return 0;
}
