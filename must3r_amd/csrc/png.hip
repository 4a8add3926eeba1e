// PNG decoding on the device (include/must3r_hip.h "PNG decoding"): from the IDAT bytes of a file to pixels in the caller's layout.
//   png_inflate_kernel    RFC 1951.  A stream is serial: one workgroup of one wave per image, all of what it shares in LDS -- the 32 KiB history as a ring that
//                         goes to the scanline buffer in 16 KiB pieces with 16-byte stores, 2 KiB of the compressed stream staged with 16-byte loads (zeros
//                         beyond the end), the two decode tables.  The symbol is decoded wave-uniformly (png_inflate.hpp, the text a host program runs too); a
//                         match is read by all lanes, then written by all lanes, through the ring and barriers and never through global memory.
//   png_adler_kernel      Adler-32 of the inflated bytes as a parallel reduction, against the trailer the inflate read
//   png_unfilter_kernel   a wave takes 64 consecutive rows, lane k one byte behind lane k - 1: the byte above arrives by a lane shuffle, the bytes to the left
//                         and above left are the lane's own history.  rowbytes + 63 steps per 64 rows; the last row of a group reaches the next through the
//                         scanline buffer, behind a barrier.  In place.
//   png_pack_kernel       scanlines -> RGB (grey replicated, alpha dropped), uint8 grey or little-endian uint16 grey; 16 pixels a thread, 16-byte stores where
//                         the row is aligned
// Every launch covers the whole batch; the sizes follow from the headers, nothing is read back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "abi.hpp"
#include "png_inflate.hpp"
#include "png_parse.hpp"

namespace m3r {
namespace png {

constexpr int kT = 256;
constexpr uint32_t kStageWords = 512;   // 2 KiB of the compressed stream

struct ImgDev {
    const uint8_t* z;        // the zlib stream
    uint8_t* scan;           // the inflated scanlines: expected bytes, in a buffer of up256(expected) + 256
    uint8_t* out;
    long long out_stride;
    uint32_t zbytes, expected, rowbytes, height, width;
    int32_t bpp, out_format, pad;
};

// ---- inflate ---------------------------------------------------------------------------------------------------------------------------------------------
struct DevSrc {
    const uint8_t* z;
    uint32_t zbytes;
    uint32_t* stage;   // LDS [kStageWords]
    uint32_t w0;       // the first staged word; a multiple of 4
    // stage the kStageWords words from the 16-byte block of word i on: every lane of the workgroup calls it together
    __device__ __forceinline__ void restage(uint32_t i) {
        __syncthreads();
        w0 = i & ~3u;
        const uint4* z16 = reinterpret_cast<const uint4*>(z);
        for (uint32_t k = threadIdx.x; k < kStageWords / 4; k += 64u) {
            const uint32_t q = w0 / 4 + k;
            const uint64_t byte0 = (uint64_t)q * 16u;
            uint32_t w[4] = {0, 0, 0, 0};
            if (byte0 < zbytes) {
                const uint4 v = z16[q];
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                const uint32_t left = zbytes - (uint32_t)byte0;   // bytes of the block that belong to the stream
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t valid = left > 4 * j ? left - 4 * j : 0;
                    if (valid < 4) w[j] &= valid ? (1u << (8 * valid)) - 1u : 0u;
                }
            }
            reinterpret_cast<uint4*>(stage)[k] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if (i - w0 >= kStageWords) restage(i);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[(i - w0) & (kStageWords - 1)]);   // one address for the wave: the word is uniform
    }
};

struct DevCtx {
    uint8_t* ring;     // LDS [kWindow]
    Huff* tabs;        // LDS [2]
    uint8_t* lens_;    // LDS [kLensBytes]
    uint8_t* cl_;      // LDS [32]
    uint16_t* count_;  // LDS [16]
    const uint8_t* z;
    uint8_t* out;
    uint32_t flushed;  // a multiple of kFlushBytes

    __device__ __forceinline__ uint8_t* lens() { return lens_; }
    __device__ __forceinline__ uint8_t* code_lens() { return cl_; }
    __device__ __forceinline__ Huff* litlen() { return &tabs[0]; }
    __device__ __forceinline__ Huff* dist() { return &tabs[1]; }

    __device__ __forceinline__ int build(const uint8_t* lens, int n, bool is_code_lengths, Huff* h) {
        const uint32_t lane = threadIdx.x;
        __syncthreads();
        if (lane < 16) count_[lane] = lane ? (uint16_t)huff_count(lens, n, (int)lane) : (uint16_t)0;
        __syncthreads();
        const int bad = huff_offsets(count_, is_code_lengths, h);   // every lane writes the same values
        __syncthreads();
        if (bad) return 1;
        if (lane >= 1 && lane < 16) huff_fill_vals(lens, n, (int)lane, h);
        __syncthreads();
        for (uint32_t e = lane; e < (1u << kLookBits); e += 64u) h->look[e] = huff_look_entry(h, e);
        __syncthreads();
        return 0;
    }
    // ring bytes [from, from + n) -> the scanline buffer; from is a multiple of 16 and the buffer holds n rounded up to 16
    __device__ __forceinline__ void flush_piece(uint32_t from, uint32_t n) {
        __syncthreads();
        const uint4* r16 = reinterpret_cast<const uint4*>(ring);
        uint4* o16 = reinterpret_cast<uint4*>(out);
        for (uint32_t k = threadIdx.x; k < (n + 15u) / 16u; k += 64u) o16[from / 16u + k] = r16[(from / 16u + k) & (kWindow / 16u - 1u)];
        __syncthreads();
    }
    __device__ __forceinline__ void advance(uint32_t opos) {
        flushed = (uint32_t)__builtin_amdgcn_readfirstlane((int)flushed);
        for (int k = 0; k < 2 && opos - flushed >= kFlushBytes; ++k) {
            flush_piece(flushed, kFlushBytes);
            flushed += kFlushBytes;
        }
    }
    __device__ __forceinline__ void literal(uint32_t at, uint32_t b) {
        ring[at & kWindowMask] = (uint8_t)b;   // every lane the same byte
        advance(at + 1u);
    }
    __device__ __forceinline__ void match(uint32_t at, uint32_t len, uint32_t d) {
        const uint32_t lane = threadIdx.x;
        uint8_t v[5];
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = lane + 64u * k;
            v[k] = i < len ? ring[(at - d + periodic_index(i, d, len)) & kWindowMask] : (uint8_t)0;
        }
        __syncthreads();   // every source byte is read before any byte of the match is written: a distance near 32768 puts them in the same ring slots
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = lane + 64u * k;
            if (i < len) ring[(at + i) & kWindowMask] = v[k];
        }
        __syncthreads();
        advance(at + len);
    }
    __device__ __forceinline__ void stored(uint32_t at, uint32_t src, uint32_t n) {
        for (uint32_t off = 0; off < n; off += kStoredChunk) {
            const uint32_t m = n - off < kStoredChunk ? n - off : kStoredChunk;
            for (uint32_t i = threadIdx.x; i < m; i += 64u) ring[(at + off + i) & kWindowMask] = z[src + off + i];
            __syncthreads();
            advance(at + off + m);
        }
    }
    __device__ __forceinline__ void finish(uint32_t total) { flush_piece(flushed, total - flushed); }
};

__global__ __launch_bounds__(64) void png_inflate_kernel(const ImgDev* imgs, int32_t* status, uint32_t* trailers) {
    const ImgDev& I = imgs[blockIdx.x];
    __shared__ __attribute__((aligned(16))) uint8_t ring[kWindow];
    __shared__ __attribute__((aligned(16))) uint32_t stage[kStageWords];
    __shared__ Huff tabs[2];
    __shared__ uint8_t lens[kLensBytes], cl[32];
    __shared__ uint16_t count[16];
    static_assert(kWindow + 4 * kStageWords + 2 * sizeof(Huff) + kLensBytes + 32 + 32 < 40 * 1024, "four workgroups a CU");
    BitReader<DevSrc> br;
    br.src = DevSrc{I.z, I.zbytes, stage, 0};
    br.src.restage(0);
    br.bb = 0, br.bc = 0, br.next_w = 0, br.pos = 0;
    DevCtx ctx{ring, tabs, lens, cl, count, I.z, I.scan, 0};
    uint32_t trailer = 0;
    const int rc = inflate(br, I.zbytes, I.expected, ctx, nullptr, &trailer);
    if (threadIdx.x == 0) {
        status[blockIdx.x] = rc;
        trailers[blockIdx.x] = trailer;
    }
}

// ---- Adler-32 ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void png_adler_kernel(const ImgDev* imgs, int32_t* status, const uint32_t* trailers) {
    const ImgDev& I = imgs[blockIdx.x];
    if (status[blockIdx.x] != MUST3R_PNG_STATUS_OK) return;
    __shared__ uint32_t p1[kT], p2[kT];
    const uint32_t n = I.expected;
    const uint4* in16 = reinterpret_cast<const uint4*>(I.scan);
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t q = threadIdx.x; q < (n + 15u) / 16u; q += kT) {   // up to 2^28 / 16 / 256 blocks of 16 bytes a thread
        const uint4 v = in16[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = q * 16u + 4u * j;
            const uint32_t valid = i >= n ? 0u : (n - i < 4u ? n - i : 4u);
            adler_word(w[j], n - i, valid, s1, s2);
        }
    }
    p1[threadIdx.x] = (uint32_t)(s1 % kAdlerMod);
    p2[threadIdx.x] = (uint32_t)(s2 % kAdlerMod);
    __syncthreads();
    for (uint32_t off = kT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            p1[threadIdx.x] += p1[threadIdx.x + off];   // 256 x 65521 fits
            p2[threadIdx.x] += p2[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && adler_finish(p1[0], p2[0], n) != trailers[blockIdx.x]) status[blockIdx.x] = MUST3R_PNG_STATUS_ADLER;
}

// ---- the scanline filters ------------------------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t byte_of(uint64_t lo, uint64_t hi, uint32_t k) { return (uint32_t)(((k & 8u) ? hi : lo) >> (8u * (k & 7u))) & 255u; }

__global__ __launch_bounds__(64) void png_unfilter_kernel(const ImgDev* imgs, int32_t* status) {
    const ImgDev& I = imgs[blockIdx.x];
    uint8_t* scan = I.scan;
    const uint32_t lane = threadIdx.x, stride = I.rowbytes + 1u, rowbytes = I.rowbytes, H = I.height;
    const uint32_t hshift = 8u * (uint32_t)(I.bpp - 1);
    bool bad = false;
    for (uint32_t g0 = 0; g0 < H; g0 += 64u) {
        const uint32_t r = g0 + lane;
        const bool active = r < H;
        const uint32_t base = active ? r * stride : 0u;   // below 2^28
        uint32_t ft = active ? scan[base] : 0u;
        if (ft > 4u) {
            bad = true;
            ft = 0;
        }
        const uint32_t upbase = g0 ? (g0 - 1u) * stride + 1u : 0u;   // the row above lane 0's: the last of the group before, complete behind the barrier
        uint32_t a_hist = 0, b_hist = 0, prev = 0;   // the last bpp bytes of this row and of the row above; this lane's byte of the step before
        uint64_t lo = 0, hi = 0, ulo = 0, uhi = 0;
        const uint32_t steps = rowbytes + 63u;
        for (uint32_t t = 0; t < steps; ++t) {
            uint32_t up = (uint32_t)__shfl_up((int)prev, 1);   // lane k - 1 was at this lane's byte a step ago
            const uint32_t x = t - lane;
            if (active && t >= lane && x < rowbytes) {
                const uint32_t p = base + 1u + x;
                if (x == 0 || (p & 15u) == 0) {
                    const uint4 v = *reinterpret_cast<const uint4*>(scan + (p & ~15u));
                    lo = v.x | ((uint64_t)v.y << 32);
                    hi = v.z | ((uint64_t)v.w << 32);
                }
                const uint32_t raw = byte_of(lo, hi, p & 15u);
                if (lane == 0) {
                    up = 0;
                    if (g0) {
                        const uint32_t q = upbase + x;
                        if (x == 0 || (q & 15u) == 0) {
                            const uint4 v = *reinterpret_cast<const uint4*>(scan + (q & ~15u));
                            ulo = v.x | ((uint64_t)v.y << 32);
                            uhi = v.z | ((uint64_t)v.w << 32);
                        }
                        up = byte_of(ulo, uhi, q & 15u);
                    }
                }
                const uint32_t a = (a_hist >> hshift) & 255u, c = (b_hist >> hshift) & 255u;
                const uint32_t rec = unfilter_byte(ft, raw, a, up, c);
                scan[p] = (uint8_t)rec;
                a_hist = (a_hist << 8) | rec;
                b_hist = (b_hist << 8) | up;
                prev = rec;
            }
        }
        __syncthreads();
    }
    if (bad && status[blockIdx.x] == MUST3R_PNG_STATUS_OK) status[blockIdx.x] = MUST3R_PNG_STATUS_FILTER;
}

// ---- the caller's layout -------------------------------------------------------------------------------------------------------------------------------------
// 16 pixels of BPP bytes at src -> OB bytes a pixel: FMT RGB8 (BPP 1, 3, 4), GRAY8 (BPP 1) or GRAY16 (BPP 2, byte-swapped)
template <int BPP, int FMT>
__device__ inline void pack16(const uint8_t* src, uint8_t* dst, int npx) {
    constexpr int OB = FMT == MUST3R_PNG_OUT_RGB8 ? 3 : FMT == MUST3R_PNG_OUT_GRAY8 ? 1 : 2;
    constexpr int NW = 4 * BPP;
    const uint32_t sh = 8u * (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(src) & ~(uintptr_t)3);
    uint32_t w[NW + 1], r[NW];
#pragma unroll
    for (int k = 0; k <= NW; ++k) w[k] = a[k];   // the buffer has 256 spare bytes behind the scanlines
#pragma unroll
    for (int k = 0; k < NW; ++k) r[k] = (uint32_t)(((((uint64_t)w[k + 1]) << 32) | w[k]) >> sh);
    uint32_t packed[4 * OB];
#pragma unroll
    for (int k = 0; k < 4 * OB; ++k) packed[k] = 0;
    if (FMT == MUST3R_PNG_OUT_GRAY8) {
#pragma unroll
        for (int k = 0; k < 4; ++k) packed[k] = r[k];
    } else if (FMT == MUST3R_PNG_OUT_GRAY16) {
#pragma unroll
        for (int k = 0; k < 8; ++k) packed[k] = ((r[k] & 0x00FF00FFu) << 8) | ((r[k] >> 8) & 0x00FF00FFu);   // PNG's samples are big-endian
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int sb = e * BPP + (BPP == 1 ? 0 : ch), ob = e * 3 + ch;
                packed[ob >> 2] |= ((r[sb >> 2] >> (8 * (sb & 3))) & 255u) << (8 * (ob & 3));
            }
        }
    }
    if (npx == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (int k = 0; k < OB; ++k) d4[k] = make_uint4(packed[4 * k], packed[4 * k + 1], packed[4 * k + 2], packed[4 * k + 3]);
    } else {
        for (int b = 0; b < npx * OB; ++b) dst[b] = (uint8_t)(packed[b >> 2] >> (8 * (b & 3)));
    }
}

__global__ __launch_bounds__(kT) void png_pack_kernel(const ImgDev* imgs) {
    const ImgDev& I = imgs[blockIdx.y];
    const uint32_t W = I.width, gw = (W + 15u) >> 4;
    const uint64_t item = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (item >= (uint64_t)gw * I.height) return;
    const uint32_t y = (uint32_t)(item / gw), x0 = (uint32_t)(item % gw) * 16u;
    const int npx = (int)(W - x0 < 16u ? W - x0 : 16u);
    const uint8_t* src = I.scan + (size_t)y * (I.rowbytes + 1u) + 1u + (size_t)x0 * (uint32_t)I.bpp;
    const int ob = I.out_format == MUST3R_PNG_OUT_RGB8 ? 3 : I.out_format == MUST3R_PNG_OUT_GRAY8 ? 1 : 2;
    uint8_t* dst = I.out + (size_t)y * I.out_stride + (size_t)x0 * ob;
    if (I.out_format == MUST3R_PNG_OUT_RGB8) {
        if (I.bpp == 1) pack16<1, MUST3R_PNG_OUT_RGB8>(src, dst, npx);
        else if (I.bpp == 3) pack16<3, MUST3R_PNG_OUT_RGB8>(src, dst, npx);
        else pack16<4, MUST3R_PNG_OUT_RGB8>(src, dst, npx);
    } else if (I.out_format == MUST3R_PNG_OUT_GRAY8) {
        pack16<1, MUST3R_PNG_OUT_GRAY8>(src, dst, npx);
    } else {
        pack16<2, MUST3R_PNG_OUT_GRAY16>(src, dst, npx);
    }
}

// ---- host: the plan of one call --------------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t scan_capacity(int64_t inflated) { return up256((size_t)inflated) + 256; }

struct Plan {
    std::vector<unsigned char> host;   // what travels to the front of the scratch: ImgDev[n]
    size_t trailers_off = 0, total = 0;
    int max_pack_blocks = 0;
};

static int plan_decode(const must3r_hip_png_image* im, int n, unsigned char* scratch, Plan& P) {
    if (n <= 0 || n > 4096) return fail("png: %d images (1 ... 4096 per call)", n);
    if (!im) return fail("png: null image table");
    size_t off = up256(sizeof(ImgDev) * (size_t)n);
    P.host.assign(off, 0);
    ImgDev* dev = reinterpret_cast<ImgDev*>(P.host.data());
    P.trailers_off = off;
    off = up256(off + 4 * (size_t)n);
    for (int m = 0; m < n; ++m) {
        const must3r_hip_png_info* f = im[m].info;
        if (!f) return fail("png: image %d has no info", m);
        const bool ok_format = (f->color_type == 0 && (f->bit_depth == 8 || f->bit_depth == 16)) || ((f->color_type == 2 || f->color_type == 6) && f->bit_depth == 8);
        if (!ok_format) return fail("png: image %d: colour type %d at %d bits", m, f->color_type, f->bit_depth);
        const int channels = f->color_type == 0 ? 1 : f->color_type == 2 ? 3 : 4, bpp = channels * f->bit_depth / 8;
        if (f->width <= 0 || f->height <= 0 || f->channels != channels || f->bpp != bpp || f->rowbytes != (int64_t)f->width * bpp ||
            f->rowbytes + 1 > kMaxInflated || (f->rowbytes + 1) * (int64_t)f->height > kMaxInflated || f->inflated_bytes != (f->rowbytes + 1) * (int64_t)f->height)
            return fail("png: image %d: the info record does not match its geometry", m);
        if (f->idat_bytes < 7 || (uint64_t)f->idat_bytes >= kMaxIdat) return fail("png: image %d: %lld bytes of IDAT", m, (long long)f->idat_bytes);
        const int fmt = im[m].out_format;
        const bool ok_out = fmt == MUST3R_PNG_OUT_RGB8 ? f->bit_depth == 8 : fmt == MUST3R_PNG_OUT_GRAY8 ? (f->color_type == 0 && f->bit_depth == 8)
                          : fmt == MUST3R_PNG_OUT_GRAY16 ? (f->color_type == 0 && f->bit_depth == 16) : false;
        if (!ok_out) return fail("png: image %d: output format %d for colour type %d at %d bits", m, fmt, f->color_type, f->bit_depth);
        const int ob = fmt == MUST3R_PNG_OUT_RGB8 ? 3 : fmt == MUST3R_PNG_OUT_GRAY8 ? 1 : 2;
        if (scratch) {
            if (!im[m].zdata || !im[m].out) return fail("png: image %d: null data or output", m);
            if ((reinterpret_cast<uintptr_t>(im[m].zdata) & 15) || (reinterpret_cast<uintptr_t>(im[m].out) & 15)) return fail("png: image %d: data and output must be 16-byte aligned", m);
            if (reinterpret_cast<uintptr_t>(im[m].inflated) & 255) return fail("png: image %d: the inflated buffer must be 256-byte aligned", m);
            if (im[m].out_row_stride < (int64_t)ob * f->width) return fail("png: image %d: output row stride below %d x width", m, ob);
        }
        ImgDev& d = dev[m];
        d.z = static_cast<const uint8_t*>(im[m].zdata);
        d.out = static_cast<uint8_t*>(im[m].out);
        d.out_stride = im[m].out_row_stride;
        d.zbytes = (uint32_t)f->idat_bytes;
        d.expected = (uint32_t)f->inflated_bytes;
        d.rowbytes = (uint32_t)f->rowbytes;
        d.height = (uint32_t)f->height;
        d.width = (uint32_t)f->width;
        d.bpp = bpp;
        d.out_format = fmt;
        if (im[m].inflated) {
            d.scan = static_cast<uint8_t*>(im[m].inflated);
        } else {
            d.scan = scratch + off;
            off += scan_capacity(f->inflated_bytes);
        }
        const long long items = (long long)((f->width + 15) / 16) * f->height;
        P.max_pack_blocks = std::max(P.max_pack_blocks, (int)((items + kT - 1) / kT));
    }
    P.total = off;
    return 0;
}

// pinned staging of the table, a ring of slots per calling thread (as image.hip's and jpeg.hip's): the copy is asynchronous, a slot is reused once its copy
// has completed
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
    if (hipGetDevice(&dev) != hipSuccess) return fail("png: hipGetDevice failed");
    if (slot.used && hipEventSynchronize(slot.ev) != hipSuccess) return fail("png: staging event wait failed");
    slot.used = false;
    if (slot.dev != dev || slot.cap < bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        if (slot.ev) (void)hipEventDestroy(slot.ev);
        slot = StageSlot();
        const size_t cap = std::max(bytes, (size_t)1 << 16);
        if (hipHostMalloc(&slot.pin, cap) != hipSuccess) { slot.pin = nullptr; return fail("png: pinned staging allocation failed"); }
        if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) != hipSuccess) { slot.ev = nullptr; return fail("png: event creation failed"); }
        slot.cap = cap;
        slot.dev = dev;
    }
    std::memcpy(slot.pin, src, bytes);
    if (hipMemcpyAsync(dst, slot.pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("png: table upload failed");
    if (hipEventRecord(slot.ev, s) != hipSuccess) return fail("png: staging event record failed");
    slot.used = true;
    return 0;
}

}  // namespace png
}  // namespace m3r
using namespace m3r;
using namespace m3r::png;

extern "C" int must3r_hip_png_parse(const void* data, size_t nbytes, must3r_hip_png_info* info, must3r_hip_png_range* idat_ranges, size_t max_ranges, char* reason,
                                    size_t reason_bytes) {
    return parse(static_cast<const uint8_t*>(data), nbytes, info, idat_ranges, max_ranges, reason, reason_bytes);
}

extern "C" size_t must3r_hip_png_scratch_bytes(const must3r_hip_png_image* images, int n_images) {
    Plan P;
    if (plan_decode(images, n_images, nullptr, P)) return 0;
    return P.total;
}

extern "C" int must3r_hip_png_decode(const must3r_hip_png_batch* b) {
    if (!b) return fail("png: null batch");
    if (b->n_images == 0) return 0;
    if (!b->scratch || !b->status) return fail("png: null scratch or status");
    if (reinterpret_cast<uintptr_t>(b->scratch) & 255) return fail("png: scratch must be 256-byte aligned");
    unsigned char* base = static_cast<unsigned char*>(b->scratch);
    Plan P;
    if (plan_decode(b->images, b->n_images, base, P)) return 1;
    if (b->scratch_bytes < P.total) return fail("png: scratch of %zu bytes < %zu (must3r_hip_png_scratch_bytes)", b->scratch_bytes, P.total);
    hipStream_t s = reinterpret_cast<hipStream_t>(b->stream);
    const unsigned n = (unsigned)b->n_images;
    if (stage_upload(base, P.host.data(), P.host.size(), s)) return 1;
    if (hipMemsetAsync(b->status, 0, sizeof(int32_t) * n, s) != hipSuccess) return fail("png: memset failed");
    const ImgDev* dd = reinterpret_cast<const ImgDev*>(base);
    uint32_t* trailers = reinterpret_cast<uint32_t*>(base + P.trailers_off);
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, s, dd, b->status, trailers);
    hipLaunchKernelGGL(png_adler_kernel, dim3(n), dim3(kT), 0, s, dd, b->status, trailers);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64), 0, s, dd, b->status);
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)P.max_pack_blocks, n), dim3(kT), 0, s, dd);
    if (hipGetLastError() != hipSuccess) return fail("png: launch failed");
    return 0;
}
