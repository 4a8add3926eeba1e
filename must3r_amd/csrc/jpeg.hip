// Baseline JPEG decoding on the device (include/must3r_hip.h "baseline JPEG decoding"): from the bytes of the file to interleaved RGB.
//   jpeg_sync_kernel      one thread per subsequence of MUST3R_JPEG_SUBSEQ_BYTES bytes of a restart segment: decode from an assumed state, then again from the
//                         predecessor's exit while the entries change (jpeg_entropy.hpp, the text a host program runs too)
//   jpeg_scan_kernel      exclusive scan of the completed-block counts inside every segment: where each subsequence writes
//   jpeg_write_kernel     decode once more, writing int16 coefficients [blocks][64]; flags the image when an entry is not the predecessor's recorded exit
//   jpeg_sequential_kernel  flagged images only: one thread per segment, from the segment's first bit
//   jpeg_dc_kernel        DC differences -> DC values, a segmented scan per component and restart interval
//   jpeg_idct_kernel      dequantisation and the accurate integer IDCT (13-bit constants, two passes) into uint8 planes padded to whole MCUs
//   jpeg_color_kernel     libjpeg-turbo's fancy upsampling of 2x1 / 2x2 chroma and its 16-bit YCbCr -> RGB; 16 pixels a thread, 16-byte stores where aligned
// Every launch covers the whole batch (grid.y = image); the sizes follow from the headers, nothing is read back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "abi.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_parse.hpp"

namespace m3r {
namespace jpeg {

constexpr int kT = 256;

// one subsequence: the exit state, the entry it was decoded from, its segment and its index there
struct alignas(16) Rec {
    uint32_t pos, slotzz, nblk, seg;
    uint32_t upos, uslotzz, j, pad;
};

struct ImgDev {
    const uint8_t* data;
    uint8_t* out;
    long long out_stride;
    const must3r_hip_jpeg_info* info;   // device copy
    const uint32_t* seg_off;            // [nseg + 1]: first byte of each segment; [nseg] = end of the scan + 2
    const uint32_t* seg_sub;            // [nseg + 1]: first subsequence of each segment
    Rec* rec[2];
    uint32_t* base;                     // [nsub]
    int16_t* coef;                      // [n_blocks][64]
    uint8_t* plane[3];
    int32_t pstride[3];
    int32_t nsub, nseg;
    uint16_t qnat[3][64];               // quantisation tables in row-major order
};

struct Tables {
    must3r_hip_jpeg_huff tabs[4];
    uint8_t natural[64];
};

__device__ inline void load_tables(const must3r_hip_jpeg_info* info, Tables* t) {
    static_assert(sizeof(must3r_hip_jpeg_huff) % 4 == 0, "word copy");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&info->dc[0]);   // dc[2] and ac[2] are adjacent
    uint32_t* dst = reinterpret_cast<uint32_t*>(t->tabs);
    for (uint32_t i = threadIdx.x; i < sizeof(t->tabs) / 4; i += blockDim.x) dst[i] = src[i];
    for (uint32_t i = threadIdx.x; i < 64; i += blockDim.x) t->natural[i] = info->natural[i];
    __syncthreads();
}

__device__ inline uint32_t find_segment(const uint32_t* seg_sub, int nseg, uint32_t i) {
    uint32_t lo = 0, hi = (uint32_t)nseg;   // the largest s with seg_sub[s] <= i
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_sub[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kT) void jpeg_sync_kernel(const ImgDev* imgs, int launch) {
    const ImgDev& I = imgs[blockIdx.y];
    if (blockIdx.x * kT >= (uint32_t)I.nsub) return;
    __shared__ Tables T;
    __shared__ uint32_t spos[kT], sslot[kT];
    load_tables(I.info, &T);
    const Scan sc = make_scan(I.info, T.tabs, T.natural);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    const bool active = i < (uint32_t)I.nsub;
    const Rec* rin = I.rec[(launch + 1) & 1];
    Rec* rout = I.rec[launch & 1];
    uint32_t s = 0, j = 0, n = 0, stop = 0;
    const uint8_t* d = I.data;
    State ex{0, 0, 0}, used{0, 0, 0};
    if (active) {
        if (launch == 0) {
            s = find_segment(I.seg_sub, I.nseg, i);
            j = i - I.seg_sub[s];
        } else {
            const Rec r = rin[i];
            s = r.seg;
            j = r.j;
            ex = State{r.pos, r.slotzz, r.nblk};
            used = State{r.upos, r.uslotzz, 0};
        }
        d = I.data + I.seg_off[s];
        n = I.seg_off[s + 1] - 2 - I.seg_off[s];
        stop = sub_stop(n, j);
        if (launch == 0) {
            used = assumed_state(d, n, j);
            ex = used;
            decode_span(sc, d, n, stop, 0xFFFFFFFFu, kSubSteps, ex, nullptr, 0, 0, false);
        }
    }
    spos[threadIdx.x] = ex.pos;
    sslot[threadIdx.x] = ex.slotzz;
    __syncthreads();
    for (int round = 0; round < kRounds; ++round) {
        State entry{0, 0, 0};
        bool have = active;
        if (active && j != 0) {
            if (threadIdx.x > 0) {
                entry.pos = spos[threadIdx.x - 1];
                entry.slotzz = sslot[threadIdx.x - 1];
            } else if (launch > 0) {
                entry.pos = rin[i - 1].pos;
                entry.slotzz = rin[i - 1].slotzz;
            } else {
                have = false;
            }
        }
        const bool need = have && (entry.pos != used.pos || entry.slotzz != used.slotzz);
        if (need) {
            used = entry;
            ex = entry;
            decode_span(sc, d, n, stop, 0xFFFFFFFFu, kSubSteps, ex, nullptr, 0, 0, false);
        }
        __syncthreads();
        if (need) {
            spos[threadIdx.x] = ex.pos;
            sslot[threadIdx.x] = ex.slotzz;
        }
        if (!__syncthreads_or(need ? 1 : 0)) break;
    }
    if (active) rout[i] = Rec{ex.pos, ex.slotzz, ex.nblk, s, used.pos, used.slotzz, j, 0};
}

// segmented inclusive scan of (v, f) over the block's kT threads; f: a segment starts here.  Returns the inclusive value; *open: no start at or before the thread.
__device__ inline int32_t block_segscan(int32_t v, bool f, int32_t* sv, uint32_t* sf, bool* open) {
    const uint32_t t = threadIdx.x;
    uint32_t ff = f ? 1u : 0u;
    sv[t] = v;
    sf[t] = ff;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)kT; off <<= 1) {
        int32_t pv = 0;
        uint32_t pf = 0;
        if (t >= off) {
            pv = sv[t - off];
            pf = sf[t - off];
        }
        __syncthreads();
        if (t >= off && !ff) {
            v += pv;
            ff |= pf;
        }
        sv[t] = v;
        sf[t] = ff;
        __syncthreads();
    }
    *open = ff == 0;
    return v;
}

__global__ __launch_bounds__(kT) void jpeg_scan_kernel(const ImgDev* imgs, int final_buf) {
    const ImgDev& I = imgs[blockIdx.x];
    __shared__ int32_t sv[kT];
    __shared__ uint32_t sf[kT];
    const Rec* rec = I.rec[final_buf];
    int32_t carry = 0;
    for (uint32_t t0 = 0; t0 < (uint32_t)I.nsub; t0 += kT) {
        const uint32_t i = t0 + threadIdx.x;
        const bool active = i < (uint32_t)I.nsub;
        int32_t own = 0;
        bool first = false;
        if (active) {
            own = (int32_t)rec[i].nblk;
            first = rec[i].j == 0;
        }
        bool open;
        int32_t incl = block_segscan(own, first, sv, sf, &open);
        if (open) incl += carry;
        if (active) I.base[i] = (uint32_t)(incl - own);
        __syncthreads();
        if (threadIdx.x == kT - 1) sv[0] = incl;
        __syncthreads();
        carry = sv[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kT) void jpeg_write_kernel(const ImgDev* imgs, int final_buf, int32_t* flags) {
    const ImgDev& I = imgs[blockIdx.y];
    if (blockIdx.x * kT >= (uint32_t)I.nsub) return;
    __shared__ Tables T;
    load_tables(I.info, &T);
    const Scan sc = make_scan(I.info, T.tabs, T.natural);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= (uint32_t)I.nsub) return;
    const Rec* rec = I.rec[final_buf];
    const Rec r = rec[i];
    State entry{0, 0, 0};
    if (r.j != 0) {
        entry.pos = rec[i - 1].pos;
        entry.slotzz = rec[i - 1].slotzz;
    }
    if (entry.pos != r.upos || entry.slotzz != r.uslotzz) flags[blockIdx.y] = MUST3R_JPEG_PATH_SEQUENTIAL;   // the recorded exit is not the chain's
    const uint8_t* d = I.data + I.seg_off[r.seg];
    const uint32_t n = I.seg_off[r.seg + 1] - 2 - I.seg_off[r.seg];
    uint32_t first_block, blocks;
    segment_blocks(I.info, r.seg, &first_block, &blocks);
    decode_span(sc, d, n, sub_stop(n, r.j), 0xFFFFFFFFu, kSubSteps, entry, I.coef + (size_t)first_block * 64, I.base[i], blocks, false);
}

__global__ __launch_bounds__(64) void jpeg_sequential_kernel(const ImgDev* imgs, const int32_t* flags) {
    const ImgDev& I = imgs[blockIdx.y];
    if (flags[blockIdx.y] == MUST3R_JPEG_PATH_FAST) return;
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= (uint32_t)I.nseg) return;
    const Scan sc = make_scan(I.info, &I.info->dc[0], I.info->natural);
    const uint8_t* d = I.data + I.seg_off[s];
    const uint32_t n = I.seg_off[s + 1] - 2 - I.seg_off[s];
    uint32_t first_block, blocks;
    segment_blocks(I.info, s, &first_block, &blocks);
    State st{0, 0, 0};
    decode_span(sc, d, n, n, blocks, n * 8u + 64u, st, I.coef + (size_t)first_block * 64, 0, blocks, true);
}

__global__ __launch_bounds__(kT) void jpeg_dc_kernel(const ImgDev* imgs) {
    const ImgDev& I = imgs[blockIdx.y];
    const must3r_hip_jpeg_info* info = I.info;
    const uint32_t c = blockIdx.x;
    if (c >= (uint32_t)info->components) return;
    __shared__ int32_t sv[kT];
    __shared__ uint32_t sf[kT];
    const uint32_t bpm = (uint32_t)info->blocks_per_mcu, ny = info->components == 1 ? 1u : (uint32_t)(info->hs * info->vs);
    const uint32_t per = c == 0 ? ny : 1u, off = c == 0 ? 0u : ny + c - 1u;
    const uint32_t mcus = (uint32_t)info->mcus_x * (uint32_t)info->mcus_y;
    const uint32_t ri = info->restart_interval > 0 ? (uint32_t)info->restart_interval : mcus;
    const uint32_t total = mcus * per;
    int32_t carry = 0;
    for (uint32_t t0 = 0; t0 < total; t0 += kT) {
        const uint32_t t = t0 + threadIdx.x;
        const bool active = t < total;
        int32_t own = 0;
        bool first = false;
        size_t at = 0;
        if (active) {
            const uint32_t mcu = t / per, sub = t % per;
            at = ((size_t)mcu * bpm + off + sub) * 64;
            own = I.coef[at];
            first = sub == 0 && mcu % ri == 0;
        }
        bool open;
        int32_t incl = block_segscan(own, first, sv, sf, &open);
        if (open) incl += carry;
        if (active) I.coef[at] = (int16_t)incl;
        __syncthreads();
        if (threadIdx.x == kT - 1) sv[0] = incl;
        __syncthreads();
        carry = sv[0];
        __syncthreads();
    }
}

// jidctint.c's constants: FIX(x) = round(x * 2^13)
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069,
              F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass: in[0 ... 7] -> out[0 ... 7], descaled by `shift`
__device__ inline void idct8(const int* in, int* out, int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * F_0_541;
    int tmp2 = z1 + z3 * (-F_1_847);
    int tmp3 = z1 + z2 * F_0_765;
    z2 = in[0];
    z3 = in[4];
    int tmp0 = (z2 + z3) * (1 << kConstBits);
    int tmp1 = (z2 - z3) * (1 << kConstBits);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298;
    tmp1 *= F_2_053;
    tmp2 *= F_3_072;
    tmp3 *= F_1_501;
    z1 *= -F_0_899;
    z2 *= -F_2_562;
    z3 *= -F_1_961;
    z4 *= -F_0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, shift);
    out[7] = descale(tmp10 - tmp3, shift);
    out[1] = descale(tmp11 + tmp2, shift);
    out[6] = descale(tmp11 - tmp2, shift);
    out[2] = descale(tmp12 + tmp1, shift);
    out[5] = descale(tmp12 - tmp1, shift);
    out[3] = descale(tmp13 + tmp0, shift);
    out[4] = descale(tmp13 - tmp0, shift);
}

__device__ inline uint32_t clamp_u8(int x) { return (uint32_t)(x < 0 ? 0 : x > 255 ? 255 : x); }

__global__ __launch_bounds__(kT) void jpeg_idct_kernel(const ImgDev* imgs) {
    const ImgDev& I = imgs[blockIdx.y];
    const must3r_hip_jpeg_info* info = I.info;
    const uint32_t g = blockIdx.x * kT + threadIdx.x;
    if (g >= (uint32_t)info->n_blocks) return;
    const uint32_t bpm = (uint32_t)info->blocks_per_mcu, hs = (uint32_t)info->hs, ny = info->components == 1 ? 1u : hs * (uint32_t)info->vs;
    const uint32_t mcu = g / bpm, slot = g % bpm, mx = mcu % (uint32_t)info->mcus_x, my = mcu / (uint32_t)info->mcus_x;
    uint32_t c, bx, by;
    if (slot < ny) {
        c = 0;
        bx = mx * hs + slot % hs;
        by = my * (uint32_t)info->vs + slot / hs;
    } else {
        c = slot - ny + 1;
        bx = mx;
        by = my;
    }
    const uint4* src = reinterpret_cast<const uint4*>(I.coef + (size_t)g * 64);
    const uint16_t* q = I.qnat[c];
    int ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 v = src[r];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int16_t cf = (int16_t)((w4[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
            ws[r * 8 + e] = (int)cf * (int)q[r * 8 + e];
        }
    }
    // pass 1: columns, scaled up by 2^kPass1Bits
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[r * 8 + col];
        idct8(in, out, kConstBits - kPass1Bits);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * 8 + col] = out[r];
    }
    // pass 2: rows; descale by 2^(13 + 2 + 3), centre and range-limit
    uint8_t* dst = I.plane[c] + (size_t)by * 8 * I.pstride[c] + (size_t)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int out[8];
        idct8(&ws[r * 8], out, kConstBits + kPass1Bits + 3);
        uint2 px;
        px.x = clamp_u8(out[0] + 128) | (clamp_u8(out[1] + 128) << 8) | (clamp_u8(out[2] + 128) << 16) | (clamp_u8(out[3] + 128) << 24);
        px.y = clamp_u8(out[4] + 128) | (clamp_u8(out[5] + 128) << 8) | (clamp_u8(out[6] + 128) << 16) | (clamp_u8(out[7] + 128) << 24);
        *reinterpret_cast<uint2*>(dst + (size_t)r * I.pstride[c]) = px;
    }
}

// jdsample.c: one chroma sample at full resolution.  mode 0: 1x1; 1: 2x1; 2: 2x2.  Fancy (triangle) upsampling when the chroma plane is more than two samples
// wide, replication otherwise; the edge columns repeat the edge sample, the context rows above the first and below the last REAL chroma row repeat that row.
__device__ inline int chroma_at(const uint8_t* p, int stride, int mode, int x, int y, int dw, int dh) {
    if (mode == 0) return p[(size_t)y * stride + x];
    const int i = x >> 1;
    if (mode == 1) {
        const uint8_t* row = p + (size_t)y * stride;
        if (dw <= 2) return row[i];
        const int c = row[i];
        if (x & 1) return i == dw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
        return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const uint8_t* row0 = p + (size_t)r * stride;
    if (dw <= 2) return row0[i];
    const int ro = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t* row1 = p + (size_t)ro * stride;
    const int cur = 3 * row0[i] + row1[i];
    if (x & 1) return i == dw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + 3 * row0[i + 1] + row1[i + 1] + 7) >> 4;
    return i == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + 3 * row0[i - 1] + row1[i - 1] + 8) >> 4;
}

// jdcolor.c: 16 fraction bits, FIX(x) = round(x * 2^16)
constexpr int C_CR_R = 91881, C_CB_B = 116130, C_CR_G = 46802, C_CB_G = 22554, C_HALF = 1 << 15;

__global__ __launch_bounds__(kT) void jpeg_color_kernel(const ImgDev* imgs) {
    const ImgDev& I = imgs[blockIdx.y];
    const must3r_hip_jpeg_info* info = I.info;
    const int W = info->width, H = info->height, gw = (W + 15) >> 4;
    const long long item = (long long)blockIdx.x * kT + threadIdx.x;
    if (item >= (long long)gw * H) return;
    const int y = (int)(item / gw), x0 = (int)(item % gw) * 16, npx = W - x0 < 16 ? W - x0 : 16;
    const bool grey = info->components == 1;
    const int mode = grey ? 0 : (info->hs == 1 ? 0 : (info->vs == 1 ? 1 : 2));
    const int dw = mode == 0 ? W : (W + 1) >> 1, dh = mode == 2 ? (H + 1) >> 1 : H;
    const uint8_t* yrow = I.plane[0] + (size_t)y * I.pstride[0] + x0;   // x0 is a multiple of 16 and so is the stride
    const uint4 y16 = *reinterpret_cast<const uint4*>(yrow);          // the planes are padded to whole MCUs: 16 bytes are there
    const uint32_t yw[4] = {y16.x, y16.y, y16.z, y16.w};
    uint32_t packed[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int yy = (int)((yw[e >> 2] >> (8 * (e & 3))) & 0xFFu);
        uint32_t r = (uint32_t)yy, g = (uint32_t)yy, b = (uint32_t)yy;
        if (!grey && e < npx) {
            const int cb = chroma_at(I.plane[1], I.pstride[1], mode, x0 + e, y, dw, dh) - 128;
            const int cr = chroma_at(I.plane[2], I.pstride[2], mode, x0 + e, y, dw, dh) - 128;
            r = clamp_u8(yy + ((C_CR_R * cr + C_HALF) >> 16));
            g = clamp_u8(yy + ((-C_CB_G * cb + C_HALF - C_CR_G * cr) >> 16));
            b = clamp_u8(yy + ((C_CB_B * cb + C_HALF) >> 16));
        }
        const uint32_t rgb[3] = {r, g, b};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int byte = e * 3 + ch;
            packed[byte >> 2] |= rgb[ch] << (8 * (byte & 3));
        }
    }
    uint8_t* dst = I.out + (size_t)y * I.out_stride + (size_t)x0 * 3;
    if (npx == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        d4[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
        d4[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
        d4[2] = make_uint4(packed[8], packed[9], packed[10], packed[11]);
    } else {
        for (int byte = 0; byte < npx * 3; ++byte) dst[byte] = (uint8_t)(packed[byte >> 2] >> (8 * (byte & 3)));
    }
}

// ---- host: the plan of one call --------------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Plan {
    std::vector<unsigned char> host;   // what travels to the front of the scratch: ImgDev[n], the info records, the segment tables
    size_t coef_off = 0, coef_bytes = 0, total = 0;
    int max_sub_blocks = 0, max_seg_blocks = 0, max_idct_blocks = 0, max_color_blocks = 0;
};

static int plan_decode(const must3r_hip_jpeg_image* im, int n, unsigned char* scratch, Plan& P) {
    if (n <= 0 || n > 4096) return fail("jpeg: %d images (1 ... 4096 per call)", n);
    if (!im) return fail("jpeg: null image table");
    size_t off = up256(sizeof(ImgDev) * (size_t)n);
    std::vector<size_t> info_off(n), segoff_off(n), segsub_off(n);
    std::vector<uint32_t> nsubs(n);
    for (int m = 0; m < n; ++m) {
        const must3r_hip_jpeg_info* f = im[m].info;
        if (!f || !im[m].seg_offsets) return fail("jpeg: image %d has no info or no segment offsets", m);
        if (f->width <= 0 || f->height <= 0 || f->width > 65535 || f->height > 65535 || (f->components != 1 && f->components != 3))
            return fail("jpeg: image %d: bad geometry", m);
        const bool ok_s = f->components == 1 ? (f->hs == 1 && f->vs == 1) : ((f->hs == 1 || f->hs == 2) && (f->vs == 1 || f->vs == 2) && !(f->hs == 1 && f->vs == 2));
        if (!ok_s) return fail("jpeg: image %d: sampling %d x %d", m, f->hs, f->vs);
        const long long mx = (f->width + 8 * f->hs - 1) / (8 * f->hs), my = (f->height + 8 * f->vs - 1) / (8 * f->vs);
        const long long bpm = f->components == 1 ? 1 : f->hs * f->vs + 2, mcus = mx * my;
        if (f->mcus_x != mx || f->mcus_y != my || f->blocks_per_mcu != bpm || f->n_blocks != mcus * bpm || mcus * bpm > kMaxBlocks)
            return fail("jpeg: image %d: the info record does not match its geometry", m);
        const long long nseg = f->restart_interval > 0 ? (mcus + f->restart_interval - 1) / f->restart_interval : 1;
        if (f->restart_interval < 0 || f->n_segments != nseg) return fail("jpeg: image %d: %d segments for its restart interval", m, f->n_segments);
        for (int c = 0; c < 3; ++c)
            if (f->comp_dc[c] < 0 || f->comp_dc[c] > 1 || f->comp_ac[c] < 0 || f->comp_ac[c] > 1) return fail("jpeg: image %d: table selector", m);
        for (int k = 0; k < 64; ++k)
            if (f->natural[k] != kNatural[k]) return fail("jpeg: image %d: the info record's zig-zag table is not the standard's", m);
        const long long end = f->scan_offset + f->scan_bytes;
        if (f->scan_offset < 2 || f->scan_bytes < 0 || end >= (long long)kMaxFileBytes) return fail("jpeg: image %d: bad scan range", m);
        if (scratch) {
            if (end > (long long)im[m].data_bytes) return fail("jpeg: image %d: the scan lies outside the %zu bytes of the file", m, im[m].data_bytes);
            if (!im[m].data || !im[m].out) return fail("jpeg: image %d: null data or output", m);
            if ((reinterpret_cast<uintptr_t>(im[m].data) & 15) || (reinterpret_cast<uintptr_t>(im[m].out) & 15)) return fail("jpeg: image %d: data and output must be 16-byte aligned", m);
            if (im[m].out_row_stride < 3LL * f->width) return fail("jpeg: image %d: output row stride below 3 x width", m);
        }
        // segments: increasing, inside the scan, each at least the two bytes of its marker after the one before
        uint64_t subs = 0;
        for (long long s = 0; s < nseg; ++s) {
            const long long a = im[m].seg_offsets[s], b = s + 1 < nseg ? (long long)im[m].seg_offsets[s + 1] - 2 : end;
            if (a < f->scan_offset || b < a || b > end || (s == 0 && a != f->scan_offset)) return fail("jpeg: image %d: restart segment %lld outside the scan", m, s);
            subs += segment_subs((uint32_t)(b - a));
        }
        if (subs > 0x7fffffffULL) return fail("jpeg: image %d too large", m);
        nsubs[m] = (uint32_t)subs;
        info_off[m] = off;
        off = up256(off + sizeof(must3r_hip_jpeg_info));
        segoff_off[m] = off;
        off = up256(off + 4 * (size_t)(nseg + 1));
        segsub_off[m] = off;
        off = up256(off + 4 * (size_t)(nseg + 1));
    }
    const size_t table_bytes = off;
    P.host.assign(table_bytes, 0);
    ImgDev* dev = reinterpret_cast<ImgDev*>(P.host.data());
    // first every coefficient buffer (one memset), then the rest per image
    P.coef_off = off;
    std::vector<size_t> coef_at(n);
    for (int m = 0; m < n; ++m) {
        coef_at[m] = off;
        off = up256(off + (size_t)im[m].info->n_blocks * 128);
    }
    P.coef_bytes = off - P.coef_off;
    for (int m = 0; m < n; ++m) {
        const must3r_hip_jpeg_info* f = im[m].info;
        const long long nseg = f->n_segments, end = f->scan_offset + f->scan_bytes;
        ImgDev& d = dev[m];
        std::memcpy(P.host.data() + info_off[m], f, sizeof(*f));
        uint32_t* so = reinterpret_cast<uint32_t*>(P.host.data() + segoff_off[m]);
        uint32_t* ss = reinterpret_cast<uint32_t*>(P.host.data() + segsub_off[m]);
        uint32_t acc = 0;
        for (long long s = 0; s < nseg; ++s) {
            const long long a = im[m].seg_offsets[s], b = s + 1 < nseg ? (long long)im[m].seg_offsets[s + 1] - 2 : end;
            so[s] = (uint32_t)a;
            ss[s] = acc;
            acc += segment_subs((uint32_t)(b - a));
        }
        so[nseg] = (uint32_t)(end + 2);
        ss[nseg] = acc;
        d.data = static_cast<const uint8_t*>(im[m].data);
        d.out = static_cast<uint8_t*>(im[m].out);
        d.out_stride = im[m].out_row_stride;
        d.info = reinterpret_cast<const must3r_hip_jpeg_info*>(scratch + info_off[m]);
        d.seg_off = reinterpret_cast<const uint32_t*>(scratch + segoff_off[m]);
        d.seg_sub = reinterpret_cast<const uint32_t*>(scratch + segsub_off[m]);
        d.nsub = (int32_t)nsubs[m];
        d.nseg = (int32_t)nseg;
        for (int b = 0; b < 2; ++b) {
            d.rec[b] = reinterpret_cast<Rec*>(scratch + off);
            off = up256(off + sizeof(Rec) * (size_t)nsubs[m]);
        }
        d.base = reinterpret_cast<uint32_t*>(scratch + off);
        off = up256(off + 4 * (size_t)nsubs[m]);
        d.coef = reinterpret_cast<int16_t*>(scratch + coef_at[m]);
        for (int c = 0; c < 3; ++c) {
            const int ph = c == 0 ? f->mcus_y * f->vs * 8 : f->mcus_y * 8;
            const int pw = c == 0 ? f->mcus_x * f->hs * 8 : f->mcus_x * 8;
            d.pstride[c] = (pw + 15) & ~15;
            d.plane[c] = nullptr;
            if (c < f->components) {
                d.plane[c] = scratch + off;
                off = up256(off + (size_t)d.pstride[c] * ph);
            }
            for (int k = 0; k < 64; ++k) d.qnat[c][kNatural[k]] = f->quant[c][k];
        }
        P.max_sub_blocks = std::max(P.max_sub_blocks, (int)((nsubs[m] + kT - 1) / kT));
        P.max_seg_blocks = std::max(P.max_seg_blocks, (int)((nseg + 63) / 64));
        P.max_idct_blocks = std::max(P.max_idct_blocks, (f->n_blocks + kT - 1) / kT);
        const long long items = (long long)((f->width + 15) / 16) * f->height;
        P.max_color_blocks = std::max(P.max_color_blocks, (int)((items + kT - 1) / kT));
    }
    P.total = off;
    return 0;
}

// pinned staging of the tables, a ring of slots per calling thread (as image.hip's): the copy is asynchronous, a slot is reused once its copy has completed
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
    if (hipGetDevice(&dev) != hipSuccess) return fail("jpeg: hipGetDevice failed");
    if (slot.used && hipEventSynchronize(slot.ev) != hipSuccess) return fail("jpeg: staging event wait failed");
    slot.used = false;
    if (slot.dev != dev || slot.cap < bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        if (slot.ev) (void)hipEventDestroy(slot.ev);
        slot = StageSlot();
        const size_t cap = std::max(bytes, (size_t)1 << 16);
        if (hipHostMalloc(&slot.pin, cap) != hipSuccess) { slot.pin = nullptr; return fail("jpeg: pinned staging allocation failed"); }
        if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) != hipSuccess) { slot.ev = nullptr; return fail("jpeg: event creation failed"); }
        slot.cap = cap;
        slot.dev = dev;
    }
    std::memcpy(slot.pin, src, bytes);
    if (hipMemcpyAsync(dst, slot.pin, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail("jpeg: table upload failed");
    if (hipEventRecord(slot.ev, s) != hipSuccess) return fail("jpeg: staging event record failed");
    slot.used = true;
    return 0;
}

}  // namespace jpeg
}  // namespace m3r
using namespace m3r;
using namespace m3r::jpeg;

extern "C" int must3r_hip_jpeg_parse(const void* data, size_t data_bytes, must3r_hip_jpeg_info* info, uint32_t* seg_offsets, size_t seg_capacity, char* reason,
                                     size_t reason_capacity) {
    return parse(static_cast<const uint8_t*>(data), data_bytes, info, seg_offsets, seg_capacity, reason, reason_capacity);
}

extern "C" size_t must3r_hip_jpeg_scratch_bytes(const must3r_hip_jpeg_image* images, int n_images) {
    Plan P;
    if (plan_decode(images, n_images, nullptr, P)) return 0;
    return P.total;
}

extern "C" int must3r_hip_jpeg_decode(const must3r_hip_jpeg_batch* b) {
    if (!b) return fail("jpeg: null batch");
    if (b->n_images == 0) return 0;
    if (!b->scratch || !b->flags) return fail("jpeg: null scratch or flags");
    if (reinterpret_cast<uintptr_t>(b->scratch) & 255) return fail("jpeg: scratch must be 256-byte aligned");
    unsigned char* base = static_cast<unsigned char*>(b->scratch);
    Plan P;
    if (plan_decode(b->images, b->n_images, base, P)) return 1;
    if (b->scratch_bytes < P.total) return fail("jpeg: scratch of %zu bytes < %zu (must3r_hip_jpeg_scratch_bytes)", b->scratch_bytes, P.total);
    hipStream_t s = reinterpret_cast<hipStream_t>(b->stream);
    const unsigned n = (unsigned)b->n_images;
    if (stage_upload(base, P.host.data(), P.host.size(), s)) return 1;
    if (hipMemsetAsync(base + P.coef_off, 0, P.coef_bytes, s) != hipSuccess) return fail("jpeg: memset failed");
    if (hipMemsetAsync(b->flags, 0, sizeof(int32_t) * n, s) != hipSuccess) return fail("jpeg: memset failed");
    const ImgDev* dd = reinterpret_cast<const ImgDev*>(base);
    for (int l = 0; l < kLaunches; ++l) hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)P.max_sub_blocks, n), dim3(kT), 0, s, dd, l);
    const int fin = (kLaunches - 1) & 1;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(kT), 0, s, dd, fin);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)P.max_sub_blocks, n), dim3(kT), 0, s, dd, fin, b->flags);
    hipLaunchKernelGGL(jpeg_sequential_kernel, dim3((unsigned)P.max_seg_blocks, n), dim3(64), 0, s, dd, b->flags);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3, n), dim3(kT), 0, s, dd);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)P.max_idct_blocks, n), dim3(kT), 0, s, dd);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)P.max_color_blocks, n), dim3(kT), 0, s, dd);
    if (hipGetLastError() != hipSuccess) return fail("jpeg: launch failed");
    return 0;
}
