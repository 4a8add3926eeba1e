// PNG: chunks -> must3r_hip_png_info and the IDAT payload ranges (include/must3r_hip.h).  Plain C++ that compiles without HIP (tests/c/png_check.cpp runs it
// under the host sanitizers).  No length field is trusted: every read is checked against the buffer first, and every refusal has a reason.  Chunk CRCs are
// not verified: the pixel payload is covered by the Adler-32 check of the decode call.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/must3r_hip.h"

namespace m3r {
namespace png {

constexpr int64_t kMaxInflated = (int64_t)1 << 28;   // bit positions of the stream and byte positions of the output are 32-bit
constexpr uint64_t kMaxIdat = (uint64_t)1 << 28;

struct Refusal {
    char* buf;
    size_t cap;
    int operator()(const char* fmt, ...) const __attribute__((format(printf, 2, 3))) {
        if (buf && cap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, cap, fmt, ap);
            va_end(ap);
        }
        return 1;
    }
};

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline int parse(const uint8_t* p, size_t n, must3r_hip_png_info* info, must3r_hip_png_range* ranges, size_t max_ranges, char* reason, size_t reason_cap) {
    const Refusal no{reason, reason_cap};
    if (reason && reason_cap) reason[0] = 0;
    if (!p || !info) return no("null argument");
    std::memset(info, 0, sizeof(*info));
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || std::memcmp(p, sig, 8) != 0) return no("not a PNG file (no signature)");

    bool have_ihdr = false, have_iend = false, idat_open = false, idat_closed = false;
    uint64_t idat_bytes = 0;
    size_t n_idat = 0;
    uint8_t zhead[2] = {0, 0};
    size_t pos = 8;
    while (!have_iend) {
        if (n - pos < 8) return no(have_ihdr ? "no IEND chunk: the file ends at byte %zu" : "file ends before the IHDR chunk (cut at byte %zu)", n);
        const uint64_t L = be32(p + pos);
        const uint8_t* type = p + pos + 4;
        if (L > 0x7fffffffu || (uint64_t)(n - pos - 8) < L + 4)
            return no("chunk %.4s at byte %zu: length %llu points past the end of the file", reinterpret_cast<const char*>(type), pos, (unsigned long long)L);
        const uint8_t* s = p + pos + 8;   // payload, L bytes; the CRC follows
        const bool is_idat = std::memcmp(type, "IDAT", 4) == 0;
        if (!have_ihdr && std::memcmp(type, "IHDR", 4) != 0) return no("the first chunk is %.4s, not IHDR", reinterpret_cast<const char*>(type));
        if (idat_open && !is_idat) {
            idat_open = false;
            idat_closed = true;
        }
        if (std::memcmp(type, "IHDR", 4) == 0) {
            if (have_ihdr) return no("second IHDR chunk");
            if (L != 13) return no("IHDR of %llu bytes", (unsigned long long)L);
            const uint32_t W = be32(s), H = be32(s + 4);
            const int depth = s[8], ct = s[9];
            if (W == 0 || H == 0) return no("empty image (%u x %u)", W, H);
            if (W > 0x7fffffffu || H > 0x7fffffffu) return no("size %u x %u", W, H);
            if (s[10] != 0) return no("compression method %d", s[10]);
            if (s[11] != 0) return no("filter method %d", s[11]);
            if (s[12] != 0) return no(s[12] == 1 ? "Adam7 interlace" : "interlace method %d", s[12]);
            if (ct == 3) return no("palette image (colour type 3)");
            if (ct == 4) return no("grey + alpha (colour type 4)");
            if (ct != 0 && ct != 2 && ct != 6) return no("colour type %d", ct);
            if (depth != 8 && depth != 16) return no("bit depth %d (8, or 16 for grey)", depth);
            if (depth == 16 && ct != 0) return no("16-bit %s", ct == 2 ? "RGB" : "RGBA");
            const int channels = ct == 0 ? 1 : ct == 2 ? 3 : 4, bpp = channels * depth / 8;
            const int64_t rowbytes = (int64_t)W * bpp;
            if (rowbytes + 1 > kMaxInflated || (rowbytes + 1) * (int64_t)H > kMaxInflated)
                return no("%u x %u: more than %lld inflated bytes", W, H, (long long)kMaxInflated);
            info->width = (int32_t)W;
            info->height = (int32_t)H;
            info->color_type = ct;
            info->bit_depth = depth;
            info->channels = channels;
            info->bpp = bpp;
            info->rowbytes = rowbytes;
            info->inflated_bytes = (rowbytes + 1) * (int64_t)H;
            have_ihdr = true;
        } else if (is_idat) {
            if (idat_closed) return no("IDAT chunks that are not consecutive");
            idat_open = true;
            for (uint64_t k = 0; k < L && idat_bytes + k < 2; ++k) zhead[idat_bytes + k] = s[k];
            if (ranges && n_idat < max_ranges) ranges[n_idat] = must3r_hip_png_range{(uint64_t)(pos + 8), L};
            idat_bytes += L;
            ++n_idat;
            if (idat_bytes >= kMaxIdat) return no("more than %llu bytes of IDAT", (unsigned long long)kMaxIdat);
            if (n_idat > 0x7fffffffu) return no("too many IDAT chunks");
        } else if (std::memcmp(type, "IEND", 4) == 0) {
            have_iend = true;
        } else if (std::memcmp(type, "PLTE", 4) == 0) {
            // a suggested palette is allowed in colour types 2 and 6 and changes no pixel
            if (info->color_type == 0) return no("PLTE chunk in a grey image");
        } else if (std::memcmp(type, "tRNS", 4) == 0) {
            return no("tRNS chunk (transparency by colour key)");
        } else if (std::memcmp(type, "acTL", 4) == 0) {
            return no("animated PNG (acTL chunk)");
        } else if (!(type[0] & 0x20)) {
            return no("unknown critical chunk %.4s", reinterpret_cast<const char*>(type));
        }
        pos += 8 + (size_t)L + 4;
    }
    if (n_idat == 0) return no("no IDAT chunk");
    // the zlib header: CM 8, a window of at most 32 KiB, no preset dictionary, the check bits; then at least one deflate byte and the trailer
    if (idat_bytes < 2) return no("IDAT data of %llu bytes has no zlib header", (unsigned long long)idat_bytes);
    if ((zhead[0] & 15) != 8) return no("zlib header: compression method %d (CM must be 8)", zhead[0] & 15);
    if ((zhead[0] >> 4) > 7) return no("zlib header: window size code %d (CINFO above 7)", zhead[0] >> 4);
    if (zhead[1] & 0x20) return no("zlib header: preset dictionary (FDICT)");
    if ((((unsigned)zhead[0] << 8) | zhead[1]) % 31 != 0) return no("zlib header: the check bits are wrong (FCHECK)");
    if (idat_bytes < 2 + 1 + 4) return no("IDAT data of %llu bytes is shorter than a zlib stream can be", (unsigned long long)idat_bytes);
    info->n_idat = (int32_t)n_idat;
    info->idat_bytes = (int64_t)idat_bytes;
    return 0;
}

}  // namespace png
}  // namespace m3r
