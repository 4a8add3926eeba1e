// Baseline JPEG: marker segments -> must3r_hip_jpeg_info (include/must3r_hip.h).  Plain C++ that compiles without HIP (tests/c/jpeg_check.cpp runs it under the
// host sanitizers).  No length field is trusted: every read is checked against the buffer first, and every refusal has a reason.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/must3r_hip.h"

namespace m3r {
namespace jpeg {

constexpr size_t kMaxFileBytes = (size_t)1 << 28;   // bit positions of a segment are 32-bit
constexpr int64_t kMaxBlocks = (int64_t)1 << 23;    // 1 GiB of int16 coefficients

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

// jpeg_natural_order of the standard: zig-zag index -> row-major index
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// counts[1 ... 16] and the symbols in code order -> the lookahead and the canonical arrays; false: not a prefix code the standard allows
inline bool build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, bool is_dc, must3r_hip_jpeg_huff* h) {
    std::memset(h, 0, sizeof(*h));
    for (int i = 0; i < nvals; ++i) {
        if (is_dc && vals[i] > 15) return false;
        h->vals[i] = vals[i];
    }
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        h->valoff[l] = p - code;
        const int cnt = counts[l];
        if (cnt) {
            for (int i = 0; i < cnt; ++i, ++code, ++p) {
                if (l <= 9) {
                    const int base = code << (9 - l);
                    if (base + (1 << (9 - l)) > 512) return false;
                    for (int c = 0; c < (1 << (9 - l)); ++c) h->look[base + c] = (uint16_t)((l << 8) | vals[p]);
                }
            }
            if (code >= (1 << l)) return false;   // the all-ones code of a length is not assigned
            h->maxcode[l] = code - 1;
        } else {
            h->maxcode[l] = -1;
        }
        code <<= 1;
    }
    h->maxcode[0] = -1;
    h->maxcode[17] = 0x7fffffff;
    return true;
}

inline int parse(const uint8_t* p, size_t n, must3r_hip_jpeg_info* info, uint32_t* seg, size_t seg_cap, char* reason, size_t reason_cap) {
    const Refusal no{reason, reason_cap};
    if (reason && reason_cap) reason[0] = 0;
    if (!p || !info) return no("null argument");
    std::memset(info, 0, sizeof(*info));
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return no("not a JPEG file (no SOI marker)");
    if (n >= kMaxFileBytes) return no("file of %zu bytes (the decoder takes files below %zu)", n, kMaxFileBytes);

    uint8_t qt[4][64];
    bool qt_set[4] = {false, false, false, false}, huff_set[2][2] = {{false, false}, {false, false}};
    must3r_hip_jpeg_huff* huff[2][2] = {{&info->dc[0], &info->dc[1]}, {&info->ac[0], &info->ac[1]}};
    bool have_sof = false, have_scan = false, jfif = false, adobe = false;
    int minlen[2][2] = {{16, 16}, {16, 16}};   // the shortest code of each Huffman table
    int adobe_transform = -1, nf = 0, cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    uint32_t ri = 0;
    size_t found_segments = 0;
    size_t pos = 2;
    for (;;) {
        // the next marker: FF, any number of fill FFs, the code
        if (pos + 2 > n) return no(have_scan ? "no EOI marker after the scan" : "file ends before a scan (cut at byte %zu)", pos);
        if (p[pos] != 0xFF) return no("byte 0x%02X at %zu where a marker must stand", p[pos], pos);
        while (pos + 1 < n && p[pos + 1] == 0xFF) ++pos;
        if (pos + 2 > n) return no("file ends inside a marker");
        const int m = p[pos + 1];
        pos += 2;
        if (m == 0xD9) {
            if (!have_scan) return no("EOI before any scan");
            break;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
            if (m != 0x01) return no("restart marker outside a scan");
            continue;
        }
        if (m == 0xD8) return no("second SOI marker");
        if (m == 0x00) return no("stuffed zero outside a scan");
        if (pos + 2 > n) return no("file ends inside the length of marker 0x%02X", m);
        const size_t L = ((size_t)p[pos] << 8) | p[pos + 1];
        if (L < 2 || pos + L > n) return no("marker 0x%02X: length %zu points past the end of the file", m, L);
        const uint8_t* s = p + pos + 2;   // payload, L - 2 bytes
        const size_t pl = L - 2;
        if (have_scan) {
            if (m == 0xDA) return no("several scans (non-interleaved or progressive file)");
            if (m == 0xDC) return no("DNL marker");
            pos += L;   // tables or application data after the only scan: nothing reads them
            continue;
        }
        switch (m) {
        case 0xC0:
        case 0xC1: {
            if (have_sof) return no("second frame header");
            if (pl < 6) return no("frame header too short");
            if (s[0] != 8) return no("%d-bit samples (8-bit only)", s[0]);
            const int H = (s[1] << 8) | s[2], W = (s[3] << 8) | s[4];
            nf = s[5];
            if (H == 0 || W == 0) return no("empty frame (%d x %d; a height from a DNL marker is not supported)", W, H);
            if (nf != 1 && nf != 3) return no("%d components (1 or 3)", nf);
            if (pl != (size_t)6 + 3 * nf) return no("frame header length does not match its %d components", nf);
            for (int c = 0; c < nf; ++c) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                ctq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) return no("component %d: sampling factors %d x %d", c, ch[c], cv[c]);
                if (ctq[c] > 3) return no("component %d: quantisation table %d", c, ctq[c]);
            }
            info->width = W;
            info->height = H;
            info->components = nf;
            have_sof = true;
            break;
        }
        case 0xC2: return no("progressive JPEG");
        case 0xC3: return no("lossless JPEG");
        case 0xC5: case 0xC6: case 0xC7: return no("differential (hierarchical) JPEG");
        case 0xC8: return no("reserved JPG marker");
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return no("arithmetic coding");
        case 0xCC: return no("arithmetic conditioning table (arithmetic coding)");
        case 0xC4: {
            size_t q = 0;
            while (q < pl) {
                if (q + 17 > pl) return no("Huffman table cut short");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 1) return no("Huffman table class %d id %d (two tables per class)", tc, th);
                uint8_t counts[17] = {0};
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += (counts[l] = s[q + l]);
                if (total > 256 || q + 17 + (size_t)total > pl) return no("Huffman table with %d symbols does not fit its segment", total);
                if (!build_huff(counts, s + q + 17, total, tc == 0, huff[tc][th])) return no("Huffman table that is no valid prefix code");
                huff_set[tc][th] = true;
                minlen[tc][th] = 16;
                for (int l = 16; l >= 1; --l)
                    if (counts[l]) minlen[tc][th] = l;
                q += 17 + (size_t)total;
            }
            break;
        }
        case 0xDB: {
            size_t q = 0;
            while (q < pl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq != 0) return no("16-bit quantisation table");
                if (tq > 3) return no("quantisation table id %d", tq);
                if (q + 65 > pl) return no("quantisation table cut short");
                std::memcpy(qt[tq], s + q + 1, 64);
                qt_set[tq] = true;
                q += 65;
            }
            break;
        }
        case 0xDD:
            if (pl != 2) return no("restart interval segment of %zu bytes", L);
            ri = ((uint32_t)s[0] << 8) | s[1];
            break;
        case 0xDC: return no("DNL marker");
        case 0xE0:
            if (pl >= 5 && std::memcmp(s, "JFIF", 5) == 0) jfif = true;
            break;
        case 0xEE:
            if (pl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = s[11];
            }
            break;
        case 0xDA: {
            if (!have_sof) return no("scan before the frame header");
            if (pl < 1) return no("scan header too short");
            const int ns = s[0];
            if (ns != nf) return no("scan of %d of the %d components (several scans)", ns, nf);
            if (pl != (size_t)4 + 2 * ns) return no("scan header length does not match its %d components", ns);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) return no("scan component %d is not frame component %d", c, c);
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return no("scan component %d: Huffman tables %d / %d", c, td, ta);
                if (!huff_set[0][td] || !huff_set[1][ta]) return no("scan component %d uses a Huffman table the file does not define", c);
                if (!qt_set[ctq[c]]) return no("component %d uses a quantisation table the file does not define", c);
                info->comp_dc[c] = td;
                info->comp_ac[c] = ta;
                for (int k = 0; k < 64; ++k) info->quant[c][k] = qt[ctq[c]][k];
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return no("spectral selection or successive approximation (progressive scan)");
            // geometry and colour, before the data is looked at
            if (nf == 1) {
                info->hs = info->vs = 1;
            } else {
                if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || !((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2)))
                    return no("sampling factors %dx%d, %dx%d, %dx%d (luma 1x1, 2x1 or 2x2 with chroma 1x1)", ch[0], cv[0], ch[1], cv[1], ch[2], cv[2]);
                info->hs = ch[0];
                info->vs = cv[0];
                if (!jfif) {   // libjpeg's rule: JFIF means YCbCr; else the Adobe transform; else the component ids
                    if (adobe) {
                        if (adobe_transform != 1) return no("Adobe APP14 transform %d (not YCbCr)", adobe_transform);
                    } else if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') {
                        return no("component ids R, G, B (not YCbCr)");
                    }
                }
            }
            info->mcus_x = (info->width + 8 * info->hs - 1) / (8 * info->hs);
            info->mcus_y = (info->height + 8 * info->vs - 1) / (8 * info->vs);
            info->blocks_per_mcu = nf == 1 ? 1 : info->hs * info->vs + 2;
            const int64_t mcus = (int64_t)info->mcus_x * info->mcus_y, blocks = mcus * info->blocks_per_mcu;
            if (blocks > kMaxBlocks) return no("%lld blocks (the decoder takes up to %lld)", (long long)blocks, (long long)kMaxBlocks);
            info->n_blocks = (int32_t)blocks;
            info->restart_interval = (int32_t)ri;
            const int64_t want_segments = ri ? (mcus + ri - 1) / ri : 1;
            info->n_segments = (int32_t)want_segments;
            for (int k = 0; k < 64; ++k) info->natural[k] = kNatural[k];
            // the entropy-coded data: up to the first marker that is neither a stuffed zero nor RSTn; one pass, which also finds the restart segments
            const size_t start = pos + L;
            size_t i = start, end = n;
            if (seg && seg_cap >= 1 && (int64_t)seg_cap >= want_segments) seg[0] = (uint32_t)start;
            found_segments = 1;
            bool ended = false;
            while (i < n) {
                const uint8_t* f = static_cast<const uint8_t*>(std::memchr(p + i, 0xFF, n - i));
                if (!f) break;
                i = (size_t)(f - p);
                if (i + 1 >= n) break;
                const int c = p[i + 1];
                if (c == 0x00) { i += 2; continue; }
                if (c == 0xFF) { i += 1; continue; }   // a fill byte in front of a marker
                if (c >= 0xD0 && c <= 0xD7) {
                    if (!ri) return no("restart marker in a file without a restart interval");
                    if (c != 0xD0 + (int)((found_segments - 1) & 7)) return no("restart marker %zu out of sequence", found_segments - 1);
                    if ((int64_t)found_segments >= want_segments) return no("more restart markers than the %lld segments of the frame", (long long)want_segments);
                    if (i > start && p[i - 1] == 0xFF) return no("fill bytes in front of a restart marker");
                    if (seg && (int64_t)seg_cap >= want_segments) seg[found_segments] = (uint32_t)(i + 2);
                    ++found_segments;
                    i += 2;
                    continue;
                }
                end = i;
                ended = true;
                break;
            }
            if (!ended) return no("no EOI marker: the scan runs to the end of the file");
            if ((int64_t)found_segments != want_segments) return no("%zu restart segments where the frame has %lld", found_segments, (long long)want_segments);
            info->scan_offset = (int64_t)start;
            info->scan_bytes = (int64_t)(end - start);
            // a block takes a DC code and an AC code at least: with the standard tables 2 + 4 bits in luma and 2 + 2 in chroma
            int64_t mcu_bits = 0;
            for (int c = 0; c < nf; ++c) mcu_bits += (int64_t)(c == 0 && nf == 3 ? info->hs * info->vs : 1) * (minlen[0][info->comp_dc[c]] + minlen[1][info->comp_ac[c]]);
            if ((int64_t)(end - start) * 8 < mcu_bits * mcus)
                return no("scan of %zu bytes is shorter than its %lld MCUs can be (%lld bits each at least)", end - start, (long long)mcus, (long long)mcu_bits);
            have_scan = true;
            pos = end;
            continue;
        }
        default:
            break;   // APPn, COM and the rest: skipped by their (checked) length
        }
        pos += L;
    }
    return 0;
}

}  // namespace jpeg
}  // namespace m3r
