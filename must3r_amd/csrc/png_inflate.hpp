// PNG on the device and on the host: everything that decides a bit of the decode, as __host__ __device__ text.  csrc/png.hip compiles it into the kernels;
// tests/c/png_check.cpp compiles the same text without HIP and runs it sequentially under the host sanitizers.
//   * the canonical-code tables of RFC 1951: counts, offsets, symbols by length, a 9-bit primary look-up and maxcode / valoff for the longer codes.  Deflate
//     packs a code MSB-first into an LSB-first bit stream: the look-up is indexed by the stream's bits as they come, the long path reverses 16 of them.
//   * the bit reader, the one-symbol decode step, the dynamic header with its run codes, and the block loop.  The loop is a template over a context that
//     owns the output: on the device a 32 KiB ring in LDS that all lanes of the workgroup copy a match into, on the host the same ring in plain memory.
//   * the index of a periodic copy, the Adler-32 partial sums, the five scanline filters.
// Every loop has a bound known before it starts (a symbol takes at least a bit), every table index is masked, every write is checked against the expected size
// before the context sees it.
#pragma once
#include <cstdint>

#include "../../include/must3r_hip.h"

// In a kernel every function here is inlined, so that the bit reader and the context stay in registers, and M3R_PNG_UNIFORM tells the compiler that a value read
// from LDS at a wave-uniform address is the same in every lane: the bit buffer and the positions then live on the scalar side.
#if defined(__HIPCC__)
#define M3R_PNG_HD __host__ __device__ __forceinline__
#else
#define M3R_PNG_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define M3R_PNG_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define M3R_PNG_UNIFORM(x) (x)
#endif
#define M3R_PNG_U32(x) ((uint32_t)M3R_PNG_UNIFORM(x))

namespace m3r {
namespace png {

constexpr uint32_t kWindow = 32768, kWindowMask = kWindow - 1;
constexpr uint32_t kFlushBytes = 16384;    // the ring goes to the scanline buffer in pieces of this size: never more than kFlushBytes + 4096 bytes are unflushed
constexpr uint32_t kStoredChunk = 4096;    // a stored block enters the ring in pieces of this size
constexpr int kLookBits = 9, kMaxBits = 15;
constexpr int kMaxLitLen = 286, kMaxDist = 30, kLensBytes = 320;
constexpr uint32_t kAdlerMod = 65521;

// what tests/c/png_check.cpp sums over its corpus (a null pointer in the kernels)
struct Stats {
    uint64_t blocks[3];                  // stored, fixed, dynamic
    uint64_t matches, overlapping;       // overlapping: distance < length
    uint32_t max_distance, max_length;
    uint64_t run[3];                     // run codes 16, 17, 18
    uint64_t run_crossing;               // a run that crosses the literal / distance boundary
};

struct Huff {
    uint16_t look[1 << kLookBits];   // by the next 9 bits of the stream: (code length << 9) | symbol; 0: no code of at most 9 bits
    uint16_t vals[kLensBytes];       // the symbols in code order
    int32_t maxcode[16];             // [l]: the largest code of length l, -1 without one
    int32_t valoff[16];              // [l]: index into vals of the first code of length l, minus that code
    uint16_t offs[16];               // [l]: index into vals of the first code of length l
};

M3R_PNG_HD uint32_t length_base(uint32_t i) {
    static constexpr uint16_t t[32] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258, 0, 0, 0};
    return t[i & 31];
}
M3R_PNG_HD uint32_t length_extra(uint32_t i) {
    static constexpr uint8_t t[32] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0, 0};   // symbol 285: 258, no extra bits
    return t[i & 31];
}
M3R_PNG_HD uint32_t dist_base(uint32_t i) {
    static constexpr uint16_t t[32] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,   193,
                                257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577, 0, 0};
    return t[i & 31];
}
M3R_PNG_HD uint32_t dist_extra(uint32_t i) {
    static constexpr uint8_t t[32] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 0, 0};
    return t[i & 31];
}
M3R_PNG_HD uint32_t code_length_order(uint32_t i) {
    static constexpr uint8_t t[32] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return t[i & 31];
}
// the code length of symbol s of the fixed literal/length code (288 symbols); the fixed distance code is 32 codes of 5 bits
M3R_PNG_HD uint32_t fixed_litlen_length(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

M3R_PNG_HD uint32_t rev16(uint32_t x) {
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
    return ((x & 0x00FFu) << 8) | ((x >> 8) & 0x00FFu);
}

// ---- the table builder, in four phases that the kernel spreads over its lanes and huff_build runs one after the other -------------------------------------
// phase 1, one call per length l = 1 ... 15: how many of the n symbols have it
M3R_PNG_HD uint32_t huff_count(const uint8_t* lens, int n, int l) {
    uint32_t c = 0;
    for (int s = 0; s < n; ++s) c += lens[s] == l;
    return c;
}
// phase 2, serial: count[1 ... 15] -> maxcode, valoff, offs.  Nonzero: not a code set zlib takes -- over-subscribed, or incomplete other than a lone code of
// one bit (a literal/length or distance set) or no code at all
M3R_PNG_HD int huff_offsets(const uint16_t* count, bool is_code_lengths, Huff* h) {
    int left = 1, code = 0, p = 0, maxl = 0;
    h->maxcode[0] = -1;
    h->valoff[0] = 0;
    h->offs[0] = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
        const int c = count[l];
        left = (left << 1) - c;
        if (left < 0) return 1;
        h->offs[l] = (uint16_t)p;
        h->valoff[l] = p - code;
        h->maxcode[l] = c ? code + c - 1 : -1;
        if (c) maxl = l;
        code = (code + c) << 1;
        p += c;
    }
    if (left > 0 && maxl != 0 && (is_code_lengths || maxl != 1)) return 1;
    return 0;
}
// phase 3, one call per length l: its symbols, in symbol order
M3R_PNG_HD void huff_fill_vals(const uint8_t* lens, int n, int l, Huff* h) {
    uint32_t p = h->offs[l];
    for (int s = 0; s < n; ++s)
        if (lens[s] == l) {
            if (p < (uint32_t)kLensBytes) h->vals[p] = (uint16_t)s;
            ++p;
        }
}
// phase 4, one call per entry e = 0 ... 511 of the primary look-up: the canonical decode of the bits e as the stream would deliver them
M3R_PNG_HD uint16_t huff_look_entry(const Huff* h, uint32_t e) {
    const uint32_t code9 = rev16(e & 511u) >> (16 - kLookBits);
    for (int l = 1; l <= kLookBits; ++l) {
        const int32_t code = (int32_t)(code9 >> (kLookBits - l));
        if (code <= h->maxcode[l]) {
            const uint32_t at = (uint32_t)(code + h->valoff[l]);
            return (uint16_t)(((uint32_t)l << 9) | (h->vals[at < (uint32_t)kLensBytes ? at : 0] & 511u));
        }
    }
    return 0;
}
// the four phases in sequence; `count` is 16 entries of the caller's
M3R_PNG_HD int huff_build(const uint8_t* lens, int n, bool is_code_lengths, Huff* h, uint16_t* count) {
    count[0] = 0;
    for (int l = 1; l <= kMaxBits; ++l) count[l] = (uint16_t)huff_count(lens, n, l);
    if (huff_offsets(count, is_code_lengths, h)) return 1;
    for (int l = 1; l <= kMaxBits; ++l) huff_fill_vals(lens, n, l, h);
    for (uint32_t e = 0; e < (1u << kLookBits); ++e) h->look[e] = huff_look_entry(h, e);
    return 0;
}

// ---- the bit reader: Src::word(i) is the i-th little-endian 32-bit word of the stream, zero beyond its end --------------------------------------------------
template <class Src>
struct BitReader {
    Src src;
    uint64_t bb;        // the next bc bits, LSB first
    uint32_t bc;
    uint32_t next_w;    // the word that enters bb next
    uint32_t pos;       // bits consumed since the start of the stream
    M3R_PNG_HD void settle() {   // the state is the same in every lane
        bb = ((uint64_t)M3R_PNG_U32(bb >> 32) << 32) | M3R_PNG_U32(bb & 0xFFFFFFFFu);
        bc = M3R_PNG_U32(bc);
        next_w = M3R_PNG_U32(next_w);
        pos = M3R_PNG_U32(pos);
    }
    M3R_PNG_HD void refill() {
        for (int k = 0; k < 2 && bc <= 32; ++k) {
            bb |= (uint64_t)src.word(next_w++) << bc;
            bc += 32;
        }
        settle();
    }
    M3R_PNG_HD void seek(uint32_t byte) {
        next_w = byte >> 2;
        bb = 0;
        bc = 0;
        refill();
        const uint32_t s = (byte & 3u) * 8u;
        bb >>= s;
        bc -= s;
        pos = byte * 8u;
        settle();
    }
    M3R_PNG_HD uint32_t peek() {   // at least 32 valid bits
        refill();
        return (uint32_t)bb;
    }
    M3R_PNG_HD void drop(uint32_t n) {   // n <= 32, after a peek
        bb >>= n;
        bc -= n;
        pos += n;
        settle();
    }
    M3R_PNG_HD uint32_t take(uint32_t n) {   // n <= 16
        const uint32_t v = peek() & ((1u << n) - 1u);
        drop(n);
        return v;
    }
};

// the one-symbol decode step: the symbol, or -1 when the next bits are no code of the table
template <class Src>
M3R_PNG_HD int decode_symbol(const Huff* h, BitReader<Src>& br) {
    const uint32_t bits = br.peek();
    const uint32_t e = (uint32_t)M3R_PNG_UNIFORM(h->look[bits & ((1u << kLookBits) - 1u)]);
    if (e) {
        br.drop(e >> 9);
        return (int)(e & 511u);
    }
    const uint32_t code16 = rev16(bits & 0xFFFFu);
    for (int l = kLookBits + 1; l <= kMaxBits; ++l) {
        const int32_t code = (int32_t)(code16 >> (16 - l));
        if (code <= (int32_t)M3R_PNG_UNIFORM(h->maxcode[l])) {
            const uint32_t at = (uint32_t)(code + (int32_t)M3R_PNG_UNIFORM(h->valoff[l]));
            br.drop((uint32_t)l);
            return (int)M3R_PNG_UNIFORM(h->vals[at < (uint32_t)kLensBytes ? at : 0]);
        }
    }
    return -1;
}

// a match of `len` bytes at distance d: byte i of it is byte periodic_index(i, d, len) of the d bytes in front of it.  With d < len the copy is periodic,
// out[p + i] = out[p - d + i % d], and not a memcpy
// (i < 320, and d < 258 where the copy is periodic: i % d by a float reciprocal, exact after one correction either way -- the quotient is off by one at most)
M3R_PNG_HD uint32_t periodic_index(uint32_t i, uint32_t d, uint32_t len) {
    if (d >= len) return i;
    const uint32_t q = (uint32_t)((float)i * (1.0f / (float)d));
    int32_t r = (int32_t)i - (int32_t)(q * d);
    if (r < 0) r += (int32_t)d;
    if (r >= (int32_t)d) r -= (int32_t)d;
    return (uint32_t)r;
}

// ---- the dynamic block header ------------------------------------------------------------------------------------------------------------------------------
// Ctx: lens() -> uint8_t[kLensBytes], code_lens() -> uint8_t[32], litlen() / dist() -> Huff* (the code-length code is built in dist()'s place and gone before
// the distance code is), build(lens, n, is_code_lengths, Huff*) -> nonzero on an invalid set
template <class Src, class Ctx>
M3R_PNG_HD int read_dynamic_header(BitReader<Src>& br, uint32_t end_bits, Ctx& ctx, Stats* st) {
    if (br.pos + 14u > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
    const uint32_t nlen = br.take(5) + 257u, ndist = br.take(5) + 1u, ncode = br.take(4) + 4u;
    if (nlen > (uint32_t)kMaxLitLen || ndist > (uint32_t)kMaxDist) return MUST3R_PNG_STATUS_CODE_SET;
    uint8_t* cl = ctx.code_lens();
    for (uint32_t i = 0; i < 19; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) cl[code_length_order(i)] = (uint8_t)br.take(3);
    if (br.pos > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
    Huff* codes = ctx.dist();
    if (ctx.build(cl, 19, true, codes)) return MUST3R_PNG_STATUS_CODE_SET;
    uint8_t* lens = ctx.lens();
    const uint32_t total = nlen + ndist;   // at most 316
    uint32_t i = 0;
    for (uint32_t it = 0; it < total && i < total; ++it) {   // a step writes at least one length
        if (br.pos > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
        const int s = decode_symbol(codes, br);
        if (s < 0 || s > 18) return MUST3R_PNG_STATUS_CODE;
        if (s < 16) {
            lens[i++] = (uint8_t)s;
            continue;
        }
        uint32_t v = 0, rep;
        if (s == 16) {
            if (i == 0) return MUST3R_PNG_STATUS_CODE_SET;
            v = lens[i - 1];
            rep = 3u + br.take(2);
        } else if (s == 17) {
            rep = 3u + br.take(3);
        } else {
            rep = 11u + br.take(7);
        }
        if (i + rep > total) return MUST3R_PNG_STATUS_CODE_SET;
        if (st) {
            ++st->run[s - 16];
            if (i < nlen && i + rep > nlen) ++st->run_crossing;
        }
        for (uint32_t k = 0; k < rep; ++k) lens[(i + k) % (uint32_t)kLensBytes] = (uint8_t)v;
        i += rep;
    }
    if (i != total) return MUST3R_PNG_STATUS_CODE_SET;
    if (br.pos > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
    if (lens[256] == 0) return MUST3R_PNG_STATUS_CODE_SET;   // no end-of-block code
    if (ctx.build(lens, (int)nlen, false, ctx.litlen())) return MUST3R_PNG_STATUS_CODE_SET;
    if (ctx.build(lens + nlen, (int)ndist, false, ctx.dist())) return MUST3R_PNG_STATUS_CODE_SET;
    return 0;
}

// ---- the block loop: a zlib stream of zbytes bytes -> `expected` bytes through the context; MUST3R_PNG_STATUS_*; *trailer: the Adler-32 the stream states ---
// Ctx, beyond the header's: literal(at, byte), match(at, len, dist), stored(at, byte position in the stream, n), finish(total).  The loop has checked that
// the bytes fit the expected size and that the distance reaches no further back than `at` before it calls them.
template <class Src, class Ctx>
M3R_PNG_HD int inflate(BitReader<Src>& br, uint32_t zbytes, uint32_t expected, Ctx& ctx, Stats* st, uint32_t* trailer) {
    if (zbytes < 7u) return MUST3R_PNG_STATUS_ENDS_EARLY;
    const uint32_t end_byte = zbytes - 4u, end_bits = end_byte * 8u;   // the last four bytes at least are the trailer
    br.seek(2);   // the two bytes of the zlib header: the parser has checked them
    uint32_t opos = 0;
    bool fixed_ready = false, done = false;
    for (uint32_t blk = 0; blk <= end_bits / 3u && !done; ++blk) {   // a block takes three bits at least
        if (br.pos + 3u > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
        const uint32_t hdr = br.take(3), type = hdr >> 1;
        done = (hdr & 1u) != 0;
        if (type == 3) return MUST3R_PNG_STATUS_BLOCK_TYPE;
        if (st) ++st->blocks[type];
        if (type == 0) {
            uint32_t at = (br.pos + 7u) >> 3;
            if (at + 4u > end_byte) return MUST3R_PNG_STATUS_ENDS_EARLY;
            br.seek(at);
            const uint32_t len = br.take(16), nlen = br.take(16);
            if ((len ^ 0xFFFFu) != nlen) return MUST3R_PNG_STATUS_STORED_LEN;
            at += 4u;
            if (len > end_byte - at) return MUST3R_PNG_STATUS_ENDS_EARLY;
            if (len > expected - opos) return MUST3R_PNG_STATUS_OVERFLOW;
            ctx.stored(opos, at, len);
            opos += len;
            br.seek(at + len);
            continue;
        }
        if (type == 1) {
            if (!fixed_ready) {
                uint8_t* lens = ctx.lens();
                for (uint32_t s = 0; s < 288; ++s) lens[s] = (uint8_t)fixed_litlen_length(s);
                for (uint32_t s = 288; s < 320; ++s) lens[s] = 5;
                if (ctx.build(lens, 288, false, ctx.litlen()) || ctx.build(lens + 288, 32, false, ctx.dist())) return MUST3R_PNG_STATUS_CODE_SET;
                fixed_ready = true;
            }
        } else {
            fixed_ready = false;
            const int rc = read_dynamic_header(br, end_bits, ctx, st);
            if (rc) return rc;
        }
        const Huff* lit = ctx.litlen();
        const Huff* dst = ctx.dist();
        bool ended = false;
        for (uint32_t it = 0; it <= end_bits && !ended; ++it) {   // a symbol takes one bit at least
            if (br.pos >= end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
            const int sym = M3R_PNG_UNIFORM(decode_symbol(lit, br));
            opos = M3R_PNG_U32(opos);
            if (sym < 0) return MUST3R_PNG_STATUS_CODE;
            if (sym < 256) {
                if (opos >= expected) return MUST3R_PNG_STATUS_OVERFLOW;
                ctx.literal(opos, (uint32_t)sym);
                ++opos;
            } else if (sym == 256) {
                ended = true;
            } else {
                if (sym > 285) return MUST3R_PNG_STATUS_SYMBOL;
                const uint32_t li = (uint32_t)sym - 257u;
                const uint32_t len = M3R_PNG_U32(length_base(li) + br.take(length_extra(li)));
                const int ds = M3R_PNG_UNIFORM(decode_symbol(dst, br));
                if (ds < 0) return MUST3R_PNG_STATUS_CODE;
                if (ds > 29) return MUST3R_PNG_STATUS_SYMBOL;
                const uint32_t d = M3R_PNG_U32(dist_base((uint32_t)ds) + br.take(dist_extra((uint32_t)ds)));
                if (d > opos) return MUST3R_PNG_STATUS_DISTANCE;
                if (len > expected - opos) return MUST3R_PNG_STATUS_OVERFLOW;
                if (st) {
                    ++st->matches;
                    if (d < len) ++st->overlapping;
                    if (d > st->max_distance) st->max_distance = d;
                    if (len > st->max_length) st->max_length = len;
                }
                ctx.match(opos, len, d);
                opos += len;
            }
        }
        if (!ended || br.pos > end_bits) return MUST3R_PNG_STATUS_ENDS_EARLY;
    }
    if (!done) return MUST3R_PNG_STATUS_ENDS_EARLY;
    ctx.finish(opos);
    if (opos != expected) return MUST3R_PNG_STATUS_SIZE;
    br.seek((br.pos + 7u) >> 3);   // at most end_byte: four bytes are there
    uint32_t t = 0;
    for (int k = 0; k < 4; ++k) t = (t << 8) | br.take(8);
    *trailer = t;
    return MUST3R_PNG_STATUS_OK;
}

// ---- Adler-32 as partial sums ------------------------------------------------------------------------------------------------------------------------------
// s1 = 1 + sum b_i, s2 = n + sum (n - i) b_i (mod 65521), i from 0.  One word of the stream: its `valid` bytes (1 ... 4), the first of them with weight
// `weight` = n - i.  A part of up to 2^28 / 64 bytes cannot overflow the 64-bit sums.
M3R_PNG_HD void adler_word(uint32_t w, uint32_t weight, uint32_t valid, uint64_t& s1, uint64_t& s2) {
    for (uint32_t k = 0; k < 4; ++k) {
        if (k < valid) {
            const uint32_t b = (w >> (8u * k)) & 255u;
            s1 += b;
            s2 += (uint64_t)(weight - k) * b;
        }
    }
}
// the sums of all parts, each reduced mod 65521 or not, and n -> the Adler-32
M3R_PNG_HD uint32_t adler_finish(uint64_t s1, uint64_t s2, uint32_t n) {
    const uint32_t a = (uint32_t)((1u + s1 % kAdlerMod) % kAdlerMod), b = (uint32_t)((n % kAdlerMod + s2 % kAdlerMod) % kAdlerMod);
    return (b << 16) | a;
}

// ---- the scanline filters ------------------------------------------------------------------------------------------------------------------------------------
// which of a (left), b (above), c (above left) Paeth predicts with: 0, 1 or 2; ties break in the order a, b, c.  *tie (for the host program's coverage
// counters): the winner's distance equals another's, or, where c wins, the other two are equal
M3R_PNG_HD int paeth_branch(int a, int b, int c, bool* tie) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    if (pa <= pb && pa <= pc) {
        if (tie) *tie = pa == pb || pa == pc;
        return 0;
    }
    if (pb <= pc) {
        if (tie) *tie = pb == pc;
        return 1;
    }
    if (tie) *tie = pa == pb;   // c is the nearest while the other two tie
    return 2;
}
// one byte: the filtered byte x of a scanline of filter type ft (0 ... 4), with the reconstructed bytes a, b, c around it (0 outside the image)
M3R_PNG_HD uint32_t unfilter_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;   // the floor of a 9-bit sum
    else if (ft == 4) {
        const int k = paeth_branch((int)a, (int)b, (int)c, nullptr);
        pred = k == 0 ? a : k == 1 ? b : c;
    }
    return (x + pred) & 255u;
}

}  // namespace png
}  // namespace m3r
