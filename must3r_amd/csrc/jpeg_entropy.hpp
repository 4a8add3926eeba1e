// Baseline JPEG entropy decoding, the per-thread routine: a bit reader that skips the 00 after FF, a Huffman symbol decode through a bounded table and the
// (block slot in MCU, zig-zag index) state machine.  __host__ __device__ text: the kernels of jpeg.hip and the host program tests/c/jpeg_check.cpp run the same
// lines.  Threads of the first pass decode garbage by design, so nothing here trusts the stream: every table index is masked, every read of the stream is
// clamped to the segment (zeros beyond it), every coefficient write is checked against the segment's block count, and every loop has a bound.
#pragma once
#include <cstdint>

#include "../../include/must3r_hip.h"

#if defined(__HIPCC__)
#define M3R_JPEG_HD __host__ __device__ inline
#else
#define M3R_JPEG_HD inline
#endif

namespace m3r {
namespace jpeg {

constexpr uint32_t kSub = MUST3R_JPEG_SUBSEQ_BYTES;
constexpr int kRounds = 32;     // rounds of one synchronisation launch (a block's threads restart from their predecessors' exits)
constexpr int kLaunches = 4;    // synchronisation launches (a block's first thread takes its predecessor from the launch before)

// Where a decoder stands: `pos` is the bit position in the segment's raw bytes (stuffed zeros counted; the byte it points into is never a stuffed zero),
// `slotzz` = (block slot in the MCU << 8) | zig-zag index of the next coefficient (0: the DC symbol comes next), `nblk` the blocks completed since the entry.
struct State {
    uint32_t pos, slotzz, nblk;
};

// what the routine needs of a must3r_hip_jpeg_info (the tables may lie in LDS)
struct Scan {
    const must3r_hip_jpeg_huff* tabs;   // dc[0], dc[1], ac[0], ac[1]
    const uint8_t* natural;
    uint32_t sel;                       // per component c: bit 2c the DC table, bit 2c + 1 the AC table
    int32_t ny, bpm;                    // luma blocks per MCU, blocks per MCU
};

M3R_JPEG_HD Scan make_scan(const must3r_hip_jpeg_info* info, const must3r_hip_jpeg_huff* tabs, const uint8_t* natural) {
    Scan sc;
    sc.tabs = tabs;
    sc.natural = natural;
    sc.sel = 0;
    for (int c = 0; c < 3; ++c) sc.sel |= (uint32_t)((info->comp_dc[c] & 1) | ((info->comp_ac[c] & 1) << 1)) << (2 * c);
    sc.bpm = info->blocks_per_mcu;
    sc.ny = info->components == 1 ? 1 : info->hs * info->vs;
    return sc;
}

// restart segment s of the image: its MCUs -> (first block, blocks)
M3R_JPEG_HD void segment_blocks(const must3r_hip_jpeg_info* info, uint32_t s, uint32_t* first_block, uint32_t* blocks) {
    const uint32_t mcus = (uint32_t)info->mcus_x * (uint32_t)info->mcus_y;
    const uint32_t ri = info->restart_interval > 0 ? (uint32_t)info->restart_interval : mcus;
    const uint32_t m0 = s * ri < mcus ? s * ri : mcus;
    const uint32_t m1 = m0 + ri < mcus ? m0 + ri : mcus;
    *first_block = m0 * (uint32_t)info->blocks_per_mcu;
    *blocks = (m1 - m0) * (uint32_t)info->blocks_per_mcu;
}

M3R_JPEG_HD uint32_t byte_at(const uint8_t* d, uint32_t n, uint32_t i) { return i < n ? d[i] : 0u; }

// the state a thread assumes at the start of subsequence j of a segment: a block starts at the first bit of byte j * kSub (after a stuffed zero, if that
// byte is one); true for j = 0
M3R_JPEG_HD State assumed_state(const uint8_t* d, uint32_t n, uint32_t j) {
    uint32_t b = j * kSub;
    if (b > 0 && byte_at(d, n, b - 1) == 0xFFu && byte_at(d, n, b) == 0u) ++b;
    State s;
    s.pos = b * 8u;
    s.slotzz = 0;
    s.nblk = 0;
    return s;
}

// Decodes symbols (a Huffman code and its extra bits, at most 31 bits) from the entry state `s` while the current byte lies before `stop_byte`, fewer than
// `stop_blocks` blocks are complete and fewer than `max_steps` symbols were decoded; leaves the exit state in `s` (nblk: blocks completed here).
// coef != nullptr: writes the coefficients (row-major int16, the DC DIFFERENCE at [0]) of block `first_local + completed` of the segment at
// coef[block * 64 + ...] while block < limit_blocks; `clear`: zeroes a block when its DC symbol comes.
M3R_JPEG_HD void decode_span(const Scan& sc, const uint8_t* d, uint32_t n, uint32_t stop_byte, uint32_t stop_blocks, uint32_t max_steps, State& s, int16_t* coef,
                             uint32_t first_local, uint32_t limit_blocks, bool clear) {
    uint32_t b = s.pos >> 3, o = s.pos & 7u, slot = s.slotzz >> 8, k = s.slotzz & 63u, done = 0;
    if (slot >= (uint32_t)sc.bpm) slot = 0;
    for (uint32_t step = 0; step < max_steps && b < stop_byte && done < stop_blocks; ++step) {
        // nine raw bytes from b hold at least five data bytes (at most four FF 00 pairs in front of the fifth)
        uint64_t X = 0;
        for (uint32_t i = 0; i < 8; ++i) X = (X << 8) | byte_at(d, n, b + i);
        uint64_t Y = (uint64_t)byte_at(d, n, b + 8) << 56;
        uint64_t w = 0;
        uint32_t offs = 0, raw = 0;   // offs: nibble q = raw offset of data byte q
        for (uint32_t q = 0; q < 5; ++q) {
            const uint32_t v = (uint32_t)(X >> 56), nx = (uint32_t)(X >> 48) & 0xFFu;
            offs |= raw << (4 * q);
            w = (w << 8) | v;
            if (v == 0xFFu && nx == 0u) {
                X = (X << 16) | (Y >> 48);
                Y <<= 16;
                raw += 2;
            } else {
                X = (X << 8) | (Y >> 56);
                Y <<= 8;
                raw += 1;
            }
        }
        uint64_t x = w << (24 + o);   // the stream from the current bit, left-aligned; 40 - o >= 33 valid bits
        const uint32_t comp = slot < (uint32_t)sc.ny ? 0u : slot - (uint32_t)sc.ny + 1u;
        const uint32_t tsel = (sc.sel >> (2 * (comp < 3 ? comp : 2))) & 3u;
        const must3r_hip_jpeg_huff* h = k == 0 ? sc.tabs + (tsel & 1u) : sc.tabs + 2 + (tsel >> 1);
        uint32_t len, sym;
        const uint32_t lk = h->look[(uint32_t)(x >> 55) & 511u];
        if (lk) {
            len = lk >> 8;
            sym = lk & 255u;
        } else {
            len = 16;
            sym = 0;   // no code of 16 bits or fewer: a damaged stream; 16 bits are dropped
            for (uint32_t l = 10; l <= 16; ++l) {
                const int32_t c = (int32_t)(x >> (64 - l));
                if (c <= h->maxcode[l]) {
                    len = l;
                    sym = h->vals[(uint32_t)(c + h->valoff[l]) & 255u];
                    break;
                }
            }
        }
        x <<= len;
        const uint32_t size = sym & 15u;
        int32_t v = 0;
        if (size) {
            v = (int32_t)(x >> (64 - size));
            if (v < (1 << (size - 1))) v -= (1 << size) - 1;
        }
        const uint32_t blk = first_local + done;
        int16_t* out = (coef && blk < limit_blocks) ? coef + (size_t)blk * 64 : nullptr;
        bool end_block = false;
        if (k == 0) {
            if (out) {
                if (clear)
                    for (int i = 0; i < 64; ++i) out[i] = 0;
                out[0] = (int16_t)v;
            }
            k = 1;
        } else {
            const uint32_t run = sym >> 4;
            if (size == 0) {
                if (run == 15) k += 16;   // ZRL
                else end_block = true;    // EOB (a run code below 15 without a size is read as one too)
            } else {
                k += run;
                if (k < 64) {
                    if (out) out[sc.natural[k & 63u] & 63u] = (int16_t)v;
                }
                k += 1;
            }
        }
        if (k >= 64) end_block = true;
        if (end_block) {
            k = 0;
            slot = slot + 1 < (uint32_t)sc.bpm ? slot + 1 : 0;
            ++done;
        }
        const uint32_t used = o + len + size;   // <= 7 + 16 + 15
        b += (offs >> (4 * (used >> 3))) & 15u;
        o = used & 7u;
    }
    s.pos = b * 8u + o;
    s.slotzz = (slot << 8) | k;
    s.nblk = done;
}

// subsequence j of a segment of n bytes: [j * kSub, min((j + 1) * kSub, n)); the bound of its symbol loop (a symbol takes a bit at least)
M3R_JPEG_HD uint32_t sub_stop(uint32_t n, uint32_t j) { return (j + 1) * kSub < n ? (j + 1) * kSub : n; }
constexpr uint32_t kSubSteps = kSub * 8 + 64;
M3R_JPEG_HD uint32_t segment_subs(uint32_t n) { return n ? (n + kSub - 1) / kSub : 1u; }

}  // namespace jpeg
}  // namespace m3r
