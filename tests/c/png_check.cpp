// Stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_png_host.py and run as a child process, nothing preloaded):
// the PNG parser (csrc/png_parse.hpp) and the text the kernels compile (csrc/png_inflate.hpp) over the files named on the command line.
//   png_check --sizes                   the sizes of the ABI structs, for the ctypes layout check
//   png_check FMT:FILE ...              FMT is the MUST3R_PNG_OUT_* the pixels are wanted in; FILE.inflated holds what zlib.decompress gives for the file's
//                                       IDAT data and FILE.pixels the pixels Pillow gives, in that format
//   * every file: parsed (twice); inflated sequentially through a context that keeps the 32 KiB ring and the flush points of the kernel, into a buffer of exactly
//     the expected size; compared with FILE.inflated; the Adler-32 from 64 interleaved partial sums against the trailer; unfiltered and packed; compared with
//     FILE.pixels.
//   * first of all the index of a periodic copy, against i % d over every distance and position a match can have.
//   * every file again, damaged six ways: seeded byte flips inside the IDAT data and the data cut short.  Each must end with a status and every access stays in
//     bounds (the sanitizers); nothing is compared there.
// Prints one line per file, a "stats:" line of coverage counters summed over the files and "png_check: OK <files> files, <damaged> damaged variants"; exit
// status 0 only then.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../must3r_amd/csrc/png_inflate.hpp"
#include "../../must3r_amd/csrc/png_parse.hpp"

using namespace m3r::png;

static std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> out;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path.c_str());
        std::exit(2);
    }
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return out;
}

struct HostSrc {
    const uint8_t* z;
    uint32_t zbytes;
    uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = (uint64_t)i * 4u + k;
            if (at < zbytes) w |= (uint32_t)z[at] << (8u * k);
        }
        return w;
    }
};

// the kernel's context in plain memory: the same ring, the same flush points, the same order of reads and writes inside a match
struct HostCtx {
    std::vector<uint8_t> ring = std::vector<uint8_t>(kWindow, 0xEE);
    Huff tabs[2];
    uint8_t lens_[kLensBytes], cl_[32];
    uint16_t count_[16];
    const uint8_t* z = nullptr;
    std::vector<uint8_t>* out = nullptr;
    uint32_t flushed = 0;

    uint8_t* lens() { return lens_; }
    uint8_t* code_lens() { return cl_; }
    Huff* litlen() { return &tabs[0]; }
    Huff* dist() { return &tabs[1]; }
    int build(const uint8_t* lens, int n, bool is_code_lengths, Huff* h) { return huff_build(lens, n, is_code_lengths, h, count_); }
    void flush_piece(uint32_t from, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) out->at(from + i) = ring[(from + i) & kWindowMask];
    }
    void advance(uint32_t opos) {
        for (int k = 0; k < 2 && opos - flushed >= kFlushBytes; ++k) {
            flush_piece(flushed, kFlushBytes);
            flushed += kFlushBytes;
        }
        if (opos - flushed >= kFlushBytes) {
            std::fprintf(stderr, "more than the ring holds is unflushed\n");
            std::exit(2);
        }
    }
    void literal(uint32_t at, uint32_t b) {
        ring[at & kWindowMask] = (uint8_t)b;
        advance(at + 1u);
    }
    void match(uint32_t at, uint32_t len, uint32_t d) {
        uint8_t v[320];
        if (len > 258 || d > kWindow || d == 0 || d > at) {
            std::fprintf(stderr, "match of length %u at distance %u\n", len, d);
            std::exit(2);
        }
        for (uint32_t i = 0; i < len; ++i) v[i] = ring[(at - d + periodic_index(i, d, len)) & kWindowMask];
        for (uint32_t i = 0; i < len; ++i) ring[(at + i) & kWindowMask] = v[i];
        advance(at + len);
    }
    void stored(uint32_t at, uint32_t src, uint32_t n) {
        for (uint32_t off = 0; off < n; off += kStoredChunk) {
            const uint32_t m = n - off < kStoredChunk ? n - off : kStoredChunk;
            for (uint32_t i = 0; i < m; ++i) ring[(at + off + i) & kWindowMask] = z[src + off + i];
            advance(at + off + m);
        }
    }
    void finish(uint32_t total) { flush_piece(flushed, total - flushed); }
};

struct FilterStats {
    uint64_t rows[5] = {0, 0, 0, 0, 0};
    uint64_t paeth_tie[3] = {0, 0, 0};
    uint64_t average_carry = 0;
};

// exact-size buffers everywhere: a read or write one byte past them is a heap overflow the sanitizer reports
static int run_inflate(const std::vector<uint8_t>& z, uint32_t expected, std::vector<uint8_t>& out, Stats* st, uint32_t* trailer) {
    out.assign(expected, 0xCD);
    HostCtx ctx;
    ctx.z = z.data();
    ctx.out = &out;
    BitReader<HostSrc> br;
    br.src = HostSrc{z.data(), (uint32_t)z.size()};
    br.bb = 0, br.bc = 0, br.next_w = 0, br.pos = 0;
    return inflate(br, (uint32_t)z.size(), expected, ctx, st, trailer);
}

// Adler-32 as the kernel sums it: 64 parts, part t takes the 16-byte blocks t, t + 64, ...
static uint32_t adler_of(const std::vector<uint8_t>& b) {
    const uint32_t n = (uint32_t)b.size();
    uint64_t t1 = 0, t2 = 0;
    for (uint32_t t = 0; t < 64; ++t) {
        uint64_t s1 = 0, s2 = 0;
        for (uint32_t q = t; q < (n + 15u) / 16u; q += 64) {
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = q * 16u + 4u * j;
                const uint32_t valid = i >= n ? 0u : (n - i < 4u ? n - i : 4u);
                uint32_t w = 0;
                for (uint32_t k = 0; k < valid; ++k) w |= (uint32_t)b[i + k] << (8u * k);
                adler_word(w, n - i, valid, s1, s2);
            }
        }
        t1 += s1 % kAdlerMod;
        t2 += s2 % kAdlerMod;
    }
    return adler_finish(t1, t2, n);
}

static bool unfilter_and_pack(const must3r_hip_png_info& f, std::vector<uint8_t>& scan, int fmt, std::vector<uint8_t>& pix, FilterStats* fs) {
    const uint32_t rowbytes = (uint32_t)f.rowbytes, stride = rowbytes + 1u, bpp = (uint32_t)f.bpp, H = (uint32_t)f.height, W = (uint32_t)f.width;
    for (uint32_t r = 0; r < H; ++r) {
        const uint32_t ft = scan[(size_t)r * stride];
        if (ft > 4) return false;
        ++fs->rows[ft];
        for (uint32_t x = 0; x < rowbytes; ++x) {
            const size_t p = (size_t)r * stride + 1u + x;
            const uint32_t a = x >= bpp ? scan[p - bpp] : 0u, b = r ? scan[p - stride] : 0u, c = (r && x >= bpp) ? scan[p - stride - bpp] : 0u;
            if (ft == 3 && a + b > 255u) ++fs->average_carry;
            if (ft == 4) {
                bool tie = false;
                const int k = paeth_branch((int)a, (int)b, (int)c, &tie);
                if (tie) ++fs->paeth_tie[k];
            }
            scan[p] = (uint8_t)unfilter_byte(ft, scan[p], a, b, c);
        }
    }
    const uint32_t ob = fmt == MUST3R_PNG_OUT_RGB8 ? 3u : fmt == MUST3R_PNG_OUT_GRAY8 ? 1u : 2u;
    pix.assign((size_t)H * W * ob, 0);
    for (uint32_t r = 0; r < H; ++r)
        for (uint32_t x = 0; x < W; ++x) {
            const uint8_t* s = &scan[(size_t)r * stride + 1u + (size_t)x * bpp];
            uint8_t* d = &pix[((size_t)r * W + x) * ob];
            if (fmt == MUST3R_PNG_OUT_RGB8) {
                for (uint32_t ch = 0; ch < 3; ++ch) d[ch] = s[bpp == 1 ? 0 : ch];
            } else if (fmt == MUST3R_PNG_OUT_GRAY8) {
                d[0] = s[0];
            } else {
                d[0] = s[1];   // little-endian from PNG's big-endian samples
                d[1] = s[0];
            }
        }
    return true;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--sizes") == 0) {
        std::printf("sizes: info %zu range %zu image %zu batch %zu\n", sizeof(must3r_hip_png_info), sizeof(must3r_hip_png_range), sizeof(must3r_hip_png_image),
                    sizeof(must3r_hip_png_batch));
        return 0;
    }
    // the index of a periodic copy, over every distance and position a match can have
    for (uint32_t d = 1; d <= 258; ++d)
        for (uint32_t i = 0; i < 320; ++i)
            if (periodic_index(i, d, 259) != (d < 259 ? i % d : i) || periodic_index(i, d, d) != i) {
                std::fprintf(stderr, "periodic_index(%u, %u) is wrong\n", i, d);
                return 1;
            }
    Stats st;
    std::memset(&st, 0, sizeof(st));
    FilterStats fs;
    size_t files = 0, damaged = 0, damaged_ok = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg.size() < 3 || arg[1] != ':' || arg[0] < '0' || arg[0] > '2') {
            std::fprintf(stderr, "argument %s is not FMT:FILE\n", arg.c_str());
            return 2;
        }
        const int fmt = arg[0] - '0';
        const std::string path = arg.substr(2);
        const std::vector<uint8_t> file = read_file(path), want_inflated = read_file(path + ".inflated"), want_pixels = read_file(path + ".pixels");
        must3r_hip_png_info info, again;
        char reason[256];
        if (parse(file.data(), file.size(), &info, nullptr, 0, reason, sizeof(reason))) {
            std::fprintf(stderr, "%s: refused: %s\n", path.c_str(), reason);
            return 1;
        }
        std::vector<must3r_hip_png_range> ranges((size_t)info.n_idat);
        if (parse(file.data(), file.size(), &again, ranges.data(), ranges.size(), reason, sizeof(reason)) || std::memcmp(&again, &info, sizeof(info)) != 0) {
            std::fprintf(stderr, "%s: the second parse differs from the first\n", path.c_str());
            return 1;
        }
        std::vector<uint8_t> z;
        for (const must3r_hip_png_range& r : ranges) {
            if (r.offset + r.length > file.size()) {
                std::fprintf(stderr, "%s: IDAT range outside the file\n", path.c_str());
                return 1;
            }
            z.insert(z.end(), file.begin() + (long)r.offset, file.begin() + (long)(r.offset + r.length));
        }
        if ((int64_t)z.size() != info.idat_bytes) {
            std::fprintf(stderr, "%s: %zu bytes of IDAT where the info record has %lld\n", path.c_str(), z.size(), (long long)info.idat_bytes);
            return 1;
        }
        z.shrink_to_fit();
        std::vector<uint8_t> out, pix;
        uint32_t trailer = 0;
        const int rc = run_inflate(z, (uint32_t)info.inflated_bytes, out, &st, &trailer);
        const bool same_inflated = rc == 0 && out == want_inflated;
        const bool adler_ok = rc == 0 && adler_of(out) == trailer;
        const bool unfiltered = rc == 0 && unfilter_and_pack(info, out, fmt, pix, &fs);
        const bool same_pixels = unfiltered && pix == want_pixels;
        std::printf("%s: %d x %d, colour type %d at %d bits, %d IDAT, status %d, inflated %s, adler %s, pixels %s\n", path.c_str(), info.width, info.height,
                    info.color_type, info.bit_depth, info.n_idat, rc, same_inflated ? "equal" : "DIFFERENT", adler_ok ? "equal" : "DIFFERENT",
                    same_pixels ? "equal" : "DIFFERENT");
        if (!same_inflated || !adler_ok || !same_pixels) return 1;
        ++files;
        // damaged variants: nothing is compared, every access must stay in bounds and the decode must end with a status
        uint32_t seed = 0x9E3779B9u * (uint32_t)(a + 1);
        auto next = [&seed]() {
            seed = seed * 1664525u + 1013904223u;
            return seed >> 8;
        };
        for (int v = 0; v < 6; ++v) {
            std::vector<uint8_t> d(z);
            if (v < 4) {
                for (int k = 0; k <= v; ++k) d[2 + next() % (d.size() - 2)] ^= (uint8_t)(1u << (next() % 8));
            } else {
                d.resize(v == 4 ? d.size() / 2 + 3 : d.size() - 1 - next() % 4);
            }
            d.shrink_to_fit();
            Stats ignored;
            std::memset(&ignored, 0, sizeof(ignored));
            uint32_t t = 0;
            const int drc = run_inflate(d, (uint32_t)info.inflated_bytes, out, &ignored, &t);
            if (drc < 0 || drc > MUST3R_PNG_STATUS_FILTER) {
                std::fprintf(stderr, "%s: damaged variant %d ended with status %d\n", path.c_str(), v, drc);
                return 1;
            }
            if (drc == 0 && adler_of(out) == t) ++damaged_ok;
            ++damaged;
        }
    }
    std::printf("stats: stored=%llu fixed=%llu dynamic=%llu matches=%llu overlapping=%llu max_distance=%u max_length=%u run16=%llu run17=%llu run18=%llu "
                "run_crossing=%llu filter0=%llu filter1=%llu filter2=%llu filter3=%llu filter4=%llu paeth_tie_a=%llu paeth_tie_b=%llu paeth_tie_c=%llu "
                "average_carry=%llu damaged_intact=%zu\n",
                (unsigned long long)st.blocks[0], (unsigned long long)st.blocks[1], (unsigned long long)st.blocks[2], (unsigned long long)st.matches,
                (unsigned long long)st.overlapping, st.max_distance, st.max_length, (unsigned long long)st.run[0], (unsigned long long)st.run[1],
                (unsigned long long)st.run[2], (unsigned long long)st.run_crossing, (unsigned long long)fs.rows[0], (unsigned long long)fs.rows[1],
                (unsigned long long)fs.rows[2], (unsigned long long)fs.rows[3], (unsigned long long)fs.rows[4], (unsigned long long)fs.paeth_tie[0],
                (unsigned long long)fs.paeth_tie[1], (unsigned long long)fs.paeth_tie[2], (unsigned long long)fs.average_carry, damaged_ok);
    std::printf("png_check: OK %zu files, %zu damaged variants\n", files, damaged);
    return 0;
}
