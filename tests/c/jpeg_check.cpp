// Stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_jpeg_host.py and run as a child process, nothing preloaded):
// the JPEG parser (csrc/jpeg_parse.hpp) and the per-thread entropy routine the kernels run (csrc/jpeg_entropy.hpp) over the files named on the command line.
//   * every file: parsed; decoded sequentially (one decoder per restart segment) and by the subsequence scheme emulated on the host (assumed states, restarts
//     from the predecessors' exits, scan of the block counts, write pass with the check of the chain, sequential pass for an image that fails it); the
//     coefficients of the two must be equal.  With --dump DIR the coefficients (int16 [blocks][64], DC differences) go to DIR/<name>.coef.
//   * every file again, damaged: seeded byte flips inside the scan, and the scan cut short in front of a fresh EOI; parsed and, if accepted, decoded both ways.
//     Nothing is compared there: the sanitizers hold every access in bounds.
// Prints one line per file and "jpeg_check: OK <files> files, <damaged> damaged variants, <fast> fast, <seq> sequential"; exit status 0 only then.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../must3r_amd/csrc/jpeg_entropy.hpp"
#include "../../must3r_amd/csrc/jpeg_parse.hpp"

using namespace m3r::jpeg;

struct Parsed {
    must3r_hip_jpeg_info info;
    std::vector<uint32_t> seg;
    std::string reason;
    bool ok = false;
};

static Parsed parse_file(const std::vector<uint8_t>& f) {
    Parsed P;
    char reason[256];
    // exact-size copy: the sanitizer sees a read one byte past the file
    std::vector<uint8_t> exact(f);
    if (parse(exact.data(), exact.size(), &P.info, nullptr, 0, reason, sizeof(reason))) {
        P.reason = reason;
        if (P.reason.empty()) {
            std::fprintf(stderr, "refusal without a reason\n");
            std::exit(2);
        }
        return P;
    }
    P.seg.assign((size_t)P.info.n_segments, 0);
    must3r_hip_jpeg_info again;
    if (parse(exact.data(), exact.size(), &again, P.seg.data(), P.seg.size(), reason, sizeof(reason)) || std::memcmp(&again, &P.info, sizeof(again)) != 0) {
        std::fprintf(stderr, "the second parse differs from the first\n");
        std::exit(2);
    }
    P.ok = true;
    return P;
}

struct Segment {
    const uint8_t* d;
    uint32_t n, first_block, blocks;
};

static std::vector<Segment> segments(const std::vector<uint8_t>& f, const Parsed& P) {
    std::vector<Segment> out;
    const int64_t end = P.info.scan_offset + P.info.scan_bytes;
    for (int s = 0; s < P.info.n_segments; ++s) {
        const int64_t a = P.seg[(size_t)s], b = s + 1 < P.info.n_segments ? (int64_t)P.seg[(size_t)s + 1] - 2 : end;
        if (a < P.info.scan_offset || b < a || b > end || b > (int64_t)f.size()) {
            std::fprintf(stderr, "segment %d outside the scan\n", s);
            std::exit(2);
        }
        Segment g;
        g.d = f.data() + a;
        g.n = (uint32_t)(b - a);
        segment_blocks(&P.info, (uint32_t)s, &g.first_block, &g.blocks);
        out.push_back(g);
    }
    return out;
}

// exact-size coefficient buffer: a write past the image's blocks is a heap overflow the sanitizer reports
static std::vector<int16_t> decode_sequential(const std::vector<uint8_t>& f, const Parsed& P) {
    std::vector<int16_t> coef((size_t)P.info.n_blocks * 64, 0);
    const Scan sc = make_scan(&P.info, &P.info.dc[0], P.info.natural);
    for (const Segment& g : segments(f, P)) {
        State st{0, 0, 0};
        decode_span(sc, g.d, g.n, g.n, g.blocks, g.n * 8u + 64u, st, coef.data() + (size_t)g.first_block * 64, 0, g.blocks, true);
    }
    return coef;
}

static std::vector<int16_t> decode_subsequences(const std::vector<uint8_t>& f, const Parsed& P, bool* fast) {
    std::vector<int16_t> coef((size_t)P.info.n_blocks * 64, 0);
    const Scan sc = make_scan(&P.info, &P.info.dc[0], P.info.natural);
    bool failed = false;
    const std::vector<Segment> segs = segments(f, P);
    for (const Segment& g : segs) {
        const uint32_t ns = segment_subs(g.n);
        std::vector<State> ex(ns), used(ns);
        for (uint32_t j = 0; j < ns; ++j) {   // the first pass: every subsequence from its assumed state
            used[j] = assumed_state(g.d, g.n, j);
            ex[j] = used[j];
            decode_span(sc, g.d, g.n, sub_stop(g.n, j), 0xFFFFFFFFu, kSubSteps, ex[j], nullptr, 0, 0, false);
        }
        for (int round = 0; round < kRounds * kLaunches; ++round) {   // restarts from the predecessors' exits of the round before
            std::vector<State> prev(ex);
            bool any = false;
            for (uint32_t j = 1; j < ns; ++j) {
                if (prev[j - 1].pos == used[j].pos && prev[j - 1].slotzz == used[j].slotzz) continue;
                used[j] = State{prev[j - 1].pos, prev[j - 1].slotzz, 0};
                ex[j] = used[j];
                decode_span(sc, g.d, g.n, sub_stop(g.n, j), 0xFFFFFFFFu, kSubSteps, ex[j], nullptr, 0, 0, false);
                any = true;
            }
            if (!any) break;
        }
        uint32_t base = 0;
        for (uint32_t j = 0; j < ns; ++j) {   // the scan and the write pass
            State entry{0, 0, 0};
            if (j) entry = State{ex[j - 1].pos, ex[j - 1].slotzz, 0};
            if (entry.pos != used[j].pos || entry.slotzz != used[j].slotzz) failed = true;
            decode_span(sc, g.d, g.n, sub_stop(g.n, j), 0xFFFFFFFFu, kSubSteps, entry, coef.data() + (size_t)g.first_block * 64, base, g.blocks, false);
            base += ex[j].nblk;
        }
    }
    if (failed)
        for (const Segment& g : segs) {
            State st{0, 0, 0};
            decode_span(sc, g.d, g.n, g.n, g.blocks, g.n * 8u + 64u, st, coef.data() + (size_t)g.first_block * 64, 0, g.blocks, true);
        }
    *fast = !failed;
    return coef;
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    std::fseek(fp, 0, SEEK_END);
    const long n = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    out->resize(n > 0 ? (size_t)n : 0);
    const size_t got = out->empty() ? 0 : std::fread(out->data(), 1, out->size(), fp);
    std::fclose(fp);
    return got == out->size();
}

static uint32_t rng_state = 12345;
static uint32_t rng() {   // xorshift32, seeded per file
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

int main(int argc, char** argv) {
    const char* dump = nullptr;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--sizes")) {   // the layout ctypes must agree with
            std::printf("sizes: huff %zu info %zu image %zu batch %zu\n", sizeof(must3r_hip_jpeg_huff), sizeof(must3r_hip_jpeg_info), sizeof(must3r_hip_jpeg_image),
                        sizeof(must3r_hip_jpeg_batch));
            continue;
        }
        if (!std::strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
        else paths.push_back(argv[i]);
    }
    int files = 0, damaged = 0, n_fast = 0, n_seq = 0, refused = 0;
    for (const char* path : paths) {
        std::vector<uint8_t> f;
        if (!read_file(path, &f)) {
            std::fprintf(stderr, "cannot read %s\n", path);
            return 2;
        }
        const Parsed P = parse_file(f);
        const char* name = std::strrchr(path, '/') ? std::strrchr(path, '/') + 1 : path;
        if (!P.ok) {
            std::printf("%s: refused: %s\n", name, P.reason.c_str());
            ++refused;
            ++files;
            continue;
        }
        const std::vector<int16_t> a = decode_sequential(f, P);
        bool fast = false;
        const std::vector<int16_t> b = decode_subsequences(f, P, &fast);
        if (a != b) {
            std::fprintf(stderr, "%s: the subsequence scheme and the sequential decode differ\n", name);
            return 1;
        }
        (fast ? n_fast : n_seq)++;
        std::printf("%s: %d x %d, %d blocks, %d segments, %s\n", name, P.info.width, P.info.height, P.info.n_blocks, P.info.n_segments, fast ? "fast" : "sequential");
        if (dump) {
            const std::string out = std::string(dump) + "/" + name + ".coef";
            FILE* fp = std::fopen(out.c_str(), "wb");
            if (!fp || std::fwrite(a.data(), 2, a.size(), fp) != a.size()) return 2;
            std::fclose(fp);
        }
        ++files;
        // damaged variants: in bounds, nothing compared
        rng_state = 0x9E3779B9u ^ (uint32_t)f.size();
        const size_t s0 = (size_t)P.info.scan_offset, sn = (size_t)P.info.scan_bytes;
        for (int v = 0; v < 6 && sn > 0; ++v) {
            std::vector<uint8_t> g(f);
            if (v < 4) {
                const int flips = 1 + (int)(rng() % 8);
                for (int k = 0; k < flips; ++k) g[s0 + rng() % sn] ^= (uint8_t)(1u << (rng() % 8));
                if (v == 3) g[s0 + rng() % sn] = 0xFF;   // a stray marker prefix
            } else {
                const size_t keep = v == 4 ? sn - sn / 4 : (rng() % sn);   // the scan cut short, a fresh EOI behind it
                g.resize(s0 + keep);
                g.push_back(0xFF);
                g.push_back(0xD9);
            }
            const Parsed Q = parse_file(g);
            if (Q.ok) {
                bool dummy;
                (void)decode_sequential(g, Q);
                (void)decode_subsequences(g, Q, &dummy);
            }
            ++damaged;
        }
        // and the file cut in mid-scan with nothing behind it: the parser must refuse
        std::vector<uint8_t> cut(f.begin(), f.begin() + (long)(s0 + sn / 2));
        if (parse_file(cut).ok) {
            std::fprintf(stderr, "%s: accepted although cut in mid-scan\n", name);
            return 1;
        }
    }
    std::printf("jpeg_check: OK %d files (%d refused), %d damaged variants, %d fast, %d sequential\n", files, refused, damaged, n_fast, n_seq);
    return 0;
}
