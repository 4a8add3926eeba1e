// Which GEMM kernel family a launch gets: the rule, and nothing else.  Plain C++17 over the standard library -- no HIP header, no globals, no option reads -- so that a
// host compiler builds it alone (tests/c/gemm_route_check.cpp) and the rule can be evaluated without launching anything.  gemm.hip fills GemmShape from
// (DType, Epi, GemmArgs) and GemmOpts from the option table, asks gemm_route() and launches what it answers; model.hip asks gemm_fold256_shape_ok() through gemm.hip.
#pragma once

namespace m3r {

enum Epi {
    EPI_STORE16 = 0,   // out 16-bit [M,ldc]
    EPI_STORE16_GELU,  // out 16-bit, exact-erf GELU
    EPI_QKV_ROPE,      // out 16-bit, 2-D RoPE on columns < rope_cols (q and k of a fused qkv projection)
    EPI_RESID_F32,     // out fp32 [M,ldc] += acc + bias   (in-place residual stream update)
    EPI_F32,           // out fp32 = acc + bias (+ bias2 on rows >= row_start2) ; accumulate -> out += acc
    EPI_HEAD,          // fp32 pixel-shuffled scatter into [view][H][W][7] (weights pre-permuted) ; accumulate alike
    EPI_COUNT
};

// what the rule reads of a launch
struct GemmShape {
    bool fp16;            // DT_F16 (else bf16)
    Epi epi;
    int M, N, K;
    int wsplit;           // GemmArgs::wsplit: 2 = [hi | lo] weights, anything else plain
    int batch;            // GemmArgs::batch: 0 / 1 = one problem
    bool rope_tab;        // GemmArgs::rope_tab != nullptr
    bool sparse;          // the packed 2:4-sparse low part is there (Wlo_sp && Widx_sp)
    bool ln_consumer;     // LN-fold consumer (ln_stats != nullptr)
    bool ln_producer;     // LN-fold producer (any of x16_out, copy32_out, stats_out)
    bool fold256;         // GemmArgs::fold256
};

// the option values the rule reads (options.hpp; ranges in misc.hip::kOpts) and the CU count the persistent test compares with (read only when persist != 0)
struct GemmOpts {
    int gemm256, g256k, g256p, g256p_split, sparse_256, sparse_lo, bk128, persist;
    int cus;
};

enum GemmFamily {
    GF_NONE = 0,   // refused: no kernel
    GF_G64,        // gemm_kernel 64 x 64, 4 waves, LDS ring
    GF_G64P,       // gemm_kernel 64 x 64, 8 waves, whole-LDS ring, pipelined fragment reads
    GF_G128,       // gemm_kernel 128 x 128 (plain) / 128 x 64 (split), 2 stages
    GF_G48,        // gemm48_kernel, 64-deep K-tiles
    GF_G48K128,    // gemm48_kernel, 128-deep K-tiles
    GF_G96,        // gemm96_kernel
    GF_G256,       // gemm256_kernel, one block per CU
    GF_G256O2,     // gemm256_kernel 256 x 128, two blocks per CU
    GF_G256K,      // gemm256k_kernel
    GF_G256P,      // gemm256p_kernel, plain or dense split weights
    GF_G256PS,     // gemm256p_kernel 256 x 128, sparse low part
    GF_G256S,      // gemm256s_kernel 256 x 256, sparse low part
    GF_G256PF,     // gemm256p_kernel with the LN fold (fold256, plain)
    GF_G256SF      // gemm256s_kernel with the LN fold (fold256, split)
};

struct GemmRoute {
    GemmFamily family;
    // the trace name "<name>/e<EPI>/w<ws>/n<bn>" = one symbol of a kernel trace.  On a refusal: the name the launch leaves behind, name == nullptr when it leaves
    // the thread's previous one.
    const char* name;
    int ws, bn;
    // what the launcher needs beyond the name
    int nst, pipe, wgm;   // 64 x 64 forms (and g128): ring depth, pipelined fragment reads, waves along M
    int bk;               // gemm48: K-tile depth
    int occ;              // gemm256_kernel: blocks per CU
    bool persistent;      // g256p / g256ps / g256s: the persistent tile loop
    bool fold;            // the fold256 forms
    const char* err;      // the error of a launch on this route that fails; a refusal always does
};

// Tile selection (measured on MI355X, scripts/bench_gemm.py): two resident blocks per CU beat every larger tile that
// leaves one (128x128 3-stage, 256x128 with 4 or 8 waves: 465-613 TF/s vs 644 TF/s on the scene's big-batch shapes).
//   plain weights : 128x128x64, 2 stages (64 KB)  for chip-filling grids, 64x64x64 4-stage ring (64 KB) otherwise
//   split weights : 128x64 (+64 lo) 2 stages (64 KB) / 64x64 (+64 lo) 3-stage ring (72 KB)
// K-tile depth 32 (the BK template parameter; 3-5 resident blocks per CU) was also measured: 605-626 TF/s plain,
// 397-419 vs 409 TF/s split -- no gain, so only BK = 64 is instantiated.
// minimum number of big tiles for the big-tile kernel (tunable for experiments: M3R_GEMM_MIN_BIG / _MIN_BIG_SPLIT)
static inline long min_big(bool split) { return split ? 384 : 192; }

// Launches of at most one 64 x 64 tile per CU (M = 768: proj, fc2, projq) run it with 8 waves (4 x 2, wave tile 16 x 32), a
// 6-8 slot LDS ring (one block per CU: the whole LDS can be prefetch depth) and the fragment reads of tile kt+1 issued
// before the MFMAs of tile kt (PIPE).  Measured at M = 768 with split weights: proj 8.7 -> 8.1 us, fc2 23.4 -> 20.7 us.
// What the experiments say about these launches (scripts/bench_gemm_small.py; debug builds that drop one component):
// per K-tile DMA, LDS reads and MFMAs each cost ~0.1 us ALONE (fc2: 16.3 / 16.8 / 16.6 us with one of them removed, 5.4 us
// with all three removed, 21 us with all) -- they add up instead of overlapping, whatever the ring depth (3 vs 6 slots:
// same), the bytes per tile (half the lo tile: -2 %) or the wave count; with two blocks per CU (qkv, fc1) the 4-wave form
// is as fast or faster; 64 x 32 tiles (twice the blocks, half the work each): same time per K-tile; the staggered
// two-group structure of gemm256_kernel on the 64 x 64 tile: same (fc2 20.4-21.0 us).  The slope is 0.35 us per
// 64-deep K-tile whatever the structure (proj 12 tiles 8.0 us, fc2 48 tiles 20.5 us); K off the power-of-two strides
// (3008 / 3136 instead of 3072) changes nothing, so it is not L2-channel camping either.  Open.
static inline bool small8(long tiles64) { return tiles64 <= 256; }
#ifndef SMALL_WGM
#define SMALL_WGM 4
#endif
#ifndef SMALL8_NST_SPLIT
#define SMALL8_NST_SPLIT 6   // 6 x 24 KB = 144 KB: one block per CU anyway, so the whole LDS can be prefetch depth
#endif
#ifndef SMALL8_NST_PLAIN
#define SMALL8_NST_PLAIN 8   // 8 x 16 KB = 128 KB
#endif

static inline bool use_48(const GemmShape& g, long nb) {
    if (g.N % 48 || g.K % 64 || g.rope_tab) return false;
    const long tiles = (long)((g.M + 47) / 48) * (g.N / 48) * nb;
    return tiles <= 256 && tiles >= 192;
}
// BK128 (A/B instrument): 0 = 64-deep K-tiles everywhere (the r03 kernels).  Measured (profiles/r04_bk128_m768.txt): same
// bits; fc2 (K = 3072) 17.4 -> 14.1 us plain, 19.0 -> 17.9 us split; the K = 768 launches +-0.2 us (their 12 tiles are not what they spend their
// time on); one-scene-at-a-time 331 -> 336 views/s.  The same depth in the 64 x 64 ring kernels (2 x 128-deep stages): qkv 11.1 -> 15.1 us,
// K|V 10.2 -> 14.4 us, fc1 13.3 -> 12.5 us, scene 326 views/s -- not kept.
static inline int bk_48(int K, const GemmOpts& o) { return K % 128 == 0 && K >= 256 && o.bk128 != 0 ? 128 : 64; }

// 96 x 96 tiles: split weights, one round of 224..256 tiles (M = 768: fc1 / feedback fc1 = 256 tiles; measured 17.8 -> 13.3 us);
static inline bool use_96(const GemmShape& g, long nb) {
    if (g.N % 96 || g.K % 64) return false;
    const long tiles = (long)((g.M + 95) / 96) * (g.N / 96) * nb;
    return tiles <= 256 && tiles >= 224;   // (qkv at M = 768 is 192 tiles = 75 % of the CUs: measured 12.3 us vs 11.2 us on 64 x 64 tiles)
}

// GEMM256: 0 = never use the 8-wave kernels, 1 = by the fill rule below (default), 2 = whenever the shape allows it
// the 8-wave kernel holds one block per CU: use it when its rounds over the 256 CUs are reasonably full
static inline int fill256(long tiles) {   // percentage of the CU slots of its rounds that do work
    const long rounds = (tiles + 255) / 256;
    return (int)(tiles * 100 / (rounds * 256));
}
// G256P (r05): the phase-staggered 64-deep kernel (gemm256p_kernel, two phases per K-tile, two barriers per phase) for the chip-filling launches.
//   plain weights  (G256P, default 1): 0 never (gemm256k_kernel), 1 every epilogue but the RoPE one (its instantiation spills), measured on the
//                  nine shapes of scripts/exp_gemm256.py: 2-6 % faster on each (profiles/r05_g256p_plain_ab.txt), 987 -> 1113 TF/s at K = 16384;
//   split weights  (G256P_SPLIT, default 1): 0 never, 1 where its 256 x 128 tiles fill their rounds at least as well as the widest tile gemm256_kernel
//                  would pick (decoder qkv N = 2304: 109 -> 103 us, K|V N = 1536: 72.6 -> 65.2 us; NOT the 256-wide encoder qkv 160 -> 162 us or the
//                  192-wide decoder proj 44.7 -> 51.8 us, profiles/r05_g256p_split_ab.txt), 2 whenever the shape allows.
// The other forms measured in r05: four phases per K-tile and one barrier per phase with group 1 lagging are template arguments of gemm256p_kernel the library does
// not instantiate; gemm256n (one phase per K-tile), gemm256pp (persistent tiles), gemm256q (one barrier per K-tile) and gemm256w (four waves, 128 x 128 wave tiles) live
// in scripts/probes/lab/*.inc and are compiled only with -DM3R_GEMM_LAB (scripts/probes/kloop_lab.hip).
// (r04, measured and removed: two 256 x 128 blocks per CU -- the GELU launches' OCC = 2 form -- for the other split-weight epilogues, so that one
// block's fp32 read-modify-write epilogue runs under the other's K loop: RESID proj 44.7 -> 52.1 us (dec) / 67.2 -> 68.2 us (enc), fc2 122 -> 152 us,
// STORE16 K|V 71.9 -> 77.8 us, RoPE qkv +-1 %; nine split shapes 1246 -> 1308 us, step 497.6 -> 487.9 views/s.  profiles/r04_occ2_ab.txt.)
// (r04, measured and removed: the same two-blocks-per-CU form for the PLAIN-weight GELU launches instead of gemm256k -- enc fc1 146.8 -> 172.8 us, dec fc1 92.6 ->
// 105.4 us, step 495.9 -> 486.3 views/s: the 64-byte DMA rows and 256 x 128 tiles cost more than the hidden erf epilogue (~8 us of a 39 us tile) gives back.
// profiles/r04_plain_gelu_occ2.txt.)

// r06: does the default rule below send a chip-filling launch of this shape to gemm256s_kernel (split, sparse low part) / gemm256p_kernel<.., 1, 256> (plain)?
// Only then is the LN fold offered (kernels.hpp): forcing 256 x 256 tiles on a launch the fill rule gives to another tile would cost more than the fold returns.
static inline bool gemm_fold256_shape_ok(int M, int N, int K, bool split, const GemmOpts& o) {
    if (M <= 0 || M % 256 != 0 || N % 256 != 0 || K % 64 != 0 || o.gemm256 != 1) return false;
    const long rb256 = M / 256, t256 = rb256 * (N / 256), t128 = rb256 * (N / 128);
    if (t256 < 200 || fill256(t256) < 80) return false;
    if (!split) return o.g256p != 0;
    return o.g256p_split != 0 && o.sparse_256 != 0 && o.sparse_lo != 0 && fill256(t256) + 12 >= fill256(t128);
}

static inline GemmRoute gemm_route(const GemmShape& g, const GemmOpts& o) {
    const long nb = g.batch > 1 ? g.batch : 1;
    const Epi epi = g.epi;
    GemmRoute r = {GF_NONE, nullptr, 0, 0, 0, 0, 0, 0, 0, false, false, "gemm: kernel launch failed"};
    auto run = [&r](GemmFamily f, const char* name, int ws, int bn) { r.family = f; r.name = name; r.ws = ws; r.bn = bn; return r; };
    auto refuse = [&r](const char* name, int ws, int bn) { r.family = GF_NONE; r.name = name; r.ws = ws; r.bn = bn; return r; };
    auto ring64 = [&r](int nst, int pipe, int wgm) { r.nst = nst; r.pipe = pipe; r.wgm = wgm; };
    if (g.fold256) {   // r06: the LN fold on the chip-filling tiles -- the caller asked gemm_fold256_shape_ok first; launch_gemm validated the operands
        r.err = "gemm: fold256 is built for fp16: split STORE16 / QKV_ROPE / RESID_F32 and plain STORE16_GELU / RESID_F32";
        const bool split = g.wsplit == 2;
        if (!g.fp16 || !(split ? epi == EPI_STORE16 || epi == EPI_QKV_ROPE || epi == EPI_RESID_F32 : epi == EPI_STORE16_GELU || epi == EPI_RESID_F32)) return refuse(nullptr, 0, 0);
        r.fold = true;
        return split ? run(GF_G256SF, "g256sf", 3, 256) : run(GF_G256PF, "g256pf", 1, 256);
    }
    // LN-fold producers (x16_out / copy32_out / stats_out) need a kernel whose epilogue carries the LN paths: the 64 x 64 / 96 / 48 tiles
    const bool lnp = g.ln_producer;
    const int mode = lnp ? 0 : o.gemm256;
    const long rb256 = (long)((g.M + 255) / 256) * nb;
    // PERSIST (A/B instrument): 1 the chip-filling kernels walk their tiles in a persistent loop when the launch has more than one round, 0 (default) never.
    // Measured (profiles/r06_gemm_persist_ab.txt, one process, interleaved rounds, identical bits): x0.96 ... x1.04 per shape, x1.003 over the 16 shapes; step 526.1 (0) vs 523.6 (1) views/s.
    auto persistent = [&](int bn) {
        const long nwork = rb256 * (g.N / bn);
        r.persistent = o.persist != 0 && nwork > o.cus && nwork < (1l << 30);
    };
    const bool small = small8((long)((g.M + 63) / 64) * (g.N / 64) * nb);
    if (g.wsplit == 2) {
        if (!g.fp16) {
            r.err = "gemm: split weights are only built for fp16";
            return refuse(nullptr, 0, 0);
        }
        const long tiles = (long)((g.M + 127) / 128) * (g.N / 64) * nb;
        const long t256 = rb256 * (g.N / 256), t192 = rb256 * (g.N / 192), t128 = rb256 * (g.N / 128);
        const bool ok256 = g.N % 256 == 0 && g.K % 32 == 0, ok128 = g.N % 128 == 0 && g.K % 32 == 0;
        // 192-column tiles (wave tile 128 x 48): N = 768 at M = 15360 is 240 tiles = ONE round at 94 % fill, where 256 columns
        // give 180 tiles (70 %) and 128 columns two rounds.  Not for the RoPE epilogue (its rotate-half pairs need 32-column
        // aligned wave tiles).
        const bool ok192 = g.N % 192 == 0 && g.K % 32 == 0 && epi != EPI_QKV_ROPE;
        int pick = 0;
        if (mode == 2) pick = !ok256 ? (ok128 ? 128 : 0) : 256;
        else if (mode == 1) {
            // cost ~ rounds over the 256 CUs x tile width; eligible when its rounds are reasonably full; ties -> wider tile
            long best = -1;
            const int bns[3] = {256, 192, 128};
            const long ts[3] = {t256, t192, t128};
            const bool oks[3] = {ok256, ok192, ok128};
            for (int i = 0; i < 3; ++i) {
                if (!oks[i] || ts[i] < 200 || fill256(ts[i]) < 80) continue;
                const long cost = ((ts[i] + 255) / 256) * bns[i];
                if (best < 0 || cost < best) { best = cost; pick = bns[i]; }
            }
        }
        if (g.ln_consumer) {
            // LN-fold consumers: the kernels that carry the row-statistics prologue, whatever the tile count
            if (epi == EPI_STORE16_GELU) return g.N % 96 == 0 ? run(GF_G96, "g96", 2, 96) : refuse("g96", 2, 96);
            if (epi == EPI_STORE16) {
                r.bk = bk_48(g.K, o);
                const char* name = r.bk == 128 ? "g48k128" : "g48";
                return g.N % 48 == 0 ? run(r.bk == 128 ? GF_G48K128 : GF_G48, name, 2, 48) : refuse(name, 2, 48);
            }
            if (epi == EPI_QKV_ROPE) { ring64(3, 0, 2); return run(GF_G64, "g64", 2, 64); }
            return refuse(nullptr, 0, 0);
        }
        // fc1 (exact-erf GELU epilogue, ~17 VALU per output) of the chip-filling batches: two 256 x 128 blocks per CU, so that one block's
        // epilogue runs under the other's K loop.  Measured (r02, M = 15360): N = 3072, K = 768: 157 -> 143 us; N = 4096, K = 1024: 270 -> 265 us;
        // every other epilogue is faster with one block per CU and the deeper ring (qkv 186 vs 199-209 us, fc2 210 vs 228 us).
        if (epi == EPI_STORE16_GELU && mode != 0 && ok128 && t128 >= 1024) { r.occ = 2; return run(GF_G256O2, "g256o2", 2, 128); }
        if (epi != EPI_HEAD && use_96(g, nb)) return run(GF_G96, "g96", 2, 96);
        if (epi != EPI_QKV_ROPE && epi != EPI_HEAD && use_48(g, nb)) {
            r.bk = bk_48(g.K, o);
            return r.bk == 128 ? run(GF_G48K128, "g48k128", 2, 48) : run(GF_G48, "g48", 2, 48);
        }
        // r05: the 2:4-sparse low part (48 matrix instructions per K-tile instead of 64) wherever the launch fills the chip and the caller has the packed copy.
        // Both sparse kernels are 256-row kernels: mode 0 (GEMM256 = 0, or an LN-fold producer) keeps them off like every other one, and the launch then
        // multiplies the dense low part, as it does with G256P_SPLIT = 0.
        if (g.sparse && mode != 0 && o.g256p_split != 0 && ok128 && g.K % 64 == 0 && t128 >= 200 && (fill256(t128) >= 80 || pick != 0)) {
            // 256 x 256 sparse tiles (48 matrix instructions per phase) where they fill their rounds about as well as the 256 x 128 ones (24 per phase, load-bound)
            if (o.sparse_256 && ok256 && t256 >= 200 && fill256(t256) + 12 >= fill256(t128)) { persistent(256); return run(GF_G256S, "g256s", 3, 256); }
            persistent(128);
            return run(GF_G256PS, "g256ps", 3, 128);
        }
        if (pick != 0 && ok128 && g.K % 64 == 0 &&
            (o.g256p_split == 2 || (o.g256p_split == 1 && (pick == 128 || (pick == 192 && t128 >= 200 && fill256(t128) >= fill256(t192) && fill256(t128) >= 90))))) {
            persistent(128);
            return run(GF_G256P, "g256p", 2, 128);
        }
        if (pick != 0 && o.g256k >= 2 && ok128) return run(GF_G256K, "g256k", 2, 128);
        if (pick != 0) { r.occ = 1; return run(GF_G256, "g256", 2, pick); }   // (two blocks per CU measured slower for every epilogue but the GELU one)
        if (tiles >= min_big(true) && !lnp) { ring64(2, 0, 2); return run(GF_G128, "g128", 2, 64); }
        if (small) { ring64(SMALL8_NST_SPLIT, 1, SMALL_WGM); return run(GF_G64P, "g64p", 2, 64); }
        ring64(3, 0, 2);
        return run(GF_G64, "g64", 2, 64);
    }
    const long tiles128 = (long)((g.M + 127) / 128) * (g.N / 128) * nb;
    const long t256 = rb256 * (g.N / 256);
    const bool ok256 = g.N % 256 == 0 && g.K % 32 == 0;
    const bool fills256 = ok256 && (mode == 2 || (mode == 1 && t256 >= 200 && fill256(t256) >= 80));
    if (g.ln_consumer) {
        // LN-fold consumers on plain weights (the Mlp fc1 of a one-view update in MUST3R_F16_WA mode): the 64 x 64 ring kernel
        if (epi == EPI_STORE16_GELU || epi == EPI_STORE16 || epi == EPI_QKV_ROPE) { ring64(4, 0, 2); return run(GF_G64, "g64", 1, 64); }
        return refuse(nullptr, 0, 0);
    }
    if (epi != EPI_QKV_ROPE && epi != EPI_HEAD && use_48(g, nb)) {   // N = 768 one-view launches: 256 tiles of 48 x 48
        r.bk = bk_48(g.K, o);
        return r.bk == 128 ? run(GF_G48K128, "g48k128", 1, 48) : run(GF_G48, "g48", 1, 48);
    }
    if (fills256 && g.K % 64 == 0 && o.g256p != 0 && epi != EPI_QKV_ROPE) { persistent(256); return run(GF_G256P, "g256p", 1, 256); }
    if (fills256 && o.g256k >= 1) return run(GF_G256K, "g256k", 1, 256);
    if (fills256) { r.occ = 1; return run(GF_G256, "g256", 1, 256); }
    if (g.N % 128 == 0 && tiles128 >= min_big(false) && !lnp) { ring64(2, 0, 2); return run(GF_G128, "g128", 1, 128); }
    if (small) { ring64(SMALL8_NST_PLAIN, 1, SMALL_WGM); return run(GF_G64P, "g64p", 1, 64); }
    ring64(4, 0, 2);
    return run(GF_G64, "g64", 1, 64);
}

}  // namespace m3r
