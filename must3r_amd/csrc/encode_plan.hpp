// How the encoder cuts its views into chunks: the plan, and nothing else.  Plain C++17 over the standard library and gemm_route.hpp -- no HIP header, no globals,
// no option reads -- so that a host compiler builds it alone (tests/c/encode_plan_check.cpp).  model.hip::must3r_hip_encode asks encode_plan() and runs the chunks
// in the order it answers.
//
// The four Linears of a ViT block run on 256-row tiles with one block per CU wherever a chunk fills the chip (gemm_route.hpp), so a launch costs whole rounds over
// the 256 CUs: at 768 tokens a view and C = 1024, chunks of 40, 41 and 42 views cost the same rounds (qkv 6, proj 2, fc1 8, fc2 2), filled to 93.75 % at 40 views
// and to 98.4 % at 42.  Equal chunks (560 views under a 32768-row cap: 14 x 40) give those slots away; the plan fills them (12 x 42 + 35 + 21).
//
// The cost of a launch is  rounds x tile width x matrix passes x K,  where the rule (gemm_route) says which tile the launch gets:
//   * rounds: over 256 CUs; the tile width counts twice over where two blocks share a CU (the 256 x 128 GELU form), so a round is always one CU's 256 rows;
//   * matrix passes: 1 plain weights, 2 split weights [hi | lo], 1.5 split weights with the 2:4-sparse low part -- kept in halves (2, 4, 3), so the cost is an integer;
//   * a launch the rule sends to a smaller tile (a remainder chunk's proj and fc2) is charged as 256 x 256 tiles, no less than one full round: those kernels run at a
//     lower rate, and a remainder must not look cheap.
// The launches scored are those of MUST3R_F16_WA as encode_chunk builds them (qkv: RoPE epilogue, split weights with the sparse copy; proj: split likewise; fc1 and fc2
// plain).  The other precision modes share the plan: wherever they are on 256-row kernels their tiles are 256 wide as well, and any plan computes the same tokens.
// The model is a count, not a measurement ("Encoder chunks").
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "gemm_route.hpp"

namespace m3r {

static inline bool family_rows256(GemmFamily f) {
    return f == GF_G256 || f == GF_G256O2 || f == GF_G256K || f == GF_G256P || f == GF_G256PS || f == GF_G256S || f == GF_G256PF || f == GF_G256SF;
}

// one launch: rounds x tile width x 2 * matrix passes x K; *rows256 &= the rule sends it to a 256-row kernel
static inline int64_t encode_launch_cost(const GemmShape& g, const GemmOpts& o, bool* rows256) {
    const GemmRoute r = gemm_route(g, o);
    const int64_t passes2 = r.ws == 3 ? 3 : (r.ws == 2 || (r.ws == 0 && g.wsplit == 2)) ? 4 : 2;
    const int64_t rb = (g.M + 255) / 256;
    if (!family_rows256(r.family) || r.bn <= 0) {
        if (rows256) *rows256 = false;
        const int64_t tiles = rb * ((g.N + 255) / 256);
        return (tiles + 255) / 256 * 256 * passes2 * g.K;
    }
    const int64_t occ = r.family == GF_G256O2 ? 2 : 1;
    const int64_t tiles = rb * (g.N / r.bn);
    return (tiles + 256 * occ - 1) / (256 * occ) * r.bn * occ * passes2 * g.K;
}

// the four Linears of one encoder block on a chunk of `rows` token rows (C: width, F: hidden width of the Mlp)
static inline int64_t encode_chunk_cost(int64_t rows, int C, int F, const GemmOpts& o, bool* rows256 = nullptr) {
    if (rows256) *rows256 = true;
    if (rows <= 0 || rows > INT32_MAX) return 0;
    const int M = (int)rows;
    const bool sparse = o.sparse_lo != 0 && C % 128 == 0 && C % 64 == 0;   // model.hip::w16p packs the low part of a weight of rows % 128 == 0, K % 64 == 0
    const GemmShape qkv = {true, EPI_QKV_ROPE, M, 3 * C, C, 2, 0, true, sparse, false, false, false};
    const GemmShape proj = {true, EPI_RESID_F32, M, C, C, 2, 0, false, sparse, false, false, false};
    const GemmShape fc1 = {true, EPI_STORE16_GELU, M, F, C, 0, 0, false, false, false, false, false};
    const GemmShape fc2 = {true, EPI_RESID_F32, M, C, F, 0, 0, false, false, false, false, false};
    return encode_launch_cost(qkv, o, rows256) + encode_launch_cost(proj, o, rows256) + encode_launch_cost(fc1, o, rows256) + encode_launch_cost(fc2, o, rows256);
}
// in the unit of the counting tables: one round of 256-wide tiles, one pass over K = 1024
static inline double encode_cost_units(int64_t cost) { return (double)cost / (256.0 * 2.0 * 1024.0); }

// the largest chunk the cap allows, in views (at least one: a view of more rows than the cap is a chunk of its own)
static inline int encode_views_per_chunk(int tokens_per_view, int row_cap) {
    const int per = tokens_per_view > 0 ? row_cap / tokens_per_view : 1;
    return per < 1 ? 1 : per;
}

// chunks of equal size, the last one the remainder (80 views under a cap of 42: 2 x 40, not 42 + 38): the plan of every shape that is not on the 256-row kernels
static inline std::vector<int> encode_plan_equal(int n_views, int tokens_per_view, int row_cap) {
    std::vector<int> plan;
    if (n_views <= 0) return plan;
    int per = encode_views_per_chunk(tokens_per_view, row_cap);
    const int nch = (n_views + per - 1) / per;
    per = (n_views + nch - 1) / nch;
    for (int v0 = 0; v0 < n_views; v0 += per) plan.push_back(n_views - v0 < per ? n_views - v0 : per);
    return plan;
}

// The chunk sizes in views, largest first: they sum to n_views, none is over the cap (encode_views_per_chunk), and there are never more of them than
// encode_plan_equal makes.  Lowest total cost; ties go to fewer chunks, then to the more even split (smallest sum of squares).  A pure function of its arguments.
static inline std::vector<int> encode_plan(int n_views, int tokens_per_view, int C, int F, int row_cap, const GemmOpts& o) {
    std::vector<int> equal = encode_plan_equal(n_views, tokens_per_view, row_cap);
    if (equal.size() <= 1 || tokens_per_view <= 0 || C <= 0 || F <= 0) return equal;
    const int per = encode_views_per_chunk(tokens_per_view, row_cap);   // < n_views here
    bool rows256 = true;
    if ((int64_t)per * tokens_per_view > INT32_MAX) return equal;
    encode_chunk_cost((int64_t)per * tokens_per_view, C, F, o, &rows256);
    if (!rows256) return equal;   // the full chunk is not on the one-block-per-CU kernels: nothing to fill
    std::vector<int64_t> cost(per + 1, 0);
    for (int v = 1; v <= per; ++v) cost[v] = encode_chunk_cost((int64_t)v * tokens_per_view, C, F, o);
    struct Best { int64_t cost; int chunks; int64_t sumsq; int last; };
    std::vector<Best> best(n_views + 1, Best{0, 0, 0, 0});
    for (int n = 1; n <= n_views; ++n) {
        Best b{-1, 0, 0, 0};
        for (int v = 1; v <= per && v <= n; ++v) {
            const Best& p = best[n - v];
            const Best c{p.cost + cost[v], p.chunks + 1, p.sumsq + (int64_t)v * v, v};
            if (b.cost < 0 || c.cost < b.cost || (c.cost == b.cost && (c.chunks < b.chunks || (c.chunks == b.chunks && c.sumsq < b.sumsq)))) b = c;
        }
        best[n] = b;
    }
    if ((size_t)best[n_views].chunks > equal.size()) return equal;
    std::vector<int> plan;
    for (int n = n_views; n > 0; n -= best[n].last) plan.push_back(best[n].last);
    std::sort(plan.begin(), plan.end(), [](int a, int b) { return a > b; });
    return plan;
}

}  // namespace m3r
