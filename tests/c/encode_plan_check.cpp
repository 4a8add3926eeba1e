// Stand-alone host program over must3r_amd/csrc/encode_plan.hpp, the rule that cuts the encoder's views into chunks: the header, gemm_route.hpp and the standard
// library, nothing else, so the plan is evaluated without a GPU.  tests/test_encode_plan_host.py builds it with -fsanitize=address,undefined and runs it.
//
//   encode_plan_check                          checks the properties below, prints one line per check; exit status 1 and a "FAIL" line where one does not hold
//   encode_plan_check N TOKENS C F ROW_CAP     prints the plan of that call at the default options: "<chunks, largest first> | <cost in rounds of 256-wide tiles over K = 1024>"
//
// The equal split it compares with (what must3r_hip_encode did before the plan) and the fill of a chunk are restated here, not taken from the header.
#include "../../must3r_amd/csrc/encode_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

using namespace m3r;

static const GemmOpts kDefaults = {1, 1, 1, 1, 1, 1, 1, 0, 0};   // GEMM256 G256K G256P G256P_SPLIT SPARSE_256 SPARSE_LO BK128 PERSIST, CUS unread (misc.hip kOpts)
static int g_failed = 0;

#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);   \
            printf(__VA_ARGS__);                                     \
            printf("\n");                                            \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

// the rule the plan replaces: at most row_cap / tokens views a chunk, then that many chunks of equal size
static std::vector<int> equal_split(int n, int tokens, int cap) {
    int per = cap / tokens;
    if (per < 1) per = 1;
    const int nch = (n + per - 1) / per;
    per = (n + nch - 1) / nch;
    std::vector<int> out;
    for (int v0 = 0; v0 < n; v0 += per) out.push_back(n - v0 < per ? n - v0 : per);
    return out;
}

static double plan_units(const std::vector<int>& plan, int tokens, int C, int F, const GemmOpts& o) {
    int64_t cost = 0;
    for (int v : plan) cost += encode_chunk_cost((int64_t)v * tokens, C, F, o);
    return encode_cost_units(cost);
}

// the weighted rounds a chunk would cost if partial rounds were free, over what it is charged: ViT-L at MUST3R_F16_WA on 256 x 256 tiles
// (qkv 1.5 passes over K = C, proj 1.5 over C, fc1 1 over C, fc2 1 over F)
static double chunk_fill(int views, int tokens, int C, int F, const GemmOpts& o) {
    const double rb = (double)(((int64_t)views * tokens + 255) / 256);
    const double k = C / 1024.0, kf = F / 1024.0;
    const double ideal = rb * (3 * C / 256) / 256.0 * 1.5 * k + rb * (C / 256) / 256.0 * 1.5 * k + rb * (F / 256) / 256.0 * k + rb * (C / 256) / 256.0 * kf;
    return ideal / encode_cost_units(encode_chunk_cost((int64_t)views * tokens, C, F, o));
}

static bool valid(const std::vector<int>& plan, int n, int tokens, int cap) {
    int per = cap / tokens;
    if (per < 1) per = 1;
    long sum = 0;
    for (int v : plan) {
        if (v < 1 || v > per) return false;
        sum += v;
    }
    return sum == n;
}

static void print_plan(const char* what, const std::vector<int>& plan, double units) {
    printf("%s:", what);
    for (size_t i = 0; i < plan.size();) {
        size_t j = i;
        while (j < plan.size() && plan[j] == plan[i]) ++j;
        printf(" %zux%d", j - i, plan[i]);
        i = j;
    }
    printf(" | %.2f\n", units);
}

static int run_checks() {
    const int T = 768, C = 1024, F = 4096, CAP = 32768;
    // 1: every n_views in 1 .. 600 at the flagship shape
    int fewer = 0, cheaper = 0;
    for (int n = 1; n <= 600; ++n) {
        const std::vector<int> plan = encode_plan(n, T, C, F, CAP, kDefaults), eq = equal_split(n, T, CAP);
        CHECK(valid(plan, n, T, CAP), "n = %d: the sizes do not sum to n, or a chunk is over the cap", n);
        CHECK(plan.size() <= eq.size(), "n = %d: %zu chunks, the equal split makes %zu", n, plan.size(), eq.size());
        const double a = plan_units(plan, T, C, F, kDefaults), b = plan_units(eq, T, C, F, kDefaults);
        CHECK(a <= b, "n = %d: cost %.2f over the equal split's %.2f", n, a, b);
        CHECK(plan == encode_plan(n, T, C, F, CAP, kDefaults), "n = %d: two calls, two plans", n);
        for (size_t i = 1; i < plan.size(); ++i) CHECK(plan[i - 1] >= plan[i], "n = %d: not largest first", n);
        fewer += plan.size() < eq.size();
        cheaper += a < b;
    }
    printf("1 .. 600 views: cheaper than the equal split at %d view counts, fewer chunks at %d\n", cheaper, fewer);
    CHECK(cheaper > 0, "the plan never differs from the equal split");
    // 2: the flagship step
    {
        const std::vector<int> plan = encode_plan(560, T, C, F, CAP, kDefaults), eq = equal_split(560, T, CAP);
        const double a = plan_units(plan, T, C, F, kDefaults), b = plan_units(eq, T, C, F, kDefaults);
        print_plan("560 views, plan", plan, a);
        print_plan("560 views, equal split", eq, b);
        CHECK(b == 392.0 && eq.size() == 14 && eq[0] == 40, "14 x 40 should count 392, counted %.2f", b);
        CHECK(a <= 375.5, "560 views: %.2f weighted rounds, more than 375.5", a);
    }
    // 3: 100 views: every chunk but at most one (the remainder) fills its rounds to 90 %
    {
        const std::vector<int> plan = encode_plan(100, T, C, F, CAP, kDefaults), eq = equal_split(100, T, CAP);
        print_plan("100 views, plan", plan, plan_units(plan, T, C, F, kDefaults));
        print_plan("100 views, equal split", eq, plan_units(eq, T, C, F, kDefaults));
        int under = 0;
        for (int v : plan) {
            const double f = chunk_fill(v, T, C, F, kDefaults);
            printf("  chunk of %d views: fill %.1f %%\n", v, 100 * f);
            under += f < 0.90;
        }
        CHECK(under <= 1, "100 views: %d chunks under 90 %% fill", under);
        CHECK(chunk_fill(40, T, C, F, kDefaults) == 0.9375, "a 40-view chunk should count 93.75 %%");
    }
    // 4: 224 x 224 inputs (196 tokens a view: 167 views a chunk, row counts that are no multiple of 256)
    for (int n : {1, 2, 20, 128, 167, 168, 200, 334, 335, 560, 1000, 3000}) {
        const std::vector<int> plan = encode_plan(n, 196, C, F, CAP, kDefaults), eq = equal_split(n, 196, CAP);
        CHECK(valid(plan, n, 196, CAP) && plan.size() <= eq.size(), "196 tokens, n = %d: invalid plan", n);
        CHECK(plan_units(plan, 196, C, F, kDefaults) <= plan_units(eq, 196, C, F, kDefaults), "196 tokens, n = %d: dearer than the equal split", n);
        CHECK(plan == encode_plan(n, 196, C, F, CAP, kDefaults), "196 tokens, n = %d: two calls, two plans", n);
        if (n <= 167) CHECK(plan.size() == 1 && plan[0] == n, "196 tokens, n = %d: fits one chunk", n);
    }
    // 5: shapes the rule does not send to the 256-row kernels keep the equal split: small chunks (the smallest cap), a small model, GEMM256 = 0, one-view chunks
    {
        GemmOpts off = kDefaults;
        off.gemm256 = 0;
        struct Case { int n, tokens, C, F, cap; const GemmOpts* o; };
        const Case cases[] = {{7, 48, 1024, 4096, 256, &kDefaults},   {7, 48, 128, 512, 256, &kDefaults},   {560, 768, 1024, 4096, CAP, &off},
                              {100, 768, 1024, 4096, 768, &kDefaults}, {9, 768, 1024, 4096, 100, &kDefaults}, {50, 196, 128, 512, 2048, &kDefaults},
                              {600, 768, 1024, 4096, 4096, &kDefaults}};
        for (const Case& k : cases) {
            const std::vector<int> plan = encode_plan(k.n, k.tokens, k.C, k.F, k.cap, *k.o), eq = equal_split(k.n, k.tokens, k.cap);
            CHECK(plan == eq, "n = %d, %d tokens, C = %d, cap %d: not the equal split", k.n, k.tokens, k.C, k.cap);
            CHECK(plan == encode_plan(k.n, k.tokens, k.C, k.F, k.cap, *k.o), "n = %d, %d tokens: two calls, two plans", k.n, k.tokens);
        }
        const std::vector<int> ragged = encode_plan(7, 48, 1024, 4096, 256, kDefaults);
        CHECK(ragged.size() == 2 && ragged[0] == 4 && ragged[1] == 3, "7 views of 48 tokens under 256 rows: 4 + 3");
        CHECK(encode_plan(0, T, C, F, CAP, kDefaults).empty() && encode_plan(-3, T, C, F, CAP, kDefaults).empty(), "no views, no chunks");
    }
    // 6: a few thousand views, and the other caps the option allows
    for (int cap : {256, 16384, 49152, 1 << 22})
        for (int n : {1, 41, 1000, 4000}) {
            const std::vector<int> plan = encode_plan(n, T, C, F, cap, kDefaults), eq = equal_split(n, T, cap);
            CHECK(valid(plan, n, T, cap) && plan.size() <= eq.size(), "cap %d, n = %d: invalid plan", cap, n);
            CHECK(plan_units(plan, T, C, F, kDefaults) <= plan_units(eq, T, C, F, kDefaults), "cap %d, n = %d: dearer than the equal split", cap, n);
        }
    printf(g_failed ? "FAIL: %d checks\n" : "OK\n", g_failed);
    return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 6) {
        const int n = atoi(argv[1]), tokens = atoi(argv[2]), C = atoi(argv[3]), F = atoi(argv[4]), cap = atoi(argv[5]);
        if (tokens <= 0 || C <= 0 || F <= 0 || cap <= 0) { fprintf(stderr, "encode_plan_check: malformed arguments\n"); return 2; }
        const std::vector<int> plan = encode_plan(n, tokens, C, F, cap, kDefaults);
        print_plan("plan", plan, plan_units(plan, tokens, C, F, kDefaults));
        return 0;
    }
    if (argc != 1) { fprintf(stderr, "usage: encode_plan_check [N TOKENS C F ROW_CAP]\n"); return 2; }
    return run_checks();
}
