// Stand-alone host program over must3r_amd/csrc/gemm_route.hpp, the rule that picks the GEMM kernel family of a launch: the header and the standard library, nothing
// else, so the rule is evaluated without a GPU.  tests/test_gemm_route_host.py builds it with -fsanitize=address,undefined and compares it with the Python restatements
// of the rule (tests/gemm_forms.py, tests/lnfold_forms.py); tests/test_gemm_route_gpu.py compares what the library launched with its answer.
//
// Lines on stdin, one answer line each on stdout:
//   o GEMM256 G256K G256P G256P_SPLIT SPARSE_256 SPARSE_LO BK128 PERSIST CUS    the option values of the lines that follow (start: the table defaults, 256 CUs); no answer
//   s fp16 epi M N K wsplit batch rope_tab sparse ln_consumer ln_producer fold256
//        -> "<family>/e<EPI>/w<WS>/n<BN>", with " persistent" behind it where the route is; a refusal: "refused: <error> | <the name it leaves, or ->"
//   f M N K split  -> "1" / "0": gemm_fold256_shape_ok
// With --grid: the lines "D", "P", "M", "N", "K", "B" (fp16 flags, ln_producer flags, sizes, batches) and one line per option name, each followed by its values; then
// the product options (in the order of the `o` line, the first slowest) x D x P x M x N x K x B x epilogue (0 .. 5) x weights (0 plain, 1 split, 2 split with the sparse
// copy) is routed with rope_tab = (epilogue is the RoPE one), and one 4-byte record per point goes to stdout: family (GemmFamily), ws, bn / 16,
// flags = persistent | fold << 1 | refusal << 2 (1 the split-weights refusal, 2 another) | gemm_fold256_shape_ok(M, N, K, weights != 0) << 4.
#include "../../must3r_amd/csrc/gemm_route.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace m3r;

static const char* const kOptNames[9] = {"GEMM256", "G256K", "G256P", "G256P_SPLIT", "SPARSE_256", "SPARSE_LO", "BK128", "PERSIST", "CUS"};
static const char* const kSplitRefusal = "gemm: split weights are only built for fp16";

static GemmOpts opts_of(const int* v) { return {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]}; }

static int run_lines() {
    int ov[9] = {1, 1, 1, 1, 1, 1, 1, 0, 256};
    char buf[1 << 12];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "o") {
            for (int& v : ov)
                if (!(in >> v)) return 2;
        } else if (kind == "s") {
            int v[12];
            for (int& x : v)
                if (!(in >> x)) return 2;
            if (v[1] < 0 || v[1] >= EPI_COUNT) return 2;
            const GemmShape g = {v[0] != 0, (Epi)v[1], v[2], v[3], v[4], v[5], v[6], v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0};
            const GemmRoute r = gemm_route(g, opts_of(ov));
            if (r.family == GF_NONE) {
                printf("refused: %s | ", r.err);
                if (r.name) printf("%s/e%d/w%d/n%d\n", r.name, v[1], r.ws, r.bn);
                else printf("-\n");
            } else {
                printf("%s/e%d/w%d/n%d%s\n", r.name, v[1], r.ws, r.bn, r.persistent ? " persistent" : "");
            }
        } else if (kind == "f") {
            int v[4];
            for (int& x : v)
                if (!(in >> x)) return 2;
            printf("%d\n", gemm_fold256_shape_ok(v[0], v[1], v[2], v[3] != 0, opts_of(ov)) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}

static int run_grid() {
    std::map<std::string, std::vector<int>> ax;
    char buf[1 << 16];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        std::string key;
        if (!(in >> key)) continue;
        int x;
        while (in >> x) ax[key].push_back(x);
    }
    std::vector<const std::vector<int>*> dims;
    for (const char* n : kOptNames) dims.push_back(&ax[n]);
    for (const char* n : {"D", "P", "M", "N", "K", "B"}) dims.push_back(&ax[n]);
    for (const auto* d : dims)
        if (d->empty()) return 2;
    std::vector<size_t> idx(dims.size(), 0);
    std::vector<unsigned char> out;
    for (;;) {
        int v[15];
        for (size_t i = 0; i < dims.size(); ++i) v[i] = (*dims[i])[idx[i]];
        const GemmOpts o = opts_of(v);
        for (int epi = 0; epi < EPI_COUNT; ++epi)
            for (int w = 0; w < 3; ++w) {
                const GemmShape g = {v[9] != 0, (Epi)epi, v[11], v[12], v[13], w ? 2 : 0, v[14], epi == EPI_QKV_ROPE, w == 2, false, v[10] != 0, false};
                const GemmRoute r = gemm_route(g, o);
                const int refusal = r.family != GF_NONE ? 0 : (strcmp(r.err, kSplitRefusal) == 0 ? 1 : 2);
                out.push_back((unsigned char)r.family);
                out.push_back((unsigned char)r.ws);
                out.push_back((unsigned char)(r.bn / 16));
                out.push_back((unsigned char)((r.persistent ? 1 : 0) | (r.fold ? 2 : 0) | refusal << 2 | (gemm_fold256_shape_ok(v[11], v[12], v[13], w != 0, o) ? 16 : 0)));
            }
        if (out.size() >= (1u << 20)) {
            if (fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 3;
            out.clear();
        }
        size_t i = dims.size();
        while (i > 0 && ++idx[i - 1] == dims[i - 1]->size()) idx[--i] = 0;
        if (i == 0) break;
    }
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 3;
}

int main(int argc, char** argv) {
    const int rc = argc > 1 && strcmp(argv[1], "--grid") == 0 ? run_grid() : run_lines();
    if (rc == 2) fprintf(stderr, "gemm_route_check: malformed input\n");
    return rc;
}
