// Stand-alone host check of the optimizer's table builder (csrc/train_optim.hip: the refusals, the chunk list, the scratch layout) under the host sanitizers.
// No GPU is needed: everything up to the upload runs on the host.  Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined scripts/checks/optim_table_sanitize.hip -o /tmp/optim_table_sanitize && /tmp/optim_table_sanitize
// (the second -fsanitize is the link step's).  Prints "ok" and exits 0.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../must3r_amd/csrc/train_optim.hip"

namespace m3r {
static char last_error[512];
int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    return 1;
}
}  // namespace m3r

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, m3r::last_error); exit(1); } \
    } while (0)

static float* addr(size_t i) { return reinterpret_cast<float*>(0x7f0000000000ull + 0x100000ull * i); }

int main() {
    const long long C = MUST3R_OPTIM_CHUNK;
    const long long ns[] = {1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, 768 * 768, (1LL << 33) + 5};
    const int n = (int)(sizeof ns / sizeof ns[0]);
    std::vector<must3r_hip_optim_tensor> tab((size_t)n);
    for (int i = 0; i < n; ++i) {
        must3r_hip_optim_tensor t{};
        t.p = addr(5 * i); t.g = addr(5 * i + 1); t.m = addr(5 * i + 2); t.v = addr(5 * i + 3); t.step = addr(5 * i + 4);
        t.n = ns[i]; t.group = i % 2;
        tab[(size_t)i] = t;
    }
    must3r_hip_optim_group groups[2] = {{1e-3, 0.05, 0.9, 0.95, 1e-8}, {3e-4, 0.0, 0.9, 0.95, 1e-8}};
    must3r_hip_optim_args a{};
    a.tensors = tab.data(); a.groups = groups; a.n_tensors = n; a.n_groups = 2;
    // the plan: every element of every tensor in exactly one chunk, in table order, chunks 16-byte aligned and at most CHUNK long
    for (int step = 0; step < 2; ++step) {
        m3r::OptPlan P;
        CHECK(m3r::opt_plan(&a, step != 0, P) == nullptr);
        long long total = 0;
        size_t c = 0;
        for (int i = 0; i < n; ++i) {
            long long off = 0;
            while (off < ns[i]) {
                CHECK(c < P.chunks.size());
                const m3r::OptChunk& ch = P.chunks[c++];
                CHECK(ch.tensor == i && ch.off == off && ch.off % 4 == 0 && ch.count >= 1 && ch.count <= C && ch.off + ch.count <= ns[i]);
                CHECK(ch.count == C || ch.off + ch.count == ns[i]);
                off += ch.count;
            }
            total += ns[i];
            CHECK(P.tensors[(size_t)i].n == ns[i] && P.tensors[(size_t)i].g == tab[(size_t)i].g);
            if (step) CHECK(P.tensors[(size_t)i].b1 == 0.9f && P.tensors[(size_t)i].decay == (float)(1.0 - groups[i % 2].lr * groups[i % 2].weight_decay));
        }
        CHECK(c == P.chunks.size() && P.total == total);
        CHECK((long long)P.chunks.size() <= m3r::opt_max_chunks(n, total));
        const m3r::OptLayout L = m3r::opt_layout(n, m3r::opt_max_chunks(n, total));
        CHECK(L.total == must3r_hip_optim_scratch_bytes(n, total));
        CHECK(L.chunks + P.chunks.size() * sizeof(m3r::OptChunk) <= L.upload_bytes && L.upload_bytes <= L.partials && L.partials < L.bc && L.bc < L.total);
    }
    CHECK(must3r_hip_optim_scratch_bytes(1, 1) == 1024 && must3r_hip_optim_scratch_bytes(0, 1) == 0 && must3r_hip_optim_scratch_bytes(2, 1) == 0);
    // refusals, each before anything on the device is touched: the scratch pointer is as fake as the tensors
    auto refused = [&](bool step, const char* word) {
        const int rc = step ? must3r_hip_optim_adamw(&a, addr(900), 1u << 30) : must3r_hip_optim_norm(&a, addr(900), 1u << 30);
        return rc == 1 && strstr(m3r::last_error, word) != nullptr;
    };
    must3r_hip_optim_control* control = reinterpret_cast<must3r_hip_optim_control*>(addr(901));
    a.control = control;
    tab[3].n = 0;              CHECK(refused(false, "positive") && refused(true, "positive"));            tab[3].n = ns[3];
    tab[2].g = addr(11) + 1;   CHECK(refused(false, "aligned") && refused(true, "aligned"));              tab[2].g = addr(11);
    tab[0].p = nullptr;        CHECK(refused(true, "null"));                                              tab[0].p = addr(0);
    tab[5].group = 2;          CHECK(refused(true, "group index"));                                       tab[5].group = 1;
    groups[1].beta2 = 1.0;     CHECK(refused(true, "beta"));                                              groups[1].beta2 = 0.95;
    groups[0].eps = -1.0;      CHECK(refused(true, "eps"));                                               groups[0].eps = 1e-8;
    groups[0].lr = -1.0;       CHECK(refused(true, "lr"));                                                groups[0].lr = 1e-3;
    groups[1].weight_decay = -1.0; CHECK(refused(true, "weight_decay"));                                  groups[1].weight_decay = 0.0;
    a.scale = addr(902);       CHECK(refused(false, "come together"));                                    a.scale = nullptr;
    a.control = nullptr;       CHECK(refused(false, "control"));                                          a.control = control;
    a.n_tensors = 0;           CHECK(refused(false, "n_tensors") && refused(true, "n_tensors"));          a.n_tensors = n;
    CHECK(must3r_hip_optim_norm(&a, addr(900), 1024) == 1 && strstr(m3r::last_error, "scratch too small"));
    CHECK(must3r_hip_optim_adamw(&a, nullptr, 1u << 30) == 1 && strstr(m3r::last_error, "scratch too small"));
    CHECK(must3r_hip_optim_norm(nullptr, nullptr, 0) == 1 && must3r_hip_optim_adamw(nullptr, nullptr, 0) == 1);
    printf("ok\n");
    return 0;
}
