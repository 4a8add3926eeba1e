// Host program over must3r_amd/csrc/render_tri.hpp, the text the mesh rasteriser's kernels compile (tests/test_render_mesh_host.py builds it with the host
// sanitizers and -ffp-contract=off and runs it as a child process with nothing preloaded).
//
//   render_tri_check --sizes        the sizes and constants of include/must3r_hip.h as a C++ compiler sees them
//   render_tri_check <case file>    every triangle of the case through project / box / cover, sequentially; prints
//                                       box <id> <x0> <x1> <y0> <y1>                      for every triangle with a candidate
//                                       hit <id> <pixel> <Zp bits> <t0 bits> <t1 bits> <t2 bits>   for every covered sample (hex)
//
// Case file (little endian): int32 n_views, W, H; double fx, fy, cx, cy, z_near, z_far; float thr; then per view int32 h, w; double A[12]; float conf[h w];
// float pts[h w 3].  z_near and z_far are the camera's fp32 values widened.
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/must3r_hip.h"
#include "../../must3r_amd/csrc/render_tri.hpp"

using namespace m3r;

template <class T>
static bool get(FILE* f, T* out, size_t n = 1) { return std::fread(out, sizeof(T), n, f) == n; }

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--sizes")) {
        std::printf("sizes: mesh_desc %zu camera %zu view %zu wave_area %d scratch_offset %zu\n", sizeof(must3r_hip_render_mesh_desc),
                    sizeof(must3r_hip_render_camera), sizeof(must3r_hip_export_view), MUST3R_RENDER_MESH_WAVE_AREA,
                    offsetof(must3r_hip_render_mesh_desc, scratch));
        return 0;
    }
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[3];
    double cam[6];
    float thr;
    if (!get(f, head, 3) || !get(f, cam, 6) || !get(f, &thr)) return 3;
    const int n_views = head[0], W = head[1], H = head[2];
    long long base = 0, triangles = 0, hits = 0;
    for (int vi = 0; vi < n_views; ++vi) {
        int32_t hw[2];
        double A[12];
        if (!get(f, hw, 2) || !get(f, A, 12)) return 3;
        const int h = hw[0], w = hw[1];
        std::vector<float> conf((size_t)h * w), pts((size_t)h * w * 3);
        if (!get(f, conf.data(), conf.size()) || !get(f, pts.data(), pts.size())) return 3;
        for (int r = 0; r + 1 < h; ++r) {
            for (int c = 0; c + 1 < w; ++c) {
                const unsigned i = (unsigned)(r * w + c);
                for (int kind = 0; kind < 2; ++kind) {
                    unsigned off[3];
                    tri::corner_offsets(kind, (unsigned)w, off);
                    tri::Corner k[3];
                    bool ok = true;
                    for (int a = 0; a < 3; ++a) {
                        const size_t p = i + off[a];
                        ok = tri::project(A, cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], conf[p] >= thr, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], k[a]) && ok;
                    }
                    int x0, x1, y0, y1;
                    if (!ok || !tri::box(k[0], k[1], k[2], W, H, x0, x1, y0, y1)) continue;
                    const long long id = 2 * (base + i) + kind;
                    ++triangles;
                    std::printf("box %lld %d %d %d %d\n", id, x0, x1, y0, y1);
                    for (int y = y0; y <= y1; ++y) {
                        for (int x = x0; x <= x1; ++x) {
                            double Zp, t[3];
                            if (!tri::cover(k[0], k[1], k[2], (double)x + 0.5, (double)y + 0.5, Zp, t)) continue;
                            ++hits;
                            std::printf("hit %lld %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", id, y * W + x, bits(Zp), bits(t[0]), bits(t[1]),
                                        bits(t[2]));
                        }
                    }
                }
            }
        }
        base += (long long)h * w;
    }
    std::fclose(f);
    std::printf("render_tri_check: OK %lld triangles, %lld samples\n", triangles, hits);
    return 0;
}
