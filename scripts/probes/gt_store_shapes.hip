// What the store shape of csrc/train_data.hip costs: a lane that owns 4 consecutive pixels holds 12 consecutive floats of pts3d and writes them with three
// 16-byte stores 48 bytes apart from its neighbour's, so one store instruction of a wave touches 24 lines of 128 bytes and fills a third of each.  This
// probe writes the same 12 floats per lane (cheap integer-derived values, no fp64) in that shape (A) and, turned through the wave's part of the LDS so that
// each store instruction writes 1 KB without gaps, in the dense shape (B), on a buffer of the benchmark's size.
//   hipcc --offload-arch=gfx950 -O3 -o gt_store_shapes scripts/probes/gt_store_shapes.hip && ./gt_store_shapes [pixels = 110100480] [launches = 20] [rounds = 7]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ void values(unsigned g, float (&X)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = (float)(12 * g + k);
}

__global__ void __launch_bounds__(256) strided(f32x4* __restrict__ out, unsigned groups) {
    const unsigned g = blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    float X[12];
    values(g, X);
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * (size_t)g + j] = f32x4{X[4 * j], X[4 * j + 1], X[4 * j + 2], X[4 * j + 3]};
}

__global__ void __launch_bounds__(256) dense(f32x4* __restrict__ out, unsigned groups) {   // groups: a multiple of 64
    __shared__ f32x4 tile[4][192];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned g0 = blockIdx.x * 256 + wave * 64;      // wave-uniform
    if (g0 >= groups) return;
    float X[12];
    values(g0 + lane, X);
#pragma unroll
    for (int j = 0; j < 3; ++j) tile[wave][3 * lane + j] = f32x4{X[4 * j], X[4 * j + 1], X[4 * j + 2], X[4 * j + 3]};
    // a wave reads what it wrote itself: no barrier, the LDS operations of a wave complete in order
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * (size_t)g0 + 64 * j + lane] = tile[wave][64 * j + lane];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const long long pixels = argc > 1 ? atoll(argv[1]) : 110100480LL;
    const int launches = argc > 2 ? atoi(argv[2]) : 20, rounds = argc > 3 ? atoi(argv[3]) : 7;
    if (pixels <= 0 || pixels % 256 || pixels / 4 > 0x7fffffffLL) { fprintf(stderr, "pixels: a positive multiple of 256\n"); return 1; }
    const unsigned groups = (unsigned)(pixels / 4), blocks = (groups + 255) / 256;
    f32x4 *a, *b;
    CHECK(hipMalloc(&a, (size_t)pixels * 12));
    CHECK(hipMalloc(&b, (size_t)pixels * 12));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> us[2];
    for (int r = 0; r < rounds + 2; ++r)
        for (int k = 0; k < 2; ++k) {      // alternated
            CHECK(hipEventRecord(e0));
            for (int i = 0; i < launches; ++i) {
                if (k == 0) hipLaunchKernelGGL(strided, dim3(blocks), dim3(256), 0, 0, a, groups);
                else hipLaunchKernelGGL(dense, dim3(blocks), dim3(256), 0, 0, b, groups);
            }
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 2) us[k].push_back(ms * 1e3f / launches);
        }
    // the two shapes write the same values
    std::vector<float> ha(3 * 4096), hb(3 * 4096);
    CHECK(hipMemcpy(ha.data(), reinterpret_cast<float*>(a) + (size_t)pixels * 3 - ha.size(), ha.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hb.data(), reinterpret_cast<float*>(b) + (size_t)pixels * 3 - hb.size(), hb.size() * 4, hipMemcpyDeviceToHost));
    const bool same = ha == hb;
    for (int k = 0; k < 2; ++k) {
        std::sort(us[k].begin(), us[k].end());
        const double med = us[k][us[k].size() / 2];
        printf("%s: median %.1f us per launch (min %.1f, max %.1f), %.2f TB/s of stores\n", k ? "dense through LDS    " : "48-byte stride, 16 B ", med, us[k].front(),
               us[k].back(), (double)pixels * 12 / (med * 1e-6) / 1e12);
    }
    printf("pixels %lld, %d launches a round, %d rounds, same values: %s\n", pixels, launches, rounds, same ? "yes" : "NO");
    return same ? 0 : 1;
}
