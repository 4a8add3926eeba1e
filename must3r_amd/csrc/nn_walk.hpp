// What the callers of the exact 1-NN index share (nn_index.hip: must3r_hip_nn_index_query; slam.hip: the keyframe test): the index header, the
// per-query walk of a quadrant's bounding-box heap, and the view-direction quadrant of a ray (nn.hip: must3r_hip_quadrant_ids).  One text, so that
// every caller gets the same bits.  nn_index.hip describes the index and why the walk is exact.
#pragma once
#include "common.hpp"

namespace m3r {

constexpr int NNI_MAXQ = 128;          // quadrants (divider <= 8: 2 * 8^2)

struct NnIndexHeader {
    int divider, n_quads, leaf_log2, key_shift;
    int morton_bits, n_points, pad0, pad1;
    long long pts_off, nodes_off, node_cap, pad2;
    float lo[4], hi[4];
    int seg[NNI_MAXQ + 4];            // seg[q] .. seg[q + 1]: quadrant q in key order; seg[Q] = finite points
    int pow2[NNI_MAXQ];               // P_q: leaves of quadrant q padded to a power of two (0: empty)
    int depth[NNI_MAXQ];              // log2(P_q)
    int node_base[NNI_MAXQ];          // first node of quadrant q's heap (node k at node_base + k - 1)
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// slam/tools.py:9-31 with quadrant_divider = div, eps = 1e-5 (float32 like the numpy code fed with float32 points)
__device__ __forceinline__ int quadrant_of(const float px, const float py, const float pz, const float cx, const float cy, const float cz, const int div) {
    const float eps = 1e-5f, pi = 3.14159265358979323846f;
    float x = px - cx, y = py - cy, z = pz - cz;
    const float nrm = fmaxf(sqrtf(x * x + y * y + z * z), eps);
    x /= nrm; y /= nrm; z /= nrm;
    float theta = acosf(z) / pi;
    float phi = atan2f(y, x) / pi;
    theta = fminf(fmaxf(theta, eps), 1.0f - eps);
    phi = fminf(fmaxf(phi, -1.0f + eps), 1.0f - eps);
    const int ti = (int)floorf(theta * (float)div);
    const int pj = (int)floorf(phi * (float)div) + div;
    return ti + pj * div;
}

__device__ __forceinline__ float box_bound(const f32x4* __restrict__ nb, const int k, const float qx, const float qy, const float qz) {
    const f32x4 lo = nb[2 * (k - 1)], hi = nb[2 * (k - 1) + 1];
    const float gx = fmaxf(fmaxf(lo[0] - qx, qx - hi[0]), 0.f);
    const float gy = fmaxf(fmaxf(lo[1] - qy, qy - hi[1]), 0.f);
    const float gz = fmaxf(fmaxf(lo[2] - qz, qz - hi[2]), 0.f);
    return fmaf(gz, gz, fmaf(gy, gy, gx * gx));
}

// The squared distance of (qx, qy, qz) to its nearest point of quadrant `quad`; +inf for an empty quadrant, a quadrant outside the index or a non-finite
// query, NaN when `divider` is not the build's.  G lanes per query (G divides 64, the G lanes of a group are consecutive and all call this with the
// same query): every lane of a group walks the same path (the same boxes, the group's best), the points of a leaf are split over the group and the
// group's minimum is taken with xor shuffles (min is exact and order-free: the result is the same for every G).  Lane `sub` of the group.
template <int G>
__device__ __forceinline__ float nn_walk(const char* __restrict__ index, const int divider, const int quad, const float qx, const float qy, const float qz,
                                         const int sub) {
    const NnIndexHeader* h = reinterpret_cast<const NnIndexHeader*>(index);
    float best = INFINITY;
    const int P = (quad >= 0 && quad < h->n_quads) ? h->pow2[quad] : 0;
    if (divider != h->divider) {
        best = __builtin_nanf("");   // queried with another divider than the build's: NaN, never a plausible distance
    } else if (P > 0 && finite3(qx, qy, qz)) {
        const f32x4* nb = reinterpret_cast<const f32x4*>(index + h->nodes_off) + 2LL * h->node_base[quad];
        const f32x4* pts = reinterpret_cast<const f32x4*>(index + h->pts_off);
        const int D = h->depth[quad], L = 1 << h->leaf_log2, lg = h->leaf_log2;
        const int s_begin = h->seg[quad], s_end = h->seg[quad + 1];
        int k = 1, l = 0;
        unsigned trail = 0;   // bit l: the node on the path at level l is the second child visited (its sibling is done)
        bool go = box_bound(nb, 1, qx, qy, qz) < best;
        while (go) {
            bool down = false;
            if (l == D) {
                const int s0 = s_begin + ((k - P) << lg);
                const int s1 = min(s0 + L, s_end);
                for (int s = s0 + sub; s < s1; s += G) {
                    const f32x4 p = pts[s];
                    const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
                    best = fminf(best, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
                }
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o, G));
            } else {
                const float b0 = box_bound(nb, 2 * k, qx, qy, qz), b1 = box_bound(nb, 2 * k + 1, qx, qy, qz);
                const bool right = b1 < b0;   // the nearer child first (left on a tie)
                if ((right ? b1 : b0) < best) {
                    k = 2 * k + (right ? 1 : 0);
                    ++l;
                    down = true;
                }
            }
            if (down) continue;
            // climb to the first level whose sibling has not been visited and may still hold a smaller d2
            go = false;
            while (l > 0) {
                if ((trail >> l) & 1u) {
                    trail &= ~(1u << l);
                    k >>= 1;
                    --l;
                    continue;
                }
                trail |= 1u << l;
                k ^= 1;
                if (box_bound(nb, k, qx, qy, qz) < best) { go = true; break; }
            }
        }
    }
    return best;
}

}  // namespace m3r
