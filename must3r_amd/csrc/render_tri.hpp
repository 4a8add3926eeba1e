// The per-triangle arithmetic of the mesh rasteriser (render_mesh.hip), text that the splat kernel, the resolve kernel and a host program
// (tests/c/render_tri_check.cpp) compile alike: the projection of a corner, the candidate box of a triangle and the coverage test with the
// perspective-correct depth at one sample point.  The rule is stated in include/must3r_hip.h ("scene rendering, triangles"); every
// operation here is one rounded fp64 operation, so every translation unit that includes this file is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3R_TRI_HD __host__ __device__ __forceinline__
#else
#define M3R_TRI_HD inline
#endif

namespace m3r {
namespace tri {

// ((a0 x + a1 y) + a2 z) + a3
M3R_TRI_HD double affine_row(const double* a, const double x, const double y, const double z) {
    const double p = a[0] * x, q = a[1] * y, r = a[2] * z;
    return ((p + q) + r) + a[3];
}

struct Corner {
    double u, v, iz;             // image position and 1.0 / Z
};

// the point path's projection and its drop tests on one corner: A = w2c . M (12 fp64), the fp32 point widened.  false = the corner (and so its
// triangle) is dropped.  `conf_ok` is the fp32 comparison conf >= fp32(thr), made by the caller.
M3R_TRI_HD bool project(const double* A, const double fx, const double fy, const double cx, const double cy, const double z_near, const double z_far,
                        const bool conf_ok, const float xf, const float yf, const float zf, Corner& c) {
    if (!conf_ok || !std::isfinite(xf) || !std::isfinite(yf) || !std::isfinite(zf)) return false;
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double Z = affine_row(A + 8, x, y, z);
    if (!(Z >= z_near && Z <= z_far)) return false;
    const double iz = 1.0 / Z;
    const double X = affine_row(A, x, y, z), Y = affine_row(A + 4, x, y, z);
    c.u = fx * (X * iz) + cx;
    c.v = fy * (Y * iz) + cy;
    c.iz = iz;
    return std::isfinite(c.u) && std::isfinite(c.v);
}

// [lo, hi] = the sample indices k in [0, n) with mn <= k + 0.5 <= mx, i.e. ceil(mn - 0.5) .. floor(mx - 0.5) clipped; the clip is made in fp64,
// before any integer is formed (mn and mx are finite but may be 1e300).  false = none.
M3R_TRI_HD bool span(const double mn, const double mx, const int n, int& lo, int& hi) {
    double a = std::ceil(mn - 0.5), b = std::floor(mx - 0.5);
    if (!(a <= (double)(n - 1)) || !(b >= 0.0)) return false;
    if (a < 0.0) a = 0.0;
    if (b > (double)(n - 1)) b = (double)(n - 1);
    if (!(a <= b)) return false;
    lo = (int)a;
    hi = (int)b;
    return true;
}

// candidate box of the triangle (c0, c1, c2) in a W x H image, inclusive bounds; false = no sample point inside the bounding box
M3R_TRI_HD bool box(const Corner& c0, const Corner& c1, const Corner& c2, const int W, const int H, int& x0, int& x1, int& y0, int& y1) {
    const double un = std::fmin(std::fmin(c0.u, c1.u), c2.u), ux = std::fmax(std::fmax(c0.u, c1.u), c2.u);
    const double vn = std::fmin(std::fmin(c0.v, c1.v), c2.v), vx = std::fmax(std::fmax(c0.v, c1.v), c2.v);
    return span(un, ux, W, x0, x1) && span(vn, vx, H, y0, y1);
}

// E_jk(p) = (u_k - u_j) (py - v_j) - (v_k - v_j) (px - u_j)
M3R_TRI_HD double edge(const Corner& j, const Corner& k, const double px, const double py) {
    const double a = (k.u - j.u) * (py - j.v), b = (k.v - j.v) * (px - j.u);
    return a - b;
}

// the sample point (px, py) against the triangle, corners in ascending source index: covered?  If so Zp, the perspective-correct depth, and
// t[k] = lam_k (1 / Z_k), the weights the resolve interpolates colours with.  Every shared edge is evaluated from its lower-index endpoint.
M3R_TRI_HD bool cover(const Corner& c0, const Corner& c1, const Corner& c2, const double px, const double py, double& Zp, double (&t)[3]) {
    const double s0 = edge(c0, c1, px, py), s1 = edge(c1, c2, px, py), s2 = -edge(c0, c2, px, py);
    const double den = (s0 + s1) + s2;
    if (!std::isfinite(den) || den == 0.0) return false;
    if (!((s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) || (s0 <= 0.0 && s1 <= 0.0 && s2 <= 0.0))) return false;
    const double l0 = s1 / den, l1 = s2 / den, l2 = s0 / den;
    t[0] = l0 * c0.iz;
    t[1] = l1 * c1.iz;
    t[2] = l2 * c2.iz;
    const double iz = (t[0] + t[1]) + t[2];
    Zp = 1.0 / iz;
    return true;
}

// one colour channel at the sample: ((t0 c0 + t1 c1) + t2 c2) Zp on the corners' fp32 colours widened, rounded to fp32 once
M3R_TRI_HD float shade(const double (&t)[3], const double Zp, const float a, const float b, const float c) {
    const double p = t[0] * (double)a, q = t[1] * (double)b, r = t[2] * (double)c;
    return (float)(((p + q) + r) * Zp);
}

// the three corners of a triangle as offsets from its anchor pixel in a view W pixels wide: kind 0 = (a, b, c'), kind 1 = (b, c', d)
M3R_TRI_HD void corner_offsets(const int kind, const unsigned W, unsigned (&o)[3]) {
    o[0] = kind ? 1u : 0u;
    o[1] = kind ? W : 1u;
    o[2] = kind ? W + 1u : W;
}

}  // namespace tri
}  // namespace m3r
