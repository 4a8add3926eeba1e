// What cam.hip (postprocess(compute_cam=True)) and slam.hip (the SLAM agent's get_camera_pose, must3r/slam/model.py:147-172) share: the data pass
// of cam.hip as a host routine that leaves the solve to its caller, and the solve's two device routines -- the fixed-order sum of the per-block
// partials and the weighted Procrustes problem in Horn's quaternion form.  One text, so that both callers round alike.
#pragma once
#include "common.hpp"

namespace m3r {

// Launches the solve of views [v0, v0 + nv) of one cooperative launch: `partial` is [nv][G][16], `focal` [nv] (fp64), both of that launch.
// Returns 0, or non-zero after fail().
typedef int (*cam_solve_fn)(void* user, int v0, int nv, int G, const double* partial, const double* focal, hipStream_t s);

// cam.hip: activation + Weiszfeld focal + registration sums of n_views views, cooperative launches of as many views as are co-resident; after each
// of them `solve` is called.  `who` names the entry point in error texts.  Nothing is launched before the arguments have passed.
int cam_data_pass(const char* who, const float* pm, int activation, int n_views, int H, int W, float* p3, float* pl, float* cf, void* scratch,
                  size_t scratch_bytes, hipStream_t s, cam_solve_fn solve, void* user);

// 64 threads: lanes (q, j) add blocks b = q, q + 4, ... of sum j; the four quarter sums are then added in order.  S valid for every thread after return.
__device__ __forceinline__ void cam_sum_partials(const double* __restrict__ part, const int G, double (*S4)[16], double* S) {
    {
        const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
        double acc = 0.0;
        for (int b = q; b < G; b += 4) acc += part[(size_t)b * 16 + j];
        S4[q][j] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 16) S[threadIdx.x] = ((S4[0][threadIdx.x] + S4[1][threadIdx.x]) + S4[2][threadIdx.x]) + S4[3][threadIdx.x];
    __syncthreads();
}

// One thread.  S = [sum w, sum w x (3), sum w y (3), sum w y_i x_j (9)] -> c2w (row-major 4 x 4, fp32) of the rigid map x -> y.
// RECTIFY: the source points are diag(1, 1, ratio) x instead -- their weighted mean is diag(1, 1, ratio) xbar and their moment M diag(1, 1, ratio),
// so the sums of the unrectified points serve and no second pass over the pixels is needed.
template <bool RECTIFY>
__device__ __forceinline__ void cam_register(const double* S, const double ratio, float* c2w) {
    const double sw = S[0];
    double xb[3], yb[3], M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xb[i] = S[1 + i] / sw;
        yb[i] = S[4 + i] / sw;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = S[7 + i * 3 + j] / sw - yb[i] * xb[j];
    if constexpr (RECTIFY) {
        xb[2] *= ratio;
#pragma unroll
        for (int i = 0; i < 3; ++i) M[i][2] *= ratio;
    }
    // Horn: s[a][b] = sum x_a y_b = M^T
    const double sxx = M[0][0], sxy = M[1][0], sxz = M[2][0];
    const double syx = M[0][1], syy = M[1][1], syz = M[2][1];
    const double szx = M[0][2], szy = M[1][2], szz = M[2][2];
    double A[4][4] = {{sxx + syy + szz, syz - szy, szx - sxz, sxy - syx},
                      {syz - szy, sxx - syy - szz, sxy + syx, szx + sxz},
                      {szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy},
                      {sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz}};
    double Q[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) scale = fmax(scale, fabs(A[i][j]));
    const double inv_scale = scale > 0.0 ? 1.0 / scale : 1.0;   // eigenvectors do not care; keeps the fp32 angle in range
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] *= inv_scale;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off = fmax(off, fabs(A[p][q]));
        if (!(off > 1e-14)) break;   // R is returned in fp32
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) > 1e-30) {
                    // the angle only has to be roughly right (fp32 tangent); what must hold to fp64 is c^2 + s^2 = 1, so
                    // c comes from a Newton-refined fp64 rsqrt of 1 + t^2 and s = t c.  fp64 div/sqrt cost ~30
                    // dependent instructions each and this is a single thread per view.
                    const float thf = (float)(A[q][q] - A[p][p]) / (2.0f * (float)apq);
                    const float tf = (thf >= 0.f ? 1.0f : -1.0f) / (fabsf(thf) + sqrtf(thf * thf + 1.0f));
                    const double t = (double)tf, n2 = t * t + 1.0;
                    double c = __builtin_amdgcn_rsq(n2);
                    c = c * (1.5 - 0.5 * n2 * c * c);
                    c = c * (1.5 - 0.5 * n2 * c * c);
                    const double s = t * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {   // A <- A J
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = c * akp - s * akq;
                        A[k][q] = s * akp + c * akq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {   // A <- J^T A
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = c * apk - s * aqk;
                        A[q][k] = s * apk + c * aqk;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {   // Q <- Q J
                        const double qkp = Q[k][p], qkq = Q[k][q];
                        Q[k][p] = c * qkp - s * qkq;
                        Q[k][q] = s * qkp + c * qkq;
                    }
                }
            }
    }
    double bestv = A[0][0], qw = Q[0][0], qx = Q[1][0], qy = Q[2][0], qz = Q[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > bestv) {
            bestv = A[i][i];
            qw = Q[0][i]; qx = Q[1][i]; qy = Q[2][i]; qz = Q[3][i];
        }
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)},
                            {2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)},
                            {2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = yb[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c2w[i * 4 + j] = (float)R[i][j];
            t -= R[i][j] * xb[j];
        }
        c2w[i * 4 + 3] = (float)t;
    }
    c2w[12] = 0.f; c2w[13] = 0.f; c2w[14] = 0.f; c2w[15] = 1.f;
}

}  // namespace m3r
