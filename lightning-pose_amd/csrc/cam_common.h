// Device functions of the camera geometry, shared by cameras.hip (the calibrated losses) and mv3d.hip (the multi-view batch producer):
// undistort, the 4 x 4 DLT triangulation (one-sided Jacobi), projection with the distortion model forward, and their backward forms.
// The arithmetic and its reference lines are described at the top of cameras.hip.
#pragma once
#include "lp_common.h"

namespace lp {

constexpr int kCamDist = 12;        // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (OpenCV order; the caller pads shorter sets with zeros)
constexpr int kCamUndistIters = 5;
constexpr int kCamSweeps = 10;      // upper bound; a 4 x 4 converges in 4 - 6 sweeps
constexpr float kCamGuard = 1e-8f;

struct CamDist {
    float k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4;
};
struct CamK {
    float fx, fy, cx, cy;
};

__device__ __forceinline__ CamDist cam_load_dist(const float* d) {
    return CamDist{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}
__device__ __forceinline__ CamK cam_load_k(const float* m) { return CamK{m[0], m[4], m[2], m[5]}; }
__device__ __forceinline__ float cam_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ bool cam_isnan(float v) { return v != v; }

// pair index (itertools.combinations order) -> views j1 < j2
__device__ __forceinline__ void cam_pair_views(int p, int V, int& j1, int& j2) {
    j1 = 0;
    while (p >= V - 1 - j1) {
        p -= V - 1 - j1;
        ++j1;
    }
    j2 = j1 + 1 + p;
}

// one fixed-point iteration of the undistortion from (x, y); returns the pieces its backward needs
__device__ __forceinline__ void cam_undist_step(float x0, float y0, float x, float y, const CamDist& D, float& xn, float& yn) {
    const float r2 = x * x + y * y;
    const float num = 1.f + r2 * (D.k4 + r2 * (D.k5 + r2 * D.k6)), den = 1.f + r2 * (D.k1 + r2 * (D.k2 + r2 * D.k3));
    const float inv = num / den;
    const float dx = 2.f * D.p1 * x * y + D.p2 * (r2 + 2.f * x * x) + r2 * (D.s1 + D.s2 * r2);
    const float dy = D.p1 * (r2 + 2.f * y * y) + 2.f * D.p2 * x * y + r2 * (D.s3 + D.s4 * r2);
    xn = (x0 - dx) * inv;
    yn = (y0 - dy) * inv;
}

// pixel -> normalised, undistorted (x, y)
__device__ __forceinline__ void cam_undistort(float u, float v, const CamK& C, const CamDist& D, float& x, float& y) {
    const float x0 = (u - C.cx) / C.fx, y0 = (v - C.cy) / C.fy;
    x = x0, y = y0;
#pragma unroll
    for (int i = 0; i < kCamUndistIters; ++i) {
        float xn, yn;
        cam_undist_step(x0, y0, x, y, D, xn, yn);
        x = xn, y = yn;
    }
}

// d loss / d (x, y) of the undistorted point -> d loss / d (u, v), through the same 5 iterations
__device__ __forceinline__ void cam_undistort_bwd(float u, float v, const CamK& C, const CamDist& D, float gx, float gy, float& gu, float& gv) {
    const float x0 = (u - C.cx) / C.fx, y0 = (v - C.cy) / C.fy;
    float xs[kCamUndistIters], ys[kCamUndistIters];   // the iterate each iteration starts from (static indices: registers)
    float x = x0, y = y0;
#pragma unroll
    for (int i = 0; i < kCamUndistIters; ++i) {
        xs[i] = x, ys[i] = y;
        float xn, yn;
        cam_undist_step(x0, y0, x, y, D, xn, yn);
        x = xn, y = yn;
    }
    float gx0 = 0.f, gy0 = 0.f;
#pragma unroll
    for (int i = kCamUndistIters - 1; i >= 0; --i) {
        x = xs[i], y = ys[i];
        const float r2 = x * x + y * y;
        const float num = 1.f + r2 * (D.k4 + r2 * (D.k5 + r2 * D.k6)), den = 1.f + r2 * (D.k1 + r2 * (D.k2 + r2 * D.k3));
        const float dnum = D.k4 + r2 * (2.f * D.k5 + 3.f * D.k6 * r2), dden = D.k1 + r2 * (2.f * D.k2 + 3.f * D.k3 * r2);
        const float inv = num / den, dinv = (dnum * den - num * dden) / (den * den);
        const float dx = 2.f * D.p1 * x * y + D.p2 * (r2 + 2.f * x * x) + r2 * (D.s1 + D.s2 * r2);
        const float dy = D.p1 * (r2 + 2.f * y * y) + 2.f * D.p2 * x * y + r2 * (D.s3 + D.s4 * r2);
        gx0 += gx * inv;
        gy0 += gy * inv;
        const float g_inv = gx * (x0 - dx) + gy * (y0 - dy), g_dx = -gx * inv, g_dy = -gy * inv;
        const float g_r2 = g_inv * dinv + g_dx * (D.p2 + D.s1 + 2.f * D.s2 * r2) + g_dy * (D.p1 + D.s3 + 2.f * D.s4 * r2);
        gx = 2.f * x * g_r2 + g_dx * (2.f * D.p1 * y + 4.f * D.p2 * x) + g_dy * (2.f * D.p2 * y);
        gy = 2.f * y * g_r2 + g_dx * (2.f * D.p1 * x) + g_dy * (4.f * D.p1 * y + 2.f * D.p2 * x);
    }
    gx0 += gx;   // (the first iterate IS (x0, y0))
    gy0 += gy;
    gu = gx0 / C.fx;
    gv = gy0 / C.fy;
}

// rows of the DLT matrix for one view: x P[2] - P[0], y P[2] - P[1]
__device__ __forceinline__ void cam_dlt_rows(const float* P, float x, float y, float (&r0)[4], float (&r1)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        r0[c] = x * P[8 + c] - P[c];
        r1[c] = y * P[8 + c] - P[4 + c];
    }
}

// One-sided Jacobi: W (rows r, columns c) = A on entry, A V on exit with orthogonal columns; V accumulates the rotations.
// Every index is a compile-time constant after unrolling, so W and V stay in registers.
__device__ __forceinline__ void cam_svd4(float (&W)[4][4], float (&Vm)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) Vm[r][c] = r == c ? 1.f : 0.f;
#pragma unroll 1
    for (int sweep = 0; sweep < kCamSweeps; ++sweep) {
        bool any = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                float alpha = 0.f, beta = 0.f, gamma = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    alpha = fmaf(W[r][p], W[r][p], alpha);
                    beta = fmaf(W[r][q], W[r][q], beta);
                    gamma = fmaf(W[r][p], W[r][q], gamma);
                }
                const bool rot = fabsf(gamma) > 0x1p-24f * sqrtf(alpha * beta);   // (false for NaN and for a zero column)
                any = any || rot;
                const float zeta = (beta - alpha) / (2.f * (rot ? gamma : 1.f));
                const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(fmaf(zeta, zeta, 1.f)));
                const float cc = 1.f / sqrtf(fmaf(t, t, 1.f));
                const float c = rot ? cc : 1.f, s = rot ? cc * t : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float wp = W[r][p], wq = W[r][q], vp = Vm[r][p], vq = Vm[r][q];
                    W[r][p] = c * wp - s * wq;
                    W[r][q] = s * wp + c * wq;
                    Vm[r][p] = c * vp - s * vq;
                    Vm[r][q] = s * vp + c * vq;
                }
            }
        }
        if (!any) break;
    }
}

struct CamTri {
    float W[4][4], Vm[4][4], lam[4];   // A V, V, squared singular values
    int m;                             // column of the smallest one
    float h[4];                        // v_m
};

// triangulate one pair from the normalised points; X = h[:3] * s, s = 1 / h[3] if |h[3]| > guard else 1
__device__ __forceinline__ void cam_triangulate(const float* P1, const float* P2, float x1, float y1, float x2, float y2, CamTri& T, float (&X)[3]) {
    cam_dlt_rows(P1, x1, y1, T.W[0], T.W[1]);
    cam_dlt_rows(P2, x2, y2, T.W[2], T.W[3]);
    cam_svd4(T.W, T.Vm);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) a = fmaf(T.W[r][c], T.W[r][c], a);
        T.lam[c] = a;
    }
    T.m = 0;
    float best = T.lam[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool lt = T.lam[c] < best;
        T.m = lt ? c : T.m;
        best = lt ? T.lam[c] : best;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) T.h[r] = T.m == 0 ? T.Vm[r][0] : T.m == 1 ? T.Vm[r][1] : T.m == 2 ? T.Vm[r][2] : T.Vm[r][3];
    const float s = fabsf(T.h[3]) > kCamGuard ? 1.f / T.h[3] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) X[c] = T.h[c] * s;
}

// d loss / d X -> d loss / d (x1, y1, x2, y2)
__device__ __forceinline__ void cam_triangulate_bwd(const float* P1, const float* P2, const CamTri& T, const float (&gX)[3], float (&g)[4]) {
    const bool guarded = fabsf(T.h[3]) > kCamGuard;
    const float s = guarded ? 1.f / T.h[3] : 1.f;
    float gh[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) gh[c] = gX[c] * s;
    gh[3] = guarded ? -(gX[0] * T.h[0] + gX[1] * T.h[1] + gX[2] * T.h[2]) * s * s : 0.f;
    float z[4] = {0.f, 0.f, 0.f, 0.f}, Az[4] = {0.f, 0.f, 0.f, 0.f}, Ah[4];
    const float lmin = T.m == 0 ? T.lam[0] : T.m == 1 ? T.lam[1] : T.m == 2 ? T.lam[2] : T.lam[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float dot = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) dot = fmaf(T.Vm[r][i], gh[r], dot);
        const float gap = T.lam[i] - lmin;
        const float ci = (i != T.m && gap > 0.f) ? dot / gap : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            z[r] = fmaf(-ci, T.Vm[r][i], z[r]);
            Az[r] = fmaf(-ci, T.W[r][i], Az[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Ah[r] = T.m == 0 ? T.W[r][0] : T.m == 1 ? T.W[r][1] : T.m == 2 ? T.W[r][2] : T.W[r][3];
    // dA[r][c] = Az[r] h[c] + Ah[r] z[c];  row r depends on its coordinate through coordinate * P[2][c]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float* P = r < 2 ? P1 : P2;
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) a = fmaf(fmaf(Az[r], T.h[c], Ah[r] * z[c]), P[8 + c], a);
        g[r] = a;
    }
}

// world point -> pixel of one view (frame px, or model px with a bounding box [x, y, h, w])
__device__ __forceinline__ void cam_project(const float (&X)[3], const float* E, const CamK& C, const CamDist& D, const float* bbox, float mh,
                                            float mw, float& u, float& v) {
    float Xc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Xc[r] = fmaf(E[4 * r + 2], X[2], fmaf(E[4 * r + 1], X[1], E[4 * r] * X[0])) + E[4 * r + 3];
    const float s = fabsf(Xc[2]) > kCamGuard ? 1.f / Xc[2] : 1.f;
    const float x = Xc[0] * s, y = Xc[1] * s;
    const float r2 = x * x + y * y;
    const float num = 1.f + r2 * (D.k1 + r2 * (D.k2 + r2 * D.k3)), den = 1.f + r2 * (D.k4 + r2 * (D.k5 + r2 * D.k6));
    const float rad = num / den;
    const float xd = x * rad + 2.f * D.p1 * x * y + D.p2 * (r2 + 2.f * x * x) + r2 * (D.s1 + D.s2 * r2);
    const float yd = y * rad + D.p1 * (r2 + 2.f * y * y) + 2.f * D.p2 * x * y + r2 * (D.s3 + D.s4 * r2);
    u = C.fx * xd + C.cx;
    v = C.fy * yd + C.cy;
    if (bbox != nullptr) {
        u = (u - bbox[0]) / bbox[3] * mw;
        v = (v - bbox[1]) / bbox[2] * mh;
    }
}

// (gu, gv) -> ADDS d loss / d X into gX
__device__ __forceinline__ void cam_project_bwd(const float (&X)[3], const float* E, const CamK& C, const CamDist& D, const float* bbox, float mh,
                                                float mw, float gu, float gv, float (&gX)[3]) {
    float Xc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Xc[r] = fmaf(E[4 * r + 2], X[2], fmaf(E[4 * r + 1], X[1], E[4 * r] * X[0])) + E[4 * r + 3];
    const bool guarded = fabsf(Xc[2]) > kCamGuard;
    const float s = guarded ? 1.f / Xc[2] : 1.f;
    const float x = Xc[0] * s, y = Xc[1] * s;
    const float r2 = x * x + y * y;
    const float num = 1.f + r2 * (D.k1 + r2 * (D.k2 + r2 * D.k3)), den = 1.f + r2 * (D.k4 + r2 * (D.k5 + r2 * D.k6));
    const float dnum = D.k1 + r2 * (2.f * D.k2 + 3.f * D.k3 * r2), dden = D.k4 + r2 * (2.f * D.k5 + 3.f * D.k6 * r2);
    const float rad = num / den, drad = (dnum * den - num * dden) / (den * den);
    if (bbox != nullptr) {
        gu = gu * mw / bbox[3];
        gv = gv * mh / bbox[2];
    }
    const float g_xd = gu * C.fx, g_yd = gv * C.fy;
    const float g_r2 = (g_xd * x + g_yd * y) * drad + g_xd * (D.p2 + D.s1 + 2.f * D.s2 * r2) + g_yd * (D.p1 + D.s3 + 2.f * D.s4 * r2);
    const float g_x = g_xd * (rad + 2.f * D.p1 * y + 4.f * D.p2 * x) + g_yd * (2.f * D.p2 * y) + 2.f * x * g_r2;
    const float g_y = g_xd * (2.f * D.p1 * x) + g_yd * (rad + 4.f * D.p1 * y + 2.f * D.p2 * x) + 2.f * y * g_r2;
    float gc[3];
    gc[0] = g_x * s;
    gc[1] = g_y * s;
    gc[2] = guarded ? -(g_x * Xc[0] + g_y * Xc[1]) * s * s : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gX[c] += fmaf(E[8 + c], gc[2], fmaf(E[4 + c], gc[1], E[c] * gc[0]));
}

// mean over the pairs of one (sample, keypoint), summed in ascending pair order (one NaN pair makes it NaN, as torch.mean)
__device__ __forceinline__ void cam_pair_mean(const float* p3d_b, int P, int K, int k, float (&X)[3]) {
    X[0] = X[1] = X[2] = 0.f;
    for (int p = 0; p < P; ++p) {
        const float* q = p3d_b + ((size_t)p * K + k) * 3;
        X[0] += q[0], X[1] += q[1], X[2] += q[2];
    }
    const float n = (float)P;
    X[0] /= n, X[1] /= n, X[2] /= n;
}

struct CamRig {
    const float* points;   // (B, V, K, 2) frame px
    const float* intr;     // (B, V, 3, 3)
    const float* extr;     // (B, V, 3, 4)
    const float* dist;     // (B, V, 12)
    const float* bbox;     // (B, 4 V) [x, y, h, w] per view, or null: the reprojection stays in frame px
    float mh, mw;
    int V, K, P;
};

// undistorted points of both views of a pair; false if either point has a NaN coordinate
__device__ __forceinline__ bool cam_pair_points(const CamRig& g, int b, int j1, int j2, int k, float& x1, float& y1, float& x2, float& y2) {
    const float* q1 = g.points + (((size_t)b * g.V + j1) * g.K + k) * 2;
    const float* q2 = g.points + (((size_t)b * g.V + j2) * g.K + k) * 2;
    const float u1 = q1[0], v1 = q1[1], u2 = q2[0], v2 = q2[1];
    cam_undistort(u1, v1, cam_load_k(g.intr + ((size_t)b * g.V + j1) * 9), cam_load_dist(g.dist + ((size_t)b * g.V + j1) * kCamDist), x1, y1);
    cam_undistort(u2, v2, cam_load_k(g.intr + ((size_t)b * g.V + j2) * 9), cam_load_dist(g.dist + ((size_t)b * g.V + j2) * kCamDist), x2, y2);
    return !(cam_isnan(x1) || cam_isnan(y1) || cam_isnan(x2) || cam_isnan(y2));
}

}  // namespace lp
