// Camera geometry of the calibrated multi-view losses: undistort, triangulate every camera pair (homogeneous DLT), average the pairs,
// reproject into every view, distort, map frame px -> model px - and the pairwise 3-D loss.  gfx950, fp32, plain HIP C++: every
// (sample, pair, keypoint) is an independent 4 x 4 problem held in one lane's registers; no LDS, no atomics, every sum in a fixed order
// (the same input gives the same bits).
//
// Reference arithmetic (paths relative to the reference tree):
//   data/cameras.py:22-83     project_camera_pairs_to_3d (kornia undistort_points + triangulate_points, one small SVD per pair and sample)
//   data/cameras.py:86-171    project_3d_to_2d (kornia PinholeCamera.project + distort_points)
//   data/bboxes.py:45-71, 129-169, 194-219   frame_to_model_batch
//   losses/losses.py:999-1126 PairwiseProjectionsLoss
// The 5 fixed-point iterations of the undistortion and the 1e-8 guard of the homogeneous divisions are kornia's defaults as recollected
// (kornia is not a dependency of this package and could not be read when this was written).
//
// Layout.  cam_chain_fwd_kernel / cam_chain_bwd_kernel: ONE workgroup per sample, phases separated by __syncthreads():
//   forward   (1) lane per (pair, keypoint): undistort the two views' points, triangulate -> p3d (B, P, K, 3)
//             (2) lane per (view, keypoint): mean over the pairs (read back from p3d), project, distort, frame -> model px -> p2d (B, V, K, 2)
//   backward  (A) lane per keypoint: d mean = sum over views of the projection's backward, / P                        -> workspace
//             (B) lane per (pair, keypoint): the triangulation again, then its backward -> d (x1, y1, x2, y2) normalised -> workspace
//             (C) lane per (view, keypoint): sum over the pairs that contain the view (ascending pair index), back through the 5 iterations
// The hand-over between phases goes through global memory of the SAME workgroup (visible after the barrier); nothing crosses workgroups.
// Triangulation: one-sided (Hestenes) Jacobi on the 4 x 4 DLT matrix A - rotations of its columns until they are orthogonal; the column
// norms are the singular values, the accumulated rotations V the right singular vectors.  It works on A itself, not on A^T A, so the
// smallest singular vector keeps the accuracy of an SVD, and the three other pairs (v_i, sigma_i^2) are exactly what the backward needs:
//   h = v_min,  z = - sum_{i != min} v_i (v_i . g_h) / (sigma_i^2 - sigma_min^2),  dA = A (z h^T + h z^T) = (A z) h^T + (A h) z^T
// with A v_i = column i of the rotated matrix - the original A is not kept.
#include "cam_common.h"

namespace lp {

constexpr int kCamThreads = 256;

// p3d (B, P, K, 3) is written in phase 1 and read back in phase 2 by other lanes of the same workgroup: no __restrict__ on it
__global__ __launch_bounds__(kCamThreads) void cam_chain_fwd_kernel(CamRig g, float* p3d, float* __restrict__ p2d) {
    const int b = blockIdx.x;
    float* p3d_b = p3d + (size_t)b * g.P * g.K * 3;
    for (int e = threadIdx.x; e < g.P * g.K; e += kCamThreads) {
        const int p = e / g.K, k = e - p * g.K;
        int j1, j2;
        cam_pair_views(p, g.V, j1, j2);
        float x1, y1, x2, y2, X[3];
        if (cam_pair_points(g, b, j1, j2, k, x1, y1, x2, y2)) {
            CamTri T;
            cam_triangulate(g.extr + ((size_t)b * g.V + j1) * 12, g.extr + ((size_t)b * g.V + j2) * 12, x1, y1, x2, y2, T, X);
        } else {
            X[0] = X[1] = X[2] = cam_nan();
        }
        p3d_b[e * 3] = X[0], p3d_b[e * 3 + 1] = X[1], p3d_b[e * 3 + 2] = X[2];
    }
    if (p2d == nullptr) return;   // (the same in every lane: triangulation only)
    __syncthreads();
    for (int e = threadIdx.x; e < g.V * g.K; e += kCamThreads) {
        const int v = e / g.K, k = e - v * g.K;
        float X[3], pu, pv;
        cam_pair_mean(p3d_b, g.P, g.K, k, X);
        const size_t cam = (size_t)b * g.V + v;
        cam_project(X, g.extr + cam * 12, cam_load_k(g.intr + cam * 9), cam_load_dist(g.dist + cam * kCamDist),
                    g.bbox ? g.bbox + cam * 4 : nullptr, g.mh, g.mw, pu, pv);
        p2d[(cam * g.K + k) * 2] = pu, p2d[(cam * g.K + k) * 2 + 1] = pv;
    }
}

// ws: [B][K][3] d mean / P, then [B][P][K][4] d (x1, y1, x2, y2); g3d (B, P, K, 3) and g2d (B, V, K, 2) may each be null
__global__ __launch_bounds__(kCamThreads) void cam_chain_bwd_kernel(CamRig g, int B, const float* __restrict__ p3d, const float* __restrict__ g3d,
                                                                    const float* __restrict__ g2d, float* ws, float* __restrict__ gpoints) {
    const int b = blockIdx.x;
    float* ws_mean = ws + (size_t)b * g.K * 3;
    float* ws_part = ws + (size_t)B * g.K * 3 + (size_t)b * g.P * g.K * 4;
    if (g2d != nullptr) {
        const float* p3d_b = p3d + (size_t)b * g.P * g.K * 3;
        for (int k = threadIdx.x; k < g.K; k += kCamThreads) {
            float X[3], gX[3] = {0.f, 0.f, 0.f};
            cam_pair_mean(p3d_b, g.P, g.K, k, X);
            if (!(cam_isnan(X[0]) || cam_isnan(X[1]) || cam_isnan(X[2]))) {   // (a NaN mean reprojects to NaN in every view: no gradient)
                for (int v = 0; v < g.V; ++v) {
                    const size_t cam = (size_t)b * g.V + v;
                    const float* q = g2d + (cam * g.K + k) * 2;
                    cam_project_bwd(X, g.extr + cam * 12, cam_load_k(g.intr + cam * 9), cam_load_dist(g.dist + cam * kCamDist),
                                    g.bbox ? g.bbox + cam * 4 : nullptr, g.mh, g.mw, q[0], q[1], gX);
                }
            }
            const float n = (float)g.P;
            ws_mean[k * 3] = gX[0] / n, ws_mean[k * 3 + 1] = gX[1] / n, ws_mean[k * 3 + 2] = gX[2] / n;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < g.P * g.K; e += kCamThreads) {
        const int p = e / g.K, k = e - p * g.K;
        int j1, j2;
        cam_pair_views(p, g.V, j1, j2);
        float x1, y1, x2, y2, gp[4] = {0.f, 0.f, 0.f, 0.f};
        if (cam_pair_points(g, b, j1, j2, k, x1, y1, x2, y2)) {   // (a pair with a NaN point is NaN forward and takes no gradient)
            const float* P1 = g.extr + ((size_t)b * g.V + j1) * 12;
            const float* P2 = g.extr + ((size_t)b * g.V + j2) * 12;
            CamTri T;
            float X[3], gX[3] = {0.f, 0.f, 0.f};
            cam_triangulate(P1, P2, x1, y1, x2, y2, T, X);
            if (g3d != nullptr) {
                const float* q = g3d + (((size_t)b * g.P + p) * g.K + k) * 3;
                gX[0] = q[0], gX[1] = q[1], gX[2] = q[2];
            }
            if (g2d != nullptr) gX[0] += ws_mean[k * 3], gX[1] += ws_mean[k * 3 + 1], gX[2] += ws_mean[k * 3 + 2];
            cam_triangulate_bwd(P1, P2, T, gX, gp);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) ws_part[e * 4 + c] = gp[c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < g.V * g.K; e += kCamThreads) {
        const int v = e / g.K, k = e - v * g.K;
        float gx = 0.f, gy = 0.f;
        int j1 = 0, j2 = 1;
        for (int p = 0; p < g.P; ++p) {   // ascending pair index: a fixed order
            const float* q = ws_part + ((size_t)p * g.K + k) * 4;
            if (j1 == v) gx += q[0], gy += q[1];
            if (j2 == v) gx += q[2], gy += q[3];
            if (++j2 == g.V) ++j1, j2 = j1 + 1;
        }
        const size_t cam = (size_t)b * g.V + v;
        const float* q = g.points + (cam * g.K + k) * 2;
        const float pu = q[0], pv = q[1];
        float gu = 0.f, gv = 0.f;
        if (!(cam_isnan(pu) || cam_isnan(pv)))
            cam_undistort_bwd(pu, pv, cam_load_k(g.intr + cam * 9), cam_load_dist(g.dist + cam * kCamDist), gx, gy, gu, gv);
        gpoints[(cam * g.K + k) * 2] = gu, gpoints[(cam * g.K + k) * 2 + 1] = gv;
    }
}

// stand-alone projection: lane per (sample, view, keypoint) forward, lane per (sample, keypoint) backward (its sum over the views in order)
__global__ __launch_bounds__(kCamThreads) void cam_project_fwd_kernel(CamRig g, int B, const float* __restrict__ X3, float* __restrict__ p2d) {
    const int e = blockIdx.x * kCamThreads + threadIdx.x;
    if (e >= B * g.V * g.K) return;
    const int cam = e / g.K, k = e - cam * g.K, b = cam / g.V;
    const float* q = X3 + ((size_t)b * g.K + k) * 3;
    const float X[3] = {q[0], q[1], q[2]};
    float pu, pv;
    cam_project(X, g.extr + (size_t)cam * 12, cam_load_k(g.intr + (size_t)cam * 9), cam_load_dist(g.dist + (size_t)cam * kCamDist),
                g.bbox ? g.bbox + (size_t)cam * 4 : nullptr, g.mh, g.mw, pu, pv);
    p2d[(size_t)e * 2] = pu, p2d[(size_t)e * 2 + 1] = pv;
}

__global__ __launch_bounds__(kCamThreads) void cam_project_bwd_kernel(CamRig g, int B, const float* __restrict__ X3, const float* __restrict__ g2d,
                                                                      float* __restrict__ gX3) {
    const int e = blockIdx.x * kCamThreads + threadIdx.x;
    if (e >= B * g.K) return;
    const int b = e / g.K, k = e - b * g.K;
    const float X[3] = {X3[(size_t)e * 3], X3[(size_t)e * 3 + 1], X3[(size_t)e * 3 + 2]};
    float gX[3] = {0.f, 0.f, 0.f};
    if (!(cam_isnan(X[0]) || cam_isnan(X[1]) || cam_isnan(X[2]))) {
        for (int v = 0; v < g.V; ++v) {
            const size_t cam = (size_t)b * g.V + v;
            const float* q = g2d + (cam * g.K + k) * 2;
            cam_project_bwd(X, g.extr + cam * 12, cam_load_k(g.intr + cam * 9), cam_load_dist(g.dist + cam * kCamDist),
                            g.bbox ? g.bbox + cam * 4 : nullptr, g.mh, g.mw, q[0], q[1], gX);
        }
    }
    gX3[(size_t)e * 3] = gX[0], gX3[(size_t)e * 3 + 1] = gX[1], gX3[(size_t)e * 3 + 2] = gX[2];
}

// ---- pairwise 3-D loss ------------------------------------------------------------------------------------
// mean over the valid (sample, pair, keypoint) of ||targ[b, k] - pred[b, p, k]||; an entry is invalid if either has a NaN; 0 (and a zero
// gradient) if none is valid.  One workgroup: value and unit-upstream gradient in one launch, the count never leaves the device.
__global__ __launch_bounds__(256) void cam_pairwise_kernel(const float* __restrict__ targ, const float* __restrict__ pred, int B, int P, int K,
                                                           float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ float red[4];
    const int n = B * P * K;
    float part = 0.f, cnt = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int k = e % K, b = e / (P * K);
        const float* t = targ + ((size_t)b * K + k) * 3;
        const float d0 = pred[(size_t)e * 3] - t[0], d1 = pred[(size_t)e * 3 + 1] - t[1], d2 = pred[(size_t)e * 3 + 2] - t[2];
        const float sq = d0 * d0 + d1 * d1 + d2 * d2;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (sq == sq) {   // (a NaN in the target or the prediction makes the sum NaN)
            const float d = sqrtf(sq);
            part += d;
            cnt += 1.f;
            if (d > 0.f) g0 = d0 / d, g1 = d1 / d, g2 = d2 / d;
        }
        grad[(size_t)e * 3] = g0, grad[(size_t)e * 3 + 1] = g1, grad[(size_t)e * 3 + 2] = g2;
    }
    part = block_sum<4>(part, red);
    cnt = block_sum<4>(cnt, red);
    const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
    for (int e = threadIdx.x; e < n; e += 256) {   // (each thread rescales the entries it wrote itself)
        grad[(size_t)e * 3] *= inv, grad[(size_t)e * 3 + 1] *= inv, grad[(size_t)e * 3 + 2] *= inv;
    }
    if (threadIdx.x == 0) loss[0] = part * inv;
}

static bool cam_rig(const float* points, const float* intr, const float* extr, const float* dist, const float* bbox, float mh, float mw, int V, int K,
                    CamRig& g) {
    g = CamRig{points, intr, extr, dist, bbox, mh, mw, V, K, V * (V - 1) / 2};
    return true;
}

}  // namespace lp

extern "C" size_t lp_cam_chain_workspace_bytes(int B, int V, int K) {
    if (B <= 0 || V < 2 || K <= 0 || V > LP_CAM_MAX_VIEWS) return 0;
    return ((size_t)B * K * 3 + (size_t)B * (V * (V - 1) / 2) * K * 4) * sizeof(float);
}

extern "C" int lp_cam_chain_fwd(const float* points, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                                float model_h, float model_w, int B, int V, int K, float* p3d, float* p2d, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(points && intrinsics && extrinsics && dist12 && p3d && B > 0 && V >= 2 && K > 0);
    if (V > LP_CAM_MAX_VIEWS || B > 65535) return LP_ERR_UNSUPPORTED;
    CamRig g;
    cam_rig(points, intrinsics, extrinsics, dist12, bbox, model_h, model_w, V, K, g);
    hipLaunchKernelGGL(cam_chain_fwd_kernel, dim3(B), dim3(kCamThreads), 0, (hipStream_t)stream, g, p3d, p2d);
    return launch_status();
}

extern "C" int lp_cam_chain_bwd(const float* points, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                                float model_h, float model_w, int B, int V, int K, const float* p3d, const float* g3d, const float* g2d,
                                void* workspace, size_t workspace_bytes, float* gpoints, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(points && intrinsics && extrinsics && dist12 && gpoints && workspace && (g3d || g2d) && (!g2d || p3d) && B > 0 && V >= 2 && K > 0);
    if (V > LP_CAM_MAX_VIEWS || B > 65535) return LP_ERR_UNSUPPORTED;
    LP_REQUIRE(workspace_bytes >= lp_cam_chain_workspace_bytes(B, V, K));
    CamRig g;
    cam_rig(points, intrinsics, extrinsics, dist12, bbox, model_h, model_w, V, K, g);
    hipLaunchKernelGGL(cam_chain_bwd_kernel, dim3(B), dim3(kCamThreads), 0, (hipStream_t)stream, g, B, p3d, g3d, g2d, (float*)workspace, gpoints);
    return launch_status();
}

extern "C" int lp_cam_project_fwd(const float* points_3d, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                                  float model_h, float model_w, int B, int V, int K, float* p2d, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(points_3d && intrinsics && extrinsics && dist12 && p2d && B > 0 && V >= 1 && K > 0);
    if ((long long)B * V * K > (1LL << 30)) return LP_ERR_UNSUPPORTED;
    CamRig g;
    cam_rig(nullptr, intrinsics, extrinsics, dist12, bbox, model_h, model_w, V, K, g);
    hipLaunchKernelGGL(cam_project_fwd_kernel, dim3((B * V * K + kCamThreads - 1) / kCamThreads), dim3(kCamThreads), 0, (hipStream_t)stream, g, B,
                       points_3d, p2d);
    return launch_status();
}

extern "C" int lp_cam_project_bwd(const float* points_3d, const float* intrinsics, const float* extrinsics, const float* dist12, const float* bbox,
                                  float model_h, float model_w, int B, int V, int K, const float* g2d, float* g3d, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(points_3d && intrinsics && extrinsics && dist12 && g2d && g3d && B > 0 && V >= 1 && K > 0);
    if ((long long)B * V * K > (1LL << 30)) return LP_ERR_UNSUPPORTED;
    CamRig g;
    cam_rig(nullptr, intrinsics, extrinsics, dist12, bbox, model_h, model_w, V, K, g);
    hipLaunchKernelGGL(cam_project_bwd_kernel, dim3((B * K + kCamThreads - 1) / kCamThreads), dim3(kCamThreads), 0, (hipStream_t)stream, g, B,
                       points_3d, g2d, g3d);
    return launch_status();
}

extern "C" int lp_cam_pairwise_fwd_bwd(const float* targ_3d, const float* pred_3d, int B, int P, int K, float* loss, float* grad_unit,
                                       lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(targ_3d && pred_3d && loss && grad_unit && B > 0 && P > 0 && K > 0);
    if ((long long)B * P * K > (1LL << 24)) return LP_ERR_UNSUPPORTED;   // (one workgroup; the count is exact in fp32 up to 2^24)
    hipLaunchKernelGGL(cam_pairwise_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, targ_3d, pred_3d, B, P, K, loss, grad_unit);
    return launch_status();
}
