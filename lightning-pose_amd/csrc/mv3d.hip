// Multi-view labeled batches with the 3-D augmentation (reference data/datasets.py:853-1104, MultiviewHeatmapDataset.apply_3d_transforms),
// built on the device.  gfx950, fp32, plain HIP C++.  Three kernels:
//   mv3d_plan_kernel    ONE workgroup per sample: labels -> frame px -> undistort + triangulate every camera pair (cam_common.h, the arithmetic
//                       of lp_cam_chain_fwd) -> nanmedian over the pairs -> random 3-D scale and translation -> reprojection into every view ->
//                       per-view least-squares similarity (what cv2.estimateAffinePartial2D returns when every point is an inlier) -> model px.
//                       Phases separated by __syncthreads(); the hand-over is LDS.  No atomics; every median is a rank selection (exact, any
//                       order) and every sum runs over ascending keypoint index in one lane: the same input gives the same bits.
//   mv3d_fill_kernel    per sample the minimum normalised pixel value (the reference pads the warp with orig_img.min()): the per-channel
//                       minimum of the uint8 image, normalised - the normalisation is increasing per channel.
//   mv3d_finish_kernel  normalise -> kornia warp_affine (bilinear, align_corners=True, padding_mode="fill") -> kornia resize (bilinear,
//                       half-pixel centres, no antialiasing, clamped taps) in one pass: an output pixel's 4 resize taps are integer pixels of
//                       the warped image, each of them one bilinear sample of the source at M^-1 (X, Y).  The warped image is never written.
// The arithmetic of the two image kernels is written with contraction off, so that a tap with weights (1, 0, 0, 0) is the source value
// itself: an identity M gives the plain resize bit for bit.
#include "cam_common.h"

namespace lp {

constexpr int kMvThreads = 256;
constexpr int kMvMaxViews = LP_MV3D_MAX_VIEWS, kMvMaxKp = LP_MV3D_MAX_KEYPOINTS;
constexpr int kMvMaxPairs = kMvMaxViews * (kMvMaxViews - 1) / 2;

__device__ __forceinline__ bool mv_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // (false for NaN)

// nanmedian of vals[0], vals[stride], ..., n of them, by rank selection: element i has rank #{j : v_j < v_i or (v_j == v_i and j < i)} among
// the non-NaN ones; the median is the mean of ranks (m - 1) / 2 and m / 2 (numpy: the mean of the two middle values; the same element when m
// is odd).  NaN if every value is NaN.  O(n^2) reads of LDS, n <= 128.
__device__ __forceinline__ float mv_nanmedian(const float* vals, int n, int stride) {
    int m = 0;
    for (int j = 0; j < n; ++j) m += cam_isnan(vals[j * stride]) ? 0 : 1;
    if (m == 0) return cam_nan();
    const int r_lo = (m - 1) >> 1, r_hi = m >> 1;
    float lo = 0.f, hi = 0.f;
    for (int i = 0; i < n; ++i) {
        const float vi = vals[i * stride];
        if (cam_isnan(vi)) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float vj = vals[j * stride];
            rank += (vj < vi || (vj == vi && j < i)) ? 1 : 0;   // (false for a NaN v_j)
        }
        lo = rank == r_lo ? vi : lo;
        hi = rank == r_hi ? vi : hi;
    }
    return (lo + hi) * 0.5f;
}

struct MvPlan {
    const float* kp;       // (B, V, K, 2) stored-image px
    const float* src_hw;   // (B, V, 2)
    const float* bbox;     // (B, 4 V)
    const float* intr;     // (B, V, 3, 3)
    const float* extr;     // (B, V, 3, 4)
    const float* dist;     // (B, V, 12)
    const float* draws;    // (B, 4) scale, r_x, r_y, r_z
    int augment;
    float shift, mh, mw;
    int V, K;
    float* kp3d;           // (B, K, 3)
    float* kp2d;           // (B, V, K, 2)
    float* affine;         // (B, V, 2, 3)
    int* status;           // (B)
};

__global__ __launch_bounds__(kMvThreads) void mv3d_plan_kernel(MvPlan g) {
    __shared__ float s_pts[kMvMaxViews * kMvMaxKp * 2];      // labels in frame px
    __shared__ float s_p3d[kMvMaxPairs * kMvMaxKp * 3];      // every pair's triangulation; after the median: the reprojection q (V, K, 2)
    __shared__ float s_X[kMvMaxKp * 3], s_Xa[kMvMaxKp * 3];  // triangulated / augmented world points
    __shared__ float s_M[kMvMaxViews * 6];
    __shared__ float s_red[4], s_med[3], s_shift[3];
    __shared__ int s_short;
    const int b = blockIdx.x, V = g.V, K = g.K, P = V * (V - 1) / 2, tid = threadIdx.x;
    const float* kp_b = g.kp + (size_t)b * V * K * 2;
    float* s_q = s_p3d;

    // (1) stored px -> frame px (norm_to_frame); count the non-NaN coordinates
    float seen = 0.f;
    for (int e = tid; e < V * K; e += kMvThreads) {
        const int v = e / K;
        const size_t cam = (size_t)b * V + v;
        const float hs = g.src_hw[cam * 2], ws = g.src_hw[cam * 2 + 1];
        const float* bb = g.bbox + cam * 4;
        const float x = kp_b[e * 2], y = kp_b[e * 2 + 1];
        s_pts[e * 2] = x / ws * bb[3] + bb[0];
        s_pts[e * 2 + 1] = y / hs * bb[2] + bb[1];
        seen += (cam_isnan(x) ? 0.f : 1.f) + (cam_isnan(y) ? 0.f : 1.f);
    }
    if (tid == 0) s_short = 0;
    seen = block_sum<4>(seen, s_red);   // (counts <= 2048: exact in fp32; its barriers also publish s_pts)

    // (2) every (pair, keypoint): undistort both points, triangulate
    for (int e = tid; e < P * K; e += kMvThreads) {
        const int p = e / K, k = e - p * K;
        int j1, j2;
        cam_pair_views(p, V, j1, j2);
        const size_t c1 = (size_t)b * V + j1, c2 = (size_t)b * V + j2;
        float x1, y1, x2, y2, X[3];
        cam_undistort(s_pts[(j1 * K + k) * 2], s_pts[(j1 * K + k) * 2 + 1], cam_load_k(g.intr + c1 * 9), cam_load_dist(g.dist + c1 * kCamDist), x1, y1);
        cam_undistort(s_pts[(j2 * K + k) * 2], s_pts[(j2 * K + k) * 2 + 1], cam_load_k(g.intr + c2 * 9), cam_load_dist(g.dist + c2 * kCamDist), x2, y2);
        if (!(cam_isnan(x1) || cam_isnan(y1) || cam_isnan(x2) || cam_isnan(y2))) {
            CamTri T;
            cam_triangulate(g.extr + c1 * 12, g.extr + c2 * 12, x1, y1, x2, y2, T, X);
        } else {
            X[0] = X[1] = X[2] = cam_nan();
        }
        s_p3d[e * 3] = X[0], s_p3d[e * 3 + 1] = X[1], s_p3d[e * 3 + 2] = X[2];
    }
    __syncthreads();

    // (3) nanmedian over the pairs, per keypoint and coordinate
    for (int e = tid; e < K * 3; e += kMvThreads) s_X[e] = mv_nanmedian(s_p3d + e, P, K * 3);
    __syncthreads();
    float ok3 = 0.f;
    for (int k = tid; k < K; k += kMvThreads) ok3 += (cam_isnan(s_X[k * 3]) || cam_isnan(s_X[k * 3 + 1]) || cam_isnan(s_X[k * 3 + 2])) ? 0.f : 1.f;
    ok3 = block_sum<4>(ok3, s_red);
    int status = seen == 0.f ? 2 : ((g.augment == 0 || ok3 < 3.f) ? 1 : 0);   // (the same in every lane)

    if (status == 0) {
        // (4) scale about the median keypoint, translate by a fraction of the extent
        if (tid < 3) s_med[tid] = mv_nanmedian(s_X + tid, K, 3);
        __syncthreads();
        const float scale = g.draws[b * 4];
        for (int e = tid; e < K * 3; e += kMvThreads) {
            const float med = s_med[e % 3];
            s_Xa[e] = (s_X[e] - med) * scale + med;
        }
        __syncthreads();
        if (tid < 3) {
            float lo = cam_nan(), hi = cam_nan();
            for (int k = 0; k < K; ++k) {   // nanmin / nanmax
                const float v = s_Xa[k * 3 + tid];
                if (cam_isnan(v)) continue;
                lo = (cam_isnan(lo) || v < lo) ? v : lo;
                hi = (cam_isnan(hi) || v > hi) ? v : hi;
            }
            s_shift[tid] = g.shift * (hi - lo) * g.draws[b * 4 + 1 + tid];
        }
        __syncthreads();
        for (int e = tid; e < K * 3; e += kMvThreads) s_Xa[e] += s_shift[e % 3];
        __syncthreads();   // (s_p3d is dead from here: s_q takes its place)
        for (int e = tid; e < V * K; e += kMvThreads) {
            const int v = e / K, k = e - v * K;
            const size_t cam = (size_t)b * V + v;
            const float X[3] = {s_Xa[k * 3], s_Xa[k * 3 + 1], s_Xa[k * 3 + 2]};
            float pu, pv;
            cam_project(X, g.extr + cam * 12, cam_load_k(g.intr + cam * 9), cam_load_dist(g.dist + cam * kCamDist), nullptr, 1.f, 1.f, pu, pv);
            s_q[e * 2] = pu, s_q[e * 2 + 1] = pv;
        }
        __syncthreads();

        // (5) per view: the least-squares similarity stored px -> warped px over the keypoints finite in both; one lane per view, sums over
        // ascending keypoint index
        if (tid < V) {
            const int v = tid;
            const size_t cam = (size_t)b * V + v;
            const float hs = g.src_hw[cam * 2], ws = g.src_hw[cam * 2 + 1];
            const float bx = g.bbox[cam * 4], by = g.bbox[cam * 4 + 1], bh = g.bbox[cam * 4 + 2], bw = g.bbox[cam * 4 + 3];
            float n = 0.f, mox = 0.f, moy = 0.f, mnx = 0.f, mny = 0.f;
            for (int k = 0; k < K; ++k) {
                const float ox = kp_b[(v * K + k) * 2], oy = kp_b[(v * K + k) * 2 + 1];
                const float nx = (s_q[(v * K + k) * 2] - bx) / bw * ws, ny = (s_q[(v * K + k) * 2 + 1] - by) / bh * hs;
                if (!(mv_finite(ox) && mv_finite(oy) && mv_finite(nx) && mv_finite(ny))) continue;
                n += 1.f, mox += ox, moy += oy, mnx += nx, mny += ny;
            }
            float M[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
            if (n < 3.f) {
                s_short = 1;   // (every writer writes 1)
            } else {
                mox /= n, moy /= n, mnx /= n, mny /= n;
                float dot = 0.f, crs = 0.f, den = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float ox = kp_b[(v * K + k) * 2], oy = kp_b[(v * K + k) * 2 + 1];
                    const float nx = (s_q[(v * K + k) * 2] - bx) / bw * ws, ny = (s_q[(v * K + k) * 2 + 1] - by) / bh * hs;
                    if (!(mv_finite(ox) && mv_finite(oy) && mv_finite(nx) && mv_finite(ny))) continue;
                    const float px = ox - mox, py = oy - moy, qx = nx - mnx, qy = ny - mny;
                    dot += px * qx + py * qy;
                    crs += px * qy - py * qx;
                    den += px * px + py * py;
                }
                if (den > 0.f) {
                    const float a = dot / den, c = crs / den;
                    M[0] = a, M[1] = -c, M[2] = mnx - (a * mox - c * moy);
                    M[3] = c, M[4] = a, M[5] = mny - (c * mox + a * moy);
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) s_M[v * 6 + i] = M[i];
        }
        __syncthreads();
        if (s_short) status = 3;   // the reference raises "should have been caught earlier" here; this falls back to the unaugmented sample
    }

    // (6) outputs
    const bool aug = status == 0;
    for (int e = tid; e < K * 3; e += kMvThreads) g.kp3d[(size_t)b * K * 3 + e] = aug ? s_Xa[e] : s_X[e];
    for (int e = tid; e < V * K; e += kMvThreads) {
        const int v = e / K;
        const size_t cam = (size_t)b * V + v;
        float x, y;
        if (aug) {
            const float* bb = g.bbox + cam * 4;
            x = (s_q[e * 2] - bb[0]) / bb[3] * g.mw;
            y = (s_q[e * 2 + 1] - bb[1]) / bb[2] * g.mh;
        } else {
            x = kp_b[e * 2] / g.src_hw[cam * 2 + 1] * g.mw;
            y = kp_b[e * 2 + 1] / g.src_hw[cam * 2] * g.mh;
        }
        g.kp2d[((size_t)b * V * K + e) * 2] = x, g.kp2d[((size_t)b * V * K + e) * 2 + 1] = y;
    }
    for (int e = tid; e < V * 6; e += kMvThreads) {
        const int i = e % 6;
        g.affine[(size_t)b * V * 6 + e] = aug ? s_M[e] : ((i == 0 || i == 4) ? 1.f : 0.f);
    }
    if (tid == 0) g.status[b] = status;
}

// ---- images ---------------------------------------------------------------------------------------------------------------------------
struct MvNorm {
    float mean[3], std[3];
};

// (v / 255 - mean) / std, each operation rounded on its own (torchvision ToTensor + Normalize)
__device__ __forceinline__ float mv_normalise(int v, float mean, float stdv) {
#pragma clang fp contract(off)
    return ((float)v / 255.f - mean) / stdv;
}

constexpr int kMvFillThreads = 1024;

__device__ __forceinline__ unsigned mv_min_bytes(unsigned a, unsigned b) {   // min of two bytes held in bits 0 - 7
    return a < b ? a : b;
}

// one workgroup per sample: 16-byte loads over the aligned middle of the sample's bytes, single bytes at both ends; the channel of byte i is
// i % 3 (interleaved RGB).  A minimum does not depend on the order.
__global__ __launch_bounds__(kMvFillThreads) void mv3d_fill_kernel(const unsigned char* __restrict__ src, size_t n, MvNorm nm, float* __restrict__ fill) {
    __shared__ unsigned s_min[3][kMvFillThreads / 64];
    const unsigned char* p = src + (size_t)blockIdx.x * n;
    const size_t head0 = (size_t)((16u - (unsigned)((size_t)p & 15u)) & 15u);
    const size_t head = head0 < n ? head0 : n;
    const size_t nvec = (n - head) / 16;
    unsigned m0 = 255u, m1 = 255u, m2 = 255u;
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    for (size_t i = threadIdx.x; i < nvec; i += kMvFillThreads) {
        const uint4 q = pv[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        unsigned r0 = 255u, r1 = 255u, r2 = 255u;   // by (byte index within the 16) % 3
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned byte = (w[j >> 2] >> (8 * (j & 3))) & 255u;
            if (j % 3 == 0) r0 = mv_min_bytes(r0, byte);
            else if (j % 3 == 1) r1 = mv_min_bytes(r1, byte);
            else r2 = mv_min_bytes(r2, byte);
        }
        const unsigned c0 = (unsigned)((head + i * 16) % 3);   // channel of the first byte
        const unsigned a0 = c0 == 0 ? r0 : (c0 == 1 ? r2 : r1), a1 = c0 == 0 ? r1 : (c0 == 1 ? r0 : r2), a2 = c0 == 0 ? r2 : (c0 == 1 ? r1 : r0);
        m0 = mv_min_bytes(m0, a0), m1 = mv_min_bytes(m1, a1), m2 = mv_min_bytes(m2, a2);
    }
    const size_t tail = head + nvec * 16;
    for (size_t i = threadIdx.x; i < head + (n - tail); i += kMvFillThreads) {
        const size_t at = i < head ? i : tail + (i - head);
        const unsigned byte = p[at], c = (unsigned)(at % 3);
        m0 = c == 0 ? mv_min_bytes(m0, byte) : m0, m1 = c == 1 ? mv_min_bytes(m1, byte) : m1, m2 = c == 2 ? mv_min_bytes(m2, byte) : m2;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        m0 = mv_min_bytes(m0, (unsigned)__shfl_xor((int)m0, s, 64));
        m1 = mv_min_bytes(m1, (unsigned)__shfl_xor((int)m1, s, 64));
        m2 = mv_min_bytes(m2, (unsigned)__shfl_xor((int)m2, s, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_min[0][wave] = m0, s_min[1][wave] = m1, s_min[2][wave] = m2;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMvFillThreads / 64; ++w)
            m0 = mv_min_bytes(m0, s_min[0][w]), m1 = mv_min_bytes(m1, s_min[1][w]), m2 = mv_min_bytes(m2, s_min[2][w]);
        const float f0 = mv_normalise((int)m0, nm.mean[0], nm.std[0]), f1 = mv_normalise((int)m1, nm.mean[1], nm.std[1]),
                    f2 = mv_normalise((int)m2, nm.mean[2], nm.std[2]);
        fill[blockIdx.x] = fminf(f0, fminf(f1, f2));
    }
}

constexpr int kMvTileX = 64, kMvTileY = 4;   // 64 x 4 lanes, 4 output pixels along x each: a 256 x 4 tile of the output

struct MvFinish {
    const unsigned char* src;   // (B, Hs, Ws, 3)
    const float* affine;        // (B, V, 2, 3)
    const float* fill;          // (B)
    float* dst;                 // (B, V, 3, H, W)
    int Hs, Ws, V, v, H, W;
    float ry, rx;               // Hs / H, Ws / W
};

// torch's area_pixel_compute_source_index (align_corners=False, not cubic): the source index of an output pixel, clamped at 0
__device__ __forceinline__ void mv_resize_tap(int o, float ratio, int n_in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    float s = ratio * ((float)o + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

// bilinear sample of the normalised source at (sx, sy), pixel-index coordinates; a neighbour outside the image reads `fill`
__device__ __forceinline__ void mv_sample(const unsigned char* __restrict__ img, int Hs, int Ws, const float (*lut)[256], float sx, float sy, float fill,
                                          float (&out)[3]) {
#pragma clang fp contract(off)
    if (!(sx > -1.f && sx < (float)Ws && sy > -1.f && sy < (float)Hs)) {   // (also NaN: a singular M)
        out[0] = out[1] = out[2] = fill;
        return;
    }
    const float fx = floorf(sx), fy = floorf(sy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = sx - fx, wx0 = 1.f - wx1, wy1 = sy - fy, wy0 = 1.f - wy1;
    const bool inx0 = x0 >= 0, inx1 = x0 + 1 < Ws, iny0 = y0 >= 0, iny1 = y0 + 1 < Hs;
    const unsigned char* r0 = img + ((size_t)(iny0 ? y0 : 0) * Ws) * 3;
    const unsigned char* r1 = img + ((size_t)(iny1 ? y0 + 1 : 0) * Ws) * 3;
    const int xa = (inx0 ? x0 : 0) * 3, xb = (inx1 ? x0 + 1 : 0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = (inx0 && iny0) ? lut[c][r0[xa + c]] : fill, v01 = (inx1 && iny0) ? lut[c][r0[xb + c]] : fill;
        const float v10 = (inx0 && iny1) ? lut[c][r1[xa + c]] : fill, v11 = (inx1 && iny1) ? lut[c][r1[xb + c]] : fill;
        out[c] = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
    }
}

__global__ __launch_bounds__(kMvTileX* kMvTileY) void mv3d_finish_kernel(MvFinish g, MvNorm nm) {
#pragma clang fp contract(off)
    __shared__ float s_lut[3][256];
    __shared__ float s_inv[6];
    const int tid = threadIdx.y * kMvTileX + threadIdx.x, b = blockIdx.z;
    for (int e = tid; e < 768; e += kMvTileX * kMvTileY) {
        const int c = e >> 8;
        s_lut[c][e & 255] = mv_normalise(e & 255, c == 0 ? nm.mean[0] : (c == 1 ? nm.mean[1] : nm.mean[2]),
                                         c == 0 ? nm.std[0] : (c == 1 ? nm.std[1] : nm.std[2]));
    }
    if (tid == 0) {   // M^-1, once per image: warped (X, Y) -> source (x, y)
        const float* M = g.affine + ((size_t)b * g.V + g.v) * 6;
        const float det = M[0] * M[4] - M[1] * M[3];
        const float i00 = M[4] / det, i01 = -M[1] / det, i10 = -M[3] / det, i11 = M[0] / det;
        s_inv[0] = i00, s_inv[1] = i01, s_inv[2] = -(i00 * M[2] + i01 * M[5]);
        s_inv[3] = i10, s_inv[4] = i11, s_inv[5] = -(i10 * M[2] + i11 * M[5]);
    }
    __syncthreads();
    const int y = blockIdx.y * kMvTileY + threadIdx.y, xq = (blockIdx.x * kMvTileX + threadIdx.x) * 4;
    if (y >= g.H || xq >= g.W) return;
    const unsigned char* img = g.src + (size_t)b * g.Hs * g.Ws * 3;
    const float fill = g.fill[b];
    const float i00 = s_inv[0], i01 = s_inv[1], itx = s_inv[2], i10 = s_inv[3], i11 = s_inv[4], ity = s_inv[5];
    int Y0, Y1;
    float ly0, ly1;
    mv_resize_tap(y, g.ry, g.Hs, Y0, Y1, ly0, ly1);
    float res[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = xq + j < g.W ? xq + j : g.W - 1;   // (a lane past the row's end repeats its last pixel and does not store it)
        int X0, X1;
        float lx0, lx1;
        mv_resize_tap(x, g.rx, g.Ws, X0, X1, lx0, lx1);
        float p00[3], p01[3], p10[3], p11[3];
        mv_sample(img, g.Hs, g.Ws, s_lut, i00 * (float)X0 + i01 * (float)Y0 + itx, i10 * (float)X0 + i11 * (float)Y0 + ity, fill, p00);
        mv_sample(img, g.Hs, g.Ws, s_lut, i00 * (float)X1 + i01 * (float)Y0 + itx, i10 * (float)X1 + i11 * (float)Y0 + ity, fill, p01);
        mv_sample(img, g.Hs, g.Ws, s_lut, i00 * (float)X0 + i01 * (float)Y1 + itx, i10 * (float)X0 + i11 * (float)Y1 + ity, fill, p10);
        mv_sample(img, g.Hs, g.Ws, s_lut, i00 * (float)X1 + i01 * (float)Y1 + itx, i10 * (float)X1 + i11 * (float)Y1 + ity, fill, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c][j] = ly0 * (lx0 * p00[c] + lx1 * p01[c]) + ly1 * (lx0 * p10[c] + lx1 * p11[c]);   // (torch's order)
    }
    float* out = g.dst + ((((size_t)b * g.V + g.v) * 3) * g.H + y) * g.W + xq;
    const size_t plane = (size_t)g.H * g.W;
    const bool vec = xq + 3 < g.W && (g.W & 3) == 0 && ((size_t)g.dst & 15) == 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (vec) {
            *reinterpret_cast<float4*>(out + c * plane) = make_float4(res[c][0], res[c][1], res[c][2], res[c][3]);   // 16-byte store
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (xq + j < g.W) out[c * plane + j] = res[c][j];
        }
    }
}

static bool mv_norm(const lp_frame_norm* norm, MvNorm& nm) {
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = norm->mean[c], nm.std[c] = norm->std[c];
        if (!(nm.std[c] > 0.f)) return false;
    }
    return true;
}

}  // namespace lp

extern "C" int lp_mv3d_plan(const float* kp, const float* src_hw, const float* bbox, const float* intrinsics, const float* extrinsics,
                            const float* dist12, const float* draws, int augment, float shift_param, int H, int W, int B, int V, int K, float* kp3d,
                            float* kp2d, float* affine, int* status, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(kp && src_hw && bbox && intrinsics && extrinsics && dist12 && draws && kp3d && kp2d && affine && status);
    LP_REQUIRE(B > 0 && V >= 2 && K > 0 && H > 0 && W > 0);
    if (V > LP_MV3D_MAX_VIEWS || K > LP_MV3D_MAX_KEYPOINTS || B > 65535) return LP_ERR_UNSUPPORTED;
    MvPlan g{kp, src_hw, bbox, intrinsics, extrinsics, dist12, draws, augment != 0, shift_param, (float)H, (float)W, V, K, kp3d, kp2d, affine, status};
    hipLaunchKernelGGL(mv3d_plan_kernel, dim3(B), dim3(kMvThreads), 0, (hipStream_t)stream, g);
    return launch_status();
}

extern "C" int lp_mv3d_fill(const void* src_u8, int B, int Hs, int Ws, const lp_frame_norm* norm, float* fill, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(src_u8 && norm && fill && B > 0 && Hs > 0 && Ws > 0);
    if (B > 65535) return LP_ERR_UNSUPPORTED;
    MvNorm nm;
    LP_REQUIRE(mv_norm(norm, nm));
    hipLaunchKernelGGL(mv3d_fill_kernel, dim3(B), dim3(kMvFillThreads), 0, (hipStream_t)stream, (const unsigned char*)src_u8, (size_t)Hs * Ws * 3, nm,
                       fill);
    return launch_status();
}

extern "C" int lp_mv3d_finish(const void* src_u8, int B, int Hs, int Ws, const float* affine, const float* fill, const lp_frame_norm* norm, int V,
                              int v, int H, int W, float* dst, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(src_u8 && affine && fill && norm && dst && B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && V > 0 && v >= 0 && v < V);
    if (B > 65535 || (H + kMvTileY - 1) / kMvTileY > 65535 || Hs > (1 << 23) || Ws > (1 << 23)) return LP_ERR_UNSUPPORTED;   // (pixel indices exact in fp32)
    MvNorm nm;
    LP_REQUIRE(mv_norm(norm, nm));
    MvFinish g{(const unsigned char*)src_u8, affine, fill, dst, Hs, Ws, V, v, H, W, (float)Hs / (float)H, (float)Ws / (float)W};
    const dim3 grid((W + 4 * kMvTileX - 1) / (4 * kMvTileX), (H + kMvTileY - 1) / kMvTileY, B);
    hipLaunchKernelGGL(mv3d_finish_kernel, grid, dim3(kMvTileX, kMvTileY), 0, (hipStream_t)stream, g, nm);
    return launch_status();
}
