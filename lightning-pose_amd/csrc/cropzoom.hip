// The two-stage "crop-zoom" prediction on the device: detector keypoints -> one box per frame -> [rolling median] -> each frame's own
// region of interest resampled straight from the decoded uint8 frame into the pose model's normalised input planes.  gfx950.
//
// Reference arithmetic (paths relative to the reference tree):
//   utils/cropzoom.py:31-143   _calculate_bbox_size / _compute_bbox_df   -> lp_bbox_from_keypoints
//   utils/cropzoom.py:355-402  smooth_bbox: DataFrame.rolling(window, center=True, min_periods=1).median().round(0).astype(int)
//                                                                        -> lp_bbox_smooth
//   utils/cropzoom.py:250-325  _crop_video_moviepy (zero-padded crop) followed by the video loader's resize + normalise
//                                                                        -> lp_frames_crop_resize (one launch, nothing intermediate stored)
// Nothing here is read back to the host: the boxes go from the first kernel to the last through device memory.
#include "frames_common.h"

namespace lp {

// ---- boxes from keypoints: one lane per frame, double precision, sums in keypoint order -----------------------------------------------------
struct BboxSpec {
    int N, K, n_anchor;      // n_anchor == 0: every keypoint
    int fixed, crop_h, crop_w;  // fixed mode: the (already even) box size
    double crop_ratio;
    unsigned char anchor[LP_BBOX_MAX_ANCHORS];
};

__global__ __launch_bounds__(256) void bbox_from_keypoints_kernel(const float* __restrict__ kp, BboxSpec p, int* __restrict__ bbox) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.N) return;
    const float* f = kp + (size_t)n * p.K * 2;
    const int cnt = p.n_anchor > 0 ? p.n_anchor : p.K;
    double sx = 0.0, sy = 0.0, xmin = 0.0, xmax = 0.0, ymin = 0.0, ymax = 0.0;
    bool finite = true;
    for (int a = 0; a < cnt; ++a) {
        const int k = p.n_anchor > 0 ? (int)p.anchor[a] : a;
        const double x = (double)f[2 * k], y = (double)f[2 * k + 1];
        finite = finite && fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308;  // (false for NaN)
        sx += x;
        sy += y;
        if (a == 0) {
            xmin = xmax = x;
            ymin = ymax = y;
        } else {
            xmin = fmin(xmin, x), xmax = fmax(xmax, x);
            ymin = fmin(ymin, y), ymax = fmax(ymax, y);
        }
    }
    int h = p.crop_h, w = p.crop_w;
    if (!p.fixed && finite) {
        const double span = fmax(xmax - xmin, ymax - ymin);
        const double size = ceil(span * p.crop_ratio);
        if (size >= 1.0 && size < 1073741824.0) {
            h = (int)size;
            h += h & 1;  // even sizes (the reference: "many video players don't like odd dimensions")
        } else {
            h = 0;
        }
        w = h;
    }
    // (sic) the reference subtracts [h // 2, w // 2] from the [x, y] centroid: x moves by half the HEIGHT.  np.int64() truncates toward zero.
    const double cx = trunc(sx / (double)cnt - (double)(h / 2)), cy = trunc(sy / (double)cnt - (double)(w / 2));
    const bool ok = finite && h > 0 && w > 0 && fabs(cx) < 2147483648.0 && fabs(cy) < 2147483648.0;
    int* o = bbox + (size_t)n * 4;
    o[0] = ok ? (int)cx : 0;
    o[1] = ok ? (int)cy : 0;
    o[2] = ok ? h : 0;
    o[3] = ok ? w : 0;
}

// ---- centred rolling median of each column: one lane per (frame, column); the median by counting ranks, ties broken by index -----------------
__device__ __forceinline__ int rank_select(const int* __restrict__ col, int lo, int n, int want) {  // the value of rank `want` among col[lo .. lo + n)
    for (int a = 0; a < n; ++a) {
        const int va = col[(size_t)(lo + a) * 4];
        int rank = 0;
        for (int b = 0; b < n; ++b) {
            const int vb = col[(size_t)(lo + b) * 4];
            rank += (vb < va) || (vb == va && b < a);
        }
        if (rank == want) return va;
    }
    return 0;  // not reached: ranks are a permutation of 0 .. n - 1
}

__global__ __launch_bounds__(256) void bbox_smooth_kernel(const int* __restrict__ in, int N, int window, int* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * 4) return;
    const int i = idx >> 2, c = idx & 3;
    int lo = i - window / 2, hi = i + (window - 1) / 2;  // pandas' centred window, both ends inclusive
    lo = lo < 0 ? 0 : lo;
    hi = hi > N - 1 ? N - 1 : hi;
    const int n = hi - lo + 1;
    const int* col = in + c;
    long long m;
    if (n & 1) {
        m = rank_select(col, lo, n, n / 2);
    } else {  // mean of the two middle values, rounded half to even (numpy's round): an odd sum s = 2 q + 1 is the half q + 0.5 -> the even one of q, q + 1
        const long long s = (long long)rank_select(col, lo, n, n / 2 - 1) + (long long)rank_select(col, lo, n, n / 2);
        const long long q = (s - (s & 1)) / 2;  // floor(s / 2): s - (s & 1) is even
        m = (s & 1) ? q + (q & 1) : q;
    }
    out[idx] = (int)m;
}

// ---- crop + antialiased resize + normalise --------------------------------------------------------------------------------------------------
// Frame s is the virtual image of its box: h_s x w_s pixels, pixel (i, j) = src[s][y_s + i][x_s + j] inside the frame and 0 outside it.  The
// arithmetic is frames_resize_kernel's on that image, term for term (the same windows, weights, fmaf order: horizontal chain inside, vertical
// chain outside, one division by wsum_x * wsum_y), so the planes are bit-identical to lp_frames_resize of the materialised crop.
//
// A workgroup owns a 64 x 4 output tile and walks the source rows its four output rows touch in chunks of kRows rows:
//   1. stage    the chunk's pixels [column range of the tile] -> LDS, one dword per pixel (channel c in byte c),
//               0 outside the frame (the zero padding).  A dword per pixel, not the 3 bytes of memory: neighbouring lanes of step 2 are
//               `scale` pixels apart, and a stride of 5 DWORDS (1280 -> 256) spreads a wave over all 32 banks where 15 BYTES put eight lanes
//               on one (measured: the byte layout ran at 1.2 - 1.4 x the per-pixel kernel's time);
//   2. across   per (source row, output column) the horizontal fmaf chain from the staged pixels -> three floats in LDS; a lane owns one column
//               and three rows of the chunk, so a tap's weight is formed once for the three.  A source row is filtered ONCE for the (up to
//               four) output rows whose windows hold it - the per-pixel form repeats it per output row;
//   3. down     every lane continues its own vertical chain over the rows of the chunk that lie in its window.
// Replicated rows (LP_BORDER_CLAMP outside the virtual image) reuse the edge row's sums, which is what they are.  The chunk loop has no
// upper bound on the number of rows, so any down-scale factor runs; a tile whose column range does not fit the staging buffer (more than
// kRowPix pixels) skips step 1 and reads its taps from global memory in step 2.
constexpr int kRows = 12;         // source rows per chunk (a multiple of 4): each of the four waves filters every fourth row, three per chunk
constexpr int kFar = 1 << 29, kMaxBox = 1 << 16;  // corners are pinned to +-kFar, boxes above kMaxBox pixels a side count as "no box"
constexpr int kRowPix = 340;      // staged pixels per row: a 5.1-fold horizontal down-scale of 64 output columns (1280 -> 256 needs 325)

struct CropSpec {
    int Hs, Ws, H, W;
    long long frame_stride;
    int row_stride;
    int border;
};

// The contract is BIT identity with frames_resize_kernel, and that kernel's bits depend on where the compiler contracts a multiply and an add
// into one fma: under hipcc's default (-ffp-contract=fast-honor-pragmas) it does so in the window bounds (centre - radius, centre + radius:
// the product (x + 0.5) * scale goes unrounded into the sum) and in v / 255 - mean, and nowhere else - the weights take the ROUNDED centre,
// which lives across a loop boundary.  The host compiler of the CPU-emulated build contracts nothing.  Which of these a compiler picks for a
// second copy of the same source text is not something source text can promise (it depends on which block an operand lands in), so this file
// switches contraction off and spells each of the two forms out.  tests/test_cropzoom_kernels.py holds both builds to the bits.
#if defined(__HIP_DEVICE_COMPILE__)
#define LP_CZ_FUSED(a, b, c) fmaf((a), (b), (c))
#else
#define LP_CZ_FUSED(a, b, c) ((a) * (b) + (c))
#endif

// tri_window(xf * scale, r, n, border, lo, hi) as frames_resize_kernel evaluates it
__device__ __forceinline__ void crop_window(float xf, float scale, float r, int n, int border, int& lo, int& hi) {
#pragma clang fp contract(off)
    lo = (int)floorf(LP_CZ_FUSED(xf, scale, -r) + 0.5f);
    hi = (int)floorf(LP_CZ_FUSED(xf, scale, r) + 0.5f);
    if (border == LP_BORDER_RENORM) {
        lo = lo < 0 ? 0 : lo;
        hi = hi > n ? n : hi;
    }
}

// tri_weight(j, c, inv_r) with c the rounded centre
__device__ __forceinline__ float crop_weight(int j, float c, float inv_r) {
#pragma clang fp contract(off)
    const float t = ((float)j + 0.5f) - c;
    return fmaxf(0.f, 1.f - fabsf(t * inv_r));
}

__device__ __forceinline__ float crop_centre(float xf, float scale) {
#pragma clang fp contract(off)
    return xf * scale;
}

__device__ __forceinline__ float crop_finish(float acc, float mean, float inv_std) {
#pragma clang fp contract(off)
    return LP_CZ_FUSED(acc, 1.f / 255.f, -mean) * inv_std;
}

__device__ __forceinline__ unsigned char tap_byte(const unsigned char* __restrict__ frame, const CropSpec& p, int yy, int xx, int c) {
    if (yy < 0 || yy >= p.Hs || xx < 0 || xx >= p.Ws) return 0;
    return frame[(size_t)yy * p.row_stride + (size_t)xx * 3 + c];
}

__global__ __launch_bounds__(256) void frames_crop_resize_kernel(const unsigned char* __restrict__ src, const int* __restrict__ bbox, CropSpec p,
                                                                 NormSpec nrm, float* __restrict__ dst) {
#pragma clang fp contract(off)
    __shared__ unsigned int stage[kRows * kRowPix];
    __shared__ float across[kRows * 3 * 64];
    const int tid = threadIdx.x, lx = tid & 63, ly = tid >> 6;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4, s = blockIdx.z;
    const int x = x0 + lx, y = y0 + ly;
    const size_t plane = (size_t)p.H * p.W;
    float* o = dst + (size_t)s * 3 * plane + (size_t)y * p.W + x;
    int bx = bbox[s * 4], by = bbox[s * 4 + 1];
    const int bh = bbox[s * 4 + 2], bw = bbox[s * 4 + 3];
    // a corner this far out leaves the whole box outside any frame this entry point accepts: pinning it there keeps the index arithmetic in int
    bx = clampi(bx, -kFar, kFar), by = clampi(by, -kFar, kFar);
    if (bh <= 0 || bw <= 0 || bh > kMaxBox || bw > kMaxBox) {  // no box (or not one of a real frame): the normalised black frame (uniform over the workgroup)
        if (x < p.W && y < p.H) {
            o[0] = crop_finish(0.f, nrm.mean[0], nrm.inv_std[0]);
            o[plane] = crop_finish(0.f, nrm.mean[1], nrm.inv_std[1]);
            o[2 * plane] = crop_finish(0.f, nrm.mean[2], nrm.inv_std[2]);
        }
        return;
    }
    const float scale_y = (float)((double)bh / p.H), scale_x = (float)((double)bw / p.W);
    const float ry = scale_y > 1.f ? scale_y : 1.f, rx = scale_x > 1.f ? scale_x : 1.f;
    const float irx = 1.f / rx, iry = 1.f / ry;
    const unsigned char* frame = src + (size_t)s * p.frame_stride;

    // the tile's source range: windows move monotonically with the output index, so the first and the last live row / column bound it
    const int xl = (x0 + 63 < p.W ? x0 + 63 : p.W - 1), yl = (y0 + 3 < p.H ? y0 + 3 : p.H - 1);
    int t_lo, t_hi, ilo, ihi, jlo, jhi;
    crop_window((float)x0 + 0.5f, scale_x, rx, bw, p.border, ilo, t_hi);
    crop_window((float)xl + 0.5f, scale_x, rx, bw, p.border, t_lo, ihi);
    crop_window((float)y0 + 0.5f, scale_y, ry, bh, p.border, jlo, t_hi);
    crop_window((float)yl + 0.5f, scale_y, ry, bh, p.border, t_lo, jhi);
    ilo = clampi(ilo, 0, bw - 1), ihi = clampi(ihi - 1, 0, bw - 1) + 1;  // the distinct pixels behind the (possibly replicated) taps
    jlo = clampi(jlo, 0, bh - 1), jhi = clampi(jhi - 1, 0, bh - 1) + 1;
    const int npx = ihi - ilo;  // pixels per staged row
    const bool staged = npx <= kRowPix;

    // this lane's column (the horizontal pass) and pixel (the vertical pass)
    const bool colive = x < p.W, live = colive && y < p.H;
    const float cx = crop_centre((float)x + 0.5f, scale_x), cy = crop_centre((float)y + 0.5f, scale_y);
    int xlo = 0, xhi = 0, ylo = 0, yhi = 0;
    float wsum_x = 0.f, wsum_y = 0.f, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    if (colive) crop_window((float)x + 0.5f, scale_x, rx, bw, p.border, xlo, xhi);
    if (live) {
        crop_window((float)y + 0.5f, scale_y, ry, bh, p.border, ylo, yhi);
        for (int i = xlo; i < xhi; ++i) wsum_x += crop_weight(i, cx, irx);
    }
    int j = ylo;  // next row of this lane's vertical chain

    for (int c0 = jlo; c0 < jhi; c0 += kRows) {
        const int nrow = jhi - c0 < kRows ? jhi - c0 : kRows;
        if (staged) {  // wave ly stages rows ly, ly + 4, ..: the row's address is uniform over the wave, lanes stride over its pixels
            for (int r = ly; r < nrow; r += 4) {
                const int yy = by + c0 + r;
                const bool in = yy >= 0 && yy < p.Hs;
                const unsigned char* row = frame + (size_t)(in ? yy : 0) * p.row_stride;
                for (int d = lx; d < npx; d += 64) {
                    const int xx = bx + ilo + d;
                    unsigned int v = 0;  // outside the frame: the zero padding
                    if (in && xx >= 0 && xx < p.Ws) {
                        const unsigned char* px = row + (size_t)xx * 3;
                        v = (unsigned int)px[0] | ((unsigned int)px[1] << 8) | ((unsigned int)px[2] << 16);
                    }
                    stage[r * kRowPix + d] = v;
                }
            }
            __syncthreads();
        }
        if (colive) {  // lane (lx, ly) filters column x of rows ly, ly + 4, ly + 8: one weight per tap serves the three rows
            float h[kRows / 4][3];
            int yy[kRows / 4];
            const unsigned int* pix[kRows / 4];
#pragma unroll
            for (int k = 0; k < kRows / 4; ++k) {
                h[k][0] = h[k][1] = h[k][2] = 0.f;
                const int r = ly + 4 * k < nrow ? ly + 4 * k : nrow - 1;  // (a row past the chunk repeats its last row and is not stored)
                yy[k] = by + c0 + r;
                pix[k] = stage + r * kRowPix - ilo;
            }
            if (staged) {
                for (int i = xlo; i < xhi; ++i) {
                    const float wx = crop_weight(i, cx, irx);
                    const int off = clampi(i, 0, bw - 1);
#pragma unroll
                    for (int k = 0; k < kRows / 4; ++k) {
                        const unsigned int px = pix[k][off];
                        h[k][0] = fmaf(wx, (float)(px & 255u), h[k][0]);
                        h[k][1] = fmaf(wx, (float)((px >> 8) & 255u), h[k][1]);
                        h[k][2] = fmaf(wx, (float)((px >> 16) & 255u), h[k][2]);
                    }
                }
            } else {
                for (int i = xlo; i < xhi; ++i) {
                    const float wx = crop_weight(i, cx, irx);
                    const int xx = bx + clampi(i, 0, bw - 1);
#pragma unroll
                    for (int k = 0; k < kRows / 4; ++k) {
                        h[k][0] = fmaf(wx, (float)tap_byte(frame, p, yy[k], xx, 0), h[k][0]);
                        h[k][1] = fmaf(wx, (float)tap_byte(frame, p, yy[k], xx, 1), h[k][1]);
                        h[k][2] = fmaf(wx, (float)tap_byte(frame, p, yy[k], xx, 2), h[k][2]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kRows / 4; ++k) {
                if (ly + 4 * k < nrow) {
                    float* q = across + (ly + 4 * k) * 192 + lx;
                    q[0] = h[k][0];
                    q[64] = h[k][1];
                    q[128] = h[k][2];
                }
            }
        }
        __syncthreads();
        if (live) {
            while (j < yhi) {
                const int r = clampi(j, 0, bh - 1) - c0;
                if (r >= nrow) break;
                const float wy = crop_weight(j, cy, iry);
                wsum_y += wy;
                const float* q = across + r * 192 + lx;
                acc0 = fmaf(wy, q[0], acc0);
                acc1 = fmaf(wy, q[64], acc1);
                acc2 = fmaf(wy, q[128], acc2);
                ++j;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const float inv = 1.f / (wsum_x * wsum_y);
    acc0 *= inv;
    acc1 *= inv;
    acc2 *= inv;
    o[0] = crop_finish(acc0, nrm.mean[0], nrm.inv_std[0]);
    o[plane] = crop_finish(acc1, nrm.mean[1], nrm.inv_std[1]);
    o[2 * plane] = crop_finish(acc2, nrm.mean[2], nrm.inv_std[2]);
}

}  // namespace lp

// ------------------------------------------------------------------------------------------------------- C ABI
extern "C" int lp_bbox_from_keypoints(const float* keypoints, int N, int K, const int* anchors, int n_anchors, double crop_ratio, int crop_height,
                                      int crop_width, int* bbox, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(keypoints && bbox && N > 0 && K > 0 && n_anchors >= 0 && (n_anchors == 0 || anchors));
    const bool fixed = crop_height > 0 && crop_width > 0;
    LP_REQUIRE(fixed ? !(crop_ratio > 0.0) : (crop_ratio > 0.0 && crop_height <= 0 && crop_width <= 0 && crop_ratio < 1e300));
    if (n_anchors > LP_BBOX_MAX_ANCHORS || (n_anchors > 0 && K > 256)) return LP_ERR_UNSUPPORTED;  // anchor indices travel as bytes
    LP_REQUIRE(crop_height < 1073741824 && crop_width < 1073741824);
    BboxSpec p{};
    p.N = N, p.K = K, p.n_anchor = n_anchors, p.fixed = fixed, p.crop_ratio = crop_ratio;
    p.crop_h = fixed ? crop_height + crop_height % 2 : 0, p.crop_w = fixed ? crop_width + crop_width % 2 : 0;
    for (int a = 0; a < n_anchors; ++a) {
        LP_REQUIRE(anchors[a] >= 0 && anchors[a] < K);
        p.anchor[a] = (unsigned char)anchors[a];
    }
    hipLaunchKernelGGL(bbox_from_keypoints_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, keypoints, p, bbox);
    return launch_status();
}

extern "C" int lp_bbox_smooth(const int* bbox_in, int N, int window, int* bbox_out, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(bbox_in && bbox_out && bbox_in != bbox_out && N > 0 && window >= 1);
    if (window > LP_BBOX_SMOOTH_MAX_WINDOW) return LP_ERR_UNSUPPORTED;
    LP_REQUIRE(N <= 536870911);
    hipLaunchKernelGGL(bbox_smooth_kernel, dim3((N * 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, bbox_in, N, window, bbox_out);
    return launch_status();
}

extern "C" int lp_frames_crop_resize(const void* src_u8, int S, int Hs, int Ws, long long frame_stride, int row_stride, const int* bbox, int H,
                                     int W, int border, const lp_frame_norm* norm, float* dst, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(src_u8 && bbox && norm && dst && S > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0);
    LP_REQUIRE(row_stride >= Ws * 3 && frame_stride >= (long long)row_stride * Hs);
    LP_REQUIRE(border == LP_BORDER_RENORM || border == LP_BORDER_CLAMP);
    if (S > 65535 || (H + 3) / 4 > 65535 || Ws > 268435456) return LP_ERR_UNSUPPORTED;
    CropSpec p{};
    p.Hs = Hs, p.Ws = Ws, p.H = H, p.W = W, p.frame_stride = frame_stride, p.row_stride = row_stride, p.border = border;
    NormSpec nrm{};
    LP_REQUIRE(norm_spec(norm, nrm));
    hipLaunchKernelGGL(frames_crop_resize_kernel, dim3((W + 63) / 64, (H + 3) / 4, S), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)src_u8, bbox, p, nrm, dst);
    return launch_status();
}
