// Labeled-frame augmentation on the device: the imgaug operators behind the reference's "dlc" presets (data/augmentations.py:122-238,
// applied per sample in data/datasets.py:279-293), one launch sequence per BATCH.  gfx950.
//
// imgaug and OpenCV are not vendored and cannot be run here: every operator below restates the library's documented definition, pixel
// parity with imgaug itself is UNPINNED.  What is pinned (tests/test_labeled_augmentation*.py) is each operator against an independent
// numpy / scipy restatement and the agreement of images and keypoints.
//
// Conventions chosen where the reference tree and imgaug's documentation leave them open (every preset range is symmetric, so none of the
// sign choices changes the distribution the model sees):
//   coordinates   continuous, the centre of pixel (row i, column j) is (x, y) = (j + 0.5, i + 0.5); keypoints live in the same frame
//   Affine        positive `rotate` turns the image clockwise on the screen (y down), about (W / 2, H / 2); bilinear, fill 0
//   Rot90         k quarter turns clockwise, then scaled back to (H, W) in the same bilinear gather (exact for k even or H == W)
//   rounding      every stage stores uint8: floor(v + 0.5), saturated
//   stencils      MotionBlur / Emboss are correlations with the border reflected without repeating the edge pixel (reflect-101)
//   coarse masks  cell (y gh / H, x gw / W) in integers; masked when (Philox word >> 8) < p 2^24
//   salt, pepper  imgaug draws 255 (0.5 +- |Beta(0.5, 0.5) - 0.5|) = 127.5 +- 127.5 |cos(pi u)|: here through a 256-entry quantile table of
//                 that law (host-made), one value per pixel shared by the three channels; pepper = 255 - salt
//   Elastic       out(x, y) = in(x + dx, y + dy); (dx, dy) = alpha * Gaussian(sigma, cut at 4 sigma, reflect-101) of U(-1, 1) noise; Keys
//                 bicubic (A = -0.75) stands for imgaug's order 3; taps outside the image read 0
//   HistEq        lut[v] = round(255 (cdf[v] - cdf_min) / (n - cdf_min)), ties up, in integer arithmetic
//   CLAHE         OpenCV's algorithm (clip, redistribute excess / 256 + one more to every step-th bin, bilinear blend of the four nearest
//                 tiles' tables at y / tile_h - 0.5), except that lut = round(255 cdf / area) is rounded in integers, ties up.  The host
//                 reads imgaug's `tile_grid_size_px` as the number of TILES per side (see data/augmentations.py: clahe_geometry)
//
// The kernels are byte movers: one lane per pixel with x fastest, the parameter row of the image read through scalar loads, LDS for the
// stencil tile, the elastic noise row and the histograms (privatised per wave; a workgroup adds each bin to memory once).
#include "frames_common.h"

namespace lp {

typedef unsigned char u8;

__device__ __forceinline__ u8 to_u8(float v) { return (u8)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f); }

// reflect-101 (dcb|abcd|cba), then clamped: any i is mapped into [0, n)
__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return clampi(i, 0, n - 1);
}

__device__ __forceinline__ unsigned philox_word(unsigned long long seed, unsigned c0, unsigned c1) {
    Philox r;
    r.init(seed, c0, c1);
    r.round4();
    return r.o0;
}

#define LP_AUG_PIXEL                                                                                                \
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;

// ---- Rot90 + Affine ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void labelaug_geom_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm, int H,
                                                            int W, u8* __restrict__ dst) {
    LP_AUG_PIXEL
    if (x >= W || y >= H) return;
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    const u8* frame = src + (size_t)b * H * W * 3;
    u8* o = dst + ((size_t)b * H * W + (size_t)y * W + x) * 3;
    if (!(p->flags & LP_AUG_GEOM)) {
        const u8* q = frame + ((size_t)y * W + x) * 3;
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        return;
    }
    const float dx = (float)x + 0.5f, dy = (float)y + 0.5f;
    const float sx = fmaf(p->geom[0], dx, fmaf(p->geom[1], dy, p->geom[2])) - 0.5f;
    const float sy = fmaf(p->geom[3], dx, fmaf(p->geom[4], dy, p->geom[5])) - 0.5f;
    float v[3] = {0.f, 0.f, 0.f};
    if (sx > -2.f && sy > -2.f && sx < (float)W + 1.f && sy < (float)H + 1.f) {  // otherwise (or non-finite): every tap is fill
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const float ax = sx - fx0, ay = sy - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xi = x0 + i, yi = y0 + j;
                if (xi < 0 || yi < 0 || xi >= W || yi >= H) continue;
                const float w = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay);
                const u8* q = frame + ((size_t)yi * W + xi) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = fmaf(w, (float)q[c], v[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = to_u8(v[c]);
}

// ---- MotionBlur -> CoarseDropout -> CoarseSalt -> CoarsePepper, or Emboss: a 5 x 5 (3 x 3) correlation over an LDS tile ----------------
constexpr int kHalo = 2, kTileW = 64 + 2 * kHalo, kTileH = 4 + 2 * kHalo;

__device__ __forceinline__ bool coarse_hit(uniform_ptr<lp_labelaug_image> p, int op, int ch, int x, int y, int H, int W,
                                           unsigned long long seed) {
    const int gh = p->coarse_gh[op], gw = p->coarse_gw[op];
    const int cell = (int)(((long long)y * gh) / H) * gw + (int)(((long long)x * gw) / W);
    return (philox_word(seed, (unsigned)cell, (unsigned)p->image_id | ((unsigned)op << 16) | ((unsigned)ch << 20)) >> 8) < p->coarse_thr[op];
}

__global__ __launch_bounds__(256) void labelaug_local_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm, int H,
                                                             int W, int which, const u8* __restrict__ salt_lut, unsigned long long seed,
                                                             u8* __restrict__ dst) {
    __shared__ u8 tile[kTileH][kTileW][4];
    LP_AUG_PIXEL
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    const int flags = p->flags;
    const bool conv = which == LP_AUG_LOCAL_EMBOSS ? (flags & LP_AUG_EMBOSS) != 0 : (flags & LP_AUG_BLUR) != 0;
    const u8* frame = src + (size_t)b * H * W * 3;
    if (conv) {  // (uniform over the workgroup: `flags` belongs to the image)
        const int x0 = blockIdx.x * 64 - kHalo, y0 = blockIdx.y * 4 - kHalo;
        for (int i = threadIdx.x; i < kTileH * kTileW; i += 256) {
            const int ty = i / kTileW, tx = i - ty * kTileW;
            const u8* q = frame + ((size_t)reflect101(y0 + ty, H) * W + reflect101(x0 + tx, W)) * 3;
            tile[ty][tx][0] = q[0], tile[ty][tx][1] = q[1], tile[ty][tx][2] = q[2];
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const int lx = (threadIdx.x & 63) + kHalo, ly = (threadIdx.x >> 6) + kHalo;
    u8 v[3];
    if (!conv) {
        const u8* q = frame + ((size_t)y * W + x) * 3;
        v[0] = q[0], v[1] = q[1], v[2] = q[2];
    } else if (which == LP_AUG_LOCAL_EMBOSS) {
        float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float w = p->emboss[j * 3 + i];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = fmaf(w, (float)tile[ly + j - 1][lx + i - 1][c], a[c]);
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = to_u8(a[c]);
    } else {
        float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float w = p->blur[j * 5 + i];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = fmaf(w, (float)tile[ly + j - 2][lx + i - 2][c], a[c]);
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = to_u8(a[c]);
    }
    if (which == LP_AUG_LOCAL_BLUR_COARSE) {
        if (flags & LP_AUG_DROPOUT) {
            if (flags & LP_AUG_DROP_PER_CHANNEL) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (coarse_hit(p, LP_AUG_OP_DROPOUT, c, x, y, H, W, seed)) v[c] = 0;
            } else if (coarse_hit(p, LP_AUG_OP_DROPOUT, 0, x, y, H, W, seed)) {
                v[0] = v[1] = v[2] = 0;
            }
        }
#pragma unroll
        for (int op = LP_AUG_OP_SALT; op <= LP_AUG_OP_PEPPER; ++op) {
            if (!(flags & (op == LP_AUG_OP_SALT ? LP_AUG_SALT : LP_AUG_PEPPER))) continue;
            if (!coarse_hit(p, op, 0, x, y, H, W, seed)) continue;
            const unsigned w = philox_word(seed, (unsigned)(y * W + x), (unsigned)p->image_id | ((unsigned)op << 16) | (1u << 24));
            const u8 s = salt_lut[w >> 24];
            v[0] = v[1] = v[2] = op == LP_AUG_OP_SALT ? s : (u8)(255 - s);
        }
    }
    u8* o = dst + ((size_t)b * H * W + (size_t)y * W + x) * 3;
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
}

// ---- ElasticTransformation ---------------------------------------------------------------------------------------------------------------
struct GaussTaps {
    int radius;
    float w[2 * LP_AUG_ELASTIC_MAX_RADIUS + 1];
};

// pass 1: the U(-1, 1) noise of a row segment (with its reflected halo) goes to LDS straight from Philox - the noise field is never stored -
// and is filtered along x
__global__ __launch_bounds__(256) void labelaug_elastic_rows_kernel(const lp_labelaug_image* __restrict__ prm, int H, int W, GaussTaps g,
                                                                    unsigned long long seed, float* __restrict__ tmp) {
    constexpr int kSpan = 64 + 2 * LP_AUG_ELASTIC_MAX_RADIUS;
    __shared__ float noise[2][4][kSpan];
    LP_AUG_PIXEL
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    if (!(p->flags & LP_AUG_ELASTIC)) return;
    const int R = g.radius, span = 64 + 2 * R;
    for (int i = threadIdx.x; i < 4 * span; i += 256) {
        const int r = i / span, cx = i - r * span;
        const int gy = blockIdx.y * 4 + r, gx = reflect101(blockIdx.x * 64 + cx - R, W);
        float nx = 0.f, ny = 0.f;
        if (gy < H) {
            Philox rng;
            rng.init(seed, (unsigned)(gy * W + gx), (unsigned)p->image_id | ((unsigned)LP_AUG_OP_ELASTIC << 16));
            nx = 2.f * rng.uniform() - 1.f;
            ny = 2.f * rng.uniform() - 1.f;
        }
        noise[0][r][cx] = nx, noise[1][r][cx] = ny;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const int lx = threadIdx.x & 63, r = threadIdx.x >> 6;
    float ax = 0.f, ay = 0.f;
    for (int t = 0; t <= 2 * R; ++t) {
        ax = fmaf(g.w[t], noise[0][r][lx + t], ax);
        ay = fmaf(g.w[t], noise[1][r][lx + t], ay);
    }
    const size_t plane = (size_t)H * W;
    tmp[((size_t)b * 2) * plane + (size_t)y * W + x] = ax;
    tmp[((size_t)b * 2 + 1) * plane + (size_t)y * W + x] = ay;
}

// pass 2: along y, times alpha
__global__ __launch_bounds__(256) void labelaug_elastic_cols_kernel(const lp_labelaug_image* __restrict__ prm, int H, int W, GaussTaps g,
                                                                    const float* __restrict__ tmp, float* __restrict__ field) {
    LP_AUG_PIXEL
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    if (!(p->flags & LP_AUG_ELASTIC) || x >= W || y >= H) return;
    const size_t plane = (size_t)H * W;
    const float* t0 = tmp + ((size_t)b * 2) * plane + x;
    float ax = 0.f, ay = 0.f;
    for (int t = 0; t <= 2 * g.radius; ++t) {
        const size_t row = (size_t)reflect101(y + t - g.radius, H) * W;
        ax = fmaf(g.w[t], t0[row], ax);
        ay = fmaf(g.w[t], t0[plane + row], ay);
    }
    field[((size_t)b * 2) * plane + (size_t)y * W + x] = p->elastic_alpha * ax;
    field[((size_t)b * 2 + 1) * plane + (size_t)y * W + x] = p->elastic_alpha * ay;
}

__global__ __launch_bounds__(256) void labelaug_elastic_apply_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm,
                                                                     int H, int W, const float* __restrict__ field, u8* __restrict__ dst) {
    LP_AUG_PIXEL
    if (x >= W || y >= H) return;
    const u8* frame = src + (size_t)b * H * W * 3;
    u8* o = dst + ((size_t)b * H * W + (size_t)y * W + x) * 3;
    if (!(as_uniform(prm + b)->flags & LP_AUG_ELASTIC)) {
        const u8* q = frame + ((size_t)y * W + x) * 3;
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        return;
    }
    const size_t plane = (size_t)H * W;
    const float dx = field[((size_t)b * 2) * plane + (size_t)y * W + x], dy = field[((size_t)b * 2 + 1) * plane + (size_t)y * W + x];
    int x0, y0;
    float wx[4], wy[4];
    cubic_taps((float)x + dx + 0.5f, x0, wx);
    cubic_taps((float)y + dy + 0.5f, y0, wy);
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yi = y0 + j;
        if (yi < 0 || yi >= H) continue;
        float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xi = x0 + i;
            if (xi < 0 || xi >= W) continue;
            const u8* q = frame + ((size_t)yi * W + xi) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = fmaf(wx[i], (float)q[c], r[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(wy[j], r[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = to_u8(acc[c]);
}

// ---- histogram equalisation ----------------------------------------------------------------------------------------------------------------
constexpr int kHistChunk = 8192;  // pixels per workgroup

// inclusive prefix sum over 256 LDS words, one thread per word (256 threads); the result is left in `a`
__device__ __forceinline__ unsigned scan256(unsigned* a, unsigned* tmp_, int i) {
    unsigned* in = a;
    unsigned* out = tmp_;
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        out[i] = in[i] + (i >= d ? in[i - d] : 0u);
        __syncthreads();
        unsigned* t = in;
        in = out, out = t;
    }
    // eight rounds: the result is back in `a`
    return in[i];
}

__global__ __launch_bounds__(256) void labelaug_hist_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm, int npix,
                                                            unsigned* __restrict__ hist) {
    __shared__ unsigned h[4][3][256];  // one copy per wave: a quarter of the LDS atomic collisions
    const int b = blockIdx.y;
    if (!(as_uniform(prm + b)->flags & LP_AUG_HISTEQ)) return;
    for (int i = threadIdx.x; i < 4 * 3 * 256; i += 256) (&h[0][0][0])[i] = 0u;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * kHistChunk, hi = min(lo + kHistChunk, npix);
    const u8* frame = src + (size_t)b * npix * 3;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const u8* q = frame + (size_t)i * 3;
        atomicAdd(&h[wave][0][q[0]], 1u);
        atomicAdd(&h[wave][1][q[1]], 1u);
        atomicAdd(&h[wave][2][q[2]], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += 256) {
        const unsigned s = (&h[0][0][0])[i] + (&h[1][0][0])[i] + (&h[2][0][0])[i] + (&h[3][0][0])[i];
        if (s) atomicAdd(&hist[(size_t)b * 768 + i], s);
    }
}

__global__ __launch_bounds__(256) void labelaug_histeq_lut_kernel(const lp_labelaug_image* __restrict__ prm, const unsigned* __restrict__ hist,
                                                                  int npix, u8* __restrict__ lut) {
    __shared__ unsigned a[256], t[256];
    __shared__ int last;
    const int c = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
    if (!(as_uniform(prm + b)->flags & LP_AUG_HISTEQ)) return;
    const unsigned hv = hist[((size_t)b * 3 + c) * 256 + i];
    a[i] = hv;
    if (i == 0) last = -1;
    __syncthreads();
    if (hv) atomicMax(&last, 255 - i);  // first occupied bin = 255 - last
    const unsigned cdf = scan256(a, t, i);
    const int first = 255 - last;
    const unsigned cmin = a[first];     // (the bins below `first` are empty: cdf[first] = hist[first])
    const unsigned long long den = (unsigned long long)npix - cmin;
    unsigned v = (unsigned)i;           // one grey level only: unchanged
    if (den > 0) v = i < first ? 0u : (unsigned)((2ull * 255ull * (cdf - cmin) + den) / (2ull * den));
    lut[((size_t)b * 3 + c) * 256 + i] = (u8)min(v, 255u);
}

__global__ __launch_bounds__(256) void labelaug_histeq_apply_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm,
                                                                    int H, int W, const u8* __restrict__ lut, u8* __restrict__ dst) {
    LP_AUG_PIXEL
    if (x >= W || y >= H) return;
    const size_t at = ((size_t)b * H * W + (size_t)y * W + x) * 3;
    const bool on = (as_uniform(prm + b)->flags & LP_AUG_HISTEQ) != 0;
    const u8* l = lut + (size_t)b * 768;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[at + c] = on ? l[c * 256 + src[at + c]] : src[at + c];
}

// ---- CLAHE -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void labelaug_clahe_lut_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm,
                                                                 const int* __restrict__ slot_image, int H, int W, int max_ty, int max_tx,
                                                                 u8* __restrict__ luts) {
    __shared__ unsigned a[256], t[256];
    __shared__ unsigned excess;
    const int slot = blockIdx.z, b = slot_image[slot], i = threadIdx.x;
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    const int ty = p->clahe_tiles_y, tx = p->clahe_tiles_x;
    if ((int)blockIdx.x >= tx || (int)blockIdx.y >= ty) return;
    const int th = (H + ty - 1) / ty, tw = (W + tx - 1) / tx, area = th * tw;
    const unsigned clip = (unsigned)p->clahe_clip;
    const u8* frame = src + (size_t)b * H * W * 3;
    for (int c = 0; c < 3; ++c) {
        a[i] = 0u;
        if (i == 0) excess = 0u;
        __syncthreads();
        for (int k = i; k < area; k += 256) {
            const int py = k / tw, px = k - py * tw;
            const int sy = reflect101(blockIdx.y * th + py, H), sx = reflect101(blockIdx.x * tw + px, W);  // beyond the edge: reflected
            atomicAdd(&a[frame[((size_t)sy * W + sx) * 3 + c]], 1u);
        }
        __syncthreads();
        unsigned hv = a[i];
        if (hv > clip) {
            atomicAdd(&excess, hv - clip);
            hv = clip;
        }
        __syncthreads();
        const unsigned ex = excess, batch = ex / 256u, resid = ex - batch * 256u;
        hv += batch;
        if (resid) {
            const unsigned step = max(256u / resid, 1u);
            if ((unsigned)i % step == 0u && (unsigned)i / step < resid) ++hv;
        }
        a[i] = hv;
        __syncthreads();
        const unsigned cdf = scan256(a, t, i);
        const unsigned v = (unsigned)((2ull * 255ull * cdf + (unsigned)area) / (2ull * (unsigned)area));
        luts[((((size_t)slot * max_ty + blockIdx.y) * max_tx + blockIdx.x) * 3 + c) * 256 + i] = (u8)min(v, 255u);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void labelaug_clahe_apply_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm,
                                                                   int H, int W, int max_ty, int max_tx, const u8* __restrict__ luts,
                                                                   u8* __restrict__ dst) {
    LP_AUG_PIXEL
    if (x >= W || y >= H) return;
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    const size_t at = ((size_t)b * H * W + (size_t)y * W + x) * 3;
    if (!(p->flags & LP_AUG_CLAHE)) {
        dst[at] = src[at], dst[at + 1] = src[at + 1], dst[at + 2] = src[at + 2];
        return;
    }
    const int ty = p->clahe_tiles_y, tx = p->clahe_tiles_x;
    const int th = (H + ty - 1) / ty, tw = (W + tx - 1) / tx;
    const float fy = (float)y / (float)th - 0.5f, fx = (float)x / (float)tw - 0.5f;   // OpenCV: tyf = y * inv_th - 0.5
    const float fy0 = floorf(fy), fx0 = floorf(fx);
    const float ay = fy - fy0, ax = fx - fx0;
    const int y1 = clampi((int)fy0, 0, ty - 1), y2 = clampi((int)fy0 + 1, 0, ty - 1);
    const int x1 = clampi((int)fx0, 0, tx - 1), x2 = clampi((int)fx0 + 1, 0, tx - 1);
    const u8* base = luts + (size_t)p->clahe_slot * max_ty * max_tx * 768;
    const u8* l11 = base + ((size_t)y1 * max_tx + x1) * 768;
    const u8* l12 = base + ((size_t)y1 * max_tx + x2) * 768;
    const u8* l21 = base + ((size_t)y2 * max_tx + x1) * 768;
    const u8* l22 = base + ((size_t)y2 * max_tx + x2) * 768;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = c * 256 + src[at + c];
        const float top = fmaf(ax, (float)l12[v] - (float)l11[v], (float)l11[v]);
        const float bot = fmaf(ax, (float)l22[v] - (float)l21[v], (float)l21[v]);
        dst[at + c] = to_u8(fmaf(ay, bot - top, top));
    }
}

// ---- CropAndPad -> cubic Resize -> /255 -> normalise -> optional mirror: lp_frames_resize_cubic's arithmetic on a per-image window ----------
struct FinishNorm {
    float mean[3], inv_std[3];
};

__global__ __launch_bounds__(256) void labelaug_finish_kernel(const u8* __restrict__ src, const lp_labelaug_image* __restrict__ prm, int Hs,
                                                              int Ws, int H, int W, FinishNorm nrm, float* __restrict__ dst) {
    LP_AUG_PIXEL
    if (x >= W || y >= H) return;
    uniform_ptr<lp_labelaug_image> p = as_uniform(prm + b);
    const int flags = p->flags;
    int top = 0, right = 0, bottom = 0, left = 0;
    if (flags & LP_AUG_CROPPAD) top = p->pad[0], right = p->pad[1], bottom = p->pad[2], left = p->pad[3];
    const int Hc = Hs + top + bottom, Wc = Ws + left + right;  // the cropped / padded image the resize sees (>= 1: checked by the host)
    const float scale_y = (float)((double)Hc / H), scale_x = (float)((double)Wc / W);
    int x0, y0;
    float wx[4], wy[4];
    cubic_taps(((float)x + 0.5f) * scale_x, x0, wx);
    cubic_taps(((float)y + 0.5f) * scale_y, y0, wy);
    const u8* frame = src + (size_t)b * Hs * Ws * 3;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sy = clampi(y0 + j, 0, Hc - 1) - top;   // taps clamped to the window, then moved into the stored image
        float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int sx = clampi(x0 + i, 0, Wc - 1) - left;
            if (sy < 0 || sy >= Hs || sx < 0 || sx >= Ws) continue;  // zero padding
            const u8* q = frame + ((size_t)sy * Ws + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = fmaf(wx[i], (float)q[c], r[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(wy[j], r[c], acc[c]);
    }
    const int xo = (flags & LP_AUG_HFLIP) ? W - 1 - x : x;
    const size_t plane = (size_t)H * W;
    float* o = dst + (size_t)b * 3 * plane + (size_t)y * W + xo;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(floorf(acc[c] + 0.5f), 0.f), 255.f);
        o[c * plane] = (v * (1.f / 255.f) - nrm.mean[c]) * nrm.inv_std[c];
    }
}

// ---- keypoints through Rot90 / Affine and the elastic field -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void labelaug_keypoints_kernel(const float* __restrict__ kp, int n, int K, const float* __restrict__ affine,
                                                                 const lp_labelaug_image* __restrict__ prm, const float* __restrict__ field,
                                                                 int H, int W, float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int b = idx / K;
    const float x0 = kp[(size_t)idx * 2], y0 = kp[(size_t)idx * 2 + 1];
    float x = x0, y = y0;
    if (affine != nullptr) {
        const float* a = affine + (size_t)b * 6;
        x = fmaf(a[0], x0, fmaf(a[1], y0, a[2]));
        y = fmaf(a[3], x0, fmaf(a[4], y0, a[5]));
    }
    if (field != nullptr && (prm[b].flags & LP_AUG_ELASTIC) && x == x && y == y) {
        // the image shows in(q + d(q)) at q: a source point s appears where q + d(q) = s, to first order q = s - d(s)
        const float sx = fminf(fmaxf(x - 0.5f, 0.f), (float)(W - 1)), sy = fminf(fmaxf(y - 0.5f, 0.f), (float)(H - 1));
        const int xa = (int)sx, ya = (int)sy, xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);
        const float ax = sx - (float)xa, ay = sy - (float)ya;
        const size_t plane = (size_t)H * W;
        float d[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* f = field + ((size_t)b * 2 + c) * plane;
            const float t = fmaf(ax, f[(size_t)ya * W + xb] - f[(size_t)ya * W + xa], f[(size_t)ya * W + xa]);
            const float u = fmaf(ax, f[(size_t)yb * W + xb] - f[(size_t)yb * W + xa], f[(size_t)yb * W + xa]);
            d[c] = fmaf(ay, u - t, t);
        }
        x -= d[0], y -= d[1];
    }
    out[(size_t)idx * 2] = x;
    out[(size_t)idx * 2 + 1] = y;
}

static inline dim3 pixel_grid(int B, int H, int W) { return dim3((W + 63) / 64, (H + 3) / 4, B); }

static inline bool pixel_grid_ok(int B, int H, int W) {
    return B <= 65535 && (H + 3) / 4 <= 65535 && (long long)B * H * W * 3 < (1ll << 40) && (long long)H * W < (1ll << 30);
}

}  // namespace lp

// ------------------------------------------------------------------------------------------------------- C ABI
#define LP_AUG_COMMON_ARGS(extra)                                            \
    using namespace lp;                                                      \
    LP_REQUIRE(params && B > 0 && H > 0 && W > 0 && (extra));               \
    if (!pixel_grid_ok(B, H, W)) return LP_ERR_UNSUPPORTED;

extern "C" int lp_labelaug_geom(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, void* dst_u8, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(src_u8 && dst_u8 && src_u8 != dst_u8)
    hipLaunchKernelGGL(labelaug_geom_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, H, W,
                       (u8*)dst_u8);
    return launch_status();
}

extern "C" int lp_labelaug_local(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, int which, const void* salt_lut,
                                 unsigned long long seed, void* dst_u8, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(src_u8 && dst_u8 && src_u8 != dst_u8)
    LP_REQUIRE(which == LP_AUG_LOCAL_EMBOSS || (which == LP_AUG_LOCAL_BLUR_COARSE && salt_lut));
    hipLaunchKernelGGL(labelaug_local_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, H, W, which,
                       (const u8*)salt_lut, seed, (u8*)dst_u8);
    return launch_status();
}

extern "C" int lp_labelaug_elastic_field(int B, int H, int W, const lp_labelaug_image* params, float sigma, unsigned long long seed,
                                         float* tmp, float* field, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(tmp && field && tmp != field && sigma > 0.f)
    GaussTaps g{};
    g.radius = (int)(4.0 * (double)sigma + 0.5);
    if (g.radius > LP_AUG_ELASTIC_MAX_RADIUS) return LP_ERR_UNSUPPORTED;
    double sum = 0.0, w[2 * LP_AUG_ELASTIC_MAX_RADIUS + 1];
    for (int t = 0; t <= 2 * g.radius; ++t) sum += w[t] = exp(-0.5 * (double)(t - g.radius) * (t - g.radius) / ((double)sigma * sigma));
    for (int t = 0; t <= 2 * g.radius; ++t) g.w[t] = (float)(w[t] / sum);
    hipLaunchKernelGGL(labelaug_elastic_rows_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, params, H, W, g, seed, tmp);
    hipLaunchKernelGGL(labelaug_elastic_cols_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, params, H, W, g,
                       (const float*)tmp, field);
    return launch_status();
}

extern "C" int lp_labelaug_elastic_apply(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, const float* field,
                                         void* dst_u8, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(src_u8 && dst_u8 && src_u8 != dst_u8 && field)
    hipLaunchKernelGGL(labelaug_elastic_apply_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, H, W,
                       field, (u8*)dst_u8);
    return launch_status();
}

extern "C" int lp_labelaug_histeq(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, unsigned* ws, void* lut_out,
                                  void* dst_u8, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(src_u8 && dst_u8 && src_u8 != dst_u8 && ws && lut_out)
    const int npix = H * W;
    if (hipMemsetAsync(ws, 0, (size_t)B * 768 * sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return launch_status();
    hipLaunchKernelGGL(labelaug_hist_kernel, dim3((npix + kHistChunk - 1) / kHistChunk, B), dim3(256), 0, (hipStream_t)stream,
                       (const u8*)src_u8, params, npix, ws);
    hipLaunchKernelGGL(labelaug_histeq_lut_kernel, dim3(3, B), dim3(256), 0, (hipStream_t)stream, params, (const unsigned*)ws, npix,
                       (u8*)lut_out);
    hipLaunchKernelGGL(labelaug_histeq_apply_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, H, W,
                       (const u8*)lut_out, (u8*)dst_u8);
    return launch_status();
}

extern "C" int lp_labelaug_clahe(const void* src_u8, int B, int H, int W, const lp_labelaug_image* params, const int* slot_image, int n_slots,
                                 int max_ty, int max_tx, void* luts, void* dst_u8, lp_stream_t stream) {
    LP_AUG_COMMON_ARGS(src_u8 && dst_u8 && src_u8 != dst_u8 && n_slots >= 0 && n_slots <= B)
    if (n_slots > 0) {
        LP_REQUIRE(slot_image && luts && max_ty > 0 && max_tx > 0 && max_ty <= H && max_tx <= W);
        if (max_ty > 65535) return LP_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(labelaug_clahe_lut_kernel, dim3(max_tx, max_ty, n_slots), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8,
                           params, slot_image, H, W, max_ty, max_tx, (u8*)luts);
    }
    hipLaunchKernelGGL(labelaug_clahe_apply_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, H, W,
                       max_ty, max_tx, (const u8*)luts, (u8*)dst_u8);
    return launch_status();
}

extern "C" int lp_labelaug_finish(const void* src_u8, int B, int Hs, int Ws, const lp_labelaug_image* params, int H, int W,
                                  const lp_frame_norm* norm, float* dst, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(src_u8 && params && norm && dst && B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0);
    if (!pixel_grid_ok(B, H, W) || !pixel_grid_ok(B, Hs, Ws)) return LP_ERR_UNSUPPORTED;
    FinishNorm nrm{};
    for (int c = 0; c < 3; ++c) {
        LP_REQUIRE(norm->std[c] > 0.f);
        nrm.mean[c] = norm->mean[c], nrm.inv_std[c] = 1.f / norm->std[c];
    }
    hipLaunchKernelGGL(labelaug_finish_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, params, Hs, Ws, H, W,
                       nrm, dst);
    return launch_status();
}

extern "C" int lp_labelaug_keypoints(const float* kp, int B, int K, const float* affine, const lp_labelaug_image* params, const float* field,
                                     int H, int W, float* kp_out, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(kp && kp_out && kp != kp_out && B > 0 && K > 0 && H > 0 && W > 0 && (field == nullptr || params != nullptr));
    hipLaunchKernelGGL(labelaug_keypoints_kernel, dim3((B * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, kp, B * K, K, affine, params,
                       field, H, W, kp_out);
    return launch_status();
}
