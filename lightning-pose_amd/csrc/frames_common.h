// Helpers shared by the batch-producer kernels (frames.hip, cropzoom.hip, labelaug.hip): index clamping, the Keys bicubic taps of
// OpenCV's INTER_CUBIC, the normalisation constants and the counter-based Philox4x32-10 generator.
#pragma once
#include "lp_common.h"

namespace lp {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct NormSpec {
    float mean[3], inv_std[3];
};

// Keys kernel with A = -0.75 on half-pixel centres: the four taps start at source pixel i0
__device__ __forceinline__ void cubic_taps(float c, int& i0, float (&w)[4]) {
    const float A = -0.75f;
    const float f = c - 0.5f;
    const float fl = floorf(f);
    const float t = f - fl;
    i0 = (int)fl - 1;
    auto k1 = [&](float u) { return ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f; };          // |u| <= 1
    auto k2 = [&](float u) { return ((A * u - 5.f * A) * u + 8.f * A) * u - 4.f * A; };    // 1 < |u| < 2
    w[0] = k2(t + 1.f);
    w[1] = k1(t);
    w[2] = k1(1.f - t);
    w[3] = k2(2.f - t);
}

// ---- counter-based random numbers (Philox4x32-10): a pixel's stream depends only on (seed, frame, pixel) ---------------
struct Philox {  // scalar members only: nothing here is indexed dynamically, so the state stays in registers
    unsigned c0, c1, c2, k0, k1, o0, o1, o2, o3;
    int have;
    __device__ __forceinline__ void init(unsigned long long seed, unsigned ctr0, unsigned ctr1) {
        k0 = (unsigned)seed;
        k1 = (unsigned)(seed >> 32);
        c0 = ctr0;
        c1 = ctr1;
        c2 = 0;
        have = 0;
    }
    __device__ __forceinline__ void round4() {
        unsigned ka = k0, kb = k1, x0 = c0, x1 = c1, x2 = c2, x3 = 0;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const unsigned long long p0 = (unsigned long long)0xD2511F53u * x0, p1 = (unsigned long long)0xCD9E8D57u * x2;
            const unsigned y0 = (unsigned)(p1 >> 32) ^ x1 ^ ka, y1 = (unsigned)p1, y2 = (unsigned)(p0 >> 32) ^ x3 ^ kb, y3 = (unsigned)p0;
            x0 = y0;
            x1 = y1;
            x2 = y2;
            x3 = y3;
            ka += 0x9E3779B9u;
            kb += 0xBB67AE85u;
        }
        o0 = x0;
        o1 = x1;
        o2 = x2;
        o3 = x3;
        c2 += 1;  // next block of four
        have = 4;
    }
    __device__ __forceinline__ float uniform() {  // (0, 1)
        if (have == 0) round4();
        const unsigned v = have == 4 ? o0 : (have == 3 ? o1 : (have == 2 ? o2 : o3));
        --have;
        return ((float)(v >> 8) + 0.5f) * (1.f / 16777216.f);
    }
};

}  // namespace lp

static inline bool norm_spec(const lp_frame_norm* n, lp::NormSpec& out) {
    for (int c = 0; c < 3; ++c) {
        if (!(n->std[c] > 0.f)) return false;
        out.mean[c] = n->mean[c];
        out.inv_std[c] = 1.f / n->std[c];
    }
    return true;
}
