// Patch masking for the multi-view transformer's curriculum (reference: lightning_pose/callbacks.py:279-401, PatchMasker): choose `count`
// of the N = (H / patch) (W / patch) patches of every image and write the batch with those patches zeroed - ONE launch, no host round
// trip, no workspace.  gfx950.
//
// The reference seeds a torch generator per (sample, view) with patch_seed + step + 1000 b + 100 v, takes randperm(N)[:count] and walks
// the indices in a Python loop (one device -> host copy and one slice assignment per patch).  Here the choice is a pure function of
// (key, image, patch):
//   word(i, p) = first output word of Philox4x32-10 with key `key` and counter (p, i, 0, 0)
//   patch p of image i is masked  <=>  fewer than `count` of the N pairs (word(i, q), q) are lexicographically smaller than (word(i, p), p)
// which masks exactly `count` patches for any N, does not depend on the launch geometry, and - key = seed | step << 32 - never gives two
// different (step, sample, view) the same stream (the reference's sum does: step 100 of sample 0 = step 0 of view 1).
//
// Work split: the rows of one channel fall into nh bands of `patch` rows (one row of patches each) + the rows below the grid; a
// workgroup owns a few consecutive (channel, band) units of one image.  Every workgroup first recomputes its image's N words into LDS
// and ranks them (a thread owns up to four patches and scans the N words - broadcast reads), which costs less than passing the choice
// through memory and a second launch would.  Inside a band the patch row is uniform and a thread's columns are fixed, so the copy loop
// holds no division: 16 B per lane when the rows allow it, 4 B otherwise.
#include "frames_common.h"

namespace lp {

constexpr int kPatchMaskMaxN = 1024, kPatchMaskThreads = 256;

struct PatchMaskArgs {
    const float* images;
    const float* mask_in;
    float* out;
    float* mask_out;
    unsigned long long key;
    int C, H, W, patch, nh, nw, count;
    int units_per_wg;   // (channel, band) units per workgroup
    int tx_shift;       // a row is walked by 1 << tx_shift lanes, the workgroup covers 256 >> tx_shift rows per pass
};

// kVec: W % 4 == 0, patch % 4 == 0 and both pointers 16-byte aligned - a 16-byte piece never straddles a patch edge
template <bool kVec>
__global__ __launch_bounds__(kPatchMaskThreads) void patch_mask_kernel(PatchMaskArgs a) {
    __shared__ unsigned word[kPatchMaskMaxN];
    __shared__ unsigned char keep[kPatchMaskMaxN];
    const int tid = threadIdx.x, i = blockIdx.y;
    const int N = a.nh * a.nw;

    // ---- the choice: keep[p] for every patch of image i -------------------------------------------------------------------------------
    if (a.mask_in) {
        for (int p = tid; p < N; p += kPatchMaskThreads) keep[p] = a.mask_in[(size_t)i * N + p] != 0.f;
    } else {
        for (int p = tid; p < N; p += kPatchMaskThreads) {
            Philox r;
            r.init(a.key, (unsigned)p, (unsigned)i);
            r.round4();
            word[p] = r.o0;
        }
        __syncthreads();
        unsigned mine[4];
        int rank[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = tid + k * kPatchMaskThreads;
            mine[k] = p < N ? word[p] : 0u;
        }
        for (int q = 0; q < N; ++q) {
            const unsigned wq = word[q];   // the same address in every lane: one broadcast read
#pragma unroll
            for (int k = 0; k < 4; ++k) rank[k] += (wq < mine[k]) || (wq == mine[k] && q < tid + k * kPatchMaskThreads);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = tid + k * kPatchMaskThreads;
            if (p < N) keep[p] = rank[k] >= a.count;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int p = tid; p < N; p += kPatchMaskThreads) a.mask_out[(size_t)i * N + p] = keep[p] ? 1.f : 0.f;

    // ---- copy / zero this workgroup's (channel, band) units ---------------------------------------------------------------------------
    constexpr int kE = kVec ? 4 : 1;                       // floats per piece
    const int pieces = a.W / kE;                           // pieces per row
    const int nbands = a.nh + (a.H > a.nh * a.patch);      // + the rows below the patch grid, never masked
    const int tx = tid & ((1 << a.tx_shift) - 1), ty = tid >> a.tx_shift;
    const int xs = 1 << a.tx_shift, ys = kPatchMaskThreads >> a.tx_shift;
    const bool in_place = a.images == a.out;
    const int u0 = blockIdx.x * a.units_per_wg, u1 = min(u0 + a.units_per_wg, a.C * nbands);
    for (int u = u0; u < u1; ++u) {
        const int c = u / nbands, band = u - c * nbands;
        const int y0 = band * a.patch, rows = band < a.nh ? a.patch : a.H - y0;
        const size_t base = (((size_t)i * a.C + c) * a.H + y0) * a.W;
        for (int x = tx; x < pieces; x += xs) {
            const int px = (x * kE) / a.patch;
            const bool kept = band >= a.nh || px >= a.nw || keep[band * a.nw + px];
            if (kept && in_place) continue;
            for (int y = ty; y < rows; y += ys) {
                const size_t o = base + (size_t)y * a.W + (size_t)x * kE;
                if (kVec) {
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);   // (bits, not floats: a kept NaN keeps its payload)
                    if (kept) v = *reinterpret_cast<const uint4*>(a.images + o);
                    *reinterpret_cast<uint4*>(a.out + o) = v;
                } else {
                    unsigned v = 0u;
                    if (kept) v = *reinterpret_cast<const unsigned*>(a.images + o);
                    *reinterpret_cast<unsigned*>(a.out + o) = v;
                }
            }
        }
    }
}

}  // namespace lp

// ------------------------------------------------------------------------------------------------------- C ABI
extern "C" int lp_patch_mask_f32(const float* images, int BV, int C, int H, int W, int patch, int count, unsigned long long key,
                                 const float* mask_in, float* out, float* mask_out, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(images && out && mask_out && BV > 0 && C > 0 && H > 0 && W > 0 && patch > 0 && H >= patch && W >= patch);
    const int nh = H / patch, nw = W / patch;
    const long long N = (long long)nh * nw;
    if (N > kPatchMaskMaxN || BV > 65535 || (long long)C * (nh + 1) >= (1ll << 30)) return LP_ERR_UNSUPPORTED;
    LP_REQUIRE(mask_in || (count >= 0 && count <= N));
    const bool vec = W % 4 == 0 && patch % 4 == 0 && (((uintptr_t)images | (uintptr_t)out) & 15) == 0;
    PatchMaskArgs a{images, mask_in, out, mask_out, key, C, H, W, patch, nh, nw, count, 1, 0};
    const int pieces = vec ? W / 4 : W;
    while ((1 << a.tx_shift) < pieces && (1 << a.tx_shift) < kPatchMaskThreads) ++a.tx_shift;
    // ~32 KB read + 32 KB written per workgroup: enough to pay for ranking the words again, small enough to fill the chip at a few images
    const long long band_bytes = (long long)patch * W * 4;
    a.units_per_wg = (int)(band_bytes >= 32768 ? 1 : 32768 / band_bytes);
    const int units = C * (nh + (H > nh * patch));
    const dim3 grid((units + a.units_per_wg - 1) / a.units_per_wg, BV);
    if (vec)
        hipLaunchKernelGGL(patch_mask_kernel<true>, grid, dim3(kPatchMaskThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(patch_mask_kernel<false>, grid, dim3(kPatchMaskThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}
